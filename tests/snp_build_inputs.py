"""Inputs and the Python model of the SNP table builder (csvgpu_snp_builder_*): what one append reports (the CHROM runs of the kept
records, the deferred offsets) and what finish leaves per contig, from the per-line rules of tests/vcf_parse_inputs.py and nothing of the
device code. A `Model` mirrors a builder call for call; names get ids in order of first appearance, as the host mirror deals them out.

Lines the device defers have no Python rule (their decision hangs on libc's conversions): `deferred_record` is the stand-in for the host
parser that the tests hand them to. What it returns is the test's own choice — the builder only has to put the record at its file
position — so it is a fixed function of the line: kept with the POS field's leading digits (7 if none) and a baf that no kept record
has, unless the line's REF is 'N' (then not kept)."""
import re

import numpy as np

import vcf_parse_inputs as inp

T = 4096                      # _lib.VCF_TILE_BYTES
DEFER_BAF = 0.015625
_DIGITS = re.compile(rb"[0-9]{1,9}")


def good(p, chrom="chr1", qual="50", dp="40", ad="10,30"):
    return (inp.GOOD % (p, qual, dp, ad)).replace("chr1", chrom, 1).encode()


def deferred(p, chrom="chr1", ref="A"):
    """a line the device defers (hex QUAL), of `chrom`"""
    line = good(p, chrom, qual="0x1p5")
    f = line.split(b"\t")
    f[3] = ref.encode()
    return b"\t".join(f)


def skipped(p, chrom="chr1"):
    return good(p, chrom, qual="3")


def body(lines, end=b"\n", last=True):
    return end.join(lines) + (end if last else b"")


def deferred_record(line: bytes):
    """-> (chrom, pos, baf) or None: the stand-in host parser for a deferred line"""
    f = line.split(b"\t")
    if len(f) > 3 and f[3] == b"N":
        return None
    m = _DIGITS.match(f[1]) if len(f) > 1 else None
    return f[0], (int(m.group()) if m else 7), DEFER_BAF


def runs_of(text: bytes, exp):
    """the CHROM runs of the kept records of one call -> (first, line_off, chrom_len, names)"""
    first, names = [], []
    for k, (off, cl) in enumerate(zip(exp["line_off"].tolist(), exp["chrom_len"].tolist())):
        name = text[off:off + cl]
        if k == 0 or name != names[-1]:
            first.append(k)
            names.append(name)
    f = np.array(first, np.int64)
    return (f.astype(np.uint32), exp["line_off"][f], exp["chrom_len"][f], names)


def expected_append(text: bytes, dp_int=True, ad_int=True):
    """what csvgpu_snp_builder_append reports for one batch"""
    exp = inp.expected_snp(text, dp_int, ad_int)
    first, loff, clen, names = runs_of(text, exp)
    return dict(exp, run_first=first, run_line_off=loff, run_chrom_len=clen, run_names=names, n_runs=len(first), n_kept=len(exp["pos"]),
                n_deferred=len(exp["defer_off"]))


def line_at(text: bytes, off: int) -> bytes:
    e = text.find(b"\n", off)
    line = text[off:len(text) if e < 0 else e]
    return line[:-1] if line.endswith(b"\r") else line


class Model:
    """a builder in Python: records as (contig id, order key, pos, baf); ids by first appearance of a name"""

    def __init__(self):
        self.ids, self.rec, self.run_contig = {}, [], []
        self.n_device = self.n_host = 0

    def id_of(self, name: bytes) -> int:
        return self.ids.setdefault(bytes(name), len(self.ids))

    def append(self, text: bytes, text_base=0, dp_int=True, ad_int=True):
        """one device append -> the expected report; the deferred lines' records are NOT added (host_deferred does that)"""
        e = expected_append(text, dp_int, ad_int)
        assert e["declined_at"] is None
        e["first_run"] = len(self.run_contig)
        ids = [self.id_of(n) for n in e["run_names"]]
        self.run_contig += ids
        bounds = e["run_first"].tolist() + [e["n_kept"]]
        for r, cid in enumerate(ids):
            for k in range(bounds[r], bounds[r + 1]):
                self.rec.append((cid, text_base + int(e["line_off"][k]), int(e["pos"][k]), float(e["value"][k])))
        self.n_device += e["n_kept"]
        return e

    def host_records(self, text: bytes, offsets, text_base=0):
        """the stand-in host parser on the lines at `offsets` -> arrays for append_host (and added to the model)"""
        cid, key, pos, baf = [], [], [], []
        for off in offsets:
            r = deferred_record(line_at(text, int(off)))
            if r is None:
                continue
            cid.append(self.id_of(r[0])); key.append(text_base + int(off)); pos.append(r[1]); baf.append(r[2])
            self.rec.append((cid[-1], key[-1], pos[-1], baf[-1]))
        self.n_host += len(cid)
        return np.array(cid, np.uint32), np.array(key, np.uint64), np.array(pos, np.uint32), np.array(baf, np.float64)

    def host_batch(self, text: bytes, text_base=0):
        """a whole batch through the host: kept lines by the Python rule, deferred ones by the stand-in -> arrays for append_host"""
        cid, key, pos, baf = [], [], [], []
        for off, line in inp.lines_of(text):
            if line[:1] == b"#":
                continue
            c = inp.snp_rule(line)
            if c[0] == "keep":
                r = (line[:c[1]], c[2], c[3])
            elif c[0] == "defer":
                r = deferred_record(line)
            else:
                r = None
            if r is None:
                continue
            cid.append(self.id_of(r[0])); key.append(text_base + off); pos.append(r[1]); baf.append(r[2])
            self.rec.append((cid[-1], key[-1], pos[-1], baf[-1]))
        self.n_host += len(cid)
        return np.array(cid, np.uint32), np.array(key, np.uint64), np.array(pos, np.uint32), np.array(baf, np.float64)

    def columns(self):
        """-> {contig id: (pos uint32, baf float64, ascending)} ordered by the key inside each contig"""
        out = {}
        for cid in sorted({r[0] for r in self.rec}):
            rs = sorted((r for r in self.rec if r[0] == cid), key=lambda r: r[1])
            assert len({r[1] for r in rs}) == len(rs), "two records of a contig share a key"
            pos = np.array([r[2] for r in rs], np.uint32)
            out[cid] = (pos, np.array([r[3] for r in rs], np.float64), bool((pos[1:] >= pos[:-1]).all()))
        return out


# ---- the CHROM name families: (label, [names]) — every pair adjacent in one text, each name on several lines ------------------------------
NAME_17 = "c" * 16 + "x"
NAME_40 = "scaffold_" + "0123456789" * 3 + "z"
NAME_FAMILIES = [
    ("chr1/chr2", ["chr1", "chr2"]),
    ("a prefix", ["chr1", "chr10"]),
    ("chr1/1", ["chr1", "1"]),
    ("one byte", ["1", "2", "1"]),
    ("17 bytes", [NAME_17, NAME_17[:-1] + "y", NAME_17[:-1]]),
    ("40 bytes", [NAME_40, NAME_40[:-1] + "y"]),
    ("equal in 16 bytes", ["0123456789abcdefA", "0123456789abcdefB", "0123456789abcdef"]),
]


def name_text(names, per=3, pad=0, start=100):
    """`per` kept lines of every name in turn, behind `pad` bytes of skipped lines"""
    lines, p = [], start
    while sum(len(l) + 1 for l in lines) < pad:
        lines.append(skipped(p, "pad"))
        p += 1
    for n in names:
        for _ in range(per):
            lines.append(good(p, n))
            p += 1
    return body(lines)


def tile_edge_texts(names):
    """the names' lines placed so that the first name's CHROM field straddles the tile edge at every split of its bytes"""
    out = []
    for cut in range(1, len(names[0])):
        lines, p = [], 100
        fill = skipped(p, "pad")
        while sum(len(l) + 1 for l in lines) + len(fill) + 1 <= T - cut - 64:
            lines.append(fill)
        used = sum(len(l) + 1 for l in lines)
        gap = T - cut - used                         # bytes up to where the name must start
        lines.append(skipped(5, "p" * (gap - (len(skipped(5, "")) + 1))))
        assert sum(len(l) + 1 for l in lines) == T - cut
        for n in names:
            for _ in range(2):
                p += 1
                lines.append(good(p, n))
        out.append(body(lines))
    return out


def generated():
    """the generated sample text (tests/vcf_parse_inputs.py) and its records"""
    return inp.generated_snp_text()


def big_text(n=70_000, seed=5):
    """about n kept records over five contigs in stretches of random length, positions ascending inside a contig, a few skipped lines
    and none deferred: the whole text is the device's"""
    rng = np.random.default_rng(seed)
    names = ["chr1", "chr2", "chr10", "chrX", "1"]
    nxt = {c: 1 for c in names}
    lines = []
    while len(lines) < n:
        c = names[int(rng.integers(len(names)))]
        for _ in range(int(rng.integers(1, 400))):
            nxt[c] += int(rng.integers(1, 50))
            lines.append(skipped(nxt[c], c) if rng.random() < 0.002 else good(nxt[c], c, ad="%d,%d" % (rng.integers(1, 60), rng.integers(1, 60))))
    return body(lines)
