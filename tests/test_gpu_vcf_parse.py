"""VCF lines parsed on the device (csvgpu_vcf_snp_parse / csvgpu_vcf_af_parse / _dev, kernels/vcfparse.hip): array for array, count for
count and offset for offset what tests/vcf_parse_inputs.py computes in Python from the host reader's rules (tests/test_vcf_parse_inputs.py
pins those against the host reader and the oracle on the CPU, and tests/test_vcf_record_core.py has run the per-line decisions against the
host reader under the sanitizers). `value` is compared bit for bit, NaN as NaN. Every output array lies between guard bytes and carries
slack behind its last element: everything outside the reported records must still hold the guard byte afterwards."""
import os
import subprocess
import sys

import numpy as np
import pytest

import vcf_parse_inputs as inp
from contextsv_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 64
T = _lib.VCF_TILE_BYTES
DTYPES = dict(line_off=np.uint32, chrom_len=np.uint32, pos=np.uint32, value=np.float64, defer_off=np.uint32)


class Out:
    """guarded output arrays with room for n kept records and d deferred lines + slack"""

    def __init__(self, n, d, af, slack=3):
        sizes = dict(line_off=n, pos=n, value=n, defer_off=d)
        if not af:
            sizes["chrom_len"] = n
        self.full, self.view = {}, {}
        for k, m in sizes.items():
            isz = np.dtype(DTYPES[k]).itemsize
            self.full[k] = np.full((m + slack + 2 * G) * isz, inp.GUARD, np.uint8)
            self.view[k] = self.full[k][G * isz:(G + m + slack) * isz].view(DTYPES[k])

    def intact_outside(self, c):
        for k, full in self.full.items():
            isz = np.dtype(DTYPES[k]).itemsize
            m = np.ones(len(full), bool)
            m[G * isz:(G + (c["n_deferred"] if k == "defer_off" else c["n_kept"])) * isz] = False
            if not (full[m] == inp.GUARD).all():
                return k
        return None


def _assert_equal(rc, c, out, exp):
    assert rc == 0 and c["status"] == 0, (rc, c)
    assert (c["n_lines"], c["n_kept"], c["n_deferred"], c["stop_off"]) == (exp["n_lines"], len(exp["pos"]), len(exp["defer_off"]), exp["stop_off"]), c
    for k in out.view:
        got = out.view[k][:len(exp[k])]
        if k == "value":
            same = (got.view(np.uint64) == exp[k].view(np.uint64)) | (np.isnan(got) & np.isnan(exp[k]))
            assert same.all(), (k, np.flatnonzero(~same)[:5], got[~same][:5], exp[k][~same][:5])
        else:
            assert np.array_equal(got, exp[k]), (k, np.flatnonzero(got != exp[k])[:5])
    assert out.intact_outside(c) is None, "written outside the reported records: " + str(out.intact_outside(c))


def _snp(ctx, text, dp_int=True, ad_int=True):
    exp = inp.expected_snp(text, dp_int, ad_int)
    assert exp["declined_at"] is None
    out = Out(len(exp["pos"]), len(exp["defer_off"]), False)
    rc, c = ctx.vcf_snp_parse_into(text, out.view, dp_int, ad_int)
    _assert_equal(rc, c, out, exp)
    return exp


def _af(ctx, text, contig, needle, pos):
    pos = np.asarray(pos, np.uint32)
    exp = inp.expected_af(text, contig, needle, pos)
    assert exp["declined_at"] is None
    out = Out(len(exp["pos"]), len(exp["defer_off"]), True)
    rc, c = ctx.vcf_af_parse_into(text, contig, needle, pos, out.view)
    _assert_equal(rc, c, out, exp)
    return exp


def good(p, qual="50", dp="40", ad="10,30", chrom="chr1"):
    return (inp.GOOD % (p, qual, dp, ad)).replace("chr1", chrom, 1).encode()


@pytest.fixture(scope="module")
def generated():
    text, snps, rng = inp.generated_snp_text()
    g = {c: inp.generated_gnomad_text(rng, snps, c)[0] for c in ("chr1", "chr2")}
    pos = {c: np.sort(np.array([q for q, l in snps if l.startswith(c + "\t")], np.uint32)) for c in ("chr1", "chr2")}
    return text, g, pos


# ---- line structure ---------------------------------------------------------------------------------------------------------------------
def test_tiny_texts(ctx):
    """texts of 0, 1, 15, 16 and 17 bytes; one line without its line end; only empty lines; \\r\\n"""
    line = good(7)
    for n in (0, 1, 15, 16, 17):
        for fill in (b"\n", b"x", b"\t"):
            exp = _snp(ctx, fill * n)
            assert exp["n_lines"] == (0 if fill == b"\n" or n == 0 else 1)
    exp = _snp(ctx, line)
    assert exp["pos"].tolist() == [7] and exp["value"].tolist() == [0.75] and exp["chrom_len"].tolist() == [4]
    assert _snp(ctx, b"\n" * 5000 + b"\r\n" * 300 + b"\r")["n_lines"] == 0
    exp = _snp(ctx, b"\r\n".join(good(p) for p in range(1, 400)) + b"\r\n")
    assert len(exp["pos"]) == 399
    exp = _snp(ctx, b"\r\n\r\n" + line + b"\r")
    assert exp["pos"].tolist() == [7] and exp["line_off"].tolist() == [4]


def test_line_ends_around_the_tile_edge(ctx):
    """a '\\n' at every offset in [T - 17, T + 17], behind a first line that fills the tile up to it; then all of them at once"""
    for at in range(T - 17, T + 18):
        first = good(1)
        first = first + b"," + b"7" * (at - len(first) - 1)           # (trailing bytes in the sample column: AD's third value)
        exp = _snp(ctx, first + b"\n" + good(2) + b"\n" + good(3))
        assert exp["line_off"].tolist() == [0, at + 1, at + 2 + len(good(2))], at
    body = bytearray(good(1) + b"," + b"7" * (T - 100))
    exp = _snp(ctx, bytes(body) + b"\n" * 60 + good(5) + b"\n")
    assert exp["pos"].tolist() == [1, 5]


def test_long_lines(ctx):
    """a line that starts in one tile and ends three tiles later; a line of 70 000 bytes, kept, skipped and deferred by its last bytes"""
    pad = good(1) + b"\n"
    lead = b"".join(good(p) + b"\n" for p in range(10, 60))             # ~2.7 KB: the next line starts inside tile 0
    assert len(lead) < T
    long_kept = good(99) + b"," + b"1" * (3 * T)
    exp = _snp(ctx, lead + long_kept + b"\n" + good(100) + b"\n")
    assert exp["pos"].tolist()[-2:] == [99, 100] and len(exp["pos"]) == 52
    base = b"chr1\t5\t.\tA\tG\t50\tPASS\t" + b"X" * 70_000 + b"\tGT:DP:AD\t0/1:40:"
    for tail, kind in ((b"10,30", "keep"), (b"10", "skip"), (b"10,3x", "defer")):
        exp = _snp(ctx, pad + base + tail + b"\n" + good(6) + b"\n")
        assert inp.snp_rule(base + tail)[0] == kind
        assert exp["pos"].tolist() == ([1, 5, 6] if kind == "keep" else [1, 6]) and len(exp["defer_off"]) == (kind == "defer")
    # the population form: the key behind 70 000 bytes of INFO, and a tab ending INFO in front of it
    info = b";".join(b"K%d=%d" % (k, k) for k in range(9000))
    assert len(info) > 70_000
    g = b"chr1\t5\trs\tA\tG\t.\tPASS\t" + info
    exp = _af(ctx, g + b";AF_nfe=0.25\n" + g + b"\tAF_nfe=0.5\n" + g + b";AF_nfe=0.5;\tx\n", "chr1", "AF_nfe=", [5])
    assert exp["value"].tolist() == [0.25, 0.5]


def test_group_widths_agree(ctx, generated):
    """the group of lanes per line follows the mean line length (8 up to 256 bytes, 16 up to 1024, 64 beyond): one text, made longer on
    average by a single long line that is skipped, gives one result at every width"""
    text, g, pos = generated
    text = text[:text.index(b"\n", 30_000) + 1]
    n = text.count(b"\n")
    base = _snp(ctx, text)
    assert len(text) // (n + 1) <= 256
    for mean in (600, 3000):
        junk = b"chr9\t" + b"j" * (mean * (n + 2))
        exp = _snp(ctx, text + junk + b"\n")
        assert 256 < (len(text) + len(junk) + 1) // (n + 2) and ((len(text) + len(junk) + 1) // (n + 2) <= 1024) == (mean == 600)
        for k in ("line_off", "chrom_len", "pos", "defer_off"):
            assert np.array_equal(exp[k], base[k])
    gt = g["chr1"][:g["chr1"].index(b"\n", 30_000) + 1]
    m = gt.count(b"\n")
    base = _af(ctx, gt, "chr1", "AF_nfe=", [4_000_000])                  # every position misses, nothing stops: all lines are walked
    hits = _af(ctx, gt, "chr1", "AF_nfe=", np.append(pos["chr1"], 4_000_000))
    assert len(base["pos"]) == 0 and len(hits["pos"]) > 30
    for mean in (600, 3000):
        junk = b"chr1\t4000000\trs\tA\tG\t.\tPASS\t" + b"j" * (mean * (m + 2))      # its whole INFO is searched for the key
        exp = _af(ctx, gt + junk + b"\n", "chr1", "AF_nfe=", np.append(pos["chr1"], 4_000_000))
        for k in ("line_off", "pos", "defer_off"):
            assert np.array_equal(exp[k], hits[k])


def test_more_lines_than_the_grid(ctx):
    """300 000 two-byte lines plus 2 000 real ones: the per-line kernel strides over the lines"""
    rng = np.random.default_rng(2)
    real = [good(int(p), ad="%d,%d" % (p % 37, p % 11 + 1)) + b"\n" for p in rng.integers(1, 1 << 29, 2000)]
    parts = []
    for j in range(2000):
        parts.append(b"x\n" * 150)
        parts.append(real[j])
    text = b"".join(parts)
    exp = _snp(ctx, text)
    assert exp["n_lines"] == 302_000 and len(exp["pos"]) == 2000


# ---- the records ------------------------------------------------------------------------------------------------------------------------
def test_every_record_kind(ctx, generated):
    """every record kind of snp_lines and gnomad_lines; the header's types; both keys, a key that is absent, a contig that is a prefix"""
    text, g, pos = generated
    exp = _snp(ctx, text)
    assert len(exp["pos"]) > 700 and len(exp["defer_off"]) == 0 and np.isnan(exp["value"]).any()
    assert len(_snp(ctx, text, dp_int=False)["pos"]) == 0 and len(_snp(ctx, text, ad_int=False)["pos"]) == 0
    for c in ("chr1", "chr2"):
        for needle in ("AF_nfe=", "AF=", "AF_zzz=", "AF_int="):
            exp = _af(ctx, g[c], c, needle, pos[c])
            assert (len(exp["pos"]) > 50) == (needle in ("AF_nfe=", "AF="))
            assert c == "chr1" or exp["stop_off"] != inp.NO_STOP         # (chr2's SNPs end at 300 000, its population file goes on)
        assert len(_af(ctx, g[c], "chr", "AF=", pos[c])["pos"]) == 0


def test_deliberate_deferrals(ctx, generated):
    text, g, pos = generated
    head = text[:text.index(b"\n", 6000) + 1]
    lines = [l for _, l in inp.DELIBERATE_SNP] + inp.NOT_DEFERRED_SNP + [inp.DEFERRED_BY_ORDER]
    full = head + ("\n".join(lines) + "\n").encode() + text[len(head):text.index(b"\n", 12_000) + 1]
    exp = _snp(ctx, full)
    assert exp["defer_off"].tolist() == sorted(full.index(l.encode()) for l in [l for _, l in inp.DELIBERATE_SNP] + [inp.DEFERRED_BY_ORDER])
    gl = [inp.GN % ("900", "AF_nfe=0.25")] + [l for _, l in inp.DELIBERATE_AF] + [inp.GN % ("1500", "AF_nfe=0.75")]
    gt = ("\n".join(gl) + "\n").encode()
    exp = _af(ctx, gt, "chr1", "AF_nfe=", [900] + inp.DELIBERATE_AF_POS + [1500])
    assert exp["defer_off"].tolist() == [gt.index(l.encode()) for _, l in inp.DELIBERATE_AF] and exp["pos"].tolist() == [900, 1500]


def test_value_table(ctx):
    """2 200 QUAL / AF tokens inside the conversion rule against float(np.float32(float(tok))): the fp64 multiply / divide and the
    double -> float conversion round on the device as libc's strtod and the host's cast do"""
    toks = inp.value_tokens()
    assert len(toks) >= 2000
    want = np.array([float(np.float32(float(t))) for t in toks])
    # AF form: the value itself comes back (those outside (0.01, 0.99) are skipped)
    gt = b"".join((inp.GN % (str(k + 1), "AC=1;AF=%s;X=1" % t)).encode() + b"\n" for k, t in enumerate(toks))
    exp = _af(ctx, gt, "chr1", "AF=", np.arange(1, len(toks) + 1))
    inside = ~((want <= 0.01) | (want >= 0.99))
    assert len(exp["defer_off"]) == 0 and inside.sum() > 300
    assert np.array_equal(exp["pos"], np.flatnonzero(inside) + 1) and np.array_equal(exp["value"].view(np.uint64), want[inside].view(np.uint64))
    # SNP form: QUAL decides through (float)qual > 30
    st = b"".join(good(k + 1, qual=t) + b"\n" for k, t in enumerate(toks))
    exp = _snp(ctx, st)
    assert len(exp["defer_off"]) == 0 and np.array_equal(exp["pos"], np.flatnonzero(want > 30) + 1) and (want > 30).sum() > 100
    # the BAF division, wrap-around and missing values included
    ads = ["0,0", "1,3", "7,.", ".,7", ".,.", "999999999,999999999", "-5,3", "3,-5", "+3,+4", "0,1", "1,0", "123456789,987654321"]
    rng = np.random.default_rng(4)
    ads += ["%d,%d" % (a, b) for a, b in rng.integers(0, 200, (300, 2))]
    exp = _snp(ctx, b"".join(good(k + 1, ad=a) + b"\n" for k, a in enumerate(ads)))
    assert len(exp["pos"]) == len(ads)


# ---- the population form ------------------------------------------------------------------------------------------------------------------
def test_stop_lines(ctx):
    """STOP in the first, a middle and the last line, and none; behind a deferred line; a later STOP line does not matter; other contigs and
    unreadable positions do not stop"""
    def g(p, chrom="chr1", af="0.5"):
        return (inp.GN % (p, "AF=%s" % af)).replace("chr1", chrom, 1).encode() + b"\n"
    lines = [g(str(p)) for p in range(1, 41)]
    for last in (0, 20, 39, 40):
        exp = _af(ctx, b"".join(lines), "chr1", "AF=", list(range(1, last + 1)))
        assert len(exp["pos"]) == last and (exp["stop_off"] == inp.NO_STOP) == (last == 40)
    text = g("1") + g("2x") + g("3") + g("50") + g("4") + g("60")
    exp = _af(ctx, text, "chr1", "AF=", [1, 2, 3, 4])
    assert exp["pos"].tolist() == [1, 3] and exp["defer_off"].tolist() == [len(g("1"))] and exp["stop_off"] == text.index(g("50"))
    text = g("1") + g("99", "chr10") + g("9999999999") + g("2") + g("99") + g("3x")
    exp = _af(ctx, text, "chr1", "AF=", [1, 2, 3])
    assert exp["pos"].tolist() == [1, 2] and len(exp["defer_off"]) == 1 and exp["n_lines"] == 4


def test_contigs_needles_and_positions(ctx):
    def g(p, info, chrom="chr1"):
        return (inp.GN % (p, info)).replace("chr1", chrom, 1).encode() + b"\n"
    text = (g("5", "AF_nfe=0.25") + g("5", "AF_nfe=0.3", "chr10") + g("5", "AF_nfe=0.35", "chr") + g("6", "XAF_nfe=0.5;AF_nfe=0.125") +
            g("6", "XAF_nfe=0.5;AC=1") + g("7", "AF_nfe=;AC=1") + g("7", "AC=1;AF_nfe=") + g("7", "AC=1;AF_nfe=.,0.5;Z") + g("8", "AF_nfe=0.5,0.6") +
            g("8", "AF_nfe") + g("8", "AC=AF_nfe=0.5") + g("8", "AC=1;AF_nfe=0.75\tAF_nfe=0.5") + g("9", "AF_nfe=0.5"))
    for contig, n in (("chr1", 5), ("chr10", 1), ("chr", 1), ("chr2", 0), ("", 0)):
        assert len(_af(ctx, text, contig, "AF_nfe=", [5, 6, 7, 8])["pos"]) == n, contig
    exp = _af(ctx, text, "chr1", "AF_nfe=", [5, 6, 7, 8])
    assert exp["pos"].tolist() == [5, 6, 7, 8, 8] and exp["stop_off"] == text.rindex(b"chr1\t9")
    assert np.isnan(exp["value"][exp["pos"] == 7]).all() and exp["value"][exp["pos"] == 6].tolist() == [0.125]
    # sorted_pos of 0 and 1 entries, and with duplicates
    assert len(_af(ctx, text, "chr1", "AF_nfe=", [])["pos"]) == 0 and _af(ctx, text, "chr1", "AF_nfe=", [])["stop_off"] == 0
    assert _af(ctx, text, "chr1", "AF_nfe=", [6])["pos"].tolist() == [6]
    assert _af(ctx, text, "chr1", "AF_nfe=", [5, 5, 5, 8, 8, 9, 9])["pos"].tolist() == [5, 8, 8, 9]
    # needles of 1 and 64 bytes
    long_key = "K" * 63 + "="
    assert _af(ctx, g("5", "A=1;%s0.5" % long_key) + g("5", "%s0.25;B" % long_key[1:]), "chr1", long_key, [5])["value"].tolist() == [0.5]
    assert _af(ctx, g("5", "==0.5") + g("5", "A;=0.25"), "chr1", "=", [5])["value"].tolist() == [0.25]


# ---- the call ---------------------------------------------------------------------------------------------------------------------------
def test_header_line_behind_data_declines(ctx):
    text = good(1) + b"\n" + good(2) + b"\n##FORMAT=<ID=DP,Number=1,Type=String>\n" + good(3) + b"\n"
    out = Out(8, 8, False)
    rc, c = ctx.vcf_snp_parse_into(text, out.view)
    assert rc == 1 and c["reason"] == _lib.VCF_HEADER_LINE and c["offset"] == text.index(b"##") == inp.expected_snp(text)["declined_at"]
    r = ctx.vcf_snp_parse(text)
    assert r["declined"] and "pos" not in r
    # behind the STOP line a '#' line is never reached
    g = (inp.GN % ("1", "AF=0.5") + "\n" + inp.GN % ("9", "AF=0.5") + "\n#late\n").encode()
    assert _af(ctx, g, "chr1", "AF=", [1])["pos"].tolist() == [1]
    out = Out(8, 8, True)
    rc, c = ctx.vcf_af_parse_into(g, "chr1", "AF=", np.array([1, 9], np.uint32), out.view)
    assert rc == 1 and c["offset"] == g.index(b"#late")


def test_capacity_then_success(ctx, generated):
    text, g, pos = generated
    text = text[:text.index(b"\n", 20_000) + 1] + ("\n".join(l for _, l in inp.DELIBERATE_SNP) + "\n").encode()
    exp = inp.expected_snp(text)
    n, d = len(exp["pos"]), len(exp["defer_off"])
    for dn, dd in ((-1, 0), (0, -1), (-n, -d)):
        out = Out(n + dn, d + dd, False, slack=0)
        rc, c = ctx.vcf_snp_parse_into(text, out.view)
        assert rc == _lib.CSV_ECAPACITY and (c["n_kept"], c["n_deferred"], c["n_lines"]) == (n, d, exp["n_lines"])
        c["n_kept"] = c["n_deferred"] = 0
        assert out.intact_outside(c) is None, "CSV_ECAPACITY writes nothing"
    out = Out(n, d, False, slack=0)
    rc, c = ctx.vcf_snp_parse_into(text, out.view)
    _assert_equal(rc, c, out, exp)
    r = ctx.vcf_snp_parse(text)
    assert np.array_equal(r["pos"], exp["pos"]) and np.array_equal(r["defer_off"], exp["defer_off"])


def test_arguments(ctx):
    """every CSV_EINVAL of the entry points, and len == 0"""
    import ctypes as C
    lib, h = ctx.lib, ctx.h
    text = np.frombuffer(good(1) + b"\n", np.uint8)
    a = {k: np.zeros(4, DTYPES[k]) for k in DTYPES}
    spos = np.array([1, 2], np.uint32)

    def out(**kw):
        o = _lib.csv_vcf_out()
        for k in DTYPES:
            setattr(o, k, kw.get(k, a[k].ctypes.data))
        o.cap, o.cap_defer = 4, 4
        return o
    c = _lib.csv_vcf_counts()
    for fn in (lib.csvgpu_vcf_snp_parse, lib.csvgpu_vcf_snp_parse_dev):
        assert fn(None, text.ctypes.data, len(text), 1, 1, C.byref(out()), C.byref(c)) == _lib.CSV_EINVAL
        assert fn(h, None, len(text), 1, 1, C.byref(out()), C.byref(c)) == _lib.CSV_EINVAL
        assert fn(h, text.ctypes.data, len(text), 1, 1, None, C.byref(c)) == _lib.CSV_EINVAL
        assert fn(h, text.ctypes.data, len(text), 1, 1, C.byref(out()), None) == _lib.CSV_EINVAL
        assert fn(h, text.ctypes.data, 1 << 32, 1, 1, C.byref(out()), C.byref(c)) == _lib.CSV_EINVAL
        for k in DTYPES:
            assert fn(h, text.ctypes.data, len(text), 1, 1, C.byref(out(**{k: None})), C.byref(c)) == _lib.CSV_EINVAL, k
        c.n_lines = 9
        assert fn(h, None, 0, 1, 1, C.byref(out()), C.byref(c)) == 0 and (c.n_lines, c.n_kept, c.n_deferred, c.status) == (0, 0, 0, 0)
    for fn in (lib.csvgpu_vcf_af_parse, lib.csvgpu_vcf_af_parse_dev):
        def call(text_p=text.ctypes.data, n_text=len(text), contig=b"chr1", needle=b"AF=", needle_len=3, pos=spos.ctypes.data, n=2, o=None, cc=c):
            return fn(h, text_p, n_text, contig, len(contig or b""), needle, needle_len, pos, n, C.byref(o or out(chrom_len=None)), C.byref(cc) if cc is not None else None)
        assert call(text_p=None) == _lib.CSV_EINVAL and call(n_text=1 << 32) == _lib.CSV_EINVAL
        assert call(needle=None) == _lib.CSV_EINVAL and call(needle_len=0) == _lib.CSV_EINVAL and call(needle=b"K" * 65, needle_len=65) == _lib.CSV_EINVAL
        assert call(needle=b"A\t=") == _lib.CSV_EINVAL and call(pos=None) == _lib.CSV_EINVAL and call(cc=None) == _lib.CSV_EINVAL
        assert call(o=out(pos=None)) == _lib.CSV_EINVAL
        assert call(text_p=None, n_text=0) == 0
    down = np.array([2, 1], np.uint32)
    assert lib.csvgpu_vcf_af_parse(h, text.ctypes.data, len(text), b"chr1", 4, b"AF=", 3, down.ctypes.data, 2, C.byref(out()), C.byref(c)) == _lib.CSV_EINVAL
    assert b"ascending" in lib.csvgpu_last_error(h)
    assert lib.csvgpu_vcf_af_parse(h, text.ctypes.data, len(text), b"chr1", 4, b"AF=", 3, spos.ctypes.data, 2, C.byref(out()), C.byref(c)) == 0


def test_workspace_growth_on_fresh_contexts(generated):
    """the per-line workspace is carved behind the line-end counts once those are known: on a context's first call, and whenever a text
    has more lines than any before it, the arena grows between the two carves and the first pass's results must be made again — both
    forms, growing and shrinking texts, on contexts of their own"""
    import contextsv_amd as cs
    text, g, pos = generated
    tiny = b"x\n" * 40_000                                    # many lines in few tiles: the second carve dwarfs the first
    with cs.Context(0) as fresh:
        _af(fresh, g["chr1"], "chr1", "AF_nfe=", pos["chr1"])            # the very first call needs the strings and the head after the growth
        _snp(fresh, tiny + good(5) + b"\n")
        _snp(fresh, text)
        _af(fresh, g["chr2"] * 3, "chr2", "AF=", pos["chr2"])
        _snp(fresh, tiny * 5 + text)
        _snp(fresh, good(5) + b"\n")
    with cs.Context(0) as fresh:
        _snp(fresh, tiny * 3 + text[:5000])
        _af(fresh, g["chr1"], "chr1", "AF=", pos["chr1"])


def test_timed_under_misc(ctx, generated):
    text = generated[0]
    ctx.timing_reset()
    ctx.timing_enable(1)
    try:
        ctx.vcf_snp_parse(text)
        t = ctx.timing()
    finally:
        ctx.timing_enable(0)
    assert t["misc"][1] >= 1 and t["misc"][0] > 0


def test_device_tensors_and_the_inflate_seam():
    """the _dev forms with the text pointer shifted by 1 to 15 bytes, and csvgpu_bgzf_inflate_dev -> csvgpu_vcf_snp_parse_dev equal to the
    host-pointer call. In a process of its own, torch first (tests/vcf_parse_dev_check.py)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "vcf_parse_dev_check.py")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0 and "vcf_parse_dev ok: 15 shifts x 2 forms" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
