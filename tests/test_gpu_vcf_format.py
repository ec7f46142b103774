"""csvgpu_vcf_format / _dev (kernels/vcfformat.hip, api/vcf_format.hip; rules in csrc/vcf_format_core.hpp): the VCF writer's record lines
assembled on the device from a genome built by Context.genome_builder() and the depth maps of resident shards, against the Python model
(tests/vcf_format_model.py, itself held against the host writer and the oracle in tests/test_vcf_format_model.py) — text byte for byte,
status bytes and counts — and, through host.save_vcf, against the host writer and the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

from contextsv_amd import _lib, host
from contextsv_amd.context import ptr
import synth_small as ss
import vcf_format_inputs as vi
import vcf_format_model as vm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = (1 << 20) + 64
NAMES = [b"abcdefghijklmnop"[:k] for k in range(1, 17)]           # contig names of length 1..16: REF begins at every residue mod 16 of the text


class World:
    """A resident genome, its FASTA file, and three resident depth maps with their host copies."""

    def __init__(self, ctx, tmp):
        rng = np.random.default_rng(77)
        self.ctx = ctx
        pairs = [(n, vi.random_seq(rng, 640 + 7 * len(n))) for n in NAMES]
        pairs += [(b"dup", vi.random_seq(rng, 500)), (b"big", vi.random_seq(rng, BIG)), (b"dup", vi.random_seq(rng, 700))]
        self.seqs = dict(pairs)                                     # (the last record of a duplicated name wins)
        self.path = str(tmp / "genome.fa")
        vi.write_fasta(self.path, pairs, width=61)
        text = open(self.path, "rb").read()
        b = ctx.genome_builder(len(text))
        cut = len(text) // 3 + 5
        b.append(text[:cut]); b.append(text[cut:])
        self.genome = b.finish()
        assert self.genome.describe()["names"] == [n for n, _ in pairs]
        self.shards, self.depths = [], []
        for seed, chr_len in ((3, 8000), (4, 9000), (5, BIG + 8)):
            reads, depth_len = ss.random_shard(seed, n_reads=1200, mean_ops=30, chr_len=chr_len)
            sh = ctx.upload(reads, depth_len)
            res = sh.pipeline()
            self.shards.append(sh)
            self.depths.append((sh.fetch(res, want_depth=True)["depth"], res.raw.depth))
        assert self.depths[0][0].max() > 9

    def set_depth(self, k, values):
        """Overwrite the first entries of resident depth map k (and of its host copy)."""
        values = np.ascontiguousarray(values, np.uint32)
        host_copy, dev = self.depths[k]
        host_copy[: len(values)] = values
        self.ctx._check(self.ctx.lib.csvgpu_upload(self.ctx.h, dev, ptr(values), values.nbytes))

    def contig(self, name, calls, alts, k=0, gaps=None, absent=False):
        c = vi.contig(name, None if absent else self.seqs[name], calls, alts, self.depths[k][0] if k is not None else None, gaps)
        c["shard"] = self.shards[k] if k is not None else None
        return c

    def args(self, contigs):
        tab = [(c["name"], len(c["calls"]), c["shard"], (([g[0] for g in c["gaps"]], [g[1] for g in c["gaps"]]) if c["gaps"] else None)) for c in contigs]
        calls = np.concatenate([c["calls"] for c in contigs]) if contigs else vi.blank_calls(0)
        return tab, calls, [a for c in contigs for a in c["alts"]]

    def check(self, contigs):
        """device == model -> (text, status, counts)"""
        want, want_status, want_counts = vm.model(contigs)
        text, status, counts = self.ctx.vcf_format(self.genome, *self.args(contigs))
        assert counts == want_counts
        if want is None:
            assert text is None
            return None, status, counts
        if text != want:
            k = next(i for i in range(min(len(text), len(want))) if text[i] != want[i]) if len(text) == len(want) else -1
            raise AssertionError("text differs at byte %d of %d / %d: %r vs %r" % (k, len(text), len(want), text[max(k - 60, 0): k + 20], want[max(k - 60, 0): k + 20]))
        assert np.array_equal(status, want_status)
        return text, status, counts

    def close(self):
        for sh in self.shards:
            sh.free()
        self.genome.free()


@pytest.fixture(scope="module")
def world(ctx, tmp_path_factory):
    w = World(ctx, tmp_path_factory.mktemp("vcffmt"))
    yield w
    w.close()


def generated(world, rng, n=120, gaps=False, names=NAMES[3:9:2]):
    contigs = []
    for k, name in enumerate(names):
        L = len(world.seqs[name])
        calls, alts = vi.random_calls(rng, n, L)
        calls["sv_type"][:3], calls["start"][:3], alts[:3] = 3, [0, 1, 2], [b"<INS>", b"ACG", b"T"]
        dl = len(world.depths[k % 2][0])                              # POS at the depth map's last entry and past it
        calls["sv_type"][3:6], calls["start"][3:6], calls["end"][3:6], alts[3:6] = 1, [dl - 1, dl, dl + 7], dl + 9, [b"<DUP>"] * 3
        g = [(int(a), int(a) + int(rng.integers(1, 200))) for a in rng.integers(0, L, 6)] if gaps else None
        contigs.append(world.contig(name, calls, alts, k % 2, g))
    return contigs


@pytest.mark.parametrize("with_gaps", [False, True])
def test_against_model_host_writer_and_oracle(world, oracle, tmp_path, with_gaps):
    contigs = generated(world, np.random.default_rng(5 + with_gaps), 300, with_gaps)
    contigs.append(world.contig(b"dup", *vi.random_calls(np.random.default_rng(9), 80, 700), 0))      # the LAST record of the name: 700 bases
    text, status, counts = world.check(contigs)
    assert counts["n_lines"] > 600 and (counts["gap_filtered"] > 0) == with_gaps and (status & vm.DEPTH_OUT_OF_RANGE).any() and (status & vm.EMPTY_REF).any()
    gap = None
    if with_gaps:
        gap = str(tmp_path / "gaps.bed")
        vi.write_gaps(gap, contigs)
    g = host.ReferenceGenome(world.path)
    (tmp_path / "h").mkdir()
    got = host.save_vcf(str(tmp_path / "h"), g, vi.items_of(contigs), gap_path=gap, file_date=vi.DATE)
    rc, want = oracle.save_vcf(str(tmp_path / "o.vcf"), world.path, vi.items_of(contigs), gap_path=gap, file_date=vi.DATE)
    assert rc == 0 and got == want == (counts["total"], counts["unclassified"], counts["gap_filtered"])
    assert vm.body_of((tmp_path / "h" / "output.vcf").read_bytes()) == text == vm.body_of((tmp_path / "o.vcf").read_bytes())


def test_empty_inputs(world):
    text, status, counts = world.check([])
    assert text == b"" and len(status) == 0 and counts == dict(text_bytes=0, n_lines=0, total=0, unclassified=0, gap_filtered=0, declined_why=0)
    none = vi.blank_calls(0)
    assert world.check([world.contig(b"a", none, [], None), world.contig(b"ab", none, [], 0)])[2]["text_bytes"] == 0
    skipped = vi.blank_calls(5)
    skipped["sv_type"], skipped["start"] = [-1, 5, 3, 3, -1], [10, 10, 0, 1, 3]
    alts = [b".", b".", b"<INS>", b"ACGT", b"."]
    text, status, counts = world.check([world.contig(b"abc", skipped, alts, None)])                   # no call asks for a depth: no shard is needed
    assert text == b"" and counts["total"] == 2 and counts["unclassified"] == 3 and list(status) == [1, 1, 2, 2, 1]
    calls, a = vi.random_calls(np.random.default_rng(1), 40, 600)
    text, _, counts = world.check([world.contig(b"abc", skipped, alts, None), world.contig(b"abcd", none, [], None), world.contig(b"abcde", calls, a, 1),
                                   world.contig(b"abcdef", skipped, alts, 0)])
    assert counts["n_lines"] > 20 and counts["unclassified"] > 6


@pytest.mark.parametrize("n_lines", [1, 2, 63, 64, 65, 257])
def test_line_counts(world, n_lines):
    calls = vi.blank_calls(n_lines + 2)
    calls["sv_type"] = np.arange(len(calls)) % 3                     # DEL DUP INV
    calls["sv_type"][[0, -1]] = -1                                   # a skipped call at either end
    calls["start"] = 3 + np.arange(len(calls)) * 2
    calls["end"] = calls["start"] + np.arange(len(calls)) % 37
    text, _, counts = world.check([world.contig(b"abcdefg", calls, [vi.default_alt(int(t)) for t in calls["sv_type"]], 0)])
    assert counts["n_lines"] == n_lines == text.count(b"\n")


def test_enums_masks_digits_and_likelihoods(world):
    name = b"abcdefghijk"
    L = len(world.seqs[name])
    edges = [e for e in vi.U32_EDGES if e < 2**31] + [2**31, 2**32 - 1]      # the last two read as outside the map
    world.set_depth(0, edges)
    c1, a1 = vi.enum_product(L)
    c2, a2 = vi.digit_edges(L)
    c3 = vi.blank_calls(len(edges))                                   # POS walks the depth map's first entries: SUPPORT / DP at every digit boundary
    c3["sv_type"], c3["start"], c3["end"] = 2, np.arange(len(c3)), 50
    c4 = vi.blank_calls(len(vi.U32_EDGES))                            # POS itself at every digit boundary
    c4["sv_type"], c4["start"], c4["end"] = 4, vi.U32_EDGES, vi.U32_EDGES[::-1]
    text, status, counts = world.check([world.contig(name, np.concatenate([c1, c2, c3, c4]), a1 + a2 + [b"<INV>"] * len(c3) + [b"<BND>"] * len(c4), 0)])
    for want in (b"HMM=0.007812;", b"HMM=0.023438;", b"HMM=1.000000;", b"HMM=-0.000000;", b"HMM=inf;", b"HMM=-inf;", b"HMM=nan;", b"HMM=-nan;", b"SUPPORT=9;", b"SUPPORT=10;",
                 b"SUPPORT=2147483647;", b"\t4294967295\t.\tN\t<BND>", b"CLUSTER=-2147483648;", b";CN=4;LOH\t", b"ALN=" + b",".join(vm.EVIDENCE) + b";"):
        assert want in text, want
    assert ((status & vm.DEPTH_OUT_OF_RANGE) != 0).sum() >= 2


def test_refused_values_decline_the_batch(world):
    name = b"abcdefghijkl"
    calls, alts = vi.random_calls(np.random.default_rng(2), 60, len(world.seqs[name]))
    calls["start"] = np.maximum(calls["start"], 2)
    assert world.check([world.contig(name, calls, alts, 0)])[0] is not None
    for why, edit in ((vm.WHY_LIKELIHOOD, dict(sv_type=1, hmm_likelihood=2.0 ** 63)), (vm.WHY_LIKELIHOOD, dict(sv_type=2, hmm_likelihood=-1e300)),
                      (vm.WHY_DEL_LENGTH, dict(sv_type=0, start=10, end=10 + 2**31 - 1)), (vm.WHY_DEL_START, dict(sv_type=0, start=2**31, end=2**31 + 1)),
                      (vm.WHY_ENUM, dict(sv_type=7)), (vm.WHY_ENUM, dict(genotype=4, sv_type=-1)), (vm.WHY_ENUM, dict(cn_state=-1))):
        bad = calls.copy()
        for k, v in edit.items():
            bad[k][40] = v
        bad_alts = list(alts)
        bad_alts[40] = b"."
        text, _, counts = world.check([world.contig(name, bad, bad_alts, 0)])
        assert text is None and counts["declined_why"] == why
    two = calls.copy()                                               # two refused calls: the first one, by call order, names the reason
    two["sv_type"][[50, 20]], two["genotype"][50], two["hmm_likelihood"][20] = 1, 9, 1e19
    assert world.check([world.contig(name, two, alts, 0)])[2]["declined_why"] == vm.WHY_LIKELIHOOD


def test_alignment_of_ref_and_alt(world):
    """A DEL's REF of 1..200 bases (and an empty one) from every source residue mod 16, on contigs whose names have 1..16 bytes; one DEL of
    1 MiB between two 1-base ones; INS ALTs of 0, 1, 15, 16, 17 and 60 bytes and <INS>."""
    contigs = []
    for k, name in enumerate(NAMES):
        L = len(world.seqs[name])
        r = np.arange(1, 201)
        calls = vi.blank_calls(len(r) + 1)
        calls["sv_type"] = 0
        calls["start"][:-1] = 2 + (k + r * 5) % 16 + r % 3 * 16      # POS = start - 1: every residue
        calls["end"][:-1] = calls["start"][:-1] - 2 + r              # REF = [start - 1, end]: r bases
        calls["start"][-1], calls["end"][-1] = L - 3, L + 1          # past the contig's end: empty
        calls["hmm_likelihood"] = -r[0] / 7.0
        contigs.append(world.contig(name, calls, [b"<DEL>"] * len(calls), k % 2))
    big = vi.blank_calls(3)
    big["sv_type"], big["start"], big["end"] = 0, [40, 9, BIG - 1], [39, BIG, BIG - 2]      # 1 base, the whole contig from base 8, 1 base
    contigs.insert(5, world.contig(b"big", big, [b"<DEL>"] * 3, 2))
    ins = vi.blank_calls(7)
    ins["sv_type"], ins["start"], ins["end"] = 3, 20 + np.arange(7) * 3, 25 + np.arange(7) * 3
    contigs.append(world.contig(b"dup", ins, [b"", b"A", b"ACGTACGTACGTACG", b"ACGTACGTACGTACGT", b"ACGTACGTACGTACGTA", b"ACGT" * 15, b"<INS>"], 0))
    text, status, counts = world.check(contigs)
    assert counts["text_bytes"] > BIG and ((status & vm.EMPTY_REF) != 0).sum() == 16
    lines = text.split(b"\n")
    assert max(len(l) for l in lines) > BIG and lines[-2].split(b"\t")[4] == b"<INS>"


def test_cuts_at_the_edges(world):
    name = b"abcdefghijklmn"
    s, depth = world.seqs[name], world.depths[1][0]
    kept, refused = [], []
    for calls, alts in vi.directed_positions(len(s), len(depth)):
        (refused if vm.decide(calls[0], alts[0], s, [], depth)[0] else kept).append((calls, alts))
    assert len(kept) > 400 and len(refused) > 10
    text, status, _ = world.check([world.contig(name, np.concatenate([c for c, _ in kept]), [a[0] for _, a in kept], 1)])
    assert (status & vm.DISPOSITION == vm.SKIP_FIRST_POSITION).sum() >= 10 and ((status & vm.EMPTY_REF) != 0).sum() > 10
    some = refused[:: max(len(refused) // 6, 1)]                     # (each refused call declines a batch of its own)
    for calls, alts in some:
        assert world.check([world.contig(name, np.concatenate([kept[0][0], calls]), kept[0][1] + alts, 1)])[0] is None


def test_gap_rows(world):
    name = b"abcdefghi"
    gaps = [(99, 119), (150, 150), (400, 500), (104, 110), (2**32 - 2, 2**32 - 1), (2**32 - 1, 5)]
    rows = [(100, 199), (101, 200), (121, 220), (120, 219), (151, 151), (152, 160), (390, 510), (1, 1), (0, 0), (5, 4), (500, 100), (2**32 - 1, 2**32 - 1)]
    calls = vi.blank_calls(3 * len(rows))
    for k, t in enumerate((0, 1, 3)):
        for i, (a, b) in enumerate(rows):
            c = calls[k * len(rows) + i]
            c["sv_type"], c["start"], c["end"] = t, a, b
    calls = calls[[i for i in range(len(calls)) if not vm.decide(calls[i], b"<INS>", world.seqs[name], gaps, world.depths[0][0])[0]]]
    alts = [vi.default_alt(int(t)) for t in calls["sv_type"]]
    _, status, counts = world.check([world.contig(b"abcd", calls, alts, 0, [(0, 2**31)]), world.contig(name, calls, alts, 0, gaps), world.contig(b"abcdefgh", calls, alts, 0)])
    n = len(calls)
    assert (status[n: 2 * n][0] & vm.GAP_FILTERED) and not (status[n: 2 * n][1] & vm.GAP_FILTERED) and not (status[2 * n:] & vm.GAP_FILTERED).any()
    assert counts["gap_filtered"] >= 10
    thousand = [(600 + i, 600 + i) for i in range(999)] + [(99, 119)]
    assert world.check([world.contig(name, calls, alts, 0, thousand)])[2]["gap_filtered"] > 0
    assert world.check([world.contig(name, calls, alts, 0)])[2]["gap_filtered"] == 0


def test_records_and_absent_contigs(world):
    calls, alts = vi.random_calls(np.random.default_rng(6), 50, 500)
    calls["start"] = np.maximum(calls["start"], 2)
    calls["end"][0], calls["sv_type"][0], alts[0] = 690, 0, b"<DEL>"           # inside the last "dup" record (700 bases), past the first (500)
    text, status, _ = world.check([world.contig(b"dup", calls, alts, 0)])
    assert not status[0] & vm.EMPTY_REF
    absent = calls.copy()
    absent["sv_type"] = np.where(np.isin(absent["sv_type"], (0, 3)), 1, absent["sv_type"])
    absent_alts = [vi.default_alt(int(t)) for t in absent["sv_type"]]
    assert world.check([world.contig(b"nowhere", absent, absent_alts, 0, absent=True)])[0] is not None
    absent["sv_type"][7] = 0
    assert world.check([world.contig(b"nowhere", absent, absent_alts, 0, absent=True)])[2]["declined_why"] == vm.WHY_NO_RECORD
    # what the host can see is CSV_EINVAL, nothing launched
    tab, c, a = world.args([world.contig(b"dup", calls, alts, 0)])
    for bad_tab in ([(b"dup", len(calls), world.shards[0], None, 99)], [(b"dup", len(calls), None, None)]):
        rc, _, _ = world.ctx.vcf_format_raw(world.genome, bad_tab, c, a, vm.METHOD, 0, None)
        assert rc == _lib.CSV_EINVAL
    assert world.ctx.vcf_format_raw(world.genome, tab, c, a, b"x" * 65, 0, None)[0] == _lib.CSV_EINVAL
    assert world.check([world.contig(b"dup", calls, alts, 0)])[0] == text


def test_more_calls_than_one_pass_of_the_capped_grids(world):
    """70 000 calls on one contig: the per-call grid (256 workgroups of 256) and the per-piece grid (4 MiB of text a pass) both stride."""
    n = 70_000
    rng = np.random.default_rng(12)
    L = len(world.seqs[b"abcdefghijklmnop"])
    calls = vi.blank_calls(n)
    calls["sv_type"] = rng.choice([-1, 0, 1, 2, 3], n)
    calls["start"] = rng.integers(2, L, n)
    calls["end"] = calls["start"] + rng.integers(0, 40, n)
    calls["hmm_likelihood"] = -rng.random(n) * 1000
    calls["aln_flags"], calls["genotype"], calls["cn_state"] = rng.integers(0, 1024, n), rng.integers(0, 4, n), rng.integers(0, 7, n)
    alts = [vi.default_alt(int(t)) for t in calls["sv_type"]]
    text, _, counts = world.check([world.contig(b"abcdefghijklmnop", calls, alts, 0, [(100, 130)])])
    assert counts["n_lines"] > 50_000 and counts["text_bytes"] > (4 << 20)


def test_capacity_and_guards(world):
    contigs = generated(world, np.random.default_rng(15), 50)
    want, _, want_counts = vm.model(contigs)
    tab, calls, alts = world.args(contigs)
    n = len(want)
    buf = np.full(n + 64, 0xA5, np.uint8)
    rc, _, counts = world.ctx.vcf_format_raw(world.genome, tab, calls, alts, vm.METHOD, n - 1, buf.ctypes.data + 32)
    assert rc == _lib.CSV_ECAPACITY and counts == want_counts and (buf == 0xA5).all()
    rc, status, counts = world.ctx.vcf_format_raw(world.genome, tab, calls, alts, vm.METHOD, n, buf.ctypes.data + 32)
    assert rc == _lib.CSV_OK and counts == want_counts and buf[32: 32 + n].tobytes() == want and (buf[:32] == 0xA5).all() and (buf[32 + n:] == 0xA5).all()


@pytest.mark.parametrize("shift", [0, 3])
def test_dev_form(world, shift):
    """csvgpu_vcf_format_dev into a device buffer (at a 16-byte boundary, and 3 bytes behind one) gives the same bytes after csvgpu_download."""
    ctx = world.ctx
    contigs = generated(world, np.random.default_rng(16), 60)
    big = vi.blank_calls(1)
    big["sv_type"], big["start"], big["end"] = 0, 100, 70_000
    contigs.append(world.contig(b"big", big, [b"<DEL>"], 2))
    want, _, want_counts = vm.model(contigs)
    tab, calls, alts = world.args(contigs)
    n = len(want)
    dev = ctx.lib.csvgpu_dev_alloc(ctx.h, n + 64)
    assert dev
    try:
        fill = np.full(n + 64, 0x5A, np.uint8)
        ctx._check(ctx.lib.csvgpu_upload(ctx.h, dev, ptr(fill), n + 64))
        rc, _, counts = ctx.vcf_format_raw(world.genome, tab, calls, alts, vm.METHOD, n, dev + 16 + shift, dev=True)
        assert rc == _lib.CSV_OK and counts == want_counts
        back = np.zeros(n + 64, np.uint8)
        ctx._check(ctx.lib.csvgpu_download(ctx.h, ptr(back), dev, n + 64))
        at = 16 + shift
        assert back[at: at + n].tobytes() == want and (back[:at] == 0x5A).all() and (back[at + n:] == 0x5A).all()
    finally:
        ctx.lib.csvgpu_dev_free(ctx.h, dev)


def test_allocation_failure_leaves_the_context_usable():
    """csvgpu_test_fail_next_alloc in front of the call's guarded reservation (libcsvgpu_testhooks.so, in a child process): CSV_ENOMEM, and
    the next call is correct."""
    env = dict(os.environ, CSVGPU_LIB=os.path.join(ROOT, "contextsv_amd", "lib", "libcsvgpu_testhooks.so"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "vcf_format_alloc_check.py")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "vcf_format_alloc_check: ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
