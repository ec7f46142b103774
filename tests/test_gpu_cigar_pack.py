"""Resident long-read shards keep their CIGAR ops in 16 bits (4 of op, 12 of length; csrc/cigar_pack_core.hpp, kernels/cigarpack.hip): an op
of length >= 4095 is an ESCAPE whose full word sits in a side table with a per-512-op-piece index, and the wave forms of the scan and of the
depth walk read that form. Every case here runs one resident shard through pipeline + fetch twice — packing on, packing off
(csvgpu_set_cigar_packing) — each against the oracle (signatures, ref_end / q_start / q_end, depth map, sum, non-zero count) and the two
runs against each other bit for bit. The escapes sit where the kernels change path: a read's first and last op, the 256-op chunk and 512-op
piece edges of the array, the 64-op checkpoint grid of a read, a chunk shared by two reads, several in one lane's four ops, long runs, the
shard's last partial piece, deletions across depth tile edges. csvgpu_shard_cigar_bytes tells which form a shard took."""
import ctypes as C

import numpy as np
import pytest

import contextsv_amd as cs
from contextsv_amd import Reads, _lib, host, make_hmm

pytestmark = pytest.mark.gpu

M, I, D, N, S, H, P, EQ, X = range(9)
PAD = 512                  # CIGAR_PAD_WORDS
ESC = 4095                 # the first length that does not fit 12 bits
BIG = (1 << 28) - 1        # the longest length a CIGAR word holds
DEPTH_LEN = 400_000
TILE = 1 << 14             # positions per depth tile


@pytest.fixture
def wave(ctx):
    """Small shards would take a short-read form by their mean ops per read; only the wave form packs."""
    ctx.set_tuning(scan_form=0)
    ctx.set_cigar_packing(True)
    yield ctx
    ctx.set_cigar_packing(True)
    ctx.set_tuning()


def _n_esc(reads):
    return int(np.count_nonzero((reads.cigar >> 4) >= ESC))


def _bytes(reads, packed):
    m = int(reads.n_cigar)
    if not packed:
        return 4 * (m + PAD)
    pieces = (m + 511) // 512
    return 2 * (pieces * 512 + PAD) + 4 * (pieces + 1) + 8 * (_n_esc(reads) + 1)


def _packs(reads):
    m = int(reads.n_cigar)
    return m > 0 and _n_esc(reads) * 64 <= m


def _run(ctx, reads, depth_len, on, min_oplen=50, min_mapq=20):
    ctx.set_cigar_packing(on)
    try:
        sh = ctx.upload(reads, depth_len)
    finally:
        ctx.set_cigar_packing(True)
    try:
        nbytes = sh.cigar_bytes()
        res = sh.pipeline(eps=0.1, min_pts_pct=0.1, min_oplen=min_oplen, min_mapq=min_mapq)
        out = sh.fetch(res, want_depth=True)
        back = sh.fetch_reads()
    finally:
        sh.free()
    return dict(bytes=nbytes, res=res, out=out, back=back)


def _check(ctx, oracle, reads, depth_len=DEPTH_LEN, packed=None, min_oplen=50, min_mapq=20):
    """Packing on and off, each against the oracle and against each other; `packed`: the form the packing-on shard must take (None: by rule)."""
    sig = oracle.cigar_scan(reads, depth_len, min_oplen, min_mapq)
    iv = oracle.aln_intervals(reads)
    od, osum, onz = oracle.depth(reads, depth_len)
    kind = sig["qpos_kind"] & 3
    runs = {on: _run(ctx, reads, depth_len, on, min_oplen, min_mapq) for on in (True, False)}
    want = _packs(reads) if packed is None else packed
    assert runs[True]["bytes"] == _bytes(reads, want), (runs[True]["bytes"], _bytes(reads, True), _bytes(reads, False))
    assert runs[False]["bytes"] == _bytes(reads, False)
    for on, r in runs.items():
        out, res = r["out"], r["res"]
        for g, e in ((out["sig_del"], sig[kind == 1]), (out["sig_ins"], sig[kind != 1])):
            assert len(g) == len(e), on
            for f in ("start", "end", "read", "qpos_kind"):
                assert np.array_equal(g[f], e[f]), (on, f)
        for name, o in zip(("ref_end", "q_start", "q_end"), iv):
            assert np.array_equal(out[name].view(np.uint32), np.asarray(o).view(np.uint32)), (on, name)
        assert np.array_equal(out["depth"], od) and (res.depth_sum, res.depth_nonzero) == (osum, onz), on
        # the fetch gives the uploaded 32-bit words back, escapes included
        assert np.array_equal(r["back"].cigar, reads.cigar) and np.array_equal(r["back"].cigar_off, reads.cigar_off), on
        assert np.array_equal(r["back"].pos, reads.pos) and np.array_equal(r["back"].flag, reads.flag) and np.array_equal(r["back"].mapq, reads.mapq), on
    a, b = runs[True]["out"], runs[False]["out"]
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    ra, rb = runs[True]["res"], runs[False]["res"]
    assert (ra.n_sig, ra.n_del, ra.n_ins, ra.depth_sum, ra.depth_nonzero, ra.min_pts, ra.mean_cov) == \
           (rb.n_sig, rb.n_del, rb.n_ins, rb.depth_sum, rb.depth_nonzero, rb.min_pts, rb.mean_cov)
    return runs


def _plain(n, seed=0):
    """n ops of an ordinary long read: aligned runs with small indels between them."""
    rng = np.random.default_rng(1000 + seed + n)
    ops = []
    for k in range(n):
        ops.append((M, int(rng.integers(5, 40))) if k % 2 == 0 else (int(rng.choice([I, D, D, X])), int(rng.integers(1, 4))))
    return ops


def _shard(cigs, fill_to=None, pos0=100, step=37, unsorted=False, tail_fill=True):
    """Reads from op lists at growing positions; plain reads of 300 ops are appended until the shard has 64 ops per escape (so that it packs),
    or fill_to ops."""
    cigs = [list(c) for c in cigs]
    n_esc = sum(1 for c in cigs for _, ln in c if ln >= ESC)
    m = sum(len(c) for c in cigs)
    need = max(64 * n_esc + 1, fill_to or 0) if tail_fill else 0
    k = 0
    while m < need:
        n = min(300, need - m)
        cigs.append(_plain(n, k)); m += n; k += 1
    pos = [pos0 + step * i for i in range(len(cigs))]
    order = list(range(len(cigs)))
    if unsorted:
        order = list(np.random.default_rng(5).permutation(len(cigs)))
    return Reads.from_cigar_lists(np.asarray([pos[i] for i in order], np.int32), np.zeros(len(cigs), np.uint16), np.full(len(cigs), 60, np.uint8),
                                  [cigs[i] for i in order])


def _with(ops, at, op, ln):
    ops = list(ops)
    ops[at] = (op, ln)
    return ops


# ------------------------------------------------------------------------------------------------------------------ lengths
@pytest.mark.parametrize("ln", [4094, 4095, 4096, 65_535, 300_000])
def test_lengths_at_the_edge_of_the_field(wave, oracle, ln):
    """D and N of the length inside depth_len (they move the reference cursor and open gaps in the depth map), I / S / H of the same length
    (the query cursor only): one read each, the op in mid-read; and clips of that length as a read's first and last op."""
    cigs = [_with(_plain(41), 20, op, ln) for op in (D, N, I, S, H)]
    cigs.append([(S, ln)] + _plain(30) + [(S, ln)])
    cigs.append([(H, ln), (S, ln)] + _plain(9) + [(I, ln), (M, 7), (H, ln)])
    reads = _shard(cigs)
    assert (_n_esc(reads) > 0) == (ln >= ESC)
    _check(wave, oracle, reads, packed=True)


def test_longest_lengths_touch_only_the_query_cursor(wave, oracle):
    """S / H / I of 2^28 - 1: q_end is exact in uint32 (nine of them in one read pass 2^31). The insertions of that read are kept apart by
    aligned runs: a signature holds the query offset in 30 bits, so insertions at one reference position with offsets beyond 2^30 would tie
    in the ordering pass's key, at either width."""
    cigs = [_with(_plain(41), 20, op, BIG) for op in (I, S, H)]
    cigs.append([(S, BIG)] + _plain(21) + [(I, BIG), (M, 5)] * 7 + [(M, 3), (S, BIG)])
    reads = _shard(cigs)
    runs = _check(wave, oracle, reads, packed=True)
    assert int(runs[True]["out"]["q_end"].view(np.uint32).max()) > (1 << 31)


# ------------------------------------------------------------------------------------------------------------------ where the escape sits
@pytest.mark.parametrize("at", [0, 255, 256, 257, 511, 512, 513, 1023, 1024])
def test_escape_at_the_chunk_and_piece_edges_of_the_array(wave, oracle, at):
    """One long first read: op `at` of the read is op `at` of the array (256-op chunk edges, 512-op piece edges)."""
    for op, ln in ((D, 70_000), (I, ESC)):
        _check(wave, oracle, _shard([_with(_plain(1300), at, op, ln)]), packed=True)


@pytest.mark.parametrize("lead", [0, 37, 255])
def test_escape_at_a_reads_ends_and_checkpoints(wave, oracle, lead):
    """A read behind `lead` ops of another one (so its checkpoint grid is not the chunks'): escapes at its first and its last op and at
    ops 63 / 64 / 65 of it, one at a time and all five together."""
    first = [_plain(lead)] if lead else []
    for where in ([0], [199], [63], [64], [65], [0, 63, 64, 65, 199]):
        ops = _plain(200)
        for k, at in enumerate(where):
            ops[at] = ((D, 5_000 + at), (I, 6_000), (N, ESC), (S, 70_000), (D, 4_096))[k % 5] if at not in (0, 199) else (S, 4_100 + at)
        _check(wave, oracle, _shard(first + [ops, _plain(90)]), packed=True)


def test_escape_in_the_neighbours_part_of_a_shared_chunk(wave, oracle):
    """Two (and three) reads inside one 256-op chunk: the escape of one is masked in the other's visit of the chunk and live in its own."""
    a, b, c = _plain(100), _plain(100), _plain(100)
    for cigs in ([a, _with(b, 0, S, 9_000), c], [a, _with(b, 50, D, 9_000), c], [_with(a, 99, I, 9_000), b, c],
                 [_with(a, 99, S, 5_000), _with(b, 0, S, 5_001), _with(b, 99, D, 5_002), _with(c, 0, H, 5_003)]):
        _check(wave, oracle, _shard(cigs), packed=True)


def test_several_escapes_in_one_lanes_four_ops(wave, oracle):
    """Ops 4 k .. 4 k + 3 of the array belong to one lane: two and four escapes among them."""
    ops = _plain(600)
    for at, (op, ln) in {8: (I, 4_095), 9: (D, 4_096), 300: (D, 5_000), 301: (I, 5_001), 302: (N, 5_002), 303: (S, 70_000)}.items():
        ops[at] = (op, ln)
    _check(wave, oracle, _shard([ops]), packed=True)


@pytest.mark.parametrize("run", [64, 300])
def test_escapes_in_a_row(wave, oracle, run):
    """A run of escapes inside a read (it crosses chunk, piece and checkpoint edges), mostly insertions with a deletion every tenth."""
    ops = _plain(900)
    for k in range(run):
        ops[200 + k] = (D, 4_095 + k) if k % 10 == 0 else (I, 4_095 + k)
    _check(wave, oracle, _shard([_plain(77), ops]), packed=True)


def test_read_made_only_of_escapes(wave, oracle):
    cigs = [_plain(120), [(S, 5_000), (D, 6_000), (I, 7_000), (D, 8_000), (N, 9_000), (I, BIG), (D, 4_095), (S, 4_096)], _plain(50),
            [(D, 10_000)], [(I, 10_000)], [(H, 10_000)]]
    _check(wave, oracle, _shard(cigs), packed=True)


@pytest.mark.parametrize("m", [1, 3, 513])
def test_last_partial_piece(wave, oracle, m):
    """Shards of 1, 3 and 513 ops: the last piece holds 1, 3 and 1 ops. With no escape they pack; a shard of 513 ops packs with an escape in
    its last piece's lone op (8 escapes would still pack, 9 would not); the shards of 1 and 3 ops with an escape are over the 1 / 64
    threshold and stay at 32 bits. All equal the oracle."""
    base = [(M, 30), (D, 2), (M, 30)][:m] if m <= 3 else _plain(513)
    _check(wave, oracle, _shard([base], tail_fill=False), packed=True)
    esc = _with(base, m - 1, D, 50_000)
    _check(wave, oracle, _shard([esc], tail_fill=False), packed=(m == 513))
    if m == 513:
        _check(wave, oracle, _shard([_plain(300), _with(_plain(213), 212, S, 4_095)], tail_fill=False), packed=True)      # ... as a read's last op
        ops = list(base)
        for k in range(8):
            ops[505 + k] = (I, 4_095 + k)
        _check(wave, oracle, _shard([ops], tail_fill=False), packed=True)
        ops[504] = (I, 4_200)
        _check(wave, oracle, _shard([ops], tail_fill=False), packed=False)


def test_escaped_deletions_across_depth_tile_edges(wave, oracle):
    """An escaped D (and N) that starts left of a tile's edge and ends right of it, one that crosses two tiles, one that covers whole tiles,
    one that ends exactly on an edge and one that starts on it."""
    cigs, pos = [], []
    for p, pre, op, ln in ((TILE - 400, 100, D, 5_000), (TILE - 400, 100, N, 5_000), (2 * TILE - 3_000, 1_000, D, TILE + 4_100),
                           (3 * TILE + 10, 20, D, 5 * TILE), (5 * TILE - 5_000, 905, D, 4_095), (6 * TILE - 120, 120, N, 4_096),
                           (10, 50, D, 300_000)):
        cigs.append([(M, pre), (op, ln), (M, 200), (I, 2), (M, 100)]); pos.append(p)
    order = np.argsort(pos, kind="stable")
    fill = [_plain(300, k) for k in range(2)]
    reads = Reads.from_cigar_lists(np.asarray([pos[i] for i in order] + [7 * TILE, 7 * TILE + 5], np.int32), np.zeros(len(cigs) + 2, np.uint16),
                                   np.full(len(cigs) + 2, 60, np.uint8), [cigs[i] for i in order] + fill)
    _check(wave, oracle, reads, packed=True)
    _check(wave, oracle, reads, depth_len=3 * TILE + 77, packed=True)          # ... and across the contig's end


def test_unsorted_shard(wave, oracle):
    """The same kinds of reads in a shard that is not coordinate-sorted: the depth pass goes through the read permutation."""
    cigs = [_with(_plain(300), 150, D, 70_000), [(S, 5_000)] + _plain(200) + [(S, 6_000)], _with(_plain(700), 511, N, 4_095),
            _with(_with(_plain(64), 63, I, BIG), 0, H, 4_095), _plain(33), _with(_plain(500), 256, D, 2 * TILE)]
    _check(wave, oracle, _shard(cigs, step=911, unsorted=True), packed=True)
    _check(wave, oracle, _shard(cigs, step=911, unsorted=False), packed=True)


# ------------------------------------------------------------------------------------------------------------------ which form a shard takes
def test_threshold_of_one_escape_in_64(wave, oracle):
    """100 reads of 64 ops with one escape each are at the threshold (6 400 ops, 100 escapes) and pack; one more escape and the shard stays at
    32 bits. Both equal the oracle."""
    cigs = [_with(_plain(64, k), 10 + k % 40, I, 4_095 + k) for k in range(100)]
    at = _shard(cigs, tail_fill=False)
    assert at.n_cigar == 6_400 and _n_esc(at) == 100
    _check(wave, oracle, at, packed=True)
    cigs[7] = _with(cigs[7], 60, D, 4_095)
    over = _shard(cigs, tail_fill=False)
    assert _n_esc(over) == 101
    _check(wave, oracle, over, packed=False)


@pytest.mark.parametrize("form", [1, 2, 3])
def test_short_read_forms_stay_at_32_bits(ctx, oracle, form):
    ctx.set_tuning(scan_form=form)
    try:
        _check(ctx, oracle, _shard([_with(_plain(300), 100, D, 5_000), _plain(40), _plain(41)]), packed=False)
    finally:
        ctx.set_tuning()


def test_default_form_choice_packs_long_reads_only(ctx, oracle):
    """No forced form: a shard of long reads (>= 192 ops per read) takes the wave form and packs, a shard of short reads does not."""
    ctx.set_tuning()
    _check(ctx, oracle, _shard([_with(_plain(900), 300, D, 5_000), _plain(800), _plain(700)], tail_fill=False), packed=True)
    _check(ctx, oracle, _shard([_plain(40, k) for k in range(30)], tail_fill=False), packed=False)


# ------------------------------------------------------------------------------------------------------------------ the switch
def test_switch_is_checked_per_context_and_read_at_upload(wave, oracle):
    ctx = wave
    reads = _shard([_with(_plain(600), 300, D, 5_000), _plain(500)])
    for bad in (2, -1):
        assert ctx.lib.csvgpu_set_cigar_packing(ctx.h, bad) == _lib.CSV_EINVAL
    sh = ctx.upload(reads, DEPTH_LEN)
    try:
        assert sh.cigar_bytes() == _bytes(reads, True)                       # the refused calls changed nothing
        job = ctx.lib.csvgpu_chr_job_begin(ctx.h, sh.h, 50, 20, 0.1)
        assert job
        try:
            assert ctx.lib.csvgpu_set_cigar_packing(ctx.h, 0) == _lib.CSV_EINVAL
        finally:
            assert ctx.lib.csvgpu_chr_job_abort(ctx.h, job) == 0
        # a shard keeps the form it was uploaded with: packing goes off, the packed shard runs as before and a new one is at 32 bits
        ctx.set_cigar_packing(False)
        sh2 = ctx.upload(reads, DEPTH_LEN)
        try:
            assert sh.cigar_bytes() == _bytes(reads, True) and sh2.cigar_bytes() == _bytes(reads, False)
            od, osum, onz = oracle.depth(reads, DEPTH_LEN)
            for s in (sh, sh2):
                res = s.pipeline(eps=0.1, min_pts_pct=0.1)
                out = s.fetch(res, want_depth=True)
                assert np.array_equal(out["depth"], od) and (res.depth_sum, res.depth_nonzero) == (osum, onz)
        finally:
            sh2.free()
    finally:
        sh.free()
        ctx.set_cigar_packing(True)
    # per context: another context of the process is not touched by this one's switch
    other = cs.Context(0)
    try:
        other.set_tuning(scan_form=0)
        ctx.set_cigar_packing(False)
        a, b = other.upload(reads, DEPTH_LEN), ctx.upload(reads, DEPTH_LEN)
        try:
            assert a.cigar_bytes() == _bytes(reads, True) and b.cigar_bytes() == _bytes(reads, False)
        finally:
            a.free(); b.free()
    finally:
        ctx.set_cigar_packing(True)
        other.close()


# ------------------------------------------------------------------------------------------------------------------ a genome
def test_genome_run_is_the_same_with_packing_on_and_off(ctx):
    """One Genome.run over three small long-read contigs, uploaded with packing on and with packing off: the same call records and
    per-contig statistics."""
    from hmm_params import WGS_HMM
    hmm = make_hmm(**WGS_HMM)
    host.set_context(ctx)
    ctx.set_tuning()
    fields = ("start", "end", "sv_type", "cluster_size", "aln_flags", "genotype", "cn_state", "aln_offset", "hmm_likelihood")
    stats = ("n_signatures", "n_del", "n_ins", "depth_sum", "depth_nonzero", "min_pts", "mean_cov", "n_calls")
    results = {}
    try:
        for on in (True, False):
            ctx.set_cigar_packing(on)
            g = host.Genome()
            try:
                for t, L in enumerate([400_000, 250_000, 300_000]):
                    syn = host.SynthShard(0xC16A + 17 * t, L, 12.0, 0, 4, sv_per_bp=1.0 / 30000.0)
                    try:
                        r = syn.reads
                        assert r.n_cigar // max(r.n_reads, 1) >= 192          # long reads: the wave form, which packs
                        reads = cs.Reads(r.pos.copy(), r.flag.copy(), r.mapq.copy(), r.cigar_off.copy(), r.cigar.copy())
                        qid = syn.qname_id.astype(np.uint32) + np.uint32(t << 24)
                        rng = np.random.default_rng(t)
                        n_snp = L // 1000
                        pos = np.sort(rng.choice(np.arange(1000, L - 1000), n_snp, replace=False)).astype(np.uint32)
                        snps = {"pos": pos, "baf": np.where(rng.random(n_snp) < 0.66, 0.45 + 0.1 * rng.random(n_snp), 1.0), "pfb": np.zeros(n_snp),
                                "has_pfb": np.zeros(n_snp, np.uint8)}
                        g.add(ctx, "contig%d" % t, t, reads, syn.depth_len, qid, snps, name_style=0)
                    finally:
                        syn.free()
                got, tid, st, per = g.run(ctx, hmm)
                results[on] = (got, tid, [tuple(getattr(p, f) for f in stats) for p in per])
            finally:
                g.free()
    finally:
        ctx.set_cigar_packing(True)
    (a, ta, pa), (b, tb, pb) = results[True], results[False]
    assert len(a) == len(b) and len(a) > 0 and np.array_equal(ta, tb)
    for f in fields:
        assert np.array_equal(a[f], b[f]), f
    assert pa == pb and len(pa) == 3 and all(p[0] > 0 for p in pa)
