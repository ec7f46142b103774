"""The split-read pass with its overlap groups from the device (SplitParams::device_groups -> csvgpu_split_groups): the same calls as the
oracle's literal restatement and as the host tree, through every place the pass builds groups (SplitPass::finishEarly, finishFor and
finish), and the proof that the device entry point is what ran."""
import numpy as np
import pytest

import contextsv_amd as cs
from contextsv_amd import Reads, host, make_hmm
from hmm_params import WGS_HMM
from test_gpu_genome import _many_small, _same
from test_gpu_split import _make_split_shard

pytestmark = pytest.mark.gpu
M, S, H = 0, 4, 5


def _signatures_both_ways(ctx, oracle, reads, tid, qn, n_contigs):
    g_end, g_qs, g_qe = ctx.aln_intervals(reads)
    o_end, o_qs, o_qe = oracle.aln_intervals(reads)
    exp = oracle.split_signatures(tid, reads.pos, reads.flag, reads.mapq, o_end, o_qs, o_qe, qn)
    ctx.timing_enable(1)
    try:
        ctx.timing_reset()
        on_host = host.split_signatures(ctx, tid, reads.pos, reads.flag, reads.mapq, g_end, g_qs, g_qe, qn, n_contigs)
        assert ctx.timing()["split_groups"][1] == 0
        got = host.split_signatures(ctx, tid, reads.pos, reads.flag, reads.mapq, g_end, g_qs, g_qe, qn, n_contigs, device_groups=True)
        assert ctx.timing()["split_groups"][1] >= 1
    finally:
        ctx.timing_enable(0)
    assert len(exp) > 5
    assert got.tobytes() == exp.tobytes()
    assert on_host.tobytes() == exp.tobytes()
    return got


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_split_signatures_with_device_groups_match_oracle(ctx, oracle, seed):
    reads, tid, qn, n_contigs = _make_split_shard(seed)
    _signatures_both_ways(ctx, oracle, reads, tid, qn, n_contigs)


def _make_dense_shard(seed, n_events=420, n_contigs=3, contig_len=40_000_000):
    """Many events of up to 200 reads, a quarter of them next to the event before (so that reads are shared between overlap groups), each read a
    primary ending at the breakpoint and a supplementary piece `span` further on."""
    rng = np.random.default_rng(seed)
    recs = []
    qid = 0
    tid, L = 0, 1_000_000
    for ev in range(n_events):
        if ev == 0 or rng.random() > 0.25:
            tid = int(rng.integers(0, n_contigs))
            L = int(rng.integers(100_000, contig_len - 2_000_000))
        else:
            L += int(rng.integers(-9000, 9001))
        span = int(np.exp(rng.uniform(np.log(2500), np.log(300_000))))
        k = int(rng.choice([2, 5, 12, 30, 70, 120, 200]))
        rev_event = bool(rng.random() < 0.2)
        for _ in range(k):
            a, b = int(rng.integers(3000, 15000)), int(rng.integers(3000, 15000))
            j1, j2 = int(rng.integers(-8, 9)), int(rng.integers(-8, 9))
            f = 0x10 if rng.random() < 0.5 else 0
            mq = 60 if rng.random() > 0.05 else int(rng.integers(0, 20))
            recs.append((tid, L - a + j1, f, mq, [(M, a), (S, b)], qid))
            recs.append((tid, L + span + j2, (f ^ 0x10 if rev_event else f) | 0x800, mq, [(H, a), (M, b)], qid))
            qid += 1
    for _ in range(600):                                  # primaries without a supplementary record
        recs.append((int(rng.integers(0, n_contigs)), int(rng.integers(1000, contig_len - 20000)), 0, 60, [(M, int(rng.integers(2000, 15000)))], qid))
        qid += 1
    recs.sort(key=lambda r: (r[0], r[1]))
    reads = Reads.from_cigar_lists([r[1] for r in recs], [r[2] for r in recs], [r[3] for r in recs], [r[4] for r in recs])
    return reads, np.array([r[0] for r in recs], np.int32), np.array([r[5] for r in recs], np.uint32), n_contigs


@pytest.mark.parametrize("seed", [11, 12])
def test_dense_events_with_device_groups_match_oracle(ctx, oracle, seed):
    reads, tid, qn, n_contigs = _make_dense_shard(seed)
    got = _signatures_both_ways(ctx, oracle, reads, tid, qn, n_contigs)
    assert got["cluster_size"].max() >= 100               # groups of hundreds went through


def _generated(ctx, tech, depth):
    g = host.Genome()
    for t, L in enumerate([1_500_000, 900_000, 1_200_000]):
        syn = host.SynthShard(0xC0FFEE + 17 * t + tech, L, depth, tech, 4, sv_per_bp=1.0 / 30000.0)
        r = syn.reads
        reads = cs.Reads(r.pos.copy(), r.flag.copy(), r.mapq.copy(), r.cigar_off.copy(), r.cigar.copy())
        qid = syn.qname_id.astype(np.uint32) + np.uint32(t << 24)
        rng = np.random.default_rng(t)
        n_snp = L // 1000
        pos = np.sort(rng.choice(np.arange(1000, L - 1000), n_snp, replace=False)).astype(np.uint32)
        snps = {"pos": pos, "baf": np.where(rng.random(n_snp) < 0.66, 0.45 + 0.1 * rng.random(n_snp), 1.0), "pfb": np.zeros(n_snp), "has_pfb": np.zeros(n_snp, np.uint8)}
        g.add(ctx, "contig%d" % t, t, reads, syn.depth_len, qid, snps, name_style=0)
        syn.free()
    return g


def _run_both(ctx, g, hmm, **kw):
    """-> the records with the option off; asserts that the option gives the same ones and that csvgpu_split_groups ran only with it."""
    ctx.timing_enable(1)
    try:
        ctx.timing_reset()
        ref, ref_tid, st0, _ = g.run(ctx, hmm, **kw)
        assert ctx.timing()["split_groups"][1] == 0, kw
        ctx.timing_reset()
        got, tid, st, _ = g.run(ctx, hmm, split_groups_on_device=True, **kw)
        assert ctx.timing()["split_groups"][1] >= 1, kw
    finally:
        ctx.timing_enable(0)
    assert np.array_equal(tid, ref_tid), kw
    _same(got, ref)
    assert st.n_split_calls == st0.n_split_calls
    return ref, st0


@pytest.mark.parametrize("tech,depth", [(0, 30.0), (1, 60.0)])
def test_genome_run_on_generated_contigs(ctx, tech, depth):
    hmm = make_hmm(**WGS_HMM)
    host.set_context(ctx)
    g = _generated(ctx, tech, depth)
    try:
        ref, st0 = _run_both(ctx, g, hmm)
        assert len(ref) > 10
        if tech == 0:
            assert st0.n_split_calls > 0
    finally:
        g.free()


def test_genome_run_through_every_schedule(ctx):
    """Fourteen small contigs through three lanes: early batches inside the CIGAR pass (finishFor), the split chain beside the pass
    (finishEarly, then finishFor), everything behind the pass (finish), and the run without lanes."""
    hmm = make_hmm(**WGS_HMM)
    host.set_context(ctx)
    g = _many_small(ctx)
    lanes = [cs.Context(0) for _ in range(3)]
    gate = cs.Gate()
    try:
        for c in lanes:
            c.set_gate(gate)
        ref, st0 = _run_both(ctx, g, hmm)
        assert len(ref) > 20 and st0.n_split_calls > 0
        for kw in ({}, {"early_batches": "none"}, {"early_batches": "all"}, {"early_batches": "every3"}, {"split_beside_pass": False},
                   {"early_batches": "none", "split_beside_pass": False}, {"overlap_split": False}):
            again, _ = _run_both(ctx, g, hmm, lanes=lanes, **kw)
            _same(again, ref)
    finally:
        for c in lanes:
            c.set_gate(None)
            c.close()
        gate.close()
        g.free()
