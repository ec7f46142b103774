"""The split-read pass with its groups' evidence from the device (SplitParams::device_fits -> csvgpu_split_fits, with device_groups also set
csvgpu_split_groups_fits): the same calls as the oracle's literal restatement and as the host's sets + DBSCAN1D batch, through every place the
pass works on groups (SplitPass::finishEarly, finishFor and finish), and the proof that the device entry point is what ran and that neither
the point sets nor the DBSCAN1D batch ran beside it."""
import numpy as np
import pytest

import contextsv_amd as cs
from contextsv_amd import host, make_hmm
from hmm_params import WGS_HMM
from test_gpu_genome import _many_small, _same
from test_gpu_split import _make_split_shard
from test_gpu_split_device_groups import _generated, _make_dense_shard

pytestmark = pytest.mark.gpu


def _signatures_every_way(ctx, oracle, reads, tid, qn, n_contigs):
    g_end, g_qs, g_qe = ctx.aln_intervals(reads)
    o_end, o_qs, o_qe = oracle.aln_intervals(reads)
    exp = oracle.split_signatures(tid, reads.pos, reads.flag, reads.mapq, o_end, o_qs, o_qe, qn)
    assert len(exp) > 5
    args = (ctx, tid, reads.pos, reads.flag, reads.mapq, g_end, g_qs, g_qe, qn, n_contigs)
    ctx.timing_enable(1)
    try:
        for groups in (False, True):
            ctx.timing_reset()
            off = host.split_signatures(*args, device_groups=groups)
            tm = ctx.timing()
            assert tm["split_fits"][1] == 0 and tm["dbscan1d"][1] >= 1, groups
            assert off.tobytes() == exp.tobytes(), groups
            ctx.timing_reset()
            on = host.split_signatures(*args, device_groups=groups, device_fits=True)
            tm = ctx.timing()
            assert tm["split_fits"][1] >= 1 and tm["dbscan1d"][1] == 0, groups
            assert (tm["split_groups"][1] >= 1) == groups
            assert on.tobytes() == exp.tobytes(), groups
    finally:
        ctx.timing_enable(0)
    return exp


@pytest.mark.parametrize("seed", [1, 2, 3, 4])
def test_split_signatures_with_device_fits_match_oracle(ctx, oracle, seed):
    reads, tid, qn, n_contigs = _make_split_shard(seed)
    _signatures_every_way(ctx, oracle, reads, tid, qn, n_contigs)


@pytest.mark.parametrize("seed", [11, 12])
def test_dense_events_with_device_fits_match_oracle(ctx, oracle, seed):
    reads, tid, qn, n_contigs = _make_dense_shard(seed)
    got = _signatures_every_way(ctx, oracle, reads, tid, qn, n_contigs)
    assert got["cluster_size"].max() >= 100               # groups of hundreds went through


def _run_all(ctx, g, hmm, **kw):
    """-> the records of the default run; asserts that split_fits_on_device, alone and with split_groups_on_device, gives the same ones, that
    csvgpu_split_fits ran only with it and that the DBSCAN1D batch did not run beside it."""
    ctx.timing_enable(1)
    try:
        ctx.timing_reset()
        ref, ref_tid, st0, _ = g.run(ctx, hmm, **kw)
        tm = ctx.timing()
        assert tm["split_fits"][1] == 0, kw
        had_groups = tm["dbscan1d"][1] >= 1
        for groups in (False, True):
            ctx.timing_reset()
            got, tid, st, _ = g.run(ctx, hmm, split_fits_on_device=True, split_groups_on_device=groups, **kw)
            tm = ctx.timing()
            assert (tm["split_fits"][1] >= 1) == had_groups and tm["dbscan1d"][1] == 0, (kw, groups)
            assert np.array_equal(tid, ref_tid), (kw, groups)
            _same(got, ref)
            assert st.n_split_calls == st0.n_split_calls
    finally:
        ctx.timing_enable(0)
    return ref, st0


@pytest.mark.parametrize("tech,depth", [(0, 30.0), (1, 60.0)])
def test_genome_run_on_generated_contigs(ctx, tech, depth):
    hmm = make_hmm(**WGS_HMM)
    host.set_context(ctx)
    g = _generated(ctx, tech, depth)
    try:
        ref, st0 = _run_all(ctx, g, hmm)
        assert len(ref) > 10
        if tech == 0:
            assert st0.n_split_calls > 0
    finally:
        g.free()


def test_genome_run_through_every_schedule(ctx):
    """Fourteen small contigs through three lanes, every schedule variant that tests/test_gpu_split_device_groups.py lists: early batches inside
    the CIGAR pass (finishFor), the split chain beside the pass (finishEarly, then finishFor), everything behind the pass (finish), and the
    run without lanes."""
    hmm = make_hmm(**WGS_HMM)
    host.set_context(ctx)
    g = _many_small(ctx)
    lanes = [cs.Context(0) for _ in range(3)]
    gate = cs.Gate()
    try:
        for c in lanes:
            c.set_gate(gate)
        ref, st0 = _run_all(ctx, g, hmm)
        assert len(ref) > 20 and st0.n_split_calls > 0
        for kw in ({}, {"early_batches": "none"}, {"early_batches": "all"}, {"early_batches": "every3"}, {"split_beside_pass": False},
                   {"early_batches": "none", "split_beside_pass": False}, {"overlap_split": False}):
            again, _ = _run_all(ctx, g, hmm, lanes=lanes, **kw)
            _same(again, ref)
    finally:
        for c in lanes:
            c.set_gate(None)
            c.close()
        gate.close()
        g.free()
