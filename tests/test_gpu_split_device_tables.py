"""The split-read pass with its tables built on the device from the resident shards (RunParams::split_tables_on_device ->
SplitParams::device_tables -> csvgpu_split_resident_fits): the same records as the default run through every place the pass works on groups
(SplitPass::finishEarly, finishFor and finish), with supplementary records on other contigs passing through the run, and the proof that the
table kernel, the groups chain and the fits are what ran — and neither the DBSCAN1D batch beside them nor the table kernel without the option."""
import numpy as np
import pytest

import contextsv_amd as cs
from contextsv_amd import Reads, host, make_hmm
from hmm_params import WGS_HMM
from test_gpu_genome import _many_small, _same
from test_gpu_split import _make_split_shard
from test_gpu_split_device_groups import _generated

pytestmark = pytest.mark.gpu


def _run_both(ctx, g, hmm, **kw):
    """-> the records of the default run; asserts that split_tables_on_device gives the same ones (alone and with the two older switches, which it
    overrides) and which kernels ran."""
    ctx.timing_enable(1)
    try:
        ctx.timing_reset()
        ref, ref_tid, st0, _ = g.run(ctx, hmm, **kw)
        tm = ctx.timing()
        assert tm["misc"][1] == 0 and tm["split_fits"][1] == 0 and tm["split_groups"][1] == 0, kw
        had_groups = tm["dbscan1d"][1] >= 1
        assert had_groups, kw                                  # (every genome of this file has overlap groups: the chain below has work)
        for older in (False, True):
            ctx.timing_reset()
            got, tid, st, _ = g.run(ctx, hmm, split_tables_on_device=True, split_groups_on_device=older, split_fits_on_device=older, **kw)
            tm = ctx.timing()
            assert tm["misc"][1] >= 1 and tm["split_fits"][1] >= 1 and tm["split_groups"][1] >= 1 and tm["dbscan1d"][1] == 0, (kw, older, tm)
            assert np.array_equal(tid, ref_tid), (kw, older)
            _same(got, ref)
            assert st.n_split_calls == st0.n_split_calls
    finally:
        ctx.timing_enable(0)
    return ref, st0, had_groups


@pytest.mark.parametrize("tech,depth", [(0, 30.0), (1, 60.0)])
def test_genome_run_on_generated_contigs(ctx, tech, depth):
    hmm = make_hmm(**WGS_HMM)
    host.set_context(ctx)
    g = _generated(ctx, tech, depth)
    try:
        ref, st0, had_groups = _run_both(ctx, g, hmm)
        assert len(ref) > 10
        if tech == 0:
            assert st0.n_split_calls > 0 and had_groups
    finally:
        g.free()


def test_genome_run_with_supplementary_records_on_other_contigs(ctx):
    """_make_split_shard(2)'s records as a genome of three contigs: its `xchr` events put supplementary records on another contig than their
    primary, so entries that are only a flags byte pass through the run."""
    hmm = make_hmm(**WGS_HMM)
    host.set_context(ctx)
    reads, tid, qn, n_contigs = _make_split_shard(2)
    lo = np.searchsorted(tid, np.arange(n_contigs + 1))
    refs, seg_off, supp_tid = host.split_refs(tid, reads.pos, reads.flag, reads.mapq, qn, n_contigs)
    assert (refs.supp_where != 0).sum() > 10
    g = host.Genome()
    try:
        for t in range(n_contigs):
            a, b = int(lo[t]), int(lo[t + 1])
            w0, w1 = int(reads.cigar_off[a]), int(reads.cigar_off[b])
            r = Reads(reads.pos[a:b].copy(), reads.flag[a:b].copy(), reads.mapq[a:b].copy(), (reads.cigar_off[a:b + 1] - np.uint64(w0)).copy(), reads.cigar[w0:w1].copy())
            g.add(ctx, "contig%d" % t, t, r, 3_000_001, qn[a:b], None, name_style=0)
        ref, st0, had_groups = _run_both(ctx, g, hmm)
        assert had_groups and st0.n_split_calls > 5
    finally:
        g.free()


def test_genome_run_through_every_schedule(ctx):
    """Fourteen small contigs through three lanes, every schedule variant that tests/test_gpu_split_device_fits.py lists: early batches inside
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
        ref, st0, _ = _run_both(ctx, g, hmm)
        assert len(ref) > 20 and st0.n_split_calls > 0
        for kw in ({}, {"early_batches": "none"}, {"early_batches": "all"}, {"early_batches": "every3"}, {"split_beside_pass": False},
                   {"early_batches": "none", "split_beside_pass": False}, {"overlap_split": False}):
            again, _, _ = _run_both(ctx, g, hmm, lanes=lanes, **kw)
            _same(again, ref)
    finally:
        for c in lanes:
            c.set_gate(None)
            c.close()
        gate.close()
        g.free()
