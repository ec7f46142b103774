"""The copy-number passes with their observation vectors built and decoded on the device (CNVCaller::device_observations,
RunParams::cn_observations_on_device -> csvgpu_cn_decode_resident_many): the same calls as the default route field for field, the
likelihoods bit for bit, on tests/test_gpu_cnv.py's call sets, against the oracle under that file's tolerances, through the host route
for a batch outside the device call's domain, and through Genome.run in every schedule variant of tests/test_gpu_split_device_tables.py."""
import numpy as np
import pytest

import contextsv_amd as cs
from contextsv_amd import host, make_hmm
from hmm_params import WGS_HMM
from test_gpu_cnv import DEL, DUP, INS, INV, UNKNOWN, _calls, _same_calls, cnv_setup  # noqa: F401  (cnv_setup: that file's fixture)
from test_gpu_genome import _many_small, _same
from test_gpu_split_device_groups import _generated

pytestmark = pytest.mark.gpu
FIELDS = ("pos", "baf", "pfb", "log2_cov", "is_snp")


def _cigar_calls():
    calls = _calls(np.random.default_rng(3), 120, [DEL, INS, DUP, INV])
    calls[:4]["start"] = [62_000, 205_000, 62_000, 120_000]; calls[:4]["end"] = [105_000, 255_000, 105_000, 160_000]
    calls[:4]["sv_type"] = [DEL, INS, INS, DEL]
    return calls


def _split_calls():
    calls = _calls(np.random.default_rng(4), 80, [UNKNOWN, INV, INS, DEL, DUP])
    calls[:5]["start"] = [62_000, 205_000, 63_000, 206_000, 64_000]; calls[:5]["end"] = [105_000, 255_000, 104_000, 254_000, 103_000]
    calls[:5]["sv_type"] = [UNKNOWN, UNKNOWN, INV, DEL, DUP]
    return calls[np.lexsort((calls["end"], calls["start"]))]


def _identical(a, b):
    assert a.dtype == b.dtype and len(a) == len(b)
    for f in a.dtype.names:
        assert a[f].tobytes() == b[f].tobytes(), f                 # hmm_likelihood included: bitwise


@pytest.mark.parametrize("split", [False, True])
def test_cn_prediction_is_the_default_routes_and_the_oracles(ctx, oracle, cnv_setup, split):
    sh, res, depth, snps = cnv_setup
    hmm = make_hmm(**WGS_HMM)
    calls = _split_calls() if split else _cigar_calls()
    ctx.timing_enable(1)
    try:
        ctx.timing_reset()
        off = host.cn_prediction(ctx, sh, calls, hmm, res.mean_cov, snps, split=split)
        on = host.cn_prediction(ctx, sh, calls, hmm, res.mean_cov, snps, split=split, observations_on_device=True)
        tm = ctx.timing()
    finally:
        ctx.timing_enable(0)
    _identical(on, off)
    _same_calls(on, oracle.cn_prediction(depth, calls, hmm, res.mean_cov, snps, split=split))
    assert (on["cn_state"] != 0).any()
    assert tm["window"][1] >= 2 and tm["viterbi"][1] >= 2          # both routes ran their window group and their Viterbi launch on this context


def test_query_snp_regions_on_device_returns_all_five_arrays(ctx, oracle, cnv_setup):
    sh, res, depth, snps = cnv_setup
    starts = np.asarray([70_000, 1, 205_000, 301_000, 150_000, 50_000, 399_000, 9000], np.uint32)
    ends = np.asarray([100_000, 399_999, 215_000, 305_000, 150_009, 52_500, 400_600, 8000], np.uint32)      # the last one is invalid: no observation
    off = host.query_snp_regions(ctx, sh, starts, ends, res.mean_cov, 20, snps, on_device=False)
    on = host.query_snp_regions(ctx, sh, starts, ends, res.mean_cov, 20, snps, on_device=True)
    assert np.array_equal(on["obs_off"], off["obs_off"]) and on["obs_off"][-1] == on["obs_off"][-2] == len(on["pos"])
    for f in FIELDS:
        assert len(on[f]) == len(on["pos"]) > 0 and on[f].tobytes() == off[f].tobytes(), f
    for i in range(len(starts) - 1):
        exp = oracle.query_snp_region(depth, int(starts[i]), int(ends[i]), res.mean_cov, 20, snps)
        a, b = int(on["obs_off"][i]), int(on["obs_off"][i + 1])
        assert np.array_equal(on["pos"][a:b], exp["pos"]) and np.array_equal(on["is_snp"][a:b], exp["is_snp"])
        np.testing.assert_allclose(on["log2_cov"][a:b], exp["log2_cov"], rtol=0, atol=1e-6)


def test_a_batch_outside_the_domain_takes_the_host_route(ctx, cnv_setup):
    """5088 windows in one region: the device call would refuse the batch, the mirror gives the option-off result."""
    sh, res, depth, snps = cnv_setup
    starts, ends = np.asarray([10_000, 70_000], np.uint32), np.asarray([80_000, 100_000], np.uint32)
    off = host.query_snp_regions(ctx, sh, starts, ends, res.mean_cov, 5088, snps, on_device=False)
    on = host.query_snp_regions(ctx, sh, starts, ends, res.mean_cov, 5088, snps, on_device=True)
    inside = host.query_snp_regions(ctx, sh, starts, ends, res.mean_cov, 5087, snps, on_device=True)
    assert np.array_equal(on["obs_off"], off["obs_off"]) and all(on[f].tobytes() == off[f].tobytes() for f in FIELDS)
    assert int(np.diff(inside["obs_off"].astype(np.int64)).min()) >= 5087


def _run_both(ctx, g, hmm, **kw):
    """-> the records of the default run; asserts that cn_observations_on_device gives the same ones, alone and with split_tables_on_device."""
    ref, ref_tid, st0, _ = g.run(ctx, hmm, **kw)
    for tables in (False, True):
        got, tid, st, _ = g.run(ctx, hmm, cn_observations_on_device=True, split_tables_on_device=tables, **kw)
        assert np.array_equal(tid, ref_tid), (kw, tables)
        _same(got, ref)
        assert got["hmm_likelihood"].tobytes() == ref["hmm_likelihood"].tobytes(), (kw, tables)
        assert st.n_split_calls == st0.n_split_calls and st.n_cigar_cn_regions == st0.n_cigar_cn_regions
    return ref, st0


@pytest.mark.parametrize("tech,depth", [(0, 30.0), (1, 60.0)])
def test_genome_run_on_generated_contigs(ctx, tech, depth):
    hmm = make_hmm(**WGS_HMM)
    host.set_context(ctx)
    g = _generated(ctx, tech, depth)
    try:
        ref, st0 = _run_both(ctx, g, hmm)
        assert len(ref) > 10 and st0.n_cigar_cn_regions + st0.n_split_calls > 0          # the copy-number passes had candidates
    finally:
        g.free()


def test_genome_run_through_every_schedule(ctx):
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
