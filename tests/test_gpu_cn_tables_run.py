"""The copy-number passes of the host mirror with their SNPs looked up in resident tables (SNPSource::residentTable ->
csvgpu_cn_decode_tables_many / csvgpu_cn_observations_tables_many): host.cn_prediction(..., snp_table=) and host.query_snp_regions(...,
snp_table=) against the default route field for field, the likelihoods bit for bit, a batch the device declines through the route the
options select, and Genome.run with snp_tables_resident(True) against (False) on the generated contigs and through the schedule variants
of tests/test_gpu_cn_device_observations.py, each with cn_observations_on_device on and off."""
import numpy as np
import pytest

import contextsv_amd as cs
from contextsv_amd import host, make_hmm
from hmm_params import WGS_HMM
from test_gpu_cn_device_observations import FIELDS, _cigar_calls, _identical, _split_calls
from test_gpu_cnv import cnv_setup  # noqa: F401  (that file's fixture)
from test_gpu_genome import _many_small, _same
from test_gpu_split_device_groups import _generated

pytestmark = pytest.mark.gpu


def _table(ctx, snps):
    return ctx.snp_table(snps["pos"], snps["baf"], snps["pfb"], snps["has_pfb"])


@pytest.mark.parametrize("split", [False, True])
def test_cn_prediction_with_a_table_is_the_default_route(ctx, cnv_setup, split):
    sh, res, depth, snps = cnv_setup
    hmm = make_hmm(**WGS_HMM)
    calls = _split_calls() if split else _cigar_calls()
    tab = _table(ctx, snps)
    try:
        off = host.cn_prediction(ctx, sh, calls, hmm, res.mean_cov, snps, split=split)
        assert (off["cn_state"] != 0).any()
        for on_device in (False, True):
            _identical(host.cn_prediction(ctx, sh, calls, hmm, res.mean_cov, snps, split=split, observations_on_device=on_device, snp_table=tab), off)
    finally:
        tab.free()


def test_the_remembered_capacity_saves_the_second_plan(ctx, cnv_setup):
    """One table call per cn_prediction. Its window groups on the context: plan + chain = 2 when the remembered capacity is enough;
    plan, CSV_ECAPACITY, plan + chain = 3 when the call has to ask for it."""
    sh, res, depth, snps = cnv_setup
    hmm = make_hmm(**WGS_HMM)
    calls = _cigar_calls()
    tab = _table(ctx, snps)
    run = lambda: host.cn_prediction(ctx, sh, calls, hmm, res.mean_cov, snps, split=False, snp_table=tab)
    try:
        want = run()                                                     # (the arenas and the page-locked block are grown by now)
        ctx.timing_enable(1)
        groups = []
        host.cn_table_capacity_hint(forget=True)
        for _ in range(3):
            ctx.timing_reset()
            _identical(run(), want)
            groups.append((ctx.timing()["window"][1], ctx.timing()["viterbi"][1]))
        needed = host.cn_table_capacity_hint()
        assert groups == [(3, 1), (2, 1), (2, 1)], groups
        assert needed > len(calls)                                       # the bound: at least a window per candidate
        host.cn_table_capacity_hint(forget=True)                         # ... and it is only ever raised: a smaller call leaves it
        run()
        host.cn_prediction(ctx, sh, calls[:10], hmm, res.mean_cov, snps, split=False, snp_table=tab)
        assert host.cn_table_capacity_hint() == needed
    finally:
        ctx.timing_enable(0)
        tab.free()


def test_query_snp_regions_with_a_table(ctx, cnv_setup):
    sh, res, depth, snps = cnv_setup
    starts = np.asarray([70_000, 1, 205_000, 301_000, 150_000, 50_000, 399_000, 9000], np.uint32)
    ends = np.asarray([100_000, 399_999, 215_000, 305_000, 150_009, 52_500, 400_600, 8000], np.uint32)      # the last one is invalid: no observation
    tab = _table(ctx, snps)
    try:
        off = host.query_snp_regions(ctx, sh, starts, ends, res.mean_cov, 20, snps)
        on = host.query_snp_regions(ctx, sh, starts, ends, res.mean_cov, 20, snps, snp_table=tab)
        assert np.array_equal(on["obs_off"], off["obs_off"]) and on["obs_off"][-1] == on["obs_off"][-2] == len(on["pos"]) > 0
        assert all(on[f].tobytes() == off[f].tobytes() for f in FIELDS)
    finally:
        tab.free()


def test_a_declined_batch_gives_the_default_routes_result(ctx, cnv_setup):
    """5088 SNPs inside one candidate: only the device sees it, declines, and the whole batch takes the route the options select."""
    sh, res, depth, snps = cnv_setup
    hmm = make_hmm(**WGS_HMM)
    dense = np.arange(120_000, 120_000 + 5088, dtype=np.uint32)
    keep = (snps["pos"] < 120_000) | (snps["pos"] >= 120_000 + 5088)
    rng = np.random.default_rng(9)
    many = {"pos": np.concatenate([snps["pos"][keep], dense]), "baf": np.concatenate([snps["baf"][keep], rng.uniform(0.3, 0.7, 5088)]),
            "pfb": np.concatenate([snps["pfb"][keep], rng.uniform(0.1, 0.9, 5088)]), "has_pfb": np.concatenate([snps["has_pfb"][keep], np.ones(5088, np.uint8)])}
    order = np.argsort(many["pos"], kind="stable")
    many = {k: v[order] for k, v in many.items()}
    calls = _cigar_calls()
    calls[0]["start"], calls[0]["end"] = 119_000, 126_000
    tab = _table(ctx, many)
    try:
        off = host.cn_prediction(ctx, sh, calls, hmm, res.mean_cov, many, split=False)
        for on_device in (False, True):
            _identical(host.cn_prediction(ctx, sh, calls, hmm, res.mean_cov, many, split=False, observations_on_device=on_device, snp_table=tab), off)
        assert "5087" in ctx.last_error()
        starts, ends = np.asarray([119_000, 70_000], np.uint32), np.asarray([126_000, 100_000], np.uint32)
        a = host.query_snp_regions(ctx, sh, starts, ends, res.mean_cov, 20, many)
        b = host.query_snp_regions(ctx, sh, starts, ends, res.mean_cov, 20, many, snp_table=tab)
        assert np.array_equal(a["obs_off"], b["obs_off"]) and all(a[f].tobytes() == b[f].tobytes() for f in FIELDS)
    finally:
        tab.free()


def _run_both(ctx, g, hmm, **kw):
    """-> the records of the run with the tables off; asserts that the run with the tables on gives the same ones, with
    cn_observations_on_device off and on."""
    out = None
    for on_device in (False, True):
        assert g.snp_tables_resident(False) == 0
        ref, ref_tid, st0, _ = g.run(ctx, hmm, cn_observations_on_device=on_device, **kw)
        assert g.snp_tables_resident(True) > 0
        got, tid, st, _ = g.run(ctx, hmm, cn_observations_on_device=on_device, **kw)
        assert np.array_equal(tid, ref_tid), (kw, on_device)
        _same(got, ref)
        assert got["hmm_likelihood"].tobytes() == ref["hmm_likelihood"].tobytes(), (kw, on_device)
        assert st.n_split_calls == st0.n_split_calls and st.n_cigar_cn_regions == st0.n_cigar_cn_regions
        out = out or (ref, st0)
    return out


@pytest.mark.parametrize("tech,depth", [(0, 30.0), (1, 60.0)])
def test_genome_run_on_generated_contigs(ctx, tech, depth):
    hmm = make_hmm(**WGS_HMM)
    host.set_context(ctx)
    g = _generated(ctx, tech, depth)
    try:
        ref, st0 = _run_both(ctx, g, hmm)
        assert len(ref) > 10 and st0.n_cigar_cn_regions + st0.n_split_calls > 0          # the copy-number passes had candidates
        # The tables are still on and the arenas are warm. With the remembered capacity forgotten, the first table call of a run starts
        # from capacity 1, is answered CSV_ECAPACITY behind its plan and runs again: one window group more per such call (no lanes: every
        # group of the run is on this context). The run after it reuses the remembered capacity: no extra window group.
        ctx.timing_enable(1)
        try:
            counts = []
            assert host.cn_table_capacity_hint(forget=True) > 0 and host.cn_table_capacity_hint() == 0
            for _ in range(3):
                ctx.timing_reset()
                again, _, _, _ = g.run(ctx, hmm)
                counts.append(ctx.timing()["window"][1])
                _same(again, ref)
        finally:
            ctx.timing_enable(0)
        assert host.cn_table_capacity_hint() > 0
        assert counts[1] == counts[2] > 0 and counts[1] % 2 == 0, counts                  # a plan group and a chain group per table call
        assert 1 <= counts[0] - counts[1] <= counts[1] // 2, counts                       # the forgotten capacity cost a plan group per retried call
        assert g.snp_tables_resident(False) == 0                                          # off again: freed, and the run still matches
        last, _, _, _ = g.run(ctx, hmm)
        _same(last, ref)
        assert last["hmm_likelihood"].tobytes() == ref["hmm_likelihood"].tobytes()
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
