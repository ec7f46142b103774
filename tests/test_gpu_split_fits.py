"""csvgpu_split_fits / csvgpu_split_groups_fits (Context.split_fits): the evidence of every overlap group — strand vote, six point sets, their
DBSCAN1D fits, largest clusters, medians — computed on the device, against the literal restatement of the reference kept in
tests/test_split_fits_ref.py. Every comparison is of the 64-byte records, byte for byte, on every input family of that file: groups given
(from the restatement, from the host tree, from csvgpu_split_groups) and groups computed and consumed on the device (the fused call),
sets beyond the LDS kernel's 512 points included."""
import ctypes as C

import numpy as np
import pytest

import contextsv_amd as cs
from contextsv_amd import host
from contextsv_amd._lib import CSV_EINVAL, SPLIT_FIT_DTYPE, ptr
from test_split_fits_ref import EPS, FAMILIES, MIN_PTS, expected, one_group, reference_fits, tables_of

pytestmark = pytest.mark.gpu


def _tables(t):
    return cs.SplitTables(**t)


def _same_records(got, want, what):
    assert got.dtype == SPLIT_FIT_DTYPE and len(got) == len(want), what
    if got.tobytes() != want.tobytes():
        bad = [g for g in range(len(want)) if got[g].tobytes() != want[g].tobytes()]
        raise AssertionError("%s: %d of %d records differ, first %d: got %s, want %s" % (what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]]))


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_families_match_reference_every_way(ctx, oracle, name):
    t, off, groups, want = expected(oracle, name)
    T = _tables(t)
    sgo, got = ctx.split_fits(T, off, groups)
    _same_records(got, want, name + ": given groups")
    on_host = host.split_groups_host(t["start"], t["end"], off)
    _same_records(ctx.split_fits(T, off, on_host)[1], want, name + ": host tree's groups")
    on_dev = ctx.split_groups(t["start"], t["end"], off)
    assert all(np.array_equal(a, b) for a, b in zip(on_dev, groups))
    _same_records(ctx.split_fits(T, off, on_dev)[1], want, name + ": csvgpu_split_groups' groups")
    sgo, fused = ctx.split_fits(T, off)
    assert np.array_equal(sgo, groups[0])
    _same_records(fused, want, name + ": fused")


@pytest.mark.parametrize("seed", [2, 3])
def test_more_seeds_of_the_mixed_and_oversize_families(ctx, oracle, seed):
    for name in ("mixed24", "multi_supp", "oversize") if seed == 2 else ("mixed24", "duplicates"):
        t, off, groups, want = expected(oracle, name, seed)
        _same_records(ctx.split_fits(_tables(t), off, groups)[1], want, name)
        sgo, fused = ctx.split_fits(_tables(t), off)
        assert np.array_equal(sgo, groups[0])
        _same_records(fused, want, name + ": fused")


def test_other_eps_and_min_pts(ctx, oracle):
    t, off, groups, _ = expected(oracle, "multi_supp")
    for eps, min_pts in ((0.0, 1), (25.0, 3), (5000.0, 40)):
        want = reference_fits(oracle, t, off, groups, eps, min_pts)
        _same_records(ctx.split_fits(_tables(t), off, groups, eps=eps, min_pts=min_pts)[1], want, (eps, min_pts))
        _same_records(ctx.split_fits(_tables(t), off, eps=eps, min_pts=min_pts)[1], want, (eps, min_pts, "fused"))


def test_host_route_gives_the_same_records(ctx, oracle):
    """host.split_fits_host — the sets and reductions the pass does on the host without the option, around one csvgpu_dbscan_1d batch —
    is what tools/bench_split_fits.py measures the device entry points against."""
    for name in ("mixed24", "multi_supp", "no_same_tid"):
        t, off, groups, want = expected(oracle, name)
        _same_records(host.split_fits_host(ctx, _tables(t), off, groups), want, name + ": host route")


def test_empty_calls(ctx):
    z = tables_of([])
    for off in (np.zeros(1, np.uint64), np.zeros(4, np.uint64)):
        n_seg = len(off) - 1
        sgo, fits = ctx.split_fits(_tables(z), off)
        assert sgo.tolist() == [0] * (n_seg + 1) and len(fits) == 0
        sgo, fits = ctx.split_fits(_tables(z), off, (np.zeros(n_seg + 1, np.uint64), np.zeros(1, np.uint64), np.zeros(0, np.uint32)))
        assert len(fits) == 0
    # members, but no segment with two of them / no overlap: no group
    t = tables_of([(10, 20, 0, 5, 0, []), (100, 200, 0, 5, 1, [(5, 6, 7, 8, 0)]), (300, 400, 0, 5, 0, [])])
    sgo, fits = ctx.split_fits(_tables(t), np.array([0, 1, 1, 2, 3], np.uint64))
    assert sgo.tolist() == [0, 0, 0, 0, 0] and len(fits) == 0
    sgo, fits = ctx.split_fits(_tables(t), np.array([0, 3], np.uint64))
    assert sgo.tolist() == [0, 0] and len(fits) == 0


def _raises_einval(f):
    with pytest.raises(cs.CsvError) as ei:
        f()
    assert ei.value.status == CSV_EINVAL


def test_invalid_input_and_the_context_afterwards(ctx, oracle):
    mem = [(100 + i, 5000, 0, 4000, 0, [(20000 + i, 23000, 4100, 7000, 0)]) for i in range(6)]
    t, off, groups = one_group(mem)
    want = reference_fits(oracle, t, off, groups)

    def changed(**kw):
        d = dict(t)
        for k, (i, v) in kw.items():
            d[k] = d[k].copy()
            d[k][i] = v
        return _tables(d)

    for bad in (changed(start=(2, -1)), changed(end=(2, 50)), changed(q_start=(0, -5)), changed(q_end=(5, -1)), changed(supp_start=(1, -7)),
                changed(supp_end=(1, 3)), changed(supp_q_start=(3, -1)), changed(supp_q_end=(3, -2)), changed(supp_off=(3, 1)), changed(supp_off=(6, 5))):
        _raises_einval(lambda: ctx.split_fits(bad, off, groups))
        _raises_einval(lambda: ctx.split_fits(bad, off))
    # a record on another tid may hold anything but its flags
    other = changed(supp_flags=(1, 2), supp_start=(1, -7), supp_end=(1, -9))
    assert ctx.split_fits(other, off, groups)[1]["size"].tolist() == [[6, 6, 5, 5, 5, 5]]
    T = _tables(t)
    _raises_einval(lambda: ctx.split_fits(T, np.array([0, 5], np.uint64), groups))                      # seg_off does not end at n_members
    _raises_einval(lambda: ctx.split_fits(T, np.array([0, 5], np.uint64)))
    _raises_einval(lambda: ctx.split_fits(T, np.array([0, 7, 6], np.uint64)))                           # not ascending
    sgo, go, m = groups
    _raises_einval(lambda: ctx.split_fits(T, off, (sgo, go, np.array([0, 1, 2, 3, 4, 6], np.uint32))))    # member outside its segment
    _raises_einval(lambda: ctx.split_fits(T, np.array([0, 3, 6], np.uint64), (np.array([0, 2, 1], np.uint64), go, m)))     # seg_group_off not ascending
    _raises_einval(lambda: ctx.split_fits(T, off, (sgo, go, np.array([0, 1, 2, 3, 4, 0], np.uint32))))    # a member twice in one group
    two = (np.array([0, 2], np.uint64), np.array([0, 3, 6], np.uint64), np.array([0, 1, 2, 2, 3, 0], np.uint32))   # ... in two groups: fine
    assert ctx.split_fits(T, off, two)[1]["n_members"].tolist() == [3, 3]
    _raises_einval(lambda: ctx.split_fits(T, off, (np.array([0, 2], np.uint64), np.array([0, 4, 2], np.uint64), m)))       # group_off not ascending
    for eps, min_pts in ((-1.0, 5), (float("nan"), 5), (100.0, 0)):
        _raises_einval(lambda: ctx.split_fits(T, off, groups, eps=eps, min_pts=min_pts))
        _raises_einval(lambda: ctx.split_fits(T, off, eps=eps, min_pts=min_pts))
    # null arrays at the raw entry points
    ts, out, n = T.c_struct(), np.zeros(6, SPLIT_FIT_DTYPE), C.c_uint64(0)
    assert ctx.lib.csvgpu_split_fits(ctx.h, None, ptr(off), 1, ptr(sgo), ptr(go), ptr(m), EPS, MIN_PTS, ptr(out)) == CSV_EINVAL
    assert ctx.lib.csvgpu_split_fits(ctx.h, C.byref(ts), ptr(off), 1, ptr(sgo), ptr(go), ptr(m), EPS, MIN_PTS, None) == CSV_EINVAL
    assert ctx.lib.csvgpu_split_fits(ctx.h, C.byref(ts), ptr(off), 1, ptr(sgo), None, ptr(m), EPS, MIN_PTS, ptr(out)) == CSV_EINVAL
    assert ctx.lib.csvgpu_split_groups_fits(ctx.h, C.byref(ts), ptr(off), 1, EPS, MIN_PTS, None, ptr(out), C.byref(n)) == CSV_EINVAL
    assert ctx.lib.csvgpu_split_groups_fits(ctx.h, C.byref(ts), ptr(off), 1, EPS, MIN_PTS, ptr(sgo.copy()), None, C.byref(n)) == CSV_EINVAL
    ts.supp_flags = None
    assert ctx.lib.csvgpu_split_fits(ctx.h, C.byref(ts), ptr(off), 1, ptr(sgo), ptr(go), ptr(m), EPS, MIN_PTS, ptr(out)) == CSV_EINVAL
    # the context is usable afterwards, both ways
    _same_records(ctx.split_fits(T, off, groups)[1], want, "after the errors")
    _same_records(ctx.split_fits(T, off)[1], want, "after the errors, fused")


def test_pending_split_order_is_refused(ctx, oracle):
    t, off, groups, want = expected(oracle, "no_same_tid")
    reads = cs.Reads.from_cigar_lists([1, 2, 3], [0, 0, 0x800], [60, 60, 60], [[(0, 10)]] * 3)
    sh = ctx.upload(reads, 100)
    try:
        sh.set_qname_hash(np.array([5, 9, 5], np.uint64))
        hs = (C.c_void_p * 1)(sh.h)
        assert ctx.lib.csvgpu_split_order_begin(ctx.h, 1, hs, 20) == 0
        try:
            _raises_einval(lambda: ctx.split_fits(_tables(t), off, groups))
            _raises_einval(lambda: ctx.split_fits(_tables(t), off))
        finally:
            out_rec, out_off = np.zeros(8, np.uint32), np.zeros(2, np.uint64)
            supp = np.array([5], np.uint64)
            assert ctx.lib.csvgpu_split_order_finish(ctx.h, ptr(supp), 1, ptr(out_rec), 8, ptr(out_off)) == 0
        assert out_off.tolist() == [0, 1] and out_rec[0] == 0
    finally:
        sh.free()
    _same_records(ctx.split_fits(_tables(t), off)[1], want, "after the order")


def test_timing_counts_the_launches(ctx, oracle):
    t, off, groups, _ = expected(oracle, "duplicates")
    ctx.timing_enable(1)
    try:
        ctx.timing_reset()
        ctx.split_fits(_tables(t), off, groups)
        tm = ctx.timing()
        assert tm["split_fits"][1] == 1 and tm["split_groups"][1] == 0 and tm["dbscan1d"][1] == 0
        ctx.timing_reset()
        ctx.split_fits(_tables(t), off)
        tm = ctx.timing()
        assert tm["split_fits"][1] == 1 and tm["split_groups"][1] >= 1 and tm["dbscan1d"][1] == 0
        # oversize sets: the large-set path is one more launch group of the same kernel id
        t, off, groups, _ = expected(oracle, "oversize")
        ctx.timing_reset()
        ctx.split_fits(_tables(t), off, groups)
        tm = ctx.timing()
        assert tm["split_fits"][1] == 2 and tm["dbscan1d"][1] == 0
    finally:
        ctx.timing_enable(0)
