"""Batches beyond the grid caps of dbscan1d_kernel, sf_fits_kernel and the two small-set interval kernels (tests/large_batches.py): every
wave (workgroup) takes a second and a third set and starts on them with the LDS the set before left — large behind small, small behind
large, behind an empty set, behind one that went to the large-set path (tests/test_large_batches_inputs.py asserts the batches hold
such pairs). Every set of every batch against the oracle, exactly; a failure names the set and the one W items in front of it."""
import numpy as np
import pytest

import large_batches as lb
from contextsv_amd import host
from test_gpu_split_fits import _same_records, _tables
from test_split_fits_ref import expected

pytestmark = pytest.mark.gpu


def _same_labels(got, want, off, W, what):
    if np.array_equal(got, want):
        return
    sizes = np.diff(off.astype(np.int64))
    bad = np.unique(np.searchsorted(off.astype(np.int64), np.flatnonzero(got != want), side="right") - 1)
    k = int(bad[0])
    a, b = int(off[k]), int(off[k + 1])
    raise AssertionError("%s: %d of %d sets differ, first %d (%d points; the set before it on its wave, %d: %s points): got %s, want %s"
                         % (what, len(bad), len(sizes), k, sizes[k], k - W, lb.predecessor_size(sizes, k, W), got[a:b][:16], want[a:b][:16]))


@pytest.mark.parametrize("eps,min_pts", [(100.0, 5), (10.0, 2), (0.0, 1)])
def test_dbscan_1d_batch_of_four_trips(ctx, oracle, eps, min_pts):
    pts, off = lb.dbscan1d_batch()
    _same_labels(ctx.dbscan_1d(pts, off, eps, min_pts), lb.dbscan1d_want(oracle, eps, min_pts), off, lb.W_DBSCAN1D, "dbscan_1d%s" % ((eps, min_pts),))


def test_dbscan_1d_batch_three_launch_sort(ctx, oracle):
    pts, off = lb.dbscan1d_batch()
    ctx.set_tuning(sort_three_launch=True)                   # the segments beyond 512 points are sorted by the other radix sort
    try:
        got = ctx.dbscan_1d(pts, off, 100.0, 5)
    finally:
        ctx.set_tuning()
    _same_labels(got, lb.dbscan1d_want(oracle, 100.0, 5), off, lb.W_DBSCAN1D, "dbscan_1d, three-launch sort")


def _same_fits(got, want, what):
    try:
        _same_records(got, want, what)
    except AssertionError as err:
        sizes, W = lb.split_set_sizes(), lb.W_SPLIT_FITS
        g = next(g for g in range(len(want)) if got[g].tobytes() != want[g].tobytes())
        sets = [s for s in range(6) if got["median"][g, s] != want["median"][g, s] or got["size"][g, s] != want["size"][g, s]]
        items = ", ".join("item %d (%d points) behind item %d (%s points)" % (6 * g + s, sizes[6 * g + s], 6 * g + s - W, lb.predecessor_size(sizes, 6 * g + s, W))
                          for s in sets)
        raise AssertionError("%s; group %d: %s" % (err, g, items or "the strand vote")) from None


def test_split_fits_given_groups(ctx, oracle):
    t, off, groups = lb.split_fits_batch()
    want = lb.split_fits_want(oracle, 100.0, 5)
    ctx.timing_enable(1)
    try:
        ctx.timing_reset()
        sgo, got = ctx.split_fits(_tables(t), off, groups)
        tm = ctx.timing()
    finally:
        ctx.timing_enable(0)
    _same_fits(got, want, "given groups")
    assert (lb.split_set_sizes() > lb.D1_CAP).any()
    assert tm["split_fits"][1] == 2 and tm["dbscan1d"][1] == 0      # the LDS kernel's launch, and the large sets' as one more group


def test_split_fits_fused(ctx, oracle):
    t, off, groups = lb.split_fits_batch()
    want = lb.split_fits_want(oracle, 100.0, 5)
    ctx.timing_enable(1)
    try:
        ctx.timing_reset()
        sgo, got = ctx.split_fits(_tables(t), off)
        tm = ctx.timing()
    finally:
        ctx.timing_enable(0)
    assert np.array_equal(sgo, groups[0])
    _same_fits(got, want, "fused")
    assert tm["split_fits"][1] == 2 and tm["split_groups"][1] >= 1 and tm["dbscan1d"][1] == 0


def test_split_fits_host_route(ctx, oracle):
    """The same batch as the pass sends it without the option: one csvgpu_dbscan_1d call of 6 x groups segments, those beyond 512 points
    in between."""
    t, off, groups = lb.split_fits_batch()
    _same_fits(host.split_fits_host(ctx, _tables(t), off, groups), lb.split_fits_want(oracle, 100.0, 5), "host route")


def test_split_fits_other_eps_and_min_pts(ctx, oracle):
    t, off, groups = lb.split_fits_batch()
    want = lb.split_fits_want(oracle, 25.0, 3)
    _same_fits(ctx.split_fits(_tables(t), off, groups, eps=25.0, min_pts=3)[1], want, "given groups, (25, 3)")
    sgo, got = ctx.split_fits(_tables(t), off, eps=25.0, min_pts=3)
    assert np.array_equal(sgo, groups[0])
    _same_fits(got, want, "fused, (25, 3)")


@pytest.mark.parametrize("eps,min_pts", [(0.1, 2), (0.3, 5)])
def test_interval_batch_of_three_trips(ctx, oracle, eps, min_pts):
    s, e, off = lb.interval_batch()
    want = lb.interval_want(oracle, eps, min_pts)
    _same_labels(ctx.dbscan_iv_batch(s, e, off, eps, min_pts), want, off, lb.W_INTERVAL, "dbscan_iv_batch%s" % ((eps, min_pts),))
    ctx.set_tuning(dbscan_all_pairs=True)
    try:
        got = ctx.dbscan_iv_batch(s, e, off, eps, min_pts)
    finally:
        ctx.set_tuning()
    _same_labels(got, want, off, lb.W_INTERVAL, "dbscan_iv_batch%s, all pairs" % ((eps, min_pts),))


def test_context_is_usable_after_the_large_calls(ctx, oracle):
    """The arena and the page-locked block have grown for the batches above; a small family afterwards, every way."""
    pts, off = lb.dbscan1d_batch()
    ctx.dbscan_1d(pts, off, 100.0, 5)                         # (so that this test does not depend on the ones above having run)
    t, off, groups, want = expected(oracle, "mixed24")
    _same_records(ctx.split_fits(_tables(t), off, groups)[1], want, "mixed24 after the large batches")
    sgo, fused = ctx.split_fits(_tables(t), off)
    assert np.array_equal(sgo, groups[0])
    _same_records(fused, want, "mixed24 after the large batches, fused")
    _same_records(host.split_fits_host(ctx, _tables(t), off, groups), want, "mixed24 after the large batches, host route")
