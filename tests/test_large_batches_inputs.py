"""The batches of tests/large_batches.py are not vacuous: from set sizes and reference answers alone (no GPU), the pairs of items that
share a wave of the capped grids — item w and item w + W — hold what tests/test_gpu_large_batches.py is there to run: large sets in front
of small ones and the other way round, sets behind empty ones, and behind every set that is too large for LDS a set that is not.
The caps themselves are read from the launch functions, so a cap that moves fails here instead of leaving the pairs W apart by an
old W."""
import os
import re

import numpy as np
import pytest

import large_batches as lb
from test_split_groups_host import reference_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_PAIRS = 200


def _kernel_source(name):
    return open(os.path.join(ROOT, "contextsv_amd", "csrc", "kernels", name)).read()


def _int(pattern, text):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1))


def test_w_is_what_the_launch_functions_cap_their_grids_at():
    d1 = _kernel_source("dbscan1d.hip")
    launch = d1[d1.index("void launch_dbscan_1d_batched"):]
    cap = _int(r"if \(want > (\d+)\) want = (?:\d+);", launch)
    waves = _int(r"constexpr int D1_THREADS = (\d+);", d1) // 64
    assert "(n_seg + D1_WAVES - 1) / D1_WAVES" in launch and cap * waves == lb.W_DBSCAN1D
    sf = _kernel_source("splitfits.hip")
    launch = sf[sf.index("void launch_sf_fits"):]
    cap = _int(r"if \(want > (\d+)\) want = (?:\d+);", launch)
    waves = _int(r"constexpr int SF_THREADS = (\d+);", sf) // 64
    assert "n_groups * 6 + SF_WAVES - 1) / SF_WAVES" in launch and cap * waves == lb.W_SPLIT_FITS
    iv = _kernel_source("dbscan.hip")
    launch = iv[iv.index("void launch_dbscan_iv_small_batched"):]
    assert _int(r"std::min<uint64_t>\(n_seg, (\d+)\)", launch) == lb.W_INTERVAL
    common = open(os.path.join(ROOT, "contextsv_amd", "csrc", "common.hpp")).read()
    assert _int(r"constexpr uint32_t DBSCAN1D_MAX_SEG = (\d+);", common) == lb.D1_CAP
    assert _int(r"constexpr uint32_t DBSCAN_IV_SMALL_MAX = (\d+);", common) == lb.IV_CAP


def _check_pairs(sizes, W, cap, min_trips):
    st = lb.pair_stats(sizes, W, cap)
    assert len(sizes) >= min_trips * W
    assert st["large_small"] >= MIN_PAIRS, st["large_small"]
    assert st["small_large"] >= MIN_PAIRS, st["small_large"]
    assert st["after_empty"] >= MIN_PAIRS, st["after_empty"]
    assert len(st["oversize_with_successor"]) >= 1 and st["successors_in_lds"]
    return st


def test_dbscan1d_batch():
    pts, off = lb.dbscan1d_batch()
    W = lb.W_DBSCAN1D
    sizes = np.diff(off.astype(np.int64))
    assert len(sizes) >= 3 * W + 1000 and 800_000 <= len(pts) <= 1_500_000 and pts.dtype == np.int32
    assert (sizes <= 64).mean() > 0.95 and ((sizes >= 200) & (sizes <= 512)).sum() >= 200 and {0, 1, 511, 512, 513} <= set(sizes.tolist())
    st = _check_pairs(sizes, W, lb.D1_CAP, 3)
    over = st["oversize"]
    assert len(over) >= 3 and (over < W).any() and (over >= W).any() and len(st["oversize_with_successor"]) == len(over)
    # sets over the whole int32 range, and sets with cores, borders and noise (the offsets 0 / 300 / 5000 of a base)
    o = off.astype(np.int64)
    spans = np.array([int(pts[o[k]:o[k + 1]].max()) - int(pts[o[k]:o[k + 1]].min()) for k in np.flatnonzero(sizes >= 8)])
    assert (spans > 2**31).sum() >= 100 and (spans < 6000).sum() >= 10_000


def test_interval_batch(oracle):
    s, e, off = lb.interval_batch()
    W = lb.W_INTERVAL
    sizes = np.diff(off.astype(np.int64))
    assert len(sizes) >= 2 * W + 3000 and (sizes <= 40).mean() > 0.9 and (sizes == 0).sum() >= 100
    assert ((sizes >= 300) & (sizes <= 2048)).sum() >= len(sizes) // 64 and {2047, 2048} <= set(sizes.tolist())
    st = _check_pairs(sizes, W, lb.IV_CAP, 2)
    over = st["oversize"]
    assert len(over) >= 2 and (sizes[over] >= 2049).all() and (over < W).any() and (over >= W).any() and len(st["oversize_with_successor"]) == len(over)
    # clustered, border and noise labels all occur: a border point has a cluster's label without min_pts neighbours of its own
    eps, min_pts = 0.3, 5
    want = lb.interval_want(oracle, eps, min_pts)
    assert (want >= 0).sum() >= 1000 and (want == -2).sum() >= 1000 and not ((want < 0) & (want != -2)).any()
    o = off.astype(np.int64)
    cores = borders = 0
    for k in np.flatnonzero((sizes >= 5) & (sizes <= 40))[:2000]:
        n_nb = lb.interval_neighbour_counts(s[o[k]:o[k + 1]], e[o[k]:o[k + 1]], eps)
        lab = want[o[k]:o[k + 1]]
        assert (lab[n_nb >= min_pts] >= 0).all()
        cores += int((n_nb >= min_pts).sum())
        borders += int(((lab >= 0) & (n_nb < min_pts)).sum())
    assert cores >= 100 and borders >= 100, (cores, borders)


def test_interval_batch_windowed_sets(oracle):
    """The sets beyond 2048 points take the windowed path on the device; the windowed oracle gives them the literal one's labels."""
    s, e, off = lb.interval_batch()
    o = off.astype(np.int64)
    for eps, min_pts in ((0.1, 2), (0.3, 5)):
        for k in np.flatnonzero(np.diff(o) > lb.IV_CAP):
            sk, ek = s[o[k]:o[k + 1]], e[o[k]:o[k + 1]]
            assert np.array_equal(oracle.dbscan_iv_windowed(sk, ek, eps, min_pts), oracle.dbscan_iv(sk, ek, eps, min_pts)), (k, eps, min_pts)


def test_split_fits_batch(oracle):
    t, off, groups = lb.split_fits_batch()
    W = lb.W_SPLIT_FITS
    sgo, go, mem = groups
    n_groups, n_seg = len(go) - 1, len(off) - 1
    assert n_groups >= 8400 and 6 * n_groups >= 3 * W and n_seg >= 500 and n_groups == int(sgo[-1])
    # empty segments, and segments with members but no group: at least 100 of each, at the front, in the middle and at the end
    seg_len, seg_groups = np.diff(off.astype(np.int64)), np.diff(sgo.astype(np.int64))
    for kind in (seg_len == 0, (seg_len > 0) & (seg_groups == 0)):
        where = np.flatnonzero(kind)
        assert len(where) >= 100 and where[0] < 2 and where[-1] >= n_seg - 2 and ((where > n_seg // 3) & (where < 2 * n_seg // 3)).any()
    n_mem = np.diff(go.astype(np.int64))
    assert ((n_mem >= 2) & (n_mem <= 8)).mean() > 0.9 and abs(((n_mem >= 200) & (n_mem <= 500)).sum() * 40 - n_groups) <= n_groups // 10
    sizes = lb.split_set_sizes()
    assert len(sizes) == 6 * n_groups and np.array_equal(sizes[0::6], n_mem) and np.array_equal(sizes[1::6], n_mem)
    assert ((n_mem == 200) & (sizes[2::6] > lb.D1_CAP) & (sizes[4::6] > lb.D1_CAP)).sum() >= 3       # 200 members, three records each
    st = _check_pairs(sizes, W, lb.D1_CAP, 3)
    assert len(st["oversize_with_successor"]) >= 10 and len(set((st["oversize_with_successor"] % 6).tolist())) >= 2
    # the rule of test_split_fits_ref.py::test_families_are_not_vacuous, on the reference's answers
    want = lb.split_fits_want(oracle, 100.0, 5)
    assert len(want) == n_groups and np.array_equal(want["n_members"], n_mem)
    for k in range(6):
        assert (want["size"][:, k] > 0).sum() * 10 >= n_groups, k
        assert (want["size"][:, k] == 0).any(), k
    assert (want["n_opposite"] * 2 > want["n_members"]).sum() >= 100 and (want["n_opposite"] == 0).sum() >= 100


@pytest.mark.parametrize("where", ["front", "middle", "end"])
def test_split_fits_batch_groups_are_the_restatements(where):
    """The batch takes its groups from the host tree; on slices of it they are the literal restatement's, whole segments at a time."""
    t, off, (sgo, go, mem) = lb.split_fits_batch()
    n_seg = len(off) - 1
    a = {"front": 0, "middle": n_seg // 2, "end": n_seg - 150}[where]
    b = a + 150
    o, g = off.astype(np.int64), sgo.astype(np.int64)
    wsgo, wgo, wmem = reference_groups(t["start"][o[a]:o[b]], t["end"][o[a]:o[b]], off[a:b + 1] - off[a])
    assert int(wsgo[-1]) >= 300
    assert np.array_equal(wsgo, sgo[a:b + 1] - sgo[a])
    assert np.array_equal(wgo, go[g[a]:g[b] + 1] - go[g[a]])
    assert np.array_equal(wmem, mem[int(go[g[a]]):int(go[g[b]])])
