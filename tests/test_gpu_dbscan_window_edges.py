"""The windowed DBSCAN (kernels/dbscan.hip) at its tile, split and eps edges: the families of tests/dbscan_window_inputs.py on the device
against the CPU oracle's labels, exactly. What each family reaches is asserted without a GPU in tests/test_dbscan_window_inputs.py."""
import numpy as np
import pytest

import dbscan_window_inputs as dw
from contextsv_amd import Reads

pytestmark = pytest.mark.gpu

T = dw.UF_TILE
_INTERVAL = dw.interval_cases()
_F = dw.f_cases()
_WANT = {}


def _want(oracle, case, windowed=False):
    """the oracle's labels of a case, computed once for the tests that share it"""
    name, s, e, eps, min_pts = case
    if name not in _WANT:
        _WANT[name] = (oracle.dbscan_iv_windowed if windowed else oracle.dbscan_iv)(s, e, eps, min_pts)
        _WANT[name].setflags(write=False)
    return _WANT[name]


def _assert_labels(name, s, got, want):
    assert got.shape == want.shape, name
    bad = np.flatnonzero(got != want)
    if len(bad):
        i = int(bad[0])
        pos = int(dw.sorted_position(s)[i])
        pytest.fail(f"{name}: label[{i}] = {got[i]}, oracle {want[i]}; first differing original index {i} sits at sorted position {pos} "
                    f"= {pos % T} mod {T} (tile {pos // T}); {len(bad)} of {len(want)} labels differ")


@pytest.mark.parametrize("case", _INTERVAL, ids=[c[0] for c in _INTERVAL])
def test_interval_case_matches_oracle(ctx, oracle, case):
    name, s, e, eps, min_pts = case
    _assert_labels(name, s, ctx.dbscan_iv(s, e, eps, min_pts), _want(oracle, case))


@pytest.mark.parametrize("case", _F, ids=[c[0] for c in _F])
def test_many_tiles_match_windowed_oracle(ctx, oracle, case):
    name, s, e, eps, min_pts = case
    _assert_labels(name, s, ctx.dbscan_iv(s, e, eps, min_pts), _want(oracle, case, windowed=True))


def test_batch_entry_gives_the_same_labels(ctx, oracle):
    """the sets beyond DBSCAN_IV_SMALL_MAX points through csvgpu_dbscan_iv_batch: one call per (eps, min_pts), with a 5-point set
    and an empty set between any two of them"""
    groups = {}
    for c in _INTERVAL + _F:
        if len(c[1]) > dw.DBSCAN_IV_SMALL_MAX:
            groups.setdefault((c[3], c[4]), []).append(c)
    assert len(groups) >= 6 and sum(len(g) for g in groups.values()) >= 20
    s5 = np.array([100, 110, 120, 130, 9000], np.uint32)
    e5 = s5 + 1000
    for (eps, min_pts), cases in groups.items():
        want5 = oracle.dbscan_iv(s5, e5, eps, min_pts)
        ss, ee, off = [], [], [0]
        for c in cases:
            for s, e in ((c[1], c[2]), (s5, e5), (s5[:0], e5[:0])):
                ss.append(s); ee.append(e); off.append(off[-1] + len(s))
        lab = ctx.dbscan_iv_batch(np.concatenate(ss), np.concatenate(ee), np.asarray(off, np.uint64), eps, min_pts)
        for k, c in enumerate(cases):
            a, b = off[3 * k], off[3 * k + 1]
            _assert_labels(c[0] + " (batch)", c[1], lab[a:b], _want(oracle, c, windowed=c[0].startswith("F/")))
            assert np.array_equal(lab[b:b + 5], want5), (c[0], eps, min_pts)


def _same_sigs(a, b):
    assert len(a) == len(b)
    for f in ("start", "end", "read", "qpos_kind"):
        assert np.array_equal(a[f], b[f]), f


def _shard_reads(shard):
    n = len(shard["pos"])
    return Reads.from_cigar_lists(shard["pos"], np.zeros(n, np.uint16), np.full(n, 60, np.uint8), shard["cigars"])


def _run_shard(ctx, oracle, shard, pct, min_pts):
    reads = _shard_reads(shard)
    sig = oracle.cigar_scan(reads, shard["depth_len"])
    kind = sig["qpos_kind"] & 3
    dels, inss = sig[kind == 1], sig[kind != 1]
    sh = ctx.upload(reads, shard["depth_len"])
    try:
        res = sh.pipeline(eps=0.1, min_pts_pct=pct)
        out = sh.fetch(res)
    finally:
        sh.free()
    assert res.min_pts == min_pts and (res.n_del, res.n_ins) == (shard["n_del"], shard["n_ins"])
    _same_sigs(out["sig_del"], dels); _same_sigs(out["sig_ins"], inss)
    want_del = oracle.dbscan_iv(dels["start"], dels["end"], 0.1, min_pts)
    want_ins = oracle.dbscan_iv(inss["start"], inss["end"], 0.1, min_pts)
    _assert_labels(f"{shard['name']} pct {pct!r} DEL", dels["start"], out["label_del"], want_del)
    _assert_labels(f"{shard['name']} pct {pct!r} INS", inss["start"], out["label_ins"], want_ins)
    return want_del, want_ins


@pytest.mark.parametrize("shard", dw.g_shards(), ids=[g["name"] for g in dw.g_shards()])
def test_pipeline_keeps_del_and_ins_apart(ctx, oracle, shard):
    """the DEL set's last and the INS set's first k signatures are one interval: a window that crossed the split would join them, and
    cluster ids that did not restart would number the INS set's first cluster after the DEL set's last"""
    want_del, want_ins = _run_shard(ctx, oracle, shard, 0.0, 5)
    k = shard["k"]
    assert (want_del[-k:] == (-2 if k < 5 else want_del.max())).all() and (want_ins[:k] == (-2 if k < 5 else 0)).all()


def test_pipeline_min_pts_from_coverage(ctx, oracle):
    """min_pts = ceil(mean coverage * pct) read on the device: k makes the planted signatures clusters, k + 1 noise"""
    shard = dw.g_shards()[0]
    k = shard["k"]
    _, dsum, dnz = oracle.depth(_shard_reads(shard), shard["depth_len"])
    mean = dsum / dnz
    for min_pts in (k, k + 1):
        pct = dw.g_pct_for(mean, min_pts)
        assert pct > 0 and int(np.ceil(mean * pct)) == min_pts
        want_del, want_ins = _run_shard(ctx, oracle, shard, pct, min_pts)
        assert (want_del[-k:] >= 0).all() == (min_pts == k) and (want_ins[:k] >= 0).all() == (min_pts == k)


@pytest.mark.parametrize("hset", dw.h_sets(), ids=[h[0] for h in dw.h_sets()])
def test_1d_segment_above_the_lds_cap(ctx, oracle, hset):
    name, pts, off = hset
    n, m = int(off[1]), dw.DBSCAN1D_MAX_SEG
    for eps in dw.H_EPS:
        for min_pts in dw.H_MIN_PTS:
            lab = ctx.dbscan_1d(pts, off, eps, min_pts)
            big, small = oracle.dbscan_1d(pts[:n], eps, min_pts), oracle.dbscan_1d(pts[:m], eps, min_pts)
            bad = np.flatnonzero(lab[:n] != big)
            assert len(bad) == 0, f"{name} eps {eps!r} min_pts {min_pts}: label[{bad[0]}] = {lab[bad[0]]}, oracle {big[bad[0]]}; {len(bad)} of {n} differ"
            assert np.array_equal(lab[n:], small), (name, eps, min_pts)
            # the same 512 points fitted alone (the LDS kernel both times): the large segment in front changes nothing
            assert np.array_equal(ctx.dbscan_1d(pts[:m], np.array([0, m], np.uint64), eps, min_pts), lab[n:]), (name, eps, min_pts)
