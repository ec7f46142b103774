"""The inputs of tests/dbscan_window_inputs.py hold what they claim (no GPU): the module's constants are the kernels', the two CPU
oracles (and the reference's own code where it is built) agree on every case, and each family's structural claim — what makes it reach
an edge of kernels/dbscan.hip — follows from the oracle's labels and the numpy window model."""
import os
import re

import numpy as np
import pytest

import dbscan_window_inputs as dw
import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "contextsv_amd", "csrc")
T = dw.UF_TILE


def _int(pattern, text):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1))


def test_constants_are_the_kernels():
    """a retune of the tile, the halo, the lane group or a cap has to move the module's edges with it"""
    iv = open(os.path.join(CSRC, "kernels", "dbscan.hip")).read()
    assert _int(r"constexpr int UF_TILE = (\d+);", iv) == dw.UF_TILE
    assert _int(r"constexpr int DB_HALO = (\d+);", iv) == dw.DB_HALO
    assert _int(r"constexpr int DB_G = (\d+);", iv) == dw.DB_G
    common = open(os.path.join(CSRC, "common.hpp")).read()
    assert _int(r"constexpr uint32_t DBSCAN_IV_SMALL_MAX = (\d+);", common) == dw.DBSCAN_IV_SMALL_MAX
    assert _int(r"constexpr uint32_t DBSCAN1D_MAX_SEG = (\d+);", common) == dw.DBSCAN1D_MAX_SEG
    # the cases sit where these constants put the edges
    assert dw.A_N > dw.DBSCAN_IV_SMALL_MAX and dw.B_BLOCKS * T > dw.DBSCAN_IV_SMALL_MAX and dw.E_RANDOM_N > dw.DBSCAN_IV_SMALL_MAX
    assert {T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T, dw.B_BLOCKS * T} == set(dw.B_CUTS)
    assert dw.F_SIZES == (T * T, T * T + 1, 2 * T * T)
    assert all(n > dw.DBSCAN1D_MAX_SEG for n in dw.H_SIZES) and {4 * T, 6 * T + 1} <= set(dw.H_SIZES)
    assert [d for d, _, _ in dw.G_SHARDS[:3]] == [T - 1, T, T + 1]


@pytest.fixture(scope="module")
def live_ref():
    return oracle_lib.load_ref()


_CASES = dw.interval_cases()


def test_case_names_are_unique_and_orders_differ():
    names = [c[0] for c in _CASES + dw.f_cases()]
    assert len(set(names)) == len(names)
    for name, s, e, eps, min_pts in _CASES + dw.f_cases():
        is_sorted = bool((np.diff(s.astype(np.int64)) >= 0).all())
        assert len(s) < 8 or is_sorted == (not name.endswith("/perm") and name not in ("C/planted",) and not re.fullmatch(r"E/(planted|random)/eps[^/]*", name)), name
        assert 0.0 <= eps < 1.0 and min_pts >= 1 and int(e.max()) < 2**31 and (e > s).all()


@pytest.mark.parametrize("case", _CASES, ids=[c[0] for c in _CASES])
def test_oracles_agree(oracle, live_ref, case):
    name, s, e, eps, min_pts = case
    want = oracle.dbscan_iv(s, e, eps, min_pts)
    assert np.array_equal(oracle.dbscan_iv_windowed(s, e, eps, min_pts), want)
    if live_ref is not None:
        assert np.array_equal(live_ref.dbscan_iv(s, e, eps, min_pts), want)


def _by_name(name):
    return next(c for c in _CASES if c[0] == name)


def test_a_spans_tiles_and_sits_at_the_core_threshold(oracle):
    name, s, e, eps, _ = _by_name("A/min_pts5")
    fwd, bwd = dw.window_candidates(s, e, eps)
    assert fwd.max() <= dw.DB_HALO and bwd.max() <= dw.DB_HALO            # (windows stay inside the halo: this family is about the unions)
    lab = oracle.dbscan_iv(s, e, eps, 5)
    assert (lab == 0).all() and dw.tiles_spanned(s, lab)[0] >= 16
    n_nb = np.array([len(x) for x in dw.neighbour_lists(s[:200], e[:200], eps)])
    assert (n_nb[10:190] == 21).all() and n_nb[0] == 11                    # 10 either side and itself
    lab21 = oracle.dbscan_iv(s, e, eps, 21)
    assert (lab21 == 0).all()                                             # the 10 points at either end: borders of the one cluster
    assert (oracle.dbscan_iv(s, e, eps, 22) == -2).all()
    name, sp, ep, _, _ = _by_name("A/min_pts21/perm")
    labp = oracle.dbscan_iv(sp, ep, eps, 21)
    assert (labp == 0).all() and not (np.diff(sp.astype(np.int64)) >= 0).all()


def test_b_tiles_hang_by_single_pairs(oracle):
    name, s, e, eps, mp = dw.b_linked()
    n = len(s)
    nb = dw.neighbour_lists(s, e, eps)
    for k in range(1, dw.B_BLOCKS):
        last, first = k * T - 1, k * T
        crossing = [(i, int(j)) for i in range(last - 12, last + 1) for j in nb[i] if j >= first]
        assert crossing == [(last, first)], (k, crossing)                # one pair, and it straddles the tile border
    lab = oracle.dbscan_iv(s, e, eps, mp)
    assert (lab == 0).all()
    cut = np.ones(n, bool)
    cut[T] = False                                                        # without the second block's first point ...
    lab_cut = oracle.dbscan_iv(s[cut], e[cut], eps, mp)
    assert set(lab_cut[: T].tolist()) == {0} and set(lab_cut[T:].tolist()) == {1}      # ... the chain falls apart there
    name, s1, e1, _, _ = dw.b_unlinked()
    assert np.array_equal(oracle.dbscan_iv(s1, e1, eps, mp), np.arange(n) // T)        # gap 101: one cluster per block
    name, s2, e2, _, _ = dw.b_shifted()
    lab2 = oracle.dbscan_iv(s2, e2, eps, mp)
    assert lab2[0] == -2 and (lab2[1:] == 0).all()
    nb2 = dw.neighbour_lists(s2, e2, eps)
    assert all(int(nb2[k * T].max()) == k * T + 1 and (k * T) // T == (k * T + 1) // T for k in range(1, dw.B_BLOCKS))     # links inside tiles
    for n_cut in dw.B_CUTS:
        assert len(dw.b_linked(n_cut)[1]) == n_cut


@pytest.mark.parametrize("which", ["planted", "sorted"])
def test_c_every_border_rule_decides(oracle, which):
    (name, s, e, eps, mp), inst = dw.c_planted() if which == "planted" else dw.c_sorted()
    lab = oracle.dbscan_iv(s, e, eps, mp)
    pos = dw.sorted_position(s)
    nb = dw.neighbour_lists(s, e, eps)
    decided = {}
    for it in inst:
        a, b, bb = it["a"], it["b"], it["bb"]
        a_end, b_end = a[-1], bb[0]                                      # the ends next to b
        assert sorted(nb[b].tolist()) == sorted([int(a_end), b, int(b_end)]) and len(nb[b]) < mp          # b: no core, two core neighbours
        assert pos[b] % T == it["place"] and pos[a_end] == pos[b] - 1 and pos[b_end] == pos[b] + 1
        la, lb = int(lab[a[0]]), int(lab[bb[0]])
        assert la >= 0 and lb >= 0 and la != lb and (lab[a] == la).all() and (lab[bb] == lb).all()
        a_is_start, b_is_start = a_end == a.min(), b_end == bb.min()     # start point: the cluster's smallest original index
        if not a_is_start and not b_is_start:
            rule, want = "neither", min(la, lb)
        elif a_is_start and b_is_start:
            rule, want = "both", max(la, lb)
        else:
            rule = "larger"
            want = la if a_is_start else lb
            assert want == max(la, lb) and want > min(la, lb)            # the start point's id is the larger one: min-of-cores would miss
        assert int(lab[b]) == want, (it, la, lb, int(lab[b]))
        decided.setdefault(rule, set()).add((it["place"], want == la))
    if which == "planted":
        for rule in dw.C_SCENARIOS:                                     # each rule at each placement, with either cluster the winner
            assert decided[rule] == {(p, w) for p in dw.C_PLACEMENTS for w in (False, True)}, rule
    else:
        assert set(decided) == {"larger"}                                # in start order B's end is always B's start point


def test_d_pairs_either_side_of_the_threshold():
    seen_pad = {"fwd": 0, "bwd": 0}
    for eps in dw.D_EPS:
        parts = dw.d_parts(eps)
        all_rows = {(r[0], r[1], r[2]) for rows in parts for r in rows}
        n_acc = n_rej = 0
        for part, rows in enumerate(parts):
            name, s, e, _, _ = dw.d_case(eps, part)
            assert len(s) == 2 * len(rows) and (np.diff(s.astype(np.int64)) >= 0).all()
            acc = np.array([dw.d_accepts(direction, eps, L, d) for direction, L, d, _, _ in rows])
            assert np.array_equal(acc, dw.iv_neighbour(s[0::2], e[0::2], s[1::2], e[1::2], eps))
            n_acc, n_rej = n_acc + int(acc.sum()), n_rej + int((~acc).sum())
            # isolated: nothing reaches the next pair
            assert (np.maximum(e[0::2], e[1::2])[:-1].astype(np.int64) < s[0::2][1:]).all()
            lo, hi = dw.window(s, e, eps)
            for r, (direction, L, d, t, _) in enumerate(rows):
                assert d - t in dw.D_SHIFTS
                if acc[r]:
                    assert d <= t + 1                                      # the search's finding: never two past the reach
                    assert s[2 * r + 1] <= hi[2 * r] and s[2 * r] >= lo[2 * r + 1]       # the padded window holds every accepted pair
                    if d == t + 1:                                         # ... and this one only because of the pad
                        seen_pad[direction] += 1
                        assert s[2 * r + 1] > hi[2 * r] - 2 if direction == "fwd" else s[2 * r] < lo[2 * r + 1] + 2
                else:
                    assert d >= t                                          # rejected at the reach itself only by rounding
        assert n_acc >= 20 and n_rej >= 20
        for direction in ("fwd", "bwd"):
            for L in dw.d_pad_dependent(direction, eps):
                assert (direction, L, dw.d_trunc(direction, eps, L) + 1) in all_rows
        assert {L for _, L, _ in all_rows if L > dw.D_L_SEARCH} == set(dw.D_L_BIG)
    assert seen_pad["fwd"] >= 1 and seen_pad["bwd"] >= 1
    assert 90 in dw.d_pad_dependent("fwd", 0.7) and 172 in dw.d_pad_dependent("bwd", 0.2) and 3 in dw.d_pad_dependent("bwd", 0.7)


@pytest.mark.parametrize("eps", dw.E_EPS)
def test_e_window_widths_leave_uint64(oracle, eps):
    name, s, e, _, mp = dw.e_planted(eps)
    want = oracle.dbscan_iv(s, e, eps, mp)
    assert want.tolist() == [0, 1, 1, 0]                                  # i_A sees j_A: it is A's start point
    keep = np.arange(4) != dw.E_JA
    assert oracle.dbscan_iv(s[keep], e[keep], eps, mp).tolist() == [-2, 0, 0]          # without j_A the labels change
    ln = (e.astype(np.int64) - s)[dw.E_IA]
    wb = eps * float(ln) / (1.0 - eps)
    assert (wb >= 2.0**64) == (eps > 0.9999999)                            # the two larger eps: i_A's backward reach is no uint64_t
    assert s[dw.E_IA] - s[dw.E_JA] >= 2**29
    name, s, e, _, mp = dw.e_random(eps)
    lab = oracle.dbscan_iv(s, e, eps, mp)
    assert len(s) > dw.DBSCAN_IV_SMALL_MAX and (lab >= 0).any()
    ln = e.astype(np.int64) - s
    assert ((eps * ln / (1.0 - eps)) >= 2.0**64).any() == (eps > 0.9999999)


def test_f_more_tiles_than_one_scan_round(oracle):
    for name, s, e, eps, mp in dw.f_cases():
        n = len(s)
        assert (n + T - 1) // T >= T + (n > T * T), name
    name, s, e, eps, mp = dw.f_case(dw.F_PERMUTED)
    n = len(s)
    assert (n + T - 1) // T >= T + 1                                      # >= 257 tiles: the carry loop's second round
    lab = oracle.dbscan_iv_windowed(s, e, eps, mp)
    fwd, bwd = dw.window_candidates(s, e, eps)
    assert max(fwd.max(), bwd.max()) < dw.DB_HALO
    assert lab.max() >= 10_000 and (lab == -2).sum() >= 1000
    # start-sorted: a cluster none of whose members lies in the first 256 tiles has its root beyond them
    name, s, e, eps, mp = dw.f_case(dw.F_SIZES[2])
    lab = oracle.dbscan_iv_windowed(s, e, eps, mp)
    assert len(set(lab[T * T:].tolist()) - set(lab[: T * T].tolist()) - {-2}) >= 10_000


@pytest.mark.parametrize("shard", dw.g_shards(), ids=[g["name"] for g in dw.g_shards()])
def test_g_the_sets_would_merge_as_one(oracle, shard):
    from contextsv_amd import Reads
    n = len(shard["pos"])
    reads = Reads.from_cigar_lists(shard["pos"], np.zeros(n, np.uint16), np.full(n, 60, np.uint8), shard["cigars"])
    sig = oracle.cigar_scan(reads, shard["depth_len"])
    kind = sig["qpos_kind"] & 3
    dels, inss = sig[kind == 1], sig[kind != 1]
    k = shard["k"]
    assert (len(dels), len(inss)) == (shard["n_del"], shard["n_ins"])
    for f in ("start", "end"):                                           # the DEL set's tail and the INS set's head: one interval, 2 k times
        assert len(set(dels[f][-k:].tolist()) | set(inss[f][:k].tolist())) == 1
    assert dels["start"][-k] > dels["start"][: len(dels) - k].max(initial=0) and (len(inss) == k or inss["start"][k - 1] < inss["start"][k:].min())
    apart = np.concatenate([oracle.dbscan_iv(x["start"], x["end"], 0.1, 5) for x in (dels, inss)])
    one = oracle.dbscan_iv(np.concatenate([dels["start"], inss["start"]]), np.concatenate([dels["end"], inss["end"]]), 0.1, 5)
    planted = slice(len(dels) - k, len(dels) + k)
    assert not np.array_equal(apart[planted], one[planted])
    if k == 4:
        assert (apart[planted] == -2).all() and (one[planted] >= 0).all()       # noise apart, a cluster of 8 as one set
    else:
        assert (apart[len(dels): len(dels) + k] == 0).all() and (one[len(dels): len(dels) + k] == apart[len(dels) - 1]).all()


def test_h_thresholds(oracle):
    for name, pts, off in dw.h_sets():
        n = int(off[1])
        assert n > dw.DBSCAN1D_MAX_SEG and int(off[2] - off[1]) == dw.DBSCAN1D_MAX_SEG and np.array_equal(pts[n:], pts[: dw.DBSCAN1D_MAX_SEG])
        assert pts.min() < 0 < pts.max()
    name, pts, off = dw.h_sets()[0]
    p = pts[: int(off[1])]
    below, above = oracle.dbscan_1d(p, 2 * dw.H_STEP - 0.5, 5), oracle.dbscan_1d(p, 2 * dw.H_STEP + 0.5, 5)
    assert (below == -2).all() and (above == 0).all()                    # 3 neighbours against 5: half a unit of eps decides everything
    assert (oracle.dbscan_1d(p, float("inf"), 5) == 0).all() and np.array_equal(oracle.dbscan_1d(p, 2 * dw.H_STEP - 0.5, 1), np.zeros(len(p), np.int32))
