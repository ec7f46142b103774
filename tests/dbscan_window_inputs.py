"""Seeded inputs that put the windowed DBSCAN (kernels/dbscan.hip) at its tile, split and eps edges (numpy only; cases by name).

The windowed kernels label 256-point tiles (UF_TILE) with a 128-element halo (DB_HALO) and 16 lanes per window (DB_G); interval sets
above DBSCAN_IV_SMALL_MAX points and 1-D segments above DBSCAN1D_MAX_SEG points take them. The constants below are the kernels';
tests/test_dbscan_window_inputs.py reads them out of the sources and compares, and asserts from CPU labels and the numpy window model
of this module that every family holds what it claims. tests/test_gpu_dbscan_window_edges.py runs the families on the device.

An interval case is (name, start, end, eps, min_pts) in caller order. Every case comes start-sorted (positions are original indices: the
tile ranks and the last-workgroup scan number the clusters) and in a seeded permutation (the device sorts, and an exclusive sum over
original indices numbers them).

  A  a staircase chain: one cluster over 20 tiles; every interior point exactly at the core threshold; everything noise
  B  blocks of 256 linked by ONE neighbour pair per tile border (or by none, or — one interval in front — by pairs inside tiles), and
     the same cut to sizes around multiples of 256
  C  the border rule with planted original indices, at tile borders and inside tiles
  D  isolated pairs one position either side of the neighbour threshold, those accepted only inside the window's 2 bp pad among them
  E  eps at the top of [0, 1): window widths beyond 2^64
  F  more than 256 tiles of shallow clusters (the carry loop of the tile-total scan)
  G  read shards whose last DEL and first INS signatures are the same interval (the two sets side by side in one launch)
  H  1-D staircases in one segment above 512 points, with eps up to infinity"""
import zlib

import numpy as np

UF_TILE = 256
DB_HALO = 128
DB_G = 16
DBSCAN_IV_SMALL_MAX = 2048
DBSCAN1D_MAX_SEG = 512

SEED = 0x5eed
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _rng(name):
    return np.random.default_rng(SEED + zlib.crc32(name.encode()))


def _case(name, s, e, eps, min_pts):
    s, e = _frozen(np.ascontiguousarray(s, np.uint32), np.ascontiguousarray(e, np.uint32))
    return (name, s, e, float(eps), int(min_pts))


def permutation_of(name, n):
    return _rng("perm:" + name).permutation(n)


def permuted(case):
    """the same set in a seeded caller order"""
    name, s, e, eps, min_pts = case
    p = permutation_of(name, len(s))
    return _case(name + "/perm", s[p], e[p], eps, min_pts)


def both_orders(case):
    return [case, permuted(case)]


# ---- the numpy model: the reference's predicate and the kernel's key window ------------------------------------------------------------
def iv_neighbour(s1, e1, s2, e2, eps):
    """distance(a, b) <= eps with distance = 1 - min(ov / len_a, ov / len_b) in double (elementwise; a zero length neighbours nothing)"""
    s1, e1, s2, e2 = (np.asarray(x, np.int64) for x in (s1, e1, s2, e2))
    ov = np.maximum(0, np.minimum(e1, e2) - np.maximum(s1, s2)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.minimum(ov / (e1 - s1).astype(np.float64), ov / (e2 - s2).astype(np.float64))
        return (1.0 - q) <= eps


def window(s, e, eps):
    """IntervalMetric::window as it is meant: the start keys [lo, hi] that can hold neighbours (float64, so no width overflows)"""
    s = np.asarray(s, np.int64).astype(np.float64)
    ln = np.maximum(np.asarray(e, np.int64).astype(np.float64) - s, 0.0)
    wf = np.trunc(eps * ln) + 2.0
    wb = np.trunc(eps * ln / (1.0 - eps)) + 2.0
    return np.maximum(s - wb, 0.0), s + wf


def start_order(s):
    """the device's order: by start, ties by original index"""
    return np.argsort(np.asarray(s), kind="stable")


def sorted_position(s):
    """position of every caller index in the start order"""
    o = start_order(s)
    pos = np.empty(len(o), np.int64)
    pos[o] = np.arange(len(o))
    return pos


def window_candidates(s, e, eps):
    """(forward, backward) candidate counts of every point of a START-SORTED set, the point itself not counted"""
    s = np.asarray(s, np.int64)
    lo, hi = window(s, e, eps)
    i = np.arange(len(s))
    return np.searchsorted(s, hi, "right") - i - 1, i - np.searchsorted(s, lo, "left")


def neighbour_lists(s, e, eps):
    """every point's neighbours (itself included), brute force: for sets of a few thousand points"""
    s, e = np.asarray(s, np.int64), np.asarray(e, np.int64)
    return [np.flatnonzero(iv_neighbour(s[i], e[i], s, e, eps)) for i in range(len(s))]


def tiles_spanned(s, labels):
    """per cluster id: how many UF_TILE tiles of the start order lie between its first and its last member"""
    pos = sorted_position(s)
    out = {}
    for c in np.unique(labels[labels >= 0]):
        p = pos[labels == c]
        out[int(c)] = int(p.max() // UF_TILE - p.min() // UF_TILE + 1)
    return out


# ---- A: staircase chain ----------------------------------------------------------------------------------------------------------------
STEP, LEN, EPS = 10, 1000, 0.1          # a shift of d bp is a neighbour iff 1 - (1000 - d) / 1000 <= 0.1 in double: d <= 100, 10 steps
A_N = 5000


def _staircase(n, base=1000):
    s = base + STEP * np.arange(n, dtype=np.int64)
    return s, s + LEN


def a_cases():
    """min_pts 5: one cluster; 21 = 10 + 10 + itself: every interior point exactly at the threshold, the ends border points; 22: noise"""
    s, e = _staircase(A_N)
    return _cached("A", lambda: [c for mp in (5, 21, 22) for c in both_orders(_case(f"A/min_pts{mp}", s, e, EPS, mp))])


# ---- B: blocks of a tile, one link per border ------------------------------------------------------------------------------------------
B_BLOCKS = 12
B_MIN_PTS = 3
B_CUTS = (255, 256, 257, 511, 512, 513, 768, 3072)


def _blocks(gap, n_blocks=B_BLOCKS, base=100_000):
    """staircases of UF_TILE points; the next block's first start lies `gap` after the previous block's last (100: that ONE pair is a
    neighbour, the pairs 110 apart are not; 101: none is)"""
    k = np.arange(n_blocks * UF_TILE, dtype=np.int64)
    s = base + STEP * k + (gap - STEP) * (k // UF_TILE)
    return s, s + LEN


def b_linked(n=B_BLOCKS * UF_TILE):
    s, e = _blocks(100)
    return _case(f"B/linked/n{n}", s[:n], e[:n], EPS, B_MIN_PTS)


def b_unlinked():
    s, e = _blocks(101)
    return _case("B/gap101", s, e, EPS, B_MIN_PTS)


def b_shifted():
    """a lone far-away noise interval in front: every position moves by one, so the single links lie inside tiles"""
    s, e = _blocks(100)
    return _case("B/linked/front_noise", np.concatenate([[10], s]), np.concatenate([[60], e]), EPS, B_MIN_PTS)


def b_cases():
    return _cached("B", lambda: [c for base in [b_linked(n) for n in B_CUTS] + [b_unlinked(), b_shifted()] for c in both_orders(base)])


# ---- C: the border rule --------------------------------------------------------------------------------------------------------------
C_M = 12                                # points per staircase
C_MIN_PTS = 5
C_SCENARIOS = ("neither", "both", "larger")
C_PLACEMENTS = (100, 0, UF_TILE - 1)    # sorted position of b modulo UF_TILE: inside a tile, first of a tile, last of a tile


def _c_layout():
    """Instances along the axis: staircase A, 200 bp on staircase B, and b midway, which neighbours only A's last and B's first point
    (100 bp either way; A's last but one is 110 away) and, with 3 < min_pts neighbours, is no core. Isolated 10 bp intervals pad the
    positions so that b lands where C_PLACEMENTS says."""
    s, e, inst, fillers = [], [], [], []
    x = 50_000
    for scen in C_SCENARIOS:
        for swapped in (False, True):
            for place in C_PLACEMENTS:
                for _ in range((place - len(s) - C_M) % UF_TILE):
                    fillers.append(len(s)); s.append(x); e.append(x + 10); x += 1000
                x += 5000
                a = list(range(len(s), len(s) + C_M))
                s += [x + STEP * k for k in range(C_M)]
                b = len(s)
                s.append(s[-1] + 100)
                bb = list(range(len(s), len(s) + C_M))
                s += [s[b] + 100 + STEP * k for k in range(C_M)]
                e += [v + LEN for v in s[len(e):]]
                x = s[-1] + LEN + 5000
                inst.append(dict(scenario=scen, swapped=swapped, place=place, a=a, b=b, bb=bb))
    return np.asarray(s, np.int64), np.asarray(e, np.int64), inst, fillers


def c_planted():
    """-> (case, instances): caller order planted so that, per instance, the first two of its points in index order are
         neither  A's first, B's last         no end is its cluster's start point        -> b takes the SMALLER id
         both     A's last, B's first         both ends are start points                  -> b takes the LARGER id
         larger   A's first, B's first        only the end with the larger id is one      -> b takes that larger id
       and the mirror image of each (`swapped`: B's cluster gets the smaller id). Instances hold caller indices."""
    def make():
        s, e, inst, fillers = _c_layout()
        rng = _rng("C")
        order = []
        for it in inst:
            a, bb = it["a"], it["bb"]
            first = {"neither": (a[0], bb[-1]), "both": (a[-1], bb[0]), "larger": (a[0], bb[0])}[it["scenario"]]
            if it["swapped"]:
                first = {"neither": (bb[-1], a[0]), "both": (bb[0], a[-1]), "larger": (bb[-1], a[-1])}[it["scenario"]]
            rest = [p for p in a + [it["b"]] + bb if p not in first]
            order += list(first) + [rest[k] for k in rng.permutation(len(rest))]
        order = np.asarray(order + fillers)
        at = np.empty(len(order), np.int64)
        at[order] = np.arange(len(order))
        planted = [dict(it, a=at[it["a"]], b=int(at[it["b"]]), bb=at[it["bb"]]) for it in inst]
        return _case("C/planted", s[order], e[order], EPS, C_MIN_PTS), planted
    return _cached("C", make)


def c_sorted():
    s, e, inst, _ = _c_layout()
    return _case("C/sorted", s, e, EPS, C_MIN_PTS), [dict(it, a=np.asarray(it["a"]), bb=np.asarray(it["bb"])) for it in inst]


def c_cases():
    return [c_sorted()[0], c_planted()[0]]


# ---- D: pairs at the threshold -------------------------------------------------------------------------------------------------------
D_EPS = (0.05, 0.1, 0.2, 0.3, 1 / 3, 0.35, 0.5, 0.6, 0.7, 0.9, 0.999)
D_SHIFTS = (-1, 0, 1, 2, 3)
D_L = (1, 2, 3, 5, 7, 10, 13, 17, 31, 64, 90, 100, 172, 255, 256, 257, 500, 777, 1000, 1333, 1999, 2000)
D_L_SEARCH = 2000
D_L_BIG = (10**6, 2**24 + 1, 2**28)     # 2^24 + 1: beyond float's integers (the single-precision pre-filter of iv_neighbor)
D_MIN_PTS = 2                           # a pair's labels are {c, c} or {-2, -2}


def d_trunc(direction, eps, L):
    """the window's reach without its pad: trunc(eps * L) forward, trunc(eps * L / (1 - eps)) backward"""
    return int(eps * L) if direction == "fwd" else int(eps * L / (1.0 - eps))


def d_pair(direction, L, d, at=0):
    """forward: [s, s + L] and [s + d, s + d + L]; backward: a length-L interval that ends where one of length L + d ends"""
    return ((at, at + L), (at + d, at + d + L)) if direction == "fwd" else ((at, at + L + d), (at + d, at + L + d))


def d_accepts(direction, eps, L, d):
    (s1, e1), (s2, e2) = d_pair(direction, L, d)
    return bool(iv_neighbour(s1, e1, s2, e2, eps))


def d_pad_dependent(direction, eps):
    """the L <= D_L_SEARCH whose pair at shift trunc + 1 the double expression accepts: inside the window only because of its pad"""
    return [L for L in range(1, D_L_SEARCH + 1) if d_accepts(direction, eps, L, d_trunc(direction, eps, L) + 1)]


def d_parts(eps):
    """-> parts, each a list of rows (direction, L, d, trunc, locus): the points 2 r and 2 r + 1 of the sorted case d_case(eps, part)
    are row r's pair. A part ends where the next pair's locus would leave the int range (at eps = 0.999 the backward pairs are a
    thousand times their L long, and every L is pad-dependent); a pair that no part can hold is left out."""
    def make():
        parts, at, limit = [[]], 1000, 2**31 - 2**16
        def add(direction, L, shift):
            nonlocal at
            t = d_trunc(direction, eps, L)
            d = t + shift
            span = L + d + 16
            if d < 0 or 1000 + span >= limit:
                return
            if at + span >= limit:
                parts.append([])
                at = 1000
            parts[-1].append((direction, L, d, t, at))
            at += span
        for direction in ("fwd", "bwd"):
            for L in sorted(set(D_L) | set(d_pad_dependent(direction, eps))):
                for shift in D_SHIFTS:
                    add(direction, L, shift)
        for L, shifts in zip(D_L_BIG, (D_SHIFTS, D_SHIFTS, (0, 1))):
            for shift in shifts:
                for direction in ("fwd", "bwd"):
                    add(direction, L, shift)
        return parts
    return _cached(("Drows", eps), make)


def d_case(eps, part=0):
    def make():
        iv = [p for direction, L, d, _, at in d_parts(eps)[part] for p in d_pair(direction, L, d, at)]
        a = np.asarray(iv, np.int64)
        return _case(f"D/eps{eps:.6g}/part{part}", a[:, 0], a[:, 1], eps, D_MIN_PTS)
    return _cached(("D", eps, part), make)


def d_cases():
    return [c for eps in D_EPS for part in range(len(d_parts(eps))) for c in both_orders(d_case(eps, part))]


# ---- E: eps at the top of its domain -------------------------------------------------------------------------------------------------
E_EPS = (0.999999, 1.0 - 2.0**-40, 1.0 - 2.0**-53)
E_MIN_PTS = 2
E_IA, E_JB, E_IB, E_JA = 0, 1, 2, 3
E_RANDOM_N = 3000
E_RANDOM_MIN_PTS = 3


def e_planted(eps):
    """Two long intervals j_A, j_B on disjoint loci, each with an interval i deep inside it (2^29 after its start, a 16th of its
    length: i's backward reach eps * len / (1 - eps) passes 2^64 for the two larger eps). Caller order i_A, j_B, i_B, j_A: when i_A
    sees j_A it is a core and, as index 0, the start point of A, which is then cluster 0; when it does not, B is.
    (j_A is 2^30 long; j_B is 2^14 shorter, because two disjoint intervals of 2^30 do not both end below 2^31.)"""
    ja = (1000, 1000 + 2**30)
    ia = (ja[0] + 2**29 + 5, ja[0] + 2**29 + 5 + 2**26)
    jb = (ja[1] + 4000, ja[1] + 4000 + 2**30 - 2**14)
    ib = (jb[0] + 2**29 + 7, jb[0] + 2**29 + 7 + 2**26)
    a = np.asarray([ia, jb, ib, ja], np.int64)
    assert a.max() < 2**31
    return _case(f"E/planted/eps{eps!r}", a[:, 0], a[:, 1], eps, E_MIN_PTS)


def e_random(eps):
    def make():
        rng = _rng("E/random")
        ln = rng.choice([1, 50, 10**6, 2**30], E_RANDOM_N)
        s = rng.integers(1, 2**30 - 2, E_RANDOM_N)
        return s, s + ln
    s, e = _cached("Erandom", make)
    return _case(f"E/random/eps{eps!r}", s, e, eps, E_RANDOM_MIN_PTS)


def _sorted_case(case):
    name, s, e, eps, min_pts = case
    o = start_order(s)
    return _case(name + "/sorted", s[o], e[o], eps, min_pts)


def e_cases():
    return _cached("E", lambda: [c for eps in E_EPS for c in (e_planted(eps), _sorted_case(e_planted(eps)), e_random(eps), _sorted_case(e_random(eps)))])


# ---- F: many tiles, shallow ----------------------------------------------------------------------------------------------------------
F_SIZES = (65_536, 65_537, 131_072)     # 256 tiles (one round of the carry loop, and n a multiple of the tile), 257, 512 (two full rounds)
F_PERMUTED = 65_537
F_MIN_PTS = 2


def f_case(n):
    """groups of ~6 around sorted random centres, starts jittered by +-3, lengths from {60, 300, 2000}; start-sorted"""
    def make():
        rng = _rng(f"F/{n}")
        centres = np.sort(rng.integers(1, 50_000_000, (n + 5) // 6))
        s = np.repeat(centres, 6)[:n] + rng.integers(-3, 4, n)
        s = np.maximum(s, 1)
        ln = rng.choice([60, 300, 2000], n)
        o = np.argsort(s, kind="stable")
        return _case(f"F/n{n}", s[o], (s + ln)[o], EPS, F_MIN_PTS)
    return _cached(("F", n), make)


def f_cases():
    return [f_case(n) for n in F_SIZES] + [permuted(f_case(F_PERMUTED))]


def interval_cases():
    """every interval case but F (the literal oracle is quadratic)"""
    return a_cases() + b_cases() + c_cases() + d_cases() + e_cases()


# ---- G: pipeline shards --------------------------------------------------------------------------------------------------------------
OP_M, OP_I, OP_D = 0, 1, 2
G_SHARDS = ((255, 304, 5), (256, 9, 4), (257, 5, 5), (4, 4, 4))     # (n_del, n_ins, k)
G_FILL_GROUP = 6


def g_shard(n_del, n_ins, k):
    """-> dict(pos, cigars, depth_len, k, n_del, n_ins). k reads carry a 100 bp INS and a 100 bp DEL on the same interval; before them
    n_del - k reads with one 120 bp DEL each, 6 per locus, loci 400 apart; after them n_ins - k reads with one 120 bp INS each. In start
    order the DEL set ends with the k planted signatures and the INS set begins with them."""
    pos, cig = [], []
    groups = -(-(n_del - k) // G_FILL_GROUP)
    for r in range(n_del - k):
        pos.append(1000 + 400 * (r // G_FILL_GROUP)); cig.append([(OP_M, 50), (OP_D, 120), (OP_M, 50)])
    x = 1000 + 400 * groups + 1000
    for r in range(k):
        pos.append(x - 500 + r); cig.append([(OP_M, 500 - r), (OP_I, 100), (OP_D, 100), (OP_M, 300)])
    for r in range(n_ins - k):
        pos.append(x + 2000 + 400 * (r // G_FILL_GROUP)); cig.append([(OP_M, 50), (OP_I, 120), (OP_M, 50)])
    return dict(name=f"G/del{n_del}_ins{n_ins}_k{k}", pos=np.asarray(pos, np.int32), cigars=cig, depth_len=int(pos[-1]) + 2000,
                k=k, n_del=n_del, n_ins=n_ins)


def g_shards():
    return [g_shard(*a) for a in G_SHARDS]


def g_pct_for(mean_cov, min_pts):
    """a min_pts_pct with ceil(mean_cov * pct) == min_pts, half a point away from either neighbour"""
    return (min_pts - 0.5) / mean_cov


# ---- H: 1-D, one segment above DBSCAN1D_MAX_SEG points --------------------------------------------------------------------------------
H_SIZES = (768, 1024, 1537)
H_STEP = 10
H_EPS = (100.0, 1e19, 1e30, float("inf"), 2 * H_STEP + 0.5, 2 * H_STEP - 0.5)
H_MIN_PTS = (1, 5)


def h_sets():
    """-> [(name, pts, seg_off)]: a point staircase across zero (and its seeded permutation) as one segment, then its first
    DBSCAN1D_MAX_SEG points again as a second segment, which the LDS kernel labels"""
    def make():
        out = []
        for n in H_SIZES:
            p = (-5000 + H_STEP * np.arange(n)).astype(np.int32)
            for name, q in ((f"H/n{n}", p), (f"H/n{n}/perm", p[permutation_of(f"H/n{n}", n)])):
                pts, off = _frozen(np.concatenate([q, q[:DBSCAN1D_MAX_SEG]]), np.asarray([0, n, n + DBSCAN1D_MAX_SEG], np.uint64))
                out.append((name, pts, off))
        return out
    return _cached("H", make)
