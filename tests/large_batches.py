"""Seeded batches that are larger than the capped grids of the three kernel families that give one wave (or one workgroup) a whole point
set in its LDS and let it stride over the sets its grid has no wave for (numpy only; the references are computed once per session).

Item w and item w + W run on the same wave (workgroup), in that order, so the second one starts on LDS that still holds the first.
The batches are built around such pairs: a large set in front of a small one and the other way round, a set behind an empty one, a set
behind one that is too large for LDS. tests/test_large_batches_inputs.py asserts, without a GPU, that the pairs are there;
tests/test_gpu_large_batches.py runs the batches on the device."""
import numpy as np

# W: how many waves (workgroups) the capped grid has. A cap that moves has to move here too: test_large_batches_inputs.py reads the
# launch functions' caps out of the sources and compares.
W_DBSCAN1D = 4096 * 4       # launch_dbscan_1d_batched (kernels/dbscan1d.hip): at most 4096 workgroups of D1_WAVES = 4 waves; item = segment
W_SPLIT_FITS = 8192 * 2     # launch_sf_fits (kernels/splitfits.hip): at most 8192 workgroups of SF_WAVES = 2 waves; item = 6 * group + set
W_INTERVAL = 8192           # launch_dbscan_iv_small_batched (kernels/dbscan.hip): at most 8192 workgroups; item = set
D1_CAP = 512                # DBSCAN1D_MAX_SEG (common.hpp): more points than this do not fit a wave's LDS slice
IV_CAP = 2048               # DBSCAN_IV_SMALL_MAX (common.hpp): ... a workgroup's LDS

LARGE_FROM, SMALL_TO = 200, 8          # "large": LARGE_FROM .. cap points, "small": 1 .. SMALL_TO

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _offsets(sizes):
    off = np.zeros(len(sizes) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray(sizes, np.int64))
    return off


def pair_stats(sizes, W, cap):
    """What the pairs (w, w + W) of a batch with these set sizes hold."""
    sizes = np.asarray(sizes, np.int64)
    a, b = sizes[:-W], sizes[W:]
    large = lambda x: (x >= LARGE_FROM) & (x <= cap)
    small = lambda x: (x >= 1) & (x <= SMALL_TO)
    over = np.flatnonzero(sizes > cap)
    with_succ = over[over + W < len(sizes)]
    return {"large_small": int((large(a) & small(b)).sum()), "small_large": int((small(a) & large(b)).sum()),
            "after_empty": int(((a == 0) & (b > 0)).sum()), "oversize": over, "oversize_with_successor": with_succ,
            "successors_in_lds": bool(((sizes[with_succ + W] >= 1) & (sizes[with_succ + W] <= cap)).all())}


def predecessor_size(sizes, w, W):
    return int(sizes[w - W]) if w >= W else None


def _roles(rng, W, n_free, banned=()):
    """Disjoint residues modulo W for the planted pairs; the first n_free of them lie below n_free."""
    low = rng.permutation(n_free)
    low = low[~np.isin(low % 64, banned)] if len(banned) else low
    rest = rng.permutation(W)
    rest = rest[~np.isin(rest, low[:8])]
    rest = rest[~np.isin(rest % 64, banned)] if len(banned) else rest
    return low[:8], rest


# ---- csvgpu_dbscan_1d ------------------------------------------------------------------------------------------------------------------
def _dbscan1d_batch():
    rng = np.random.default_rng(20261)
    W = W_DBSCAN1D
    n_seg = 3 * W + 1000                                     # three full trips and the start of a fourth
    sizes = np.minimum(rng.integers(0, 65, n_seg), rng.integers(0, 65, n_seg))
    low, r = _roles(rng, W, 1000)
    big = lambda n: np.where(rng.random(n) < 0.1, rng.choice([200, 511, 512], n), rng.integers(200, 513, n))
    for res, trip in ((r[:150], 0), (r[150:300], 1)):        # large in front of small
        sizes[trip * W + res] = big(len(res)); sizes[(trip + 1) * W + res] = rng.integers(1, SMALL_TO + 1, len(res))
    for res, trip in ((r[300:450], 0), (r[450:600], 1)):     # small in front of large
        sizes[trip * W + res] = rng.integers(1, SMALL_TO + 1, len(res)); sizes[(trip + 1) * W + res] = big(len(res))
    for res, trip in ((r[600:750], 0), (r[750:900], 1)):     # empty in front of non-empty
        sizes[trip * W + res] = 0; sizes[(trip + 1) * W + res] = np.maximum(1, sizes[(trip + 1) * W + res])
    # beyond the LDS kernel (the per-segment sorted path): one per trip, each with a successor on its wave, at the cap's edges
    for k, (n_over, n_next) in enumerate(((513, 5), (3000, 512), (1200, 64))):
        sizes[k * W + low[k]] = n_over; sizes[(k + 1) * W + low[k]] = n_next
    off = _offsets(sizes)
    n = int(off[-1])
    seg = np.repeat(np.arange(n_seg), sizes)
    base = rng.integers(-1000, 1_000_000, n_seg)
    pts = base[seg] + rng.choice([0, 0, 0, 300, 5000], n) + rng.integers(-120, 121, n)      # cores, borders and noise
    wide = (seg % 97 == 13)                                  # sets over the whole int32 range
    pts[wide] = rng.integers(-2**31, 2**31 - 1, int(wide.sum()))
    return pts.astype(np.int32), off


def dbscan1d_batch():
    """-> (pts int32, seg_off uint64)"""
    return _cached("d1", _dbscan1d_batch)


def dbscan1d_want(oracle, eps, min_pts):
    """oracle.dbscan_1d of every segment, concatenated"""
    def make():
        pts, off = dbscan1d_batch()
        o = off.astype(np.int64)
        return np.concatenate([oracle.dbscan_1d(pts[o[k]:o[k + 1]], eps, min_pts) for k in range(len(o) - 1)])
    return _cached(("d1", eps, min_pts), make)


# ---- csvgpu_dbscan_iv_batch ------------------------------------------------------------------------------------------------------------
def _interval_batch():
    rng = np.random.default_rng(20262)
    W = W_INTERVAL
    n_set = 2 * W + 3000
    idx = np.arange(n_set)
    sizes = rng.integers(1, 41, n_set)
    sizes[idx % 50 == 7] = 0
    phase = np.array([0, 21, 42])[idx // W]                  # every 64th set is large, but never W behind another large one
    every64 = idx % 64 == phase
    sizes[every64] = np.where(rng.random(int(every64.sum())) < 0.1, rng.choice([2047, 2048], int(every64.sum())), rng.integers(300, IV_CAP + 1, int(every64.sum())))
    low, r = _roles(rng, W, 3000, banned=(0, 21, 42))
    big = lambda n: rng.integers(LARGE_FROM, 401, n)
    sizes[r[:230]] = big(230); sizes[W + r[:230]] = rng.integers(1, SMALL_TO + 1, 230)                      # large in front of small
    sizes[r[230:460]] = rng.integers(1, SMALL_TO + 1, 230); sizes[W + r[230:460]] = big(230)                # small in front of large
    sizes[r[460:700]] = 0; sizes[W + r[460:700]] = np.maximum(1, sizes[W + r[460:700]])                     # empty in front of non-empty
    # beyond the LDS kernels (the windowed path, through the host loop): one in the first trip, one in the second, each with a successor
    for k, (n_over, n_next) in enumerate(((2049, 33), (2600, IV_CAP))):
        sizes[k * W + low[k]] = n_over; sizes[(k + 1) * W + low[k]] = n_next
    off = _offsets(sizes)
    n = int(off[-1])
    sid = np.repeat(idx, sizes)
    n_centres = sizes // 7 + 1                               # as tests/test_gpu_ref_sweep.py draws a set: a few centres, jittered, mixed lengths
    coff = _offsets(n_centres).astype(np.int64)
    centres = rng.integers(1000, 200_000, int(coff[-1]))
    c = centres[coff[sid] + (rng.random(n) * n_centres[sid]).astype(np.int64)]
    length = rng.choice([0, 1, 49, 50, 300, 2000, 40_000], n, p=[.02, .02, .06, .3, .3, .2, .1])
    s = np.maximum(1, c + rng.integers(-8, 9, n)).astype(np.uint32)
    e = (s + np.maximum(0, length + rng.integers(-3, 4, n))).astype(np.uint32)
    return s, e, off


def interval_batch():
    """-> (start uint32, end uint32, seg_off uint64)"""
    return _cached("iv", _interval_batch)


def interval_want(oracle, eps, min_pts):
    """oracle.dbscan_iv of every set, concatenated"""
    def make():
        s, e, off = interval_batch()
        o = off.astype(np.int64)
        return np.concatenate([oracle.dbscan_iv(s[o[k]:o[k + 1]], e[o[k]:o[k + 1]], eps, min_pts) for k in range(len(o) - 1)])
    return _cached(("iv", eps, min_pts), make)


def interval_neighbour_counts(s, e, eps):
    """|N(i)| of one set by the reference's distance (dbscan.cpp:59-81): 1 - min(overlap / length) <= eps, i itself included"""
    s, e = s.astype(np.int64), e.astype(np.int64)
    overlap = np.maximum(0, np.minimum(e[:, None], e[None, :]) - np.maximum(s[:, None], s[None, :])).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        x, y = overlap / (e - s)[:, None], overlap / (e - s)[None, :]
        return (1.0 - np.where(y < x, y, x) <= eps).sum(axis=1)


# ---- csvgpu_split_fits / csvgpu_split_groups_fits --------------------------------------------------------------------------------------
N_BLOCKS = 212                                               # 40 groups each: 8480 groups, 50880 items


def _split_plan(rng):
    """Segments as lists of (pile size, options) (tests/test_split_fits_ref.py); a pile of one member gives no group, every other pile
    exactly one, and a segment's groups are numbered from the number of groups in front of it."""
    def small_pile():
        supps = [0, (0, 3), (0, 3), (0, 3), (0, 3), (0, 3), 1, (1, 3)][int(rng.integers(0, 8))]
        return (int(rng.integers(2, 9)), {"supps": supps, "opposite": float(rng.choice([0.1, 0.5, 0.9]))})
    lone = lambda: [(1, {"supps": (0, 2)}) for _ in range(int(rng.integers(1, 4)))]        # members, no group
    segs = [[], lone()]
    for b in range(N_BLOCKS):
        if b % 25 == 3:                                      # 200 members with three records each: sets 2 / 3 (and 4 / 5) beyond 512 points
            segs.append([(200, {"supps": 3, "other": 0.0, "opposite": 0.05})])
        else:                                                # every 40th pile is large; from about 360 members on its sets 2 / 3 are beyond 512
            segs.append([(int(rng.integers(200, 501)), {"supps": (0, 3), "opposite": float(rng.choice([0.1, 0.5]))})])
        left = 39
        while left:
            k = int(min(left, rng.integers(1, 13)))
            seg = [small_pile() for _ in range(k)]
            if rng.random() < 0.3:
                seg.insert(int(rng.integers(0, k + 1)), (1, {"supps": 1}))
            segs.append(seg)
            left -= k
            if rng.random() < 0.25:
                segs.append([])
            if rng.random() < 0.2:
                segs.append(lone())
    segs += [lone(), []]
    # a set beyond 512 points must be followed, on its wave, by one the LDS kernel labels: the groups W items behind a large pile's sets
    # 2 .. 5 get at least one record per member, all of them on the same tid
    first = np.cumsum([0] + [sum(k >= 2 for k, _ in seg) for seg in segs])
    for c, seg in enumerate(segs):
        if len(seg) == 1 and seg[0][0] >= LARGE_FROM:
            for g in {(6 * int(first[c]) + s + W_SPLIT_FITS) // 6 for s in range(2, 6)}:
                if g < first[-1]:
                    c2 = int(np.searchsorted(first, g, side="right")) - 1
                    assert all(k <= SMALL_TO for k, _ in segs[c2]), "a large pile W items behind a large pile: the plan's period does not fit W"
                    segs[c2] = [(k, dict(o, supps=(1, 3), other=0.0)) for k, o in segs[c2]]
    return segs


def _split_fits_batch():
    from contextsv_amd import host
    from test_split_fits_ref import _build
    rng = np.random.default_rng(20263)
    t, off = _build(rng, _split_plan(rng))
    # the host tree's groups: tests/test_split_groups_host.py pins it to the literal restatement, test_large_batches_inputs.py compares the
    # two on slices of this batch
    return t, off, host.split_groups_host(t["start"], t["end"], off)


def split_fits_batch():
    """-> (tables, seg_off, (seg_group_off, group_off, members))"""
    return _cached("sf", _split_fits_batch)


def split_fits_want(oracle, eps, min_pts):
    from test_split_fits_ref import reference_fits
    return _cached(("sf", eps, min_pts), lambda: reference_fits(oracle, *split_fits_batch(), eps=eps, min_pts=min_pts))


def split_set_sizes():
    """Points of every item 6 * group + set of the split-fit batch"""
    def make():
        t, off, (sgo, go, mem) = split_fits_batch()
        n_m, n_g = len(t["start"]), len(go) - 1
        so = t["supp_off"].astype(np.int64)
        owner = np.repeat(np.arange(n_m), np.diff(so))
        same_tid = (t["supp_flags"] & 2) == 0
        same_strand = same_tid & ((t["supp_flags"] & 1) == t["reverse"][owner])
        per_member = np.stack([np.ones(n_m), np.ones(n_m), *(np.bincount(owner[m], minlength=n_m) for m in (same_tid, same_tid, same_strand, same_strand))], axis=1)
        g_of = np.repeat(np.arange(n_g), np.diff(go.astype(np.int64)))
        seg_of_g = np.searchsorted(sgo.astype(np.int64), np.arange(n_g), side="right") - 1
        m_abs = off.astype(np.int64)[seg_of_g][g_of] + mem.astype(np.int64)
        sizes = np.zeros((n_g, 6), np.int64)
        np.add.at(sizes, g_of, per_member[m_abs].astype(np.int64))
        return sizes.reshape(-1)
    return _cached("sf_sizes", make)
