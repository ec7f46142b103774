"""Inputs of the copy-number observation tests (tests/test_cn_observation_inputs.py checks them on the CPU against the oracle's real
std::unordered_map, tests/test_gpu_cn_observations.py runs them through csvgpu_cn_observations_resident_many): one 400 kb contig
built like tests/test_gpu_cnv.py's, two SNP tables (the second with injected duplicate positions), and the region families — each
region a dict(family, start, end, ss) with ss the caller's sample size.

What the device form relies on, and what each family is there for:
  rehash   long regions whose window count sits on both sides of every rehash of the reference's hash map (13, 29, 59, ... buckets)
  short    regions shorter than their window count (pos_step < 1): runs of equal keys, collapsed nodes, a SNP that lands in three nodes
  snps     more SNPs in the region than the sample size (the SNP count is the window count), and regions without any SNP
  edges    SNPs exactly on a window's start and on a window's end (both ends are inclusive: the SNP is in two nodes)
  dups     duplicate SNP positions (table 1): each record counts
  hole     regions over the zero-coverage stretch (the 1e-9 floor) and regions past the end of the depth map
  large    regions at coordinates up to 2^31 - 2: key texts of every length from 3 to 21 bytes
  random   candidate-sized regions as a genome pass has them
"""
import numpy as np

from contextsv_amd import Reads

CHR_LEN = 400_000
REHASH_SS = (1, 13, 14, 29, 30, 59, 60, 127, 128, 257, 258, 541, 542, 1109, 1110, 2357, 2358, 5087)
SMALL_MAX = 127            # regions of up to this many windows take the wave-per-region kernel (csrc/common.hpp CN_SMALL_MAX)
MAX_WINDOWS = 5087


def build_reads(seed=12):
    """~30x of 5 kb reads with a 15x stretch, a 60x stretch and a zero-coverage hole at [300 000, 306 000)."""
    rng = np.random.default_rng(seed)
    dens = np.full(CHR_LEN, 30.0)
    dens[60_000:110_000] = 15.0
    dens[200_000:260_000] = 60.0
    dens[300_000:306_000] = 0.0
    starts = []
    for p in range(0, CHR_LEN - 5000, 50):
        starts += [p + int(rng.integers(0, 50))] * int(rng.poisson(dens[p] * 50 / 5000))
    starts = np.sort(np.asarray(starts))
    keep = (starts + 5000 <= 300_000) | (starts >= 306_000)          # nothing reaches into the hole
    starts = starts[keep]
    return Reads.from_cigar_lists(starts, np.zeros(len(starts), int), np.full(len(starts), 60), [[(0, 5000)]] * len(starts))


def build_snps(seed=13):
    """-> [table 0 (400 distinct positions), table 1 (the same plus duplicates of 24 positions, two or three records each)]."""
    rng = np.random.default_rng(seed)
    n = 400
    pos = np.sort(rng.choice(np.arange(2000, CHR_LEN - 1000), n, replace=False)).astype(np.uint32)
    baf = np.clip(np.where(rng.random(n) < 0.6, 0.5 + rng.normal(0, 0.05, n), rng.choice([0.0, 1.0, 0.33, 0.67], n)), 0.0, 1.0)
    t0 = {"pos": pos, "baf": baf, "pfb": rng.uniform(0.02, 0.98, n), "has_pfb": (rng.random(n) < 0.3).astype(np.uint8)}
    dup_at = rng.choice(n, 24, replace=False)
    extra = np.concatenate([dup_at, dup_at[:8]])                       # eight positions three times
    p1 = np.concatenate([pos, pos[extra]])
    order = np.argsort(p1, kind="stable")
    m = len(p1)
    t1 = {"pos": p1[order], "baf": np.concatenate([baf, rng.uniform(0, 1, len(extra))])[order],
          "pfb": np.concatenate([t0["pfb"], rng.uniform(0.02, 0.98, len(extra))])[order],
          "has_pfb": np.concatenate([t0["has_pfb"], (rng.random(len(extra)) < 0.5).astype(np.uint8)])[order]}
    assert len(t1["pos"]) == m and (np.diff(t1["pos"].astype(np.int64)) >= 0).all()
    return [t0, t1]


def flat_snps(snps, start, end):
    """SNPTable::queryFlat: the records inside [start, end] with the values the reference's two hash maps hold for each position (baf of the
    LAST record of a position; pfb of its last record that has one, else 0.0)."""
    pos = snps["pos"]
    a, b = int(np.searchsorted(pos, start, "left")), int(np.searchsorted(pos, end, "right"))
    p = pos[a:b].copy()
    baf, pfb = np.zeros(b - a), np.zeros(b - a)
    i = a
    while i < b:
        j = i
        while j + 1 < b and pos[j + 1] == pos[i]:
            j += 1
        f = 0.0
        for k in range(i, j + 1):
            if snps["has_pfb"][k]:
                f = float(snps["pfb"][k])
        baf[i - a: j + 1 - a] = snps["baf"][j]
        pfb[i - a: j + 1 - a] = f
        i = j + 1
    return p, baf, pfb


def _gaps(pos, need):
    """Starts of SNP-free stretches of at least `need` positions inside the map, longest first."""
    edges = np.concatenate([[1000], pos.astype(np.int64), [CHR_LEN - 1000]])
    width = np.diff(edges)
    idx = np.argsort(-width)
    return [int(edges[i]) + 1 for i in idx if width[i] > need + 2]


def families(tables):
    """-> list of dict(family, table, start, end, ss): table = which SNP table (and shard) the region belongs to."""
    out = []

    def add(family, table, start, end, ss):
        out.append({"family": family, "table": table, "start": int(start), "end": int(end), "ss": int(ss)})

    for t, snps in enumerate(tables):
        pos = snps["pos"].astype(np.int64)
        gaps = _gaps(pos, 400)
        # rehash: pos_step >= 3 makes every window its own key; few enough SNPs that the sample size is the window count
        for k, ss in enumerate(REHASH_SS):
            if ss <= 128:
                g = gaps[k % len(gaps)]
                add("rehash", t, g, g + 3 * ss - 1, ss)
            else:
                s0 = 5000 + 37 * k + 1000 * t
                add("rehash", t, s0, s0 + 7 * ss - 1, ss)
        # short: L positions, ss windows, ss > L; around a SNP p the keys (p-1,p), (p,p), (p,p+1) all hold it
        for k, (L, ss) in enumerate([(1, 20), (2, 20), (3, 20), (5, 20), (9, 20), (5, 64), (40, 200), (100, 300), (17, 128), (3, 5087)]):
            p = int(pos[(37 * k + 11 + t) % len(pos)])
            add("short", t, p - L // 2, p - L // 2 + L - 1, ss)
            g = gaps[(k + 5) % len(gaps)]
            add("short", t, g + 10, g + 10 + L - 1, ss)
        # snps: SNP-driven window counts, and no SNP at all
        for s, e in [(1, CHR_LEN - 1), (50_000, 150_000), (100_000, 140_000), (200_000, 230_000), (10_000, 399_000)]:
            add("snps", t, s, e, 20)
        for k in range(5):
            g = gaps[k]
            add("snps", t, g + 1, g + 380, [20, 5, 64, 1, 100][k])
        # edges: a SNP on a window's start (the region starts at it; window 5 starts at it) and on a window's end
        for k in range(6):
            p = int(pos[(53 * k + 7 + t) % len(pos)])
            add("edges", t, p, p + 99, 10)
            add("edges", t, p - 100, p + 99, 10)
            add("edges", t, p - 39, p + 10, 25)
        # hole and past the map
        for s, e, ss in [(301_000, 305_000, 20), (299_000, 307_000, 40), (300_000, 305_999, 13), (295_000, 310_000, 64),
                         (399_000, 400_600, 20), (400_100, 401_000, 20), (399_990, 400_010, 30), (CHR_LEN, CHR_LEN + 57, 29)]:
            add("hole", t, s + t, e + t, ss)
        # large coordinates: around every power of ten, and up to 2^31 - 2
        for k in range(1, 10):
            add("large", t, 10 ** k - 6 + t, 10 ** k + 5 + t, 12)
            add("large", t, 10 ** k - 3, 10 ** k + 40 + t, 5)
        add("large", t, 2 ** 31 - 49 - t, 2 ** 31 - 2, 24)
        add("large", t, 2 ** 31 - 1200, 2 ** 31 - 2 - t, 60)
        add("large", t, 0, 9 + t, 10)
        add("large", t, 3_000_000_000 % (2 ** 31) - 5, 3_000_000_000 % (2 ** 31) + 900, 14)
    # dups (table 1): regions around the duplicated positions
    p1 = tables[1]["pos"].astype(np.int64)
    dup = np.unique(p1[1:][p1[1:] == p1[:-1]])
    for k, p in enumerate(dup[:16]):
        add("dups", 1, p - 2, p + 2, 20)
        add("dups", 1, p - 500 - k, p + 700, 20)
        add("dups", 1, p, p, 3)
    rng = np.random.default_rng(5)
    for t in range(2):
        s = rng.integers(1000, CHR_LEN - 60_000, 40)
        ln = rng.choice([300, 1500, 2500, 8000, 30_000, 55_000], 40)
        for a, b in zip(s, s + ln):
            add("random", t, a, b, 20)
    return out


def device_tables(tables, regions):
    """The arrays of csvgpu_cn_observations_resident_many for `regions` (sorted by table = shard) -> dict."""
    regions = sorted(regions, key=lambda r: r["table"])
    reg_off = [0]
    for t in range(len(tables)):
        reg_off.append(reg_off[-1] + sum(1 for r in regions if r["table"] == t))
    sp, sb, sf, so = [], [], [], [0]
    for r in regions:
        p, b, f = flat_snps(tables[r["table"]], r["start"], r["end"])
        sp.append(p); sb.append(b); sf.append(f); so.append(so[-1] + len(p))
    cat = lambda v, dt: np.concatenate(v).astype(dt) if v else np.zeros(0, dt)
    return {"regions": regions, "reg_off": np.asarray(reg_off, np.uint64),
            "region_start": np.asarray([r["start"] for r in regions], np.uint32), "region_end": np.asarray([r["end"] for r in regions], np.uint32),
            "sample_size": np.asarray([r["ss"] for r in regions], np.int32), "snp_off": np.asarray(so, np.uint64),
            "snp_pos": cat(sp, np.uint32), "snp_baf": cat(sb, np.float64), "snp_pfb": cat(sf, np.float64)}
