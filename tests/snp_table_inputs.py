"""Inputs of the resident SNP table tests (tests/test_snp_table_inputs.py checks the statements below on the CPU against the existing
loop statement of SNPTable::queryFlat and against the host mirror's SNPFile; tests/test_gpu_snp_table.py runs them through
csvgpu_snp_table_query): table and region families, and a numpy statement of what SNPSource::queryFlat appends for a region, for both
kinds of table.

  per-record kind  dict(pos, baf, pfb, has_pfb)   SNPTable::queryFlat (host/cnv_caller.cpp)
  first-hit kind   dict(pos, baf, af_pos, af)      the default SNPSource::queryFlat over SNPFileTable::query (host/snp_io.cpp)

Both: the records from lower_bound(pos, start) up to the first pos > end; every member of a run of equal positions answers with the baf
of the run's last member. Values travel as bits (a NaN stays that NaN), so the statements move uint64 views.
"""
import numpy as np

NAN_A = np.frombuffer(np.uint64(0x7ff8_0000_0000_1234).tobytes(), np.float64)[0]      # two NaNs with payloads of their own
NAN_B = np.frombuffer(np.uint64(0xfff0_0000_dead_beef).tobytes(), np.float64)[0]
POS_MAX = 2 ** 31 - 2
SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257)
BIG_N = 70_001


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def resolve_records(t):
    """-> (baf, pfb) per record of a per-record table, as every query answers them (uint64 bits)."""
    pos = np.asarray(t["pos"], np.uint32)
    n = len(pos)
    if n == 0:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    last = np.searchsorted(pos, pos, "right") - 1                     # the run's last member
    baf = _bits(t["baf"])[last]
    has = np.zeros(n, bool) if t.get("has_pfb") is None else np.asarray(t["has_pfb"]) != 0
    pfb_in = np.zeros(n, np.uint64) if t.get("pfb") is None else _bits(t["pfb"])
    flagged = np.maximum.accumulate(np.where(has, np.arange(1, n + 1), 0))[last]      # last flagged index + 1 at or in front of the run's end
    in_run = (flagged > 0) & (pos[np.maximum(flagged, 1) - 1] == pos)
    pfb = np.where(in_run, pfb_in[np.maximum(flagged, 1) - 1], np.uint64(0))
    return baf, pfb


def query(kind, t, start, end, resolved=None):
    """One region -> (pos uint32, baf bits, pfb bits)."""
    pos = np.asarray(t["pos"], np.uint32)
    if start > end:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint64)
    a, b = int(np.searchsorted(pos, start, "left")), int(np.searchsorted(pos, end, "right"))
    if kind == "records":
        baf, pfb = resolved if resolved is not None else resolve_records(t)
        return pos[a:b].copy(), baf[a:b].copy(), pfb[a:b].copy()
    last = np.searchsorted(pos, pos[a:b], "right") - 1
    baf = _bits(t["baf"])[last]
    pfb = np.zeros(b - a, np.uint64)
    af_pos = np.asarray(t["af_pos"], np.uint32)
    if b > a and len(af_pos):
        lo, hi = pos[a], pos[b - 1]
        g = int(np.searchsorted(af_pos, lo, "left"))
        if g < len(af_pos) and af_pos[g] <= hi:
            pfb[pos[a:b] == af_pos[g]] = _bits(t["af"])[g]
    return pos[a:b].copy(), baf, pfb


def query_many(kind, t, starts, ends):
    """-> dict(snp_off uint64 [R + 1], pos, baf, pfb): what csvgpu_snp_table_query returns (baf / pfb as float64 with the same bits)."""
    resolved = resolve_records(t) if kind == "records" else None
    parts = [query(kind, t, int(s), int(e), resolved) for s, e in zip(starts, ends)]
    off = np.concatenate([[0], np.cumsum([len(p[0]) for p in parts])]).astype(np.uint64)
    cat = lambda i, dt: np.concatenate([p[i] for p in parts]).astype(dt) if parts else np.zeros(0, dt)
    return {"snp_off": off, "pos": cat(0, np.uint32), "baf": cat(1, np.uint64).view(np.float64), "pfb": cat(2, np.uint64).view(np.float64)}


# ---- tables --------------------------------------------------------------------------------------------------------------------------------
def _values(rng, n):
    v = rng.uniform(0, 1, n)
    if n >= 3:
        v[rng.integers(0, n)] = NAN_A
        v[rng.integers(0, n)] = NAN_B
    return v


def random_records(seed, n, span=None, dup=0.2):
    """n records over `span` positions; about `dup` of them repeat their predecessor's position."""
    rng = np.random.default_rng(seed)
    span = span or max(4 * n, 8)
    pos = np.sort(rng.integers(0, span, n)).astype(np.uint32)
    for i in np.nonzero(rng.random(n) < dup)[0]:
        if i:
            pos[i] = pos[i - 1]
    pos = np.sort(pos)
    return {"pos": pos, "baf": _values(rng, n), "pfb": _values(rng, n), "has_pfb": (rng.random(n) < 0.4).astype(np.uint8)}


def random_hits(seed, n, n_af=None, span=None):
    rng = np.random.default_rng(seed + 1000)
    t = random_records(seed, n, span)
    span = span or max(4 * n, 8)
    n_af = n // 2 + 1 if n_af is None else n_af
    on = rng.choice(t["pos"], n_af // 2) if n else np.zeros(0, np.uint32)
    af_pos = np.sort(np.concatenate([on, rng.integers(0, span, n_af - len(on))])).astype(np.uint32)
    return {"pos": t["pos"], "baf": t["baf"], "af_pos": af_pos, "af": _values(rng, n_af)}


def record_tables():
    """name -> per-record table: the families of the issue."""
    out = {"empty": {"pos": np.zeros(0, np.uint32), "baf": np.zeros(0), "pfb": np.zeros(0), "has_pfb": np.zeros(0, np.uint8)},
           "one": {"pos": np.asarray([500], np.uint32), "baf": np.asarray([0.25]), "pfb": np.asarray([0.7]), "has_pfb": np.asarray([1], np.uint8)},
           "one_position": {"pos": np.full(300, 1234, np.uint32), "baf": np.linspace(0, 1, 300), "pfb": np.linspace(1, 0, 300),
                            "has_pfb": (np.arange(300) == 17).astype(np.uint8)},
           "extremes": {"pos": np.asarray([0, 0, 7, POS_MAX, POS_MAX], np.uint32), "baf": np.asarray([0.1, 0.2, NAN_A, 0.4, NAN_B]),
                        "pfb": np.asarray([0.5, NAN_B, 0.7, 0.8, 0.9]), "has_pfb": np.asarray([1, 1, 0, 1, 0], np.uint8)}}
    # runs of 2 and 3 with has_pfb on the first / middle / last / none, singles between them
    pos, has = [], []
    p = 100
    for run, flags in [(2, (1, 0)), (2, (0, 1)), (2, (0, 0)), (2, (1, 1)), (3, (1, 0, 0)), (3, (0, 1, 0)), (3, (0, 0, 1)), (3, (0, 0, 0)), (3, (1, 0, 1))]:
        pos += [p] * run + [p + 5]
        has += list(flags) + [run % 2]
        p += 10
    n = len(pos)
    out["runs"] = {"pos": np.asarray(pos, np.uint32), "baf": np.arange(n) / n, "pfb": 0.5 + np.arange(n) / (4 * n), "has_pfb": np.asarray(has, np.uint8)}
    t = random_records(3, 64)
    out["no_pfb"] = {"pos": t["pos"], "baf": t["baf"], "pfb": None, "has_pfb": None}
    out["no_flags"] = {"pos": t["pos"], "baf": t["baf"], "pfb": t["pfb"], "has_pfb": None}
    out["flags_no_values"] = {"pos": t["pos"], "baf": t["baf"], "pfb": None, "has_pfb": t["has_pfb"]}
    for n in SIZES:
        out["n%d" % n] = random_records(40 + n, n)
    return out


def hit_tables():
    """name -> first-hit table."""
    pos = np.asarray([100, 200, 200, 300, 400, 400, 400, 500], np.uint32)
    baf = np.asarray([0.1, 0.2, 0.3, NAN_A, 0.5, 0.6, 0.7, 0.8])
    out = {"empty": {"pos": np.zeros(0, np.uint32), "baf": np.zeros(0), "af_pos": np.asarray([5], np.uint32), "af": np.asarray([0.5])},
           "no_af": {"pos": pos, "baf": baf, "af_pos": np.zeros(0, np.uint32), "af": np.zeros(0)},
           # population records: in front of everything, between records (a hit position that is not a record), on records, a NaN, behind everything
           "edges": {"pos": pos, "baf": baf, "af_pos": np.asarray([50, 99, 100, 250, 300, 400, 400, 501, 900], np.uint32),
                     "af": np.asarray([0.01, 0.02, 0.03, 0.04, NAN_B, 0.06, 0.07, 0.08, 0.09])}}
    for n in SIZES:
        out["n%d" % n] = random_hits(70 + n, n)
    return out


# ---- regions -------------------------------------------------------------------------------------------------------------------------------
def regions_for(t, seed=0, n_random=40):
    """(starts, ends) for a table: regions that start or end exactly on a run, between records, before the first and after the last,
    start == end, start > end, at 0 and at 2^31 - 2, for the first-hit kind around every population record, and random ones."""
    rng = np.random.default_rng(seed)
    pos = np.asarray(t["pos"], np.int64)
    pts = {0, 1, POS_MAX - 1, POS_MAX}
    for p in np.unique(pos)[:: max(1, len(np.unique(pos)) // 12)]:
        pts |= {int(p) - 1, int(p), int(p) + 1}
    for p in np.asarray(t.get("af_pos", []), np.int64)[:12]:
        pts |= {int(p) - 1, int(p), int(p) + 1}
    if len(pos):
        pts |= {int(pos[0]) - 1, int(pos[0]), int(pos[-1]), int(pos[-1]) + 1}
    pts = sorted(p for p in pts if 0 <= p <= POS_MAX)
    pairs = [(a, b) for a in pts for b in pts if a <= b][:400]
    pairs += [(b, a) for a, b in pairs[1:40:3] if a != b]                      # start > end
    pairs += [(p, p) for p in pts]
    hi = int(pos[-1]) + 10 if len(pos) else 100
    for _ in range(n_random):
        a = int(rng.integers(0, hi))
        pairs.append((a, min(POS_MAX, a + int(rng.integers(0, max(2, hi // 3))))))
    s, e = np.asarray([p[0] for p in pairs], np.uint32), np.asarray([p[1] for p in pairs], np.uint32)
    return s, e


def random_regions(seed, R, hi):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, hi, R)
    e = s + rng.integers(0, max(2, hi // 50), R)
    swap = rng.random(R) < 0.02                                               # a few with start > end
    s2, e2 = np.where(swap, e + 1, s), np.where(swap, s, e)
    return s2.astype(np.uint32), np.minimum(e2, POS_MAX).astype(np.uint32)
