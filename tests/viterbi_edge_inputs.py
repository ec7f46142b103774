"""Seeded inputs shared by tests/test_viterbi_ref.py (host: what the families claim) and tests/test_gpu_viterbi_edges.py (device)."""
import numpy as np

from hmm_params import TIE_OBS

TIE_T = (1, 2, 25, 513)
PACK_PROBE_T = (1, 25, 511, 512, 513)            # around VIT_LDS_T = 512 of kernels/hmm.hip
PACK_MATE_T = (0, 1, 511, 512, 513, 1200)
PACK_N_SEQ = (1, 9, 10, 11, 20, 21)              # around the 10 sequences of a wave


def _obs(rng, T, mode):
    """the observations of test_gpu_parity.test_viterbi_matches_oracle"""
    o1 = rng.normal(0, 0.4, T)
    if mode == "del": o1 -= 0.8
    if mode == "dup": o1 += 0.45
    o2 = np.where(rng.random(T) < 0.5, -1.0, rng.choice([0.0, 1.0, 0.5, 0.33, 0.25, 0.75], T) + rng.normal(0, 0.03, T) * (rng.random(T) < 0.7))
    o2 = np.where((o2 != -1) & (o2 < 0), 0.0, o2); o2 = np.where(o2 > 1, 1.0, o2)
    pfb = np.where(o2 == -1, 0.5, rng.choice([0.0, 0.5, 0.1, 0.93], T))
    return o1, o2, pfb


def _cat(seqs):
    off = np.zeros(len(seqs) + 1, np.int64)
    off[1:] = np.cumsum([len(s[0]) for s in seqs])
    o1, o2, pfb = (np.concatenate([np.asarray(s[k], np.float64) for s in seqs]) if seqs else np.zeros(0) for k in range(3))
    return o1, o2, pfb, off


def random_family(seed):
    rng = np.random.default_rng(seed)
    return _cat([_obs(rng, T, mode) for T, mode in [(1, "n"), (2, "del"), (20, "n"), (20, "del"), (20, "dup"), (200, "dup"), (0, "n"), (1000, "del"), (37, "n")]])


def hostile_family(seed):
    """the draw of test_gpu_hostile.test_window_and_viterbi_on_extreme_values: clamped constants, BAF and frequencies of exactly 0 and 1"""
    rng = np.random.default_rng(seed)
    seqs = []
    for j in range(30):
        T = int(rng.choice([0, 1, 2, 3, 20, 200]))
        o1 = [rng.normal(0, 0.4, T), rng.choice([-50.0, -9.966, 0.0, 5.0, 50.0], T), np.zeros(T)][j % 3]
        seqs.append((o1, rng.choice([-1.0, 0.0, 1.0, 0.5, 1e-12, 1 - 1e-12, 0.3333], T), rng.choice([0.0, 1.0, 0.5, 0.01, 0.99, 1e-9], T)))
    return _cat(seqs)


def tie_batch(name):
    """No-BAF sequences of T = 1, 2, 25, 513 whose log2 ratios sit on the tied states (`on`) with stretches on state 3 (`off`) between,
    so the tie decides at initialisation, on entering, inside and on leaving the tied states, and at termination."""
    on, off = TIE_OBS[name]
    rng = np.random.default_rng(len(name))
    near = lambda v, T: v + rng.choice([0.0, 0.0, -0.02, 0.01], T)
    seqs = []
    for T in TIE_T:
        if T <= 2:
            o1 = np.full(T, on)
        elif T == 25:
            o1 = np.concatenate([near(off, 6), near(on, 14), near(off, 5)])
        else:
            parts = []
            while sum(map(len, parts)) < T:
                parts += [near(off, int(rng.integers(5, 40))), near(on, int(rng.integers(14, 60)))]
            o1 = np.concatenate(parts)[:T]
        seqs.append((o1, np.full(T, -1.0), np.full(T, 0.5)))
    return _cat(seqs)


def degenerate_batch():
    """short sequences over the values at which hmm_params.DEGENERATE_MODELS degenerate: log2 ratios on and far off the means, BAF of
    exactly 0 and 1, within 1e-12 of them, and far from every mean (7.5, -3.0: no pdf survives there)"""
    rng = np.random.default_rng(23)
    seqs = []
    for j, T in enumerate([1, 1, 2, 3, 3, 25, 25, 60, 60, 0, 1, 25]):
        o1 = rng.choice([-3.739099, -0.727964, 0.0, 0.2, 0.395454, 0.658622, -50.0, 5.0], T)
        if j % 4 == 1:
            o1 = np.full(T, 0.2)                   # off every mean: with B1_uf = 0 and sharp peaks every state is -inf
        o2 = rng.choice([-1.0, -1.0, 0.0, 1.0, 1e-12, 1 - 1e-12, 0.5, 0.12, 7.5, -3.0, 0.3333], T)
        if j % 4 == 2:
            o2 = np.full(T, -1.0)
        seqs.append((o1, o2, rng.choice([0.0, 1.0, 0.5, 0.01, 0.93], T)))
    return _cat(seqs)


def window_inputs():
    """the inputs of test_gpu_parity.test_window_log2_matches_oracle: a stretch of zero coverage, a region past the map's end (windows
    with no position), one with a step below 1, a one-position region"""
    rng = np.random.default_rng(3)
    depth = rng.poisson(30, 300_000).astype(np.uint32)
    depth[50_000:60_000] = 0
    rs = np.array([1000, 40_000, 52_000, 299_000, 100, 7, 120_000], np.uint32)
    re = np.array([21_000, 140_000, 58_000, 305_000, 110, 7, 120_019], np.uint32)
    ssz = np.array([20, 137, 20, 20, 20, 20, 20], np.int32)
    return depth, rs, re, ssz, 29.7


def pack_probes():
    """the five probe sequences whose answers must not depend on where they sit"""
    rng = np.random.default_rng(77)
    return [_obs(rng, T, mode) for T, mode in zip(PACK_PROBE_T, ("dup", "del", "n", "dup", "del"))]


def pack_calls(n_seq):
    """Calls of n_seq sequences: each probe at each slot of a wave (index % 10) the call has room for, its wave-mates drawn from
    PACK_MATE_T; alternately without a mate above 512 (the wave keeps its back-pointers in LDS unless the probe itself is 513) and with a
    1200 mate in the probe's wave (global psi). -> [(probe number, index in the call, sequences)]"""
    rng = np.random.default_rng(1000 + n_seq)
    probes = pack_probes()
    mates = {T: [_obs(rng, T, m) for m in ("n", "del", "dup")] for T in PACK_MATE_T}
    pick = lambda T: mates[int(T)][int(rng.integers(3))]
    calls = []
    for p in range(len(probes)):
        for slot in range(min(n_seq, 10)):
            waves = (n_seq + 9) // 10
            w = int(rng.integers(waves))
            while 10 * w + slot >= n_seq:
                w -= 1
            idx = 10 * w + slot
            long_mate = (slot + n_seq + p) % 2 == 1 and n_seq > 1
            others = [i for i in range(10 * w, min(10 * w + 10, n_seq)) if i != idx]
            long_mate = long_mate and bool(others)
            seqs = [pick(rng.choice(PACK_MATE_T if i // 10 != w or long_mate else PACK_MATE_T[:4])) for i in range(n_seq)]
            if long_mate:
                seqs[int(rng.choice(others))] = pick(1200)
            seqs[idx] = probes[p]
            calls.append((p, idx, seqs))
    return calls


cat = _cat
