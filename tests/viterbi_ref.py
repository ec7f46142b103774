"""A plain reference for the Viterbi path of khmm.cpp, independent of oracle/csv_oracle.c and of the device code.

Emissions (b1iot / b2iot, khmm.cpp:58-206) are evaluated in `decimal` at 50 digits from the closed-form formulas, on the exact values of
the float64 inputs, and rounded to float64 once at the end. The one quantity that is not a high-precision one is the state-1 constant
cdf_normal(0, B2_mean[4], B2_sd[4]): kc.cpp's series stop at EPS = 3e-7 by design, so its value is what the reference's own kc.cpp
returned (tests/golden/kc_normal.json), never what the oracle or the device computes.

The DP (khmm.cpp:323-381) is the reference's loop in float64, state by state: log(A), the pi == 0 -> 1e-9 floor, maxval = -VITHUGE and
ind = 1 defaults, strict '>', termination, backtrack. `strict=False` ('>=') exists only so that the tests can prove an input is
tie-sensitive.

Also here: the exact value of a window's log2 coverage ratio (cnv_caller.cpp:76-113) and the measured error of the host oracle against
both, which bound what the device may differ by."""
import functools
import json
import math
import os
from decimal import Decimal, localcontext

import numpy as np

PREC = 50
VITHUGE = 100000000000.0
FLOAT_MINIMUM = Decimal(1.175494351e-38)
PROB_MAX = Decimal(0.9999999999999999)
KC_PI = Decimal(3.141592653579893)        # kc.cpp:150: truncated, not pi; the exact value of that double
LOG_PI_FLOOR = math.log(1e-9)

# Measured on the host (tests/test_viterbi_ref.py::test_oracle_emissions_within_E_host): the largest |oracle - this reference| over the
# probe grid below, all seven probed parameter sets and six states (23 562 probes). It is 1 ulp of the largest magnitudes in the grid
# (8 <= |log-likelihood| < 16, ulp 1.776e-15): glibc's exp and log stay under 1 ulp and a probe is the rounded sum of two logs. The
# device is held to 8 * E_HOST (tests/test_gpu_viterbi_edges.py).
E_HOST = 1.7763568394002505e-15
# The same for window_log2 on the windows of test_window_log2_matches_oracle: the oracle against integer sum, decimal division and log2,
# as log2_error() below measures it: relative to max(1, |exact|). The values run from ~0.01 to the zero-coverage windows'
# log2(1e-9 / n / mean) ~ -43: the rounding of the result grows with the value (1 ulp of 43 is 7.1e-15), while the two roundings of
# the argument's divisions cost 2^-53 / ln 2 each in absolute terms however small the value is, so neither a plain absolute nor a plain
# relative error fits both ends. Measured: 2.17e-16 (test_oracle_window_log2_within_E_log2_host). The device is held to 8 * E_LOG2_HOST.
E_LOG2_HOST = 2.1684043449710089e-16

PROBE_O1 = (-50.0, -3.739099, -1.0, -0.727964, -0.3, 0.0, 0.2, 0.395454, 0.5, 0.658622, 5.0)     # below, on and above the clamp
PROBE_O2 = (-1.0, 0.0, 1.0, 1e-12, 0.1, 0.25, 0.3333, 0.5, 0.62, 0.9, 1 - 1e-12)
PROBE_PFB = (0.0, 1.0, 0.5, 0.01, 0.93)

_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kc_normal.json")


@functools.lru_cache(maxsize=None)
def _kc_cdf_table():
    with open(_GOLDEN) as f:
        return {(v["x"], v["mu"], v["sigma"]): v["cdf"] for v in json.load(f)["values"]}


def kc_cdf_normal(x, mu, sd):
    """cdf_normal as the reference's kc.cpp returns it (recorded); an argument that was not recorded is an error."""
    return _kc_cdf_table()[(float(x), float(mu), float(sd))]


def _pow(x, n):
    r = Decimal(1)                        # x**0 is 1 also for x == 0, which Decimal refuses
    for _ in range(n):
        r *= x
    return r


@functools.lru_cache(maxsize=None)
def _pdf(x, mu, sd):
    """pdf_normal (kc.cpp:2658) with the reference's PI; arguments are Decimals"""
    return (-(x - mu) * (x - mu) / (2 * sd * sd)).exp() / (sd * (2 * KC_PI).sqrt())


def _log_float(p):
    """float64 of log(p); a p below the float64 range is the 0 it is there"""
    if float(p) == 0.0:
        return Decimal("-Infinity")
    return p.ln()


@functools.lru_cache(maxsize=None)
def _b1(mean, sd, uf, state, o):
    with localcontext() as c:
        c.prec = PREC
        m = [Decimal(v) for v in mean]
        o = Decimal(o)
        if o < m[0]:
            o = m[0]
        elif o > m[5]:
            o = m[5]
        uf = Decimal(uf)
        pdf = _pdf(o, m[state - 1], Decimal(sd[state - 1]))
        if float(pdf) == 0.0:             # below the float64 range: the reference's exp() returns 0 there
            pdf = Decimal(0)
        return _log_float(uf + (1 - uf) * pdf)


@functools.lru_cache(maxsize=None)
def _b2(mean, sd, uf, state, pfb, b):
    with localcontext() as c:
        c.prec = PREC
        m, s = [Decimal(v) for v in mean], [Decimal(v) for v in sd]
        uf, pfb, b = Decimal(uf), Decimal(pfb), Decimal(b)
        q = 1 - pfb
        if state == 1:
            if b == 0 or b == 1:
                t = Decimal(kc_cdf_normal(0.0, mean[4], sd[4]))
            else:
                t = _pdf(b, m[4], s[4])
        else:
            n = {2: 1, 3: 2, 4: 1, 5: 3, 6: 4}[state]       # copies of the allele: a binomial mixture of n + 1 peaks
            if b == 0:
                t = _pow(q, n) / 2
            elif b == 1:
                t = _pow(pfb, n) / 2
            else:
                peak = {1: [(m[0], s[0]), (1 - m[0], s[0])],
                        2: [(m[0], s[0]), (m[3], s[3]), (1 - m[0], s[0])],
                        3: [(m[0], s[0]), (m[2], s[2]), (1 - m[2], s[2]), (1 - m[0], s[0])],
                        4: [(m[0], s[0]), (m[1], s[1]), (m[3], s[3]), (1 - m[1], s[1]), (1 - m[0], s[0])]}[n]
                t = sum(math.comb(n, k) * _pow(q, n - k) * _pow(pfb, k) * _pdf(b, *peak[k]) for k in range(n + 1))
        p = uf + (1 - uf) * t
        p = max(FLOAT_MINIMUM, min(PROB_MAX, p))
        return p.ln()


def emission_exact(params, state, o1, o2, pfb):
    """log b_state(O) of khmm.cpp:296-317 as a Decimal (not yet rounded); state is 1-based"""
    a = _b1(tuple(params["B1_mean"]), tuple(params["B1_sd"]), float(params["B1_uf"]), state, float(o1))
    if o2 == -1:
        return a
    with localcontext() as c:
        c.prec = PREC
        return a + _b2(tuple(params["B2_mean"]), tuple(params["B2_sd"]), float(params["B2_uf"]), state, float(pfb), float(o2))


def emissions(params, o1, o2, pfb):
    """T x 6 float64 log emissions"""
    return [[float(emission_exact(params, j, a, b, c)) for j in range(1, 7)] for a, b, c in zip(o1, o2, pfb)]


def _log(v):
    return math.log(v) if v > 0 else -math.inf


def viterbi(params, o1, o2, pfb, strict=True, biot=None):
    """ViterbiLogNP_CHMM of one sequence -> (states 1..6, log-likelihood)."""
    T = len(o1)
    if T == 0:
        return [], -VITHUGE
    better = (lambda v, m: v > m) if strict else (lambda v, m: v >= m)
    logA = [[_log(v) for v in row] for row in params["A"]]
    logpi = [math.log(1e-9 if v == 0 else v) for v in params["pi"]]
    if biot is None:
        biot = emissions(params, o1, o2, pfb)
    delta = [[0.0] * 6 for _ in range(T)]
    psi = [[0] * 6 for _ in range(T)]
    for i in range(6):
        delta[0][i] = logpi[i] + biot[0][i]
    for t in range(1, T):
        for j in range(6):
            maxval, ind = -VITHUGE, 1
            for i in range(6):
                val = delta[t - 1][i] + logA[i][j]
                if better(val, maxval):
                    maxval, ind = val, i + 1
            delta[t][j] = maxval + biot[t][j]
            psi[t][j] = ind
    q, final_lh = 1, -VITHUGE
    for i in range(6):
        if better(delta[T - 1][i], final_lh):
            final_lh, q = delta[T - 1][i], i + 1
    states = [0] * T
    states[T - 1] = q
    for t in range(T - 2, -1, -1):
        q = psi[t + 1][q - 1]
        states[t] = q
    return states, final_lh


def viterbi_batch(params, o1, o2, pfb, seq_off, strict=True):
    st, ll = [], []
    for a, b in zip(seq_off[:-1], seq_off[1:]):
        a, b = int(a), int(b)
        s, l = viterbi(params, o1[a:b], o2[a:b], pfb[a:b], strict)
        st.extend(s); ll.append(l)
    return st, ll


# ---- one-hot probes: with pi one-hot on state k and T = 1 the log-likelihood is log(1) + biot[k] exactly, provided state k still wins
# against the others' log(1e-9).

def probe_grid():
    """(o1, o2, pfb) of every probe; without BAF (o2 == -1) the population frequency is not read, so one pfb is enough"""
    return [(a, b, c) for a in PROBE_O1 for b in PROBE_O2 for c in (PROBE_PFB if b != -1 else PROBE_PFB[2:3])]


def one_hot(params, k):
    return dict(params, pi=[1.0 if i == k - 1 else 0.0 for i in range(6)])


def probe_reference(params):
    """-> (ref[k-1][n]: float64 log emission of state k at probe n, margin: the smallest lead of a probed state over another state, in
    nats, after the other's log(1e-9))"""
    grid = probe_grid()
    exact = [[emission_exact(params, k, *g) for g in grid] for k in range(1, 7)]
    margin = min(float(exact[k][n] - exact[j][n]) - LOG_PI_FLOOR for n in range(len(grid)) for k in range(6) for j in range(6) if j != k)
    return [[float(v) for v in row] for row in exact], margin


# ---- window log2 (cnv_caller.cpp:76-113), exact

def log2_error(got, exact):
    """|got - exact| / max(1, |exact|), elementwise (see E_LOG2_HOST)"""
    got, exact = np.asarray(got, np.float64), np.asarray(exact, np.float64)
    return np.abs(got - exact) / np.maximum(1.0, np.abs(exact))


def window_log2_exact(depth, start, end, sample_size, mean_cov):
    """float64 of the exact log2((sum / count) / mean_cov) of each window: positions by the reference's own double expression, integer
    sum, decimal division and log2. -> (values, n_zero_sum, n_zero_count)"""
    out, n_zero_sum, n_zero_cnt = [], 0, 0
    pos_step = float((end - start + 1) & 0xFFFFFFFF) / float(sample_size)
    with localcontext() as c:
        c.prec = PREC
        ln2 = Decimal(2).ln()
        for i in range(sample_size):
            total, cnt, j = 0, 0, 0
            while j < pos_step:
                pos = int(start + i * pos_step + j) & 0xFFFFFFFF
                if pos > end:
                    break
                if pos < len(depth):
                    total += int(depth[pos]); cnt += 1
                j += 1
            if cnt == 0:
                out.append(0.0); n_zero_cnt += 1
                continue
            if total == 0:
                n_zero_sum += 1
            s = Decimal(total) if total else Decimal(1e-9)
            out.append(float((s / cnt / Decimal(mean_cov)).ln() / ln2))
    return out, n_zero_sum, n_zero_cnt
