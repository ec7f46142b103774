"""kernels/hmm.hip where the parity tests cannot see it: emission values (the kc.cpp chain of the state-1 constant included) against the
decimal reference of tests/viterbi_ref.py, the lowest-index tie rule against khmm.cpp's loop, models with zero probabilities, the
10-sequences-per-wave packing around the LDS back-pointer limit, and window_log2 against exact values. tests/test_viterbi_ref.py proves
on the host that these inputs are sensitive to what they guard."""
import numpy as np
import pytest

import viterbi_edge_inputs as vi
import viterbi_ref as vr
from contextsv_amd import make_hmm
from hmm_params import WGS_HMM, WGS_TEST_HMM, CDF_SETS, TIE_MODELS, DEGENERATE_MODELS

pytestmark = pytest.mark.gpu

PROBED = dict(WGS_HMM=WGS_HMM, WGS_TEST_HMM=WGS_TEST_HMM, **CDF_SETS)


def _u64(a):
    return np.asarray(a, np.uint64)


# ---- a. emission probes

@pytest.fixture(scope="module")
def probe_refs():
    """decimal emissions of every probe, once per parameter set"""
    return {name: vr.probe_reference(p)[0] for name, p in PROBED.items()}


@pytest.mark.parametrize("name", list(PROBED))
def test_emission_probes_match_decimal_reference(ctx, probe_refs, name):
    """pi one-hot on state k, T = 1: loglik is log(1) + biot[k]. Held to 8 * E_HOST, E_HOST being the host oracle's own distance from the
    same reference. On the cdf sets the state-1 probes with a BAF of exactly 0 or 1 are kernel kc_cdf_normal against the reference's
    kc.cpp (tests/golden/kc_normal.json)."""
    params = PROBED[name]
    grid = vr.probe_grid()
    o1, o2, pfb = (np.array(c) for c in zip(*grid))
    off = _u64(np.arange(len(grid) + 1))
    worst = 0.0
    for k in range(1, 7):
        st, ll = ctx.viterbi(make_hmm(**vr.one_hot(params, k)), o1, o2, pfb, off)
        assert np.all(st == k), (name, k)
        err = np.abs(ll - np.array(probe_refs[name][k - 1]))
        n = int(np.argmax(err))
        print(f"{name} state {k}: max |device - reference| {err[n]:.3e} ({err[n] / vr.E_HOST:.2f} E_HOST) at probe {grid[n]}")
        worst = max(worst, float(err[n]))
        assert err[n] <= 8 * vr.E_HOST, (name, k, grid[n], float(ll[n]), probe_refs[name][k - 1][n])
    if name in CDF_SETS:
        assert vr.kc_cdf_normal(0.0, params["B2_mean"][4], params["B2_sd"][4]) > 0.02      # the constant carries weight in these probes


# ---- b. tie rule

@pytest.mark.parametrize("name", list(TIE_MODELS))
def test_ties_go_to_the_lowest_state(ctx, oracle, name):
    params = TIE_MODELS[name]
    hmm = make_hmm(**params)
    o1, o2, pfb, off = vi.tie_batch(name)
    st, ll = ctx.viterbi(hmm, o1, o2, pfb, _u64(off))
    strict, rll = vr.viterbi_batch(params, o1, o2, pfb, off, strict=True)
    ost, oll = oracle.viterbi(hmm, o1, o2, pfb, _u64(off))
    for a, b in zip(off[:-1], off[1:]):
        assert st[a:b].tolist() == strict[a:b], (name, int(b - a))
    assert np.array_equal(st, ost)
    np.testing.assert_allclose(ll, oll, rtol=0, atol=1e-6)
    np.testing.assert_allclose(ll, rll, rtol=0, atol=1e-6)
    if name == "UNIFORM":
        assert np.all(st == 1)


# ---- c. degenerate models

@pytest.mark.parametrize("name", list(DEGENERATE_MODELS))
def test_degenerate_models_match_oracle(ctx, oracle, name):
    hmm = make_hmm(**DEGENERATE_MODELS[name])
    o1, o2, pfb, off = vi.degenerate_batch()
    st, ll = ctx.viterbi(hmm, o1, o2, pfb, _u64(off))
    ost, oll = oracle.viterbi(hmm, o1, o2, pfb, _u64(off))
    assert np.array_equal(st, ost)
    np.testing.assert_allclose(ll, oll, rtol=0, atol=1e-6, equal_nan=True)


# ---- d. packing and the LDS seam

@pytest.fixture(scope="module")
def probes_alone(ctx, oracle):
    """each packing probe as the only sequence of a call, checked against the oracle: what every placement must reproduce bit for bit"""
    hmm = make_hmm(**WGS_HMM)
    alone = []
    for o1, o2, pfb in vi.pack_probes():
        off = _u64([0, len(o1)])
        st, ll = ctx.viterbi(hmm, o1, o2, pfb, off)
        ost, oll = oracle.viterbi(hmm, o1, o2, pfb, off)
        assert np.array_equal(st, ost) and abs(ll[0] - oll[0]) <= 1e-6
        alone.append((st.copy(), ll.copy()))
    return alone


@pytest.mark.parametrize("n_seq", vi.PACK_N_SEQ)
def test_answer_is_independent_of_slot_and_wave_mates(ctx, oracle, probes_alone, n_seq):
    """Every probe (T = 1, 25, 511, 512, 513) at every slot of a wave, among mates of 0, 1, 511, 512, 513 and 1200 observations, so the
    wave keeps its back-pointers in LDS in one placement and in global memory in another: the probe's path is identical and its
    log-likelihood bitwise equal (its DP is the same instruction stream wherever it sits), and the whole call equals the oracle."""
    hmm = make_hmm(**WGS_HMM)
    calls = vi.pack_calls(n_seq)
    assert {idx % 10 for _, idx, _ in calls} == set(range(min(n_seq, 10)))
    for p, idx, seqs in calls:
        o1, o2, pfb, off = vi.cat(seqs)
        st, ll = ctx.viterbi(hmm, o1, o2, pfb, _u64(off))
        a, b = int(off[idx]), int(off[idx + 1])
        assert np.array_equal(st[a:b], probes_alone[p][0]), (p, idx)
        assert ll[idx:idx + 1].tobytes() == probes_alone[p][1].tobytes(), (p, idx, float(ll[idx]), float(probes_alone[p][1][0]))
        ost, oll = oracle.viterbi(hmm, o1, o2, pfb, _u64(off))
        assert np.array_equal(st, ost), (p, idx)
        np.testing.assert_allclose(ll, oll, rtol=0, atol=1e-6)
        empty = np.diff(off) == 0
        assert np.all(ll[empty] == -vr.VITHUGE)


def test_zero_length_sequences_and_waves(ctx, oracle, probes_alone):
    """a wave made only of zero-length sequences between two that work, and a zero-length sequence first and last in a call"""
    hmm = make_hmm(**WGS_HMM)
    probes = vi.pack_probes()
    none = (np.zeros(0), np.zeros(0), np.zeros(0))
    layouts = [[none] * 10,
               [none] + [probes[1]] * 9 + [none] * 10 + [probes[3], none],
               [none, probes[4], none],
               [none] * 9 + [probes[2]] + [none] * 11]
    where = [[], [(1, 1), (3, 20)], [(4, 1)], [(2, 9)]]
    for seqs, placed in zip(layouts, where):
        o1, o2, pfb, off = vi.cat(seqs)
        st, ll = ctx.viterbi(hmm, o1, o2, pfb, _u64(off))
        ost, oll = oracle.viterbi(hmm, o1, o2, pfb, _u64(off))
        assert np.array_equal(st, ost)
        np.testing.assert_allclose(ll, oll, rtol=0, atol=1e-6)
        assert np.all(ll[np.diff(off) == 0] == -vr.VITHUGE)
        for p, idx in placed:
            assert np.array_equal(st[int(off[idx]): int(off[idx + 1])], probes_alone[p][0])
            assert ll[idx:idx + 1].tobytes() == probes_alone[p][1].tobytes()


# ---- e. window_log2 values

def test_window_log2_matches_exact_values(ctx):
    """window_log2_kernel against integer sums, decimal division and log2, on the windows of test_window_log2_matches_oracle; held to
    8 * E_LOG2_HOST, the host oracle's own distance from the same values, times 8"""
    depth, rs, re, ssz, mean = vi.window_inputs()
    l2, ws, we, off = ctx.window_log2(depth, rs, re, ssz, mean)
    zero_sum = zero_cnt = 0
    for r in range(len(rs)):
        exact, zs, zc = vr.window_log2_exact(depth, int(rs[r]), int(re[r]), int(ssz[r]), mean)
        zero_sum += zs; zero_cnt += zc
        got = l2[int(off[r]): int(off[r + 1])]
        err = vr.log2_error(got, exact)
        print(f"region {r}: max scaled |device - exact| {err.max():.3e} ({err.max() / vr.E_LOG2_HOST:.2f} E_LOG2_HOST)")
        assert err.max() <= 8 * vr.E_LOG2_HOST, (r, int(np.argmax(err)))
        assert np.all(got[np.array(exact) == 0.0] == 0.0)
    assert zero_sum > 0 and zero_cnt > 0
