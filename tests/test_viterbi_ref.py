"""tests/viterbi_ref.py (decimal emissions, khmm.cpp's loop in plain Python) against the host oracle, and the proof that the input
families of tests/test_gpu_viterbi_edges.py do what they claim: the tie models are decided by the tie rule, the one-hot probes read one
emission exactly. No GPU."""
import numpy as np
import pytest

import viterbi_edge_inputs as vi
import viterbi_ref as vr
from contextsv_amd import make_hmm
from hmm_params import WGS_HMM, WGS_TEST_HMM, CDF_SETS, TIE_MODELS, DEGENERATE_MODELS

PROBED = dict(WGS_HMM=WGS_HMM, WGS_TEST_HMM=WGS_TEST_HMM, **CDF_SETS)


def _oracle_batch(oracle, params, o1, o2, pfb, off):
    st, ll = oracle.viterbi(make_hmm(**params), o1, o2, pfb, np.asarray(off, np.uint64))
    return st.tolist(), ll.tolist()


def test_cdf_sets_take_every_kc_branch():
    """the state-1 constant of each set, as the reference's kc.cpp returned it: visible (not 0) and on the branch its name says"""
    want = {"cdf_gser": (0.1587, 0.5), "cdf_gser_edge": (0.0478, 1.3889), "cdf_gcf": (0.02275, 2.0), "cdf_zero_arg": (0.5, 0.0), "cdf_positive": (0.7475, 0.2222)}
    for name, p in CDF_SETS.items():
        mu, sd = p["B2_mean"][4], p["B2_sd"][4]
        x = (0 - mu) / (sd * np.sqrt(2))
        assert abs(vr.kc_cdf_normal(0.0, mu, sd) - want[name][0]) < 5e-5, name
        assert abs(x * x - want[name][1]) < 1e-4, name
    assert vr.kc_cdf_normal(0.0, WGS_HMM["B2_mean"][4], WGS_HMM["B2_sd"][4]) == 0.0      # why the committed sets never showed it


@pytest.mark.parametrize("name", list(PROBED))
def test_oracle_emissions_within_E_host(oracle, name):
    """One-hot probes: pi one-hot on state k and T = 1 make loglik = biot[k]. Every probe must be valid (the probed state leads every other
    by more than log(1e-9) plus a 1 nat guard), and the oracle stays within the measured E_HOST of the decimal reference."""
    params = PROBED[name]
    ref, margin = vr.probe_reference(params)
    assert margin > 1.0, margin
    o1, o2, pfb = (np.array(c) for c in zip(*vr.probe_grid()))
    off = np.arange(len(o1) + 1)
    worst = 0.0
    for k in range(1, 7):
        st, ll = _oracle_batch(oracle, vr.one_hot(params, k), o1, o2, pfb, off)
        assert st == [k] * len(o1)
        worst = max(worst, float(np.max(np.abs(np.array(ll) - np.array(ref[k - 1])))))
    print(f"{name}: {6 * len(o1)} probes, margin {margin:.3f} nats, max |oracle - reference| {worst:.3e}")
    assert worst <= vr.E_HOST


def test_reference_dp_on_probe_is_the_emission():
    ref, _ = vr.probe_reference(WGS_HMM)
    for n, g in enumerate(vr.probe_grid()[::37]):
        for k in range(1, 7):
            st, ll = vr.viterbi(vr.one_hot(WGS_HMM, k), [g[0]], [g[1]], [g[2]])
            assert st == [k] and ll == ref[k - 1][37 * n]


@pytest.mark.parametrize("params", [WGS_HMM, WGS_TEST_HMM], ids=["wgs", "wgs_test"])
def test_reference_paths_match_oracle_random_families(oracle, params):
    """the sequences of test_viterbi_matches_oracle (one round of them) and a draw of the hostile test's clamped constants"""
    o1, o2, pfb, off = vi.random_family(5)
    st, ll = vr.viterbi_batch(params, o1, o2, pfb, off)
    ost, oll = _oracle_batch(oracle, params, o1, o2, pfb, off)
    assert st == ost
    np.testing.assert_allclose(ll, oll, rtol=0, atol=1e-9)
    o1, o2, pfb, off = vi.hostile_family(11)
    st, ll = vr.viterbi_batch(params, o1, o2, pfb, off)
    ost, oll = _oracle_batch(oracle, params, o1, o2, pfb, off)
    assert st == ost
    np.testing.assert_allclose(ll, oll, rtol=0, atol=1e-9)


@pytest.mark.parametrize("name", list(TIE_MODELS))
def test_tie_models_are_tie_sensitive(oracle, name):
    params = TIE_MODELS[name]
    o1, o2, pfb, off = vi.tie_batch(name)
    strict, ll = vr.viterbi_batch(params, o1, o2, pfb, off, strict=True)
    loose, _ = vr.viterbi_batch(params, o1, o2, pfb, off, strict=False)
    for a, b in zip(off[:-1], off[1:]):
        assert strict[a:b] != loose[a:b], (name, b - a)           # every sequence, T = 1 included, is decided by the tie rule
    ost, oll = _oracle_batch(oracle, params, o1, o2, pfb, off)
    assert strict == ost
    np.testing.assert_allclose(ll, oll, rtol=0, atol=1e-9)
    if name == "UNIFORM":
        assert set(strict) == {1}
    if name == "TWIN_56":
        assert 5 in strict and 6 not in strict and 6 in loose
    if name == "TWIN_12":
        assert 1 in strict and 2 not in strict and 2 in loose
    if name == "TRIPLE_456":
        assert 4 in strict and not {5, 6} & set(strict) and 6 in loose


@pytest.mark.parametrize("name", list(DEGENERATE_MODELS))
def test_reference_paths_match_oracle_degenerate(oracle, name):
    params = DEGENERATE_MODELS[name]
    o1, o2, pfb, off = vi.degenerate_batch()
    st, ll = vr.viterbi_batch(params, o1, o2, pfb, off)
    ost, oll = _oracle_batch(oracle, params, o1, o2, pfb, off)
    assert st == ost
    np.testing.assert_allclose(ll, oll, rtol=0, atol=1e-9, equal_nan=True)


def test_degenerate_models_reach_their_edges():
    """the claims of hmm_params.DEGENERATE_MODELS, on the reference alone"""
    inf = float("-inf")
    assert float(vr.emission_exact(DEGENERATE_MODELS["B1_UF0"], 4, 0.2, -1.0, 0.5)) == inf
    assert all(float(vr.emission_exact(DEGENERATE_MODELS["B1_UF0"], k, 0.2, -1.0, 0.5)) > inf for k in (1, 2, 3, 5, 6))
    assert all(float(vr.emission_exact(DEGENERATE_MODELS["B1_UF0_SHARP"], k, 0.2, -1.0, 0.5)) == inf for k in range(1, 7))
    lo, hi = float(np.log(1.175494351e-38)), float(np.log(0.9999999999999999))
    b1 = float(vr.emission_exact(DEGENERATE_MODELS["B2_UF0"], 3, 0.0, -1.0, 0.5))
    for k in range(1, 7):
        assert float(vr.emission_exact(DEGENERATE_MODELS["B2_UF0"], k, 0.0, 7.5, 0.5) - vr.emission_exact(DEGENERATE_MODELS["B2_UF0"], k, 0.0, -1.0, 0.5)) == lo
    for k in (2, 3, 5, 6):
        assert abs(float(vr.emission_exact(WGS_HMM, k, 0.0, 1e-12, 0.0)) - float(vr.emission_exact(WGS_HMM, k, 0.0, -1.0, 0.0)) - hi) < 1e-15
    assert b1 > 0
    # a column of A that no state reaches keeps the defaults maxval = -VITHUGE, ind = 1
    st, ll = vr.viterbi(dict(DEGENERATE_MODELS["ZERO_A"], pi=[0, 0, 0, 1, 0, 0]), [0.0] * 3, [-1.0] * 3, [0.5] * 3)
    assert st[0] == 4 and 4 not in st[1:]
    st, ll = vr.viterbi(DEGENERATE_MODELS["B1_UF0_SHARP"], [0.2] * 3, [-1.0] * 3, [0.5] * 3)
    assert st == [1, 1, 1] and ll == -vr.VITHUGE


def test_pack_calls_put_every_probe_in_every_slot_on_both_paths():
    """what test_answer_is_independent_of_slot_and_wave_mates relies on: over its calls every probe sits at each of the 10 slots of a
    wave, in a wave that keeps its back-pointers in LDS (longest sequence <= 512) and in one that does not; T = 513 never fits"""
    seen = {}
    for n_seq in vi.PACK_N_SEQ:
        calls = vi.pack_calls(n_seq)
        assert all(len(seqs) == n_seq for _, _, seqs in calls)
        for p, idx, seqs in calls:
            assert len(seqs[idx][0]) == vi.PACK_PROBE_T[p]
            wave = seqs[idx - idx % 10: idx - idx % 10 + 10]
            seen.setdefault((p, idx % 10), set()).add(max(len(s[0]) for s in wave) <= 512)
    for p, T in enumerate(vi.PACK_PROBE_T):
        for slot in range(10):
            assert seen[(p, slot)] == ({True, False} if T <= 512 else {False}), (T, slot)
    lengths = {len(s[0]) for n_seq in vi.PACK_N_SEQ for _, _, seqs in vi.pack_calls(n_seq) for s in seqs}
    assert lengths >= set(vi.PACK_MATE_T)


def test_oracle_window_log2_within_E_log2_host(oracle):
    depth, rs, re, ssz, mean = vi.window_inputs()
    worst, zero_sum, zero_cnt = 0.0, 0, 0
    for r in range(len(rs)):
        exact, zs, zc = vr.window_log2_exact(depth, int(rs[r]), int(re[r]), int(ssz[r]), mean)
        zero_sum += zs; zero_cnt += zc
        l2, _, _ = oracle.window_log2(depth, int(rs[r]), int(re[r]), int(ssz[r]), mean)
        worst = max(worst, float(np.max(vr.log2_error(l2, exact))))
    assert zero_sum > 0 and zero_cnt > 0              # the sum == 0 -> 1e-9 and count == 0 -> 0.0 windows are among them
    print(f"window_log2: max |oracle - exact| / max(1, |exact|) {worst:.3e}")
    assert worst <= vr.E_LOG2_HOST
