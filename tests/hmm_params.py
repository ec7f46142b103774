"""HMM parameter sets used as test constants. The values are the numbers in the reference's data files
(data/wgs.hmm and data/wgs_test.hmm, which differ only in B2_uf), re-typed here as data because
/root/reference does not exist on the GPU box."""
import numpy as np

_A = [[0.899997, 0.009, 0.091, 0.000001, 0.000001, 0.000001],
      [0.009, 0.899997, 0.091, 0.000001, 0.000001, 0.000001],
      [0.00001, 0.00005, 0.99987, 0.00001, 0.00005, 0.00001],
      [0.000001, 0.000001, 0.00003, 0.999966, 0.000001, 0.000001],
      [0.000001, 0.000001, 0.091, 0.000001, 0.899997, 0.009],
      [0.000001, 0.000001, 0.091, 0.000001, 0.009, 0.899997]]
WGS_HMM = dict(A=_A, pi=[0.000001, 0.000500, 0.999000, 0.000001, 0.000500, 0.000001],
               B1_mean=[-3.739099, -0.727964, 0.000000, 100, 0.395454, 0.658622],
               B1_sd=[2.564467, 0.303606, 0.163877, 0.163877, 0.127181, 0.124527], B1_uf=0.01,
               B2_mean=[0.0, 0.25, 0.333333, 0.5, 0.5], B2_sd=[0.155241, 0.157236, 0.166946, 0.057305, 0.044416], B2_uf=0.01)
WGS_TEST_HMM = dict(WGS_HMM, B2_uf=0.001)


# ---- sets that make one property of the Viterbi path visible (tests/test_viterbi_ref.py, tests/test_gpu_viterbi_edges.py); all derived
# from WGS_HMM.

def _with_b2_state1(mean, sd):
    return dict(WGS_HMM, B2_mean=WGS_HMM["B2_mean"][:4] + [mean], B2_sd=WGS_HMM["B2_sd"][:4] + [sd])


# (B2_mean[4], B2_sd[4]) at which the state-1 constant cdf_normal(0, mean, sd) is not 0 and each branch of kc.cpp's chain is taken; the
# expected values are in tests/golden/kc_normal.json.
CDF_SETS = {
    "cdf_gser": _with_b2_state1(0.5, 0.5),            # x^2 = 0.5: gser, cdf 0.1587
    "cdf_gser_edge": _with_b2_state1(0.5, 0.3),       # x^2 = 1.39: gser, just below the switch at 1.5, cdf 0.0478
    "cdf_gcf": _with_b2_state1(0.5, 0.25),            # x^2 = 2.0: gcf, cdf 0.02275
    "cdf_zero_arg": _with_b2_state1(0.0, 0.2),        # x = 0: gser's x <= 0 return, cdf 0.5
    "cdf_positive": _with_b2_state1(-0.2, 0.3),       # x > 0: errorf's positive branch, cdf 0.7475
}


def _copies(src, dsts, pi, corner, mean=None):
    """WGS_HMM with the states `dsts` (1-based) made exact copies of state `src`: rows and columns of A (the block among them is
    `corner` throughout), pi, B1_mean, B1_sd. Their emissions are then identical wherever there is no BAF."""
    A = [list(r) for r in _A]
    m, sd = list(WGS_HMM["B1_mean"]), list(WGS_HMM["B1_sd"])
    if mean is not None:
        m[src - 1] = mean
    grp = [src] + list(dsts)
    for d in dsts:
        A[d - 1] = list(A[src - 1])
        for r in A:
            r[d - 1] = r[src - 1]
        m[d - 1], sd[d - 1] = m[src - 1], sd[src - 1]
    for i in grp:
        for j in grp:
            A[i - 1][j - 1] = corner
    assert all(pi[d - 1] == pi[src - 1] for d in dsts)
    return dict(WGS_HMM, A=A, pi=pi, B1_mean=m, B1_sd=sd)


# Tie models: the reference breaks every tie towards the lowest state (strict '>' from -VITHUGE, khmm.cpp:338-371). `on` is the log2
# ratio that sits on the tied states, `off` one that sits on state 3.
TIE_MODELS = {
    "UNIFORM": dict(WGS_HMM, A=[[1 / 6] * 6] * 6, pi=[1 / 6] * 6, B1_mean=[0.0] * 6, B1_sd=[0.163877] * 6),
    "TWIN_56": _copies(5, [6], [0.000001, 0.0005, 0.399, 0.000499, 0.3, 0.3], 0.45),
    "TWIN_12": _copies(1, [2], [0.3, 0.3, 0.399, 0.000001, 0.0005, 0.000499], 0.45),
    "TRIPLE_456": _copies(4, [5, 6], [0.000001, 0.0005, 0.399499, 0.2, 0.2, 0.2], 0.3, mean=0.395454),
}
TIE_OBS = {"UNIFORM": (0.0, 0.0), "TWIN_56": (0.395454, 0.0), "TWIN_12": (-3.739099, 0.0), "TRIPLE_456": (0.395454, 0.0)}


def _zero_A():
    A = [list(r) for r in _A]
    for r in A:
        r[3] = 0.0                      # no state reaches state 4: maxval stays -VITHUGE and the back-pointer stays 1
    A[0][1] = A[1][0] = A[4][5] = A[5][4] = 0.0
    A[2][0] = A[2][5] = 0.0
    return A


# Degenerate models: -inf logs, the pi floor, emissions of exactly 0 and the two clamps of b2iot as the value.
DEGENERATE_MODELS = {
    "ZERO_A": dict(WGS_HMM, A=_zero_A()),
    "ZERO_PI": dict(WGS_HMM, pi=[0.0, 0.0005, 0.9995, 0.0, 0.0, 0.0]),
    "ZERO_PI_3": dict(WGS_HMM, pi=[0.5, 0.0, 0.0, 0.0, 0.5, 0.0]),
    "B1_UF0": dict(WGS_HMM, B1_uf=0.0),                                  # state 4 (mean 100): pdf == 0, b1iot == -inf
    "B1_UF0_SHARP": dict(WGS_HMM, B1_uf=0.0, B1_sd=[0.001] * 6),         # away from the means every state is -inf: loglik stays -VITHUGE
    "B2_UF0": dict(WGS_HMM, B2_uf=0.0),                                  # a BAF far from every mean: FLOAT_MINIMUM is the value
    "BOTH_UF0": dict(WGS_HMM, B1_uf=0.0, B2_uf=0.0),
}


def write_hmm_file(path, p):
    """Write a parameter set in the .hmm text grammar ReadCHMM parses (khmm.cpp:395-553)."""
    def row(v):
        return " ".join(f"{x:.6f}" for x in v)
    B = np.full((6, 6), 0.000001)
    lines = ["M=6", "N=6", "A:"] + [row(r) for r in p["A"]] + ["B:"] + [row(r) + " " for r in B] + ["pi:", row(p["pi"]) + " ",
             "B1_mean:", row(p["B1_mean"]) + " ", "B1_sd:", row(p["B1_sd"]) + " ", "B1_uf:", f"{p['B1_uf']:.6f}",
             "B2_mean:", row(p["B2_mean"]) + " ", "B2_sd:", row(p["B2_sd"]), "B2_uf:", f"{p['B2_uf']:.6f}",
             "B3_mean:", row(p["B1_mean"]) + " ", "B3_sd:", row(p["B1_sd"]) + " ", "B3_uf:", "0.010000"]
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    return path
