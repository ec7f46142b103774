#!/usr/bin/env python3
"""Generates tests/golden/*.json from the REFERENCE's own translation units (oracle/_ref/libcsvref.so =
/root/reference/src/{dbscan,dbscan1d,kc}.cpp compiled unmodified by oracle/Makefile). Run in the build
container only (needs /root/reference); the JSON files are committed and are what the GPU box and the
CPU suite check against. Inputs are seeded; expected outputs are whatever the reference code returns.
Also writes tests/golden/ref_answers.npz: the reference code's answers to every call the tests that check against it make
(tests/test_oracle_golden.py, test_oracle_windowed.py, test_gpu_ref_sweep.py, test_gpu_reservation_edges.py, through the `ref` fixture), which that fixture
gives them where oracle/_ref is not built. The tests' own bodies are run to record them; the device side of the GPU tests is
answered by the reference code here, so no GPU is needed.

    python tests/golden/make_golden.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import oracle_lib  # noqa: E402
import synth_small as ss  # noqa: E402


def main():
    ref = oracle_lib.load_ref()
    assert ref is not None, "reference build missing"
    cases = []
    k = 0
    for n in (1, 2, 7, 40, 200, 800, 2000):
        for eps in (0.1, 0.3):
            for min_pts in (1, 2, 3, 5, 6):
                if n >= 800 and min_pts in (1, 6):
                    continue
                for sort in (False, True):
                    k += 1
                    s, e = ss.random_intervals(1000 + k, n, sort=sort, zero_len=(k % 5 == 0), span=400_000 if n <= 200 else 2_000_000)
                    cases.append({"seed": 1000 + k, "eps": eps, "min_pts": min_pts, "start": s.tolist(), "end": e.tolist(),
                                  "labels": ref.dbscan_iv(s, e, eps, min_pts).tolist()})
    json.dump({"source": "reference src/dbscan.cpp DBSCAN::fit via oracle/_ref", "cases": cases},
              open(os.path.join(HERE, "dbscan_iv.json"), "w"))

    rng = np.random.default_rng(77)
    cases = []
    for k in range(120):
        n = int(rng.choice([0, 1, 4, 5, 6, 12, 40, 150, 600]))
        base = int(rng.integers(-500, 100000))
        p = (base + rng.choice([0, 0, 0, 250, 4000], n) + rng.integers(-110, 111, n)).astype(np.int32)
        eps = float(rng.choice([100.0, 100.0, 10.0, 0.0, 99.5]))
        mp = int(rng.choice([5, 5, 1, 2, 3]))
        cases.append({"eps": eps, "min_pts": mp, "points": p.tolist(), "labels": ref.dbscan_1d(p, eps, mp).tolist(),
                      "largest": ref.largest(p, eps, mp).tolist()})
    json.dump({"source": "reference src/dbscan1d.cpp DBSCAN1D::fit / getLargestCluster via oracle/_ref", "cases": cases},
              open(os.path.join(HERE, "dbscan_1d.json"), "w"))

    vals = []
    for x, mu, sd in [(0.0, 0.5, 0.044416), (0.0, 0.5, 0.057305), (0.3, 0.0, 1.0), (-1.2, 0.0, 1.0), (2.5, 0.0, 1.0), (0.0, 0.0, 0.163877),
                      (0.1, 0.333333, 0.166946), (-3.7, -3.739099, 2.564467), (100.0, 100.0, 0.163877), (0.5, 0.25, 0.157236), (1e-9, 0.0, 0.155241),
                      # the state-1 constant cdf_normal(0, B2_mean[4], B2_sd[4]) of hmm_params.CDF_SETS: gser, gser just below the
                      # switch to gcf (x^2 = 1.39 < 1.5), gcf, the x <= 0 return, the positive errorf branch
                      (0.0, 0.5, 0.5), (0.0, 0.5, 0.3), (0.0, 0.5, 0.25), (0.0, 0.0, 0.2), (0.0, -0.2, 0.3)]:
        vals.append({"x": x, "mu": mu, "sigma": sd, "pdf": ref.lib.ref_pdf_normal(x, mu, sd), "cdf": ref.lib.ref_cdf_normal(x, mu, sd)})
    json.dump({"source": "reference src/kc.cpp pdf_normal / cdf_normal via oracle/_ref (17 significant digits)", "values": vals},
              open(os.path.join(HERE, "kc_normal.json"), "w"))
    print("golden vectors written:", [f for f in os.listdir(HERE) if f.endswith(".json")])
    record_ref_answers(ref)


class _DeviceFromRef:
    """the Context calls of tests/test_gpu_ref_sweep.py and test_gpu_reservation_edges.py, answered by the reference code (their answers
    must equal it to pass)"""

    def __init__(self, ref):
        self.ref = ref

    def dbscan_iv(self, s, e, eps, min_pts):
        return self.ref.dbscan_iv(s, e, eps, min_pts)

    def dbscan_1d(self, p, off, eps, min_pts):
        off = [int(o) for o in off]
        return np.concatenate([self.ref.dbscan_1d(p[a:b], eps, min_pts) if b > a else np.zeros(0, np.int32) for a, b in zip(off[:-1], off[1:])])

    def dbscan_iv_batch(self, s, e, off, eps, min_pts):
        return np.concatenate([self.ref.dbscan_iv(s[off[k]: off[k + 1]], e[off[k]: off[k + 1]], eps, min_pts) for k in range(len(off) - 1)])

    def close(self):
        pass


def record_ref_answers(ref):
    import test_gpu_ref_sweep as t_gpu
    import test_gpu_reservation_edges as t_edges
    import test_oracle_golden as t_golden
    import test_oracle_windowed as t_windowed
    rec = oracle_lib.RecordingRef(ref)
    orc = oracle_lib.load_oracle()
    dev = _DeviceFromRef(ref)
    t_golden.test_oracle_vs_reference_live(orc, rec)
    t_windowed.test_windowed_labeller_vs_reference_code_live(orc, rec)
    t_gpu.test_interval_dbscan_vs_reference_code(dev, rec)
    t_gpu.test_dbscan1d_vs_reference_code(dev, rec)
    t_gpu.test_interval_dbscan_batch_against_reference(dev, rec)
    t_edges.dbscan_edges(lambda: dev, rec)
    rec.save(oracle_lib.REF_ANSWERS)
    print("reference answers written:", len(rec.answers), "calls,", os.path.getsize(oracle_lib.REF_ANSWERS), "bytes")


if __name__ == "__main__":
    main()
