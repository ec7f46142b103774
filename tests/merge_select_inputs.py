"""Inputs and expectations shared by tests/test_merge_select_core.py and tests/test_gpu_merge_select.py: the key patterns of
tests/test_sort_select.py, the slots a size is probed at, and mergeSVs' representatives by the HOST rule (host.merge_type_with_labels) as
csv_merge_rep records. Nothing here touches the device."""
import re
import os

import numpy as np

from contextsv_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INS, DEL_T = 3, 0                                  # SVType codes of the host mirror's calls
PATTERNS = ("few_values", "clip_lengths", "random", "all_equal", "ascending", "descending", "organ_pipe", "sawtooth", "median3_killer_like")
# the patterns built against a median-of-three quicksort: on these std::sort can run into its depth limit and heap-sort
ADVERSARIAL = ("organ_pipe", "median3_killer_like")


def pattern(name, rng, n):
    if name == "few_values": k = rng.integers(0, 4, n)
    elif name == "clip_lengths": k = rng.integers(50, 301, n)            # the noise bucket of the CIGAR path
    elif name == "random": k = rng.integers(0, 1 << 30, n)
    elif name == "all_equal": k = np.full(n, 7)
    elif name == "ascending": k = np.arange(n)
    elif name == "descending": k = np.arange(n)[::-1]
    elif name == "organ_pipe": k = np.concatenate([np.arange(n // 2), np.arange(n - n // 2)[::-1]])
    elif name == "sawtooth": k = np.arange(n) % 17
    elif name == "median3_killer_like": k = np.concatenate([np.arange(0, n, 2), np.arange(1, n, 2)[::-1]])[:n]
    else: raise KeyError(name)
    return np.ascontiguousarray(k, np.uint32)


def slots(rng, n):
    """every slot up to 100 members; above, the ends, the tenths and 25 random ones"""
    if n <= 100:
        return list(range(n))
    return sorted(set([0, 1, n // 10, n // 5, n // 2, n - 2, n - 1] + rng.integers(0, n, 25).tolist()))


def lds_cap():
    """LDS_CAP of contextsv_amd/csrc/sort_select_core.hpp"""
    text = open(os.path.join(ROOT, "contextsv_amd", "csrc", "sort_select_core.hpp")).read()
    return int(re.search(r"constexpr uint32_t LDS_CAP = (\d+);", text).group(1))


def expected_slot(keys, nth):
    """(index std::sort leaves at the slot, or None where the library's chain runs out of depth and heap-sorts; partitions or -1)"""
    rounds = host.sort_select_rounds(keys, nth)
    return (None if rounds < 0 else host.sort_select_check(keys, nth)[0]), rounds


def make_sigs(start, end, rng=None):
    n = len(start)
    s = np.zeros(n, _lib.SIG_DTYPE)
    s["start"], s["end"] = start, end
    if rng is not None:
        s["read"] = rng.integers(0, 1 << 20, n)
        s["qpos_kind"] = rng.integers(0, 1 << 20, n)
    else:
        s["read"] = np.arange(n)
    return s


def expected_records(sig, labels, n_del):
    """mergeOrdered's rule per type (host/sv_caller.cpp), as records: a type with fewer than two signatures passes through, otherwise
    host.merge_type_with_labels picks per bucket (its calls carry the input index as id)."""
    out = []
    n_declined = [0, 0]
    for t, (a, b) in enumerate(((0, n_del), (n_del, len(sig)))):
        ts, tl = sig[a:b], labels[a:b]
        if len(ts) < 2:
            for x in ts:
                out.append((x["start"], x["end"], x["read"], x["qpos_kind"], -2, 0, _lib.REP_PASS_THROUGH, 0))
            continue
        calls = host.make_calls(ts["start"], ts["end"], np.full(len(ts), DEL_T if t == 0 else INS))
        for c in host.merge_type_with_labels(calls, tl, False):
            x = ts[int(c["id"])]
            out.append((x["start"], x["end"], x["read"], x["qpos_kind"], int(tl[int(c["id"])]), int(c["cluster_size"]), _lib.REP_CHOSEN, 0))
    return np.array(out, _lib.MERGE_REP_DTYPE) if out else np.zeros(0, _lib.MERGE_REP_DTYPE)


def same_records(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for f in _lib.MERGE_REP_DTYPE.names:
        assert np.array_equal(got[f], want[f]), (f, np.nonzero(got[f] != want[f])[0][:5])
