"""The lane-wise slot replay behind the device's representative choice (contextsv_amd/csrc/sort_select_core.hpp, csvgpu_sort_slot /
csvgpu_merge_select) on the CPU. `make -C contextsv_amd/csrc merge-select-check` builds tools/fuzz/sort_select_core_check.cpp — a program of
its own, g++ under AddressSanitizer + UBSan — which drives the core's rounds over virtual lanes and holds the chosen id against std::sort's
slot, one partition step against lib_unguarded_partition and the partition counts against the library's own loops. The GPU tests
(tests/test_gpu_merge_select.py) run the kernels built from the same header. CPU only; nothing sanitized is loaded into Python."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import merge_select_inputs as mi
from contextsv_amd import _lib, host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "contextsv_amd", "csrc")


def test_core_agrees_with_std_sort_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", CSRC, "merge-select-check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "_obj", "sort_select_core_check")], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    m = re.search(r"sort_select_core_check: (\d+) slots, (\d+) partitions, (\d+) bounded chains, (\d+) declined at the library limit, 0 failures", r.stdout)
    assert m, r.stdout[-2000:]
    n_slots, n_part, n_bound, n_limit = (int(m.group(i)) for i in range(1, 5))
    assert n_slots >= 2000 and n_part >= 20000 and n_bound >= 5000 and n_limit < n_slots // 10
    # every pattern at every size printed its chains' partition counts
    assert len(re.findall(r"^partitions per chain:", r.stdout, flags=re.M)) == 9 * 10


def _struct_fields(name):
    text = open(os.path.join(ROOT, "include", "csvgpu.h")).read()
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [re.sub(r"\[\d+\]", "", f) for decl in body.split(";") for f in re.findall(r"(\w+(?:\[\d+\])?)\s*$", decl.strip())]


def test_record_layouts_match_header():
    assert C.sizeof(_lib.csv_merge_rep) == 32 and C.sizeof(_lib.csv_merge_counts) == 32 and _lib.MERGE_REP_DTYPE.itemsize == 32
    assert _struct_fields("csv_merge_rep") == [f for f, _ in _lib.csv_merge_rep._fields_] == ["sig", "label", "cluster_size", "status", "reserved"]
    assert _struct_fields("csv_merge_counts") == [f for f, _ in _lib.csv_merge_counts._fields_] == ["n_rep", "n_declined"]
    assert list(_lib.MERGE_REP_DTYPE.names[:4]) == list(_lib.SIG_DTYPE.names) and list(_lib.MERGE_REP_DTYPE.names[4:]) == ["label", "cluster_size", "status", "reserved"]
    assert mi.lds_cap() == _lib.SORT_SLOT_LDS_CAP
    for name in ("csvgpu_sort_slot", "csvgpu_merge_select", "csvgpu_chr_merge_select"):
        assert name in _lib.ABI


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 18, 33, 100, 1000, 4097])
def test_rounds_agree_with_the_select_on_every_pattern(n):
    """host.sort_select_rounds counts the partitions of the library's chain for a slot; host.sort_select_check finishes every input (it
    heap-sorts where the library does). The two agree on which inputs finish by partitions alone: no partition up to 16 members, never more
    than 2 floor(log2 n), and the depth limit runs out (-1) only on the two patterns built against a median-of-three quicksort — on the
    others it is never reached."""
    rng = np.random.default_rng(n)
    limit = 2 * (int(n).bit_length() - 1)
    for name in mi.PATTERNS:
        keys = mi.pattern(name, rng, n)
        for p in mi.slots(rng, n):
            a, b = host.sort_select_check(keys, p)
            assert a == b, (name, n, p)
            r = host.sort_select_rounds(keys, p)
            assert -1 <= r <= limit and (r == 0) == (n <= 16), (name, n, p, r)
            if name not in mi.ADVERSARIAL:
                assert r >= 0, (name, n, p)


def test_rounds_of_the_noise_bucket_slot():
    rng = np.random.default_rng(1)
    for n in (60_000, 200_003):
        keys = rng.integers(50, 301, n).astype(np.uint32)
        top = max(1, int(n * 0.2))
        r = host.sort_select_rounds(keys, top // 2)
        assert 0 < r <= 2 * (n.bit_length() - 1)
