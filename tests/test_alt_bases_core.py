"""The per-base rule of the ALT strings cut on the device (contextsv_amd/csrc/alt_bases_core.hpp, csvgpu_alt_bases_resident) on the CPU.
`make -C contextsv_amd/csrc alt-check` builds tools/fuzz/alt_bases_core_check.cpp — a program of its own, g++ under AddressSanitizer +
UBSan — which holds the header against a literal copy of the host loop (SVCaller::toSVCall) on edge and random inputs, every packed
sequence in a heap block of exactly its size: the same characters, and no byte read that the host's bound does not cover. The GPU tests
(tests/test_gpu_alt_bases.py) run the kernel that is built from the same header. CPU only; nothing sanitized is loaded into Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "contextsv_amd", "csrc")


def test_core_agrees_with_the_host_loop_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", CSRC, "alt-check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "_obj", "alt_bases_core_check")], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    m = re.search(r"alt_bases_core_check: (\d+) cases, (\d+) inside, (\d+) outside, 0 failures", r.stdout)
    assert m, r.stdout[-2000:]
    n_cases, n_inside, n_outside = (int(m.group(i)) for i in range(1, 4))
    assert n_cases > 200_000 and n_inside > n_cases // 10 and n_outside > n_cases // 10          # both sides of the bound ran
