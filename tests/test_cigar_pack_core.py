"""The 16-bit form of a resident shard's CIGAR array (contextsv_amd/csrc/cigar_pack_core.hpp: 4 bits of op, 12 of length, longer ops escaped
into a side table with a per-piece index) on the CPU. `make -C contextsv_amd/csrc cigar-pack-check` builds
tools/fuzz/cigar_pack_core_check.cpp — a program of its own, g++ under AddressSanitizer + UBSan — which packs and unpacks 1e6 random ops at
escape rates 0, 1e-5, 1e-2 and 1, holds the escape look-up against a linear search of the table, and walks the edge positions (array ends,
chunk and piece edges, runs of escapes, shards of 1, 3 and 513 ops, op indices beyond 2^32), every array in a heap block of exactly its
size. The GPU tests (tests/test_gpu_cigar_pack.py) run the kernels built from the same header. CPU only; nothing sanitized is loaded into
Python."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "contextsv_amd", "csrc")


def test_pack_round_trip_and_lookup_under_sanitizers():
    r = subprocess.run(["make", "-s", "-C", CSRC, "cigar-pack-check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "_obj", "cigar_pack_core_check")], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    m = re.search(r"cigar_pack_core_check: (\d+) cases, (\d+) escapes, 0 failures", r.stdout)
    assert m, r.stdout[-2000:]
    assert int(m.group(1)) > 500 and int(m.group(2)) > 1_000_000          # the rate-1 array alone is 1e6 escapes
