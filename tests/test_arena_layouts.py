"""The device workspace layouts (contextsv_amd/csrc/layouts.hpp) on the CPU. `make -C contextsv_amd/csrc layouts-check` builds
tools/fuzz/arena_layouts_check.cpp — a program of its own, under AddressSanitizer + UBSan — which plans every carve function at the
rounding edges of its counts, carves it over exactly the planned bytes, fills every slice and reads all of them back: no two slices
overlap, none reaches past its reservation, the real pass uses what the plan said, every slice is 256-byte aligned, and the ordering
workspace's key arrays lie back to back. A layout of the header without a case in the program fails the run."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "contextsv_amd", "csrc")


def test_every_layout_plans_what_it_carves():
    r = subprocess.run(["make", "-s", "-C", CSRC, "layouts-check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "_obj", "arena_layouts_check")], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error:" not in r.stderr, r.stderr[-3000:]
    m = re.search(r"arena_layouts_check: (\d+) layouts, (\d+) cases, 0 failures", r.stdout)
    assert m, r.stdout[-2000:]
    # the header's name table is what the program held itself to: every name in it is a carve function's, none is missing from it
    hdr = open(os.path.join(CSRC, "layouts.hpp")).read()
    names = re.search(r"kLayoutNames\[\] = \{([^}]*)\}", hdr).group(1).count('"') // 2
    carves = len(re.findall(r"^static inline bool (?:carve_\w+|sortws_carve|sr_carve)\(", hdr, re.M))
    assert int(m.group(1)) == names == carves, (m.group(1), names, carves)
    assert int(m.group(2)) > 1000
