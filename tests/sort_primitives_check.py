"""Body of tests/test_gpu_sort_primitives.py (run as a script with CSVGPU_LIB = the test build: `sort_primitives_check.py SECTION`).
Runs the cases of tests/sort_primitives_inputs.py through the hooks on launch_radix_sort_u64, launch_radix_sort_u64_devn,
launch_exclusive_sum_u32 and launch_prefix_max, prints `ok` or the first failing case and what differed."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contextsv_amd as cs  # noqa: E402
from contextsv_amd import _lib  # noqa: E402
from contextsv_amd._lib import ptr  # noqa: E402
import sort_primitives_inputs as sp  # noqa: E402

MODE_NAMES = {1: "onesweep", 0: "three_launch"}


def fail(what):
    print("FAILED " + what)
    raise SystemExit(1)


def status(ctx, rc):
    return "%s (%s)" % (_lib.STATUS_NAMES.get(rc, rc), (ctx.lib.csvgpu_last_error(ctx.h) or b"").decode())


def run_sort(ctx, keys, vals, key_bits, mode, n_bound=None):
    """One sort through the hook -> None, or what was wrong: status, flag, guards, order."""
    n = len(keys)
    ko, vo = np.full(n, 0x1111111111111111, np.uint64), np.full(n, 0x11111111, np.uint32)
    gave_up, tail_ok = C.c_uint32(0xdead), C.c_int32(-1)
    if n_bound is None:
        rc = ctx.lib.csvgpu_test_radix_sort(ctx.h, ptr(keys), ptr(vals), n, key_bits, mode, ptr(ko), ptr(vo), C.byref(gave_up), C.byref(tail_ok))
    else:
        rc = ctx.lib.csvgpu_test_radix_sort_devn(ctx.h, ptr(keys), ptr(vals), n, n_bound, key_bits, ptr(ko), ptr(vo), C.byref(gave_up), C.byref(tail_ok))
    if rc != _lib.CSV_OK:
        return "status " + status(ctx, rc)
    if gave_up.value != 0:
        return "the look-back gave up: flag word %#x" % gave_up.value
    if tail_ok.value != 1:
        return "a slot behind the first n lost its sentinel (tail_ok = %d)" % tail_ok.value
    return ko, vo


def sort_case(ctx, name, keys, key_bits, perm, n_bound=None, modes=sp.SORT_MODES):
    for kind in sp.SORT_VALS:
        vals = sp.make_vals(kind, len(keys))
        for mode in modes:
            got = run_sort(ctx, keys, vals, key_bits, mode, n_bound)
            what = got if isinstance(got, str) else sp.check_sort(keys, vals, perm, *got)
            if what:
                fail("%s vals=%s mode=%s: %s" % (name, kind, MODE_NAMES[mode], what))


def section_sort(ctx):
    for n, kb, pattern in sp.small_sort_cases() + sp.large_sort_cases():
        keys = sp.make_keys(pattern, n, kb)
        sort_case(ctx, "sort n=%d key_bits=%d pattern=%s" % (n, kb, pattern), keys, kb, sp.sort_reference(keys, kb))
    # a large sort, then at once a small one on the same context: nothing of the first (tile counters, status words, digit totals) may
    # reach the second. (The hook also fills the workspace with its sentinel before every sort, so each case above starts from garbage.)
    a, b = sp.SORT_STATE_PAIR
    ka, kb_ = sp.make_keys("uniform", a, 41), sp.make_keys("uniform", b, 41)
    pa, pb = sp.sort_reference(ka, 41), sp.sort_reference(kb_, 41)
    for mode in sp.SORT_MODES:
        for k, p in ((ka, pa), (kb_, pb)):
            sort_case(ctx, "sort n=%d key_bits=41 pattern=uniform (pair %d then %d)" % (len(k), a, b), k, 41, p, modes=[mode])


def section_devn(ctx):
    for n, n_bound in sp.devn_cases():
        for kb in sp.DEVN_KEY_BITS:
            for pattern in sp.DEVN_PATTERNS:
                keys = sp.make_keys(pattern, n, kb)
                sort_case(ctx, "sort_devn n=%d n_bound=%d key_bits=%d pattern=%s" % (n, n_bound, kb, pattern), keys, kb, sp.sort_reference(keys, kb),
                          n_bound=n_bound, modes=[1])
    keys, vals = sp.make_keys("uniform", 2, 41), sp.make_vals("iota", 2)
    for n_bound in sp.DEVN_REFUSED_BOUNDS:
        got = run_sort(ctx, keys, vals, 41, 1, n_bound)
        if not (isinstance(got, str) and got.startswith("status CSV_EINVAL") and "refused by the launcher" in got):
            fail("sort_devn n=2 n_bound=%d key_bits=41: expected CSV_EINVAL from the launcher's refusal, got %s" % (n_bound, got if isinstance(got, str) else "CSV_OK"))


def section_exclusive_sum(ctx):
    for n, kind, spike in sp.es_cases():
        data = sp.make_es(kind, n, spike)
        got = data.copy()
        rc = ctx.lib.csvgpu_test_exclusive_sum(ctx.h, ptr(got), n)
        what = "status " + status(ctx, rc) if rc != _lib.CSV_OK else sp.check_exclusive_sum(data, got)
        if what:
            fail("exclusive_sum n=%d values=%s%s: %s" % (n, kind, "" if spike is None else " at %d" % spike, what))


def section_prefix_max(ctx):
    for n, kind in sp.pm_cases():
        data = sp.make_pm(kind, n)
        got = np.full(n, 0x11111111, np.int32)
        rc = ctx.lib.csvgpu_test_prefix_max(ctx.h, ptr(data), n, ptr(got))
        what = "status " + status(ctx, rc) if rc != _lib.CSV_OK else sp.check_prefix_max(data, got)
        if what:
            fail("prefix_max n=%d values=%s: %s" % (n, kind, what))


SECTIONS = {"sort": section_sort, "sort_devn": section_devn, "exclusive_sum": section_exclusive_sum, "prefix_max": section_prefix_max}

if __name__ == "__main__":
    section = SECTIONS[sys.argv[1]]
    with cs.Context(0) as ctx:
        for name in _lib.TEST_HOOKS:
            if not hasattr(ctx.lib, name):
                fail("%s is not in %s: CSVGPU_LIB must name the test build" % (name, _lib.LIB_PATH))
        t0 = time.perf_counter()
        section(ctx)
        print("%s: %.2f s on the device and in the checkers" % (sys.argv[1], time.perf_counter() - t0))
    print("ok")
