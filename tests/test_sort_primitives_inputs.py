"""The cases of tests/sort_primitives_inputs.py are not vacuous: the constants they were laid out for are read from the kernel sources,
rs_rounds_for is restated, and from sizes alone (no GPU) every tile size, both sides of every point at which the exclusive sum and the
prefix maximum change path, a sort whose table takes the three-launch scan and a queued sort whose grid is larger than its tiling
are shown to be present. A constant that moves fails here instead of quietly emptying a case of tests/test_gpu_sort_primitives.py.
The checkers are shown to reject the wrong answers they are there for."""
import os
import re

import numpy as np

import sort_primitives_inputs as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _source(*path):
    return open(os.path.join(ROOT, "contextsv_amd", "csrc", *path)).read()


def _constant(name, text, depth=0):
    """constexpr <type> NAME = <expression of literals and other constants>;"""
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, text)
    assert m and depth < 5, name
    expr = re.sub(r"\b(\d+)(?:ull|u)\b", r"\1", m.group(1))
    expr = re.sub(r"\b[A-Z][A-Z0-9_]*\b", lambda k: str(_constant(k.group(0), text, depth + 1)), expr)
    assert re.fullmatch(r"[\d\s*/+\-<()]+", expr), (name, expr)
    return int(eval(expr.replace("/", "//"), {"__builtins__": {}}))


SORT_SRC = "constexpr int WAVE = %d;\n" % sp.WAVE + _source("kernels", "sort.hip")
DEPTH_SRC = "constexpr int WAVE = %d;\n" % sp.WAVE + _source("kernels", "depth.hip")


def rs_rounds_for(n):
    rounds = sp.RS_ROUNDS
    while rounds > 2 and (n + rounds * sp.WAVE - 1) // (rounds * sp.WAVE) < 128:
        rounds >>= 1
    return rounds


def _wave_tiles(n):
    t = rs_rounds_for(n) * sp.WAVE
    return (n + t - 1) // t


def _os_grid_for_bound(n_bound):          # launch_radix_sort_u64_devn: os_wg_tiles_max(n_bound) - 1
    big = sp.RS_ROUNDS * sp.WAVE * sp.RS_WAVES
    return max((n_bound + big - 1) // big, 64)


def test_constants_are_the_sources():
    assert _constant("WAVE", _source("common.hpp")) == sp.WAVE
    for name in ("RS_ROUNDS", "RS_BITS", "RS_WAVES", "ES_TILE", "ES_THREADS", "ES1_CHUNK", "ES1_MAX", "OS_MAX_PASSES"):
        assert _constant(name, SORT_SRC) == getattr(sp, name), name
    for name in ("PM_TILE", "PM_THREADS"):
        assert _constant(name, DEPTH_SRC) == getattr(sp, name), name
    assert _constant("CSVGPU_TEST_GUARD", re.sub(r"#define (\w+) (\d+)", r"constexpr int \1 = \2;", open(os.path.join(ROOT, "include", "csvgpu.h")).read())) == sp.GUARD >= 4096
    # the restatements above are of these lines
    assert "while (rounds > 2 && (n + (uint64_t)rounds * WAVE - 1) / ((uint64_t)rounds * WAVE) < 128) rounds >>= 1;" in SORT_SRC
    assert "if (n <= ES1_MAX) { hipLaunchKernelGGL(es_single_kernel" in SORT_SRC
    assert "for (uint64_t c0 = 0; c0 < n; c0 += ES1_CHUNK)" in SORT_SRC and "for (uint64_t b0 = 0; b0 < nb; b0 += ES_THREADS)" in SORT_SRC
    assert "for (uint64_t b0 = 0; b0 < nb; b0 += PM_THREADS)" in DEPTH_SRC
    assert "return std::max<uint64_t>(big, 64) + 1;" in SORT_SRC and "if (n_bound >= (1ull << 30) || passes > OS_MAX_PASSES) return -1;" in SORT_SRC
    assert "const int passes = (key_bits + RS_BITS - 1) / RS_BITS;" in SORT_SRC
    assert max(sp.sort_passes(kb) for kb in sp.SORT_KEY_BITS) == sp.OS_MAX_PASSES and min(sp.DEVN_REFUSED_BOUNDS) == 1 << 30


def test_every_tile_size_is_sorted_on_both_sides_of_its_switch():
    sizes = sp.SORT_SMALL + sp.SORT_LARGE
    assert {rs_rounds_for(n) for n in sizes} == {2, 4, 8, 16, 32}
    assert sorted(rs_rounds_for(b) for _, b in sp.SORT_SWITCH_POINTS) == [4, 8, 16, 32]
    for a, b in sp.SORT_SWITCH_POINTS:
        assert b == a + 1 and 2 * rs_rounds_for(a) == rs_rounds_for(b) and a in sp.SORT_LARGE and b in sp.SORT_LARGE
        assert _wave_tiles(a) == 254 and _wave_tiles(b) == 128
    assert {0, 1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513} <= set(sp.SORT_SMALL) and max(sp.SORT_SMALL) == 513
    assert max(sizes) == 524289
    # a last workgroup with fewer than its four wave tiles, and a last wave tile that is not full
    assert _wave_tiles(300001) % sp.RS_WAVES != 0 and 300001 % (rs_rounds_for(300001) * sp.WAVE) != 0
    # the three-launch passes scan a table of 256 * tiles entries: at and beyond the one-workgroup limit
    tabs = {n: (1 << sp.RS_BITS) * _wave_tiles(n) for n in sp.SORT_LARGE}
    assert tabs[524288] == sp.ES1_MAX and tabs[524289] == sp.ES1_MAX + (1 << sp.RS_BITS) and max(tabs.values()) > sp.ES1_MAX
    assert sum(1 for t in tabs.values() if sp.ES1_CHUNK < t <= sp.ES1_MAX) >= 8           # and several chunks of the one-workgroup form
    assert sp.SORT_MODES == [1, 0] and sp.SORT_VALS == ["iota", "random"]


def test_sort_case_lists():
    small, large = sp.small_sort_cases(), sp.large_sort_cases()
    assert len(small) == 12 * 8 * 8 and len(set(small)) == len(small)
    assert len(large) == len(sp.SORT_LARGE) * 2 * 3 and sp.SORT_LARGE_KEY_BITS == [16, 41] and len(sp.SORT_LARGE_PATTERNS) == 3
    assert sp.SORT_KEY_BITS == [1, 8, 9, 16, 32, 33, 41, 64] and len(sp.SORT_PATTERNS) == 8
    a, b = sp.SORT_STATE_PAIR
    assert a == 300001 and b == 129 and rs_rounds_for(a) == 32 and rs_rounds_for(b) == 2
    for kb in sp.SORT_KEY_BITS:
        assert int(sp.digit_mask(kb)) == (1 << (8 * ((kb + 7) // 8))) - 1 and int(sp.key_mask(kb)) == (1 << kb) - 1


def test_key_patterns_are_what_they_are_named():
    for n, kb in ((513, 9), (300001, 41), (300001, 16), (129, 1)):
        km, dm = int(sp.key_mask(kb)), int(sp.digit_mask(kb))
        keys = {p: sp.make_keys(p, n, kb) for p in sp.SORT_PATTERNS}
        for p, k in keys.items():
            assert k.dtype == np.uint64 and len(k) == n, p
            assert np.array_equal(k, sp.make_keys(p, n, kb)), p                             # the child process builds the same arrays
        assert len(np.unique(keys["all_equal"])) == 1 and len(np.unique(keys["two_values"])) == 2
        for p in ("all_equal", "two_values", "ascending", "descending", "uniform"):
            assert int(keys[p].max()) <= km, p                                              # what every caller promises
        if n <= km:
            assert (np.diff(keys["ascending"].astype(object)) > 0).all() and (np.diff(keys["descending"].astype(object)) < 0).all()
        assert (keys["all_ff"] == np.uint64(sp.FULL)).all()
        # the digit is in one wave tile, in every pass
        t = rs_rounds_for(n) * sp.WAVE
        where = np.flatnonzero(keys["one_tile_digit"])
        assert len(where) == min(64, n - (n // 2) // 64 * 64) and len(set((where // t).tolist())) == 1 and _wave_tiles(n) >= 2
        for p in range(sp.sort_passes(kb)):
            assert set(((keys["one_tile_digit"] >> np.uint64(8 * p)) & np.uint64(255)).tolist()) == {0, 0x37}
        # bits inside the last digit and above it
        ab = keys["bits_above"]
        if kb < 64:
            assert (ab & np.uint64(dm & ~km)).any() == (dm != km) and (ab & np.uint64(sp.FULL & ~dm)).any()
            assert len(np.unique(ab & np.uint64(km))) <= 4 and len(np.unique(ab)) > n // 2
    v = sp.make_vals("random", 513)
    assert v.dtype == np.uint32 and (v == 0xFFFFFFFF).sum() >= 74 and len(np.unique(v)) > 400
    assert np.array_equal(sp.make_vals("iota", 5), np.arange(5, dtype=np.uint32))


def test_sort_reference_ignores_bits_above_the_last_digit_only():
    # key_bits 9 -> two digits: bits [0, 16) order, bits [16, 64) do not
    keys = np.array([0x30001, 0x20001, 0x0FF01, 0x10000, 0x00200], np.uint64)
    assert sp.sort_reference(keys, 9).tolist() == [3, 0, 1, 4, 2]
    assert sp.sort_reference(keys, 16).tolist() == [3, 0, 1, 4, 2] and sp.sort_reference(keys, 17).tolist() == [4, 2, 3, 1, 0]
    assert sp.sort_reference(keys, 1).tolist() == [3, 4, 0, 1, 2]


def test_queued_sort_cases_have_a_grid_beyond_their_tiling():
    cases = sp.devn_cases()
    assert len(cases) == 19 and (600000, 600000) in cases and (0, 0) in cases
    for n in (0, 1, 2, 129, 32513, 260097):
        assert {(n, n), (n, n + 1), (n, 600000)} <= set(cases)
    assert all(n <= nb < 1 << 30 for n, nb in cases)
    spare = [(n, nb) for n, nb in cases if _os_grid_for_bound(nb) > (_wave_tiles(n) + sp.RS_WAVES - 1) // sp.RS_WAVES]
    assert {(129, 600000), (32513, 600000), (260097, 600000), (0, 600000)} <= set(spare)
    # the kernel's own tiling differs from the one the bound would give (rounds from n, grid from n_bound), and every tile size occurs
    assert sum(1 for n, nb in cases if n and rs_rounds_for(n) != rs_rounds_for(nb)) >= 4
    assert {rs_rounds_for(n) for n, _ in cases if n} == {2, 4, 32}
    # the grid always covers the tiling that the kernel derives: otherwise a case would ask for keys nobody sorts
    for n, nb in cases:
        assert _os_grid_for_bound(nb) * sp.RS_WAVES >= _wave_tiles(n)
    assert {sp.sort_passes(kb) % 2 for kb in sp.DEVN_KEY_BITS} == {0, 1}


def test_exclusive_sum_sizes_sit_on_every_path_change():
    s = set(sp.ES_SIZES)
    assert {0, 1, 2, 15, 16, 17, 1023, 1024, 1025} <= s
    for c in (sp.ES1_CHUNK, sp.ES1_MAX):
        assert {c - 1, c, c + 1} <= s
    tiles = lambda n: (n + sp.ES_TILE - 1) // sp.ES_TILE
    assert sp.ES1_MAX + sp.ES_TILE + 1 in s and tiles(sp.ES1_MAX + sp.ES_TILE + 1) == 34                # a last tile of one entry
    spine = sp.ES_THREADS * sp.ES_TILE
    assert {spine, spine + 1, spine + sp.ES_TILE + 1} <= s and tiles(spine) == sp.ES_THREADS and tiles(spine + 1) == sp.ES_THREADS + 1
    assert tiles(spine + sp.ES_TILE + 1) == sp.ES_THREADS + 2 and max(s) == spine + sp.ES_TILE + 1
    # the single 0xFFFFFFFF sits on both sides of every boundary that the size has
    for n in sp.ES_SIZES:
        sp_i = sp.es_spikes(n)
        for c in (16, 1024, sp.ES1_CHUNK, sp.ES1_MAX, sp.ES_TILE, spine, spine + sp.ES_TILE):
            assert (c < n) == (c in sp_i) and (c < n) == (c - 1 in sp_i and c in sp_i), (n, c)
        assert all(0 <= i < n for i in sp_i)
    assert len(sp.es_spikes(526337)) == 2 * len(sp.ES_BOUNDARIES) and sp.es_spikes(16) == [7, 8]
    for n in sp.ES_SIZES:
        if n >= 16:
            assert int(sp.make_es("wrapping", n).astype(np.uint64).sum()) >= 4 << 32
        assert int(sp.make_es("below_2_16", n).max(initial=0)) < 1 << 16 and (sp.make_es("ones", n) == 1).all()
    d = sp.make_es("spike", 70000, 65536)
    assert d.sum() == 0xFFFFFFFF and d[65536] == 0xFFFFFFFF
    assert len(sp.es_cases()) < 400


def test_prefix_max_sizes_sit_on_every_path_change():
    s = set(sp.PM_SIZES)
    spine = sp.PM_THREADS * sp.PM_TILE
    assert {1, 2, 63, 64, 65, sp.PM_TILE - 1, sp.PM_TILE, sp.PM_TILE + 1, spine, spine + 1, spine + sp.PM_TILE + 1} == s
    assert sp.PM_VALUES == ["int_min", "decreasing", "increasing", "negative", "spike_2047", "spike_2048", "spike_last"]
    for n in sp.PM_SIZES:
        d = {k: sp.make_pm(k, n) for k in sp.PM_VALUES}
        assert all(v.dtype == np.int32 and len(v) == n for v in d.values())
        assert (d["int_min"] == sp.INT32_MIN).all() and d["decreasing"][0] == sp.INT32_MAX and (d["negative"] < 0).all()
        assert (np.diff(d["decreasing"].astype(np.int64)) < 0).all() and (np.diff(d["increasing"].astype(np.int64)) > 0).all()
        assert d["spike_last"][n - 1] == sp.INT32_MAX and (d["spike_last"][:n - 1] < 1000).all()
        for i in (2047, 2048):
            assert (d["spike_%d" % i] == sp.INT32_MAX).sum() == (1 if i < n else 0)
        assert (np.maximum.accumulate(d["decreasing"]) == sp.INT32_MAX).all()


def test_the_sort_checker_rejects_a_stability_failure():
    n, kb = 513, 16
    keys = sp.make_keys("two_values", n, kb)
    perm = sp.sort_reference(keys, kb)
    for kind in sp.SORT_VALS:
        vals = sp.make_vals(kind, n)
        ko, vo = keys[perm], vals[perm]
        assert sp.check_sort(keys, vals, perm, ko, vo) is None
        j = next(j for j in range(10, n - 1) if ko[j] == ko[j + 1] and vo[j] != vo[j + 1])
        bad = vo.copy()
        bad[[j, j + 1]] = bad[[j + 1, j]]                      # two values swapped inside a run of equal keys: still sorted, not stable
        msg = sp.check_sort(keys, vals, perm, ko, bad)
        assert msg and "vals_out" in msg and "index %d" % j in msg and hex(int(vo[j])) in msg and hex(int(bad[j])) in msg
    # a key that lost a bit above the sorted digits
    keys = sp.make_keys("bits_above", n, 9)
    perm = sp.sort_reference(keys, 9)
    vals = sp.make_vals("iota", n)
    ko = keys[perm].copy()
    ko[100] &= np.uint64(0x7FFFFFFFFFFFFFFF)
    ko[100] ^= np.uint64(1 << 40)
    msg = sp.check_sort(keys, vals, perm, ko, vals[perm])
    assert msg and "keys_out" in msg and "index 100" in msg
    assert "length" in sp.check_sort(keys, vals, perm, ko[:-1], vals[perm][:-1])


def test_the_exclusive_sum_checker_rejects_a_lost_carry():
    for n, c in ((16385, sp.ES1_CHUNK), (67585, sp.ES1_MAX), (526337, sp.ES_THREADS * sp.ES_TILE)):
        data = sp.make_es("below_2_16", n)
        want = sp.es_reference(data)
        assert want[0] == 0 and int(want[-1]) == int(data[:-1].astype(np.uint64).sum()) & 0xFFFFFFFF
        assert sp.check_exclusive_sum(data, want) is None
        bad = want.copy()
        bad[c:] += np.uint32(1)                                  # off by one from a chunk boundary on
        msg = sp.check_exclusive_sum(data, bad)
        assert msg and "index %d of" % c in msg and "(%d differ)" % (n - c) in msg
    wrap = sp.make_es("wrapping", 17)
    assert sp.es_reference(wrap)[-1] == np.uint32(int(wrap[:-1].astype(np.uint64).sum()) % (1 << 32))
    spike = sp.make_es("spike", 20000, 16383)
    assert sp.es_reference(spike)[16383] == 0 and (sp.es_reference(spike)[16384:] == 0xFFFFFFFF).all()


def test_the_prefix_max_checker_rejects_a_forgotten_carry():
    n = 2049
    for kind in ("decreasing", "spike_2047"):
        data = sp.make_pm(kind, n)
        want = np.maximum.accumulate(data)
        assert sp.check_prefix_max(data, want) is None
        bad = want.copy()
        bad[2048:] = np.maximum.accumulate(data[2048:])          # the second block starts over
        msg = sp.check_prefix_max(data, bad)
        assert msg and "index 2048 of" in msg and hex(sp.INT32_MAX) in msg
