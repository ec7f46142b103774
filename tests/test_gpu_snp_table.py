"""Resident SNP tables through the C-ABI (csvgpu_snp_table_create / _create_hits / their _dev twins, csvgpu_snp_table_query;
kernels/snptable.hip): the answer for every region equals the numpy statement of tests/snp_table_inputs.py byte for byte — NaN bits
included — on both kinds of table, at the table sizes and region counts where a binary search, a wave boundary or the prefix maximum
can go wrong; snp_off is exact, nothing is written behind the outputs, the capacity handshake writes nothing, unsorted input is refused,
and a table is readable from a second context of its device."""
import numpy as np
import pytest
import torch

import snp_table_inputs as sti
import contextsv_amd as cs
from contextsv_amd import CsvError, _lib

pytestmark = pytest.mark.gpu
GUARD = 64
FILL = 0xA5


def _make(ctx, kind, t):
    if kind == "records":
        return ctx.snp_table(t["pos"], t["baf"], t["pfb"], t["has_pfb"])
    return ctx.snp_table_hits(t["pos"], t["baf"], t["af_pos"], t["af"])


def _query_guarded(ctx, table, s, e, want):
    """The call into arrays of exactly the needed size + GUARD sentinel entries -> dict; asserts the sentinels."""
    R, n = len(s), len(want["pos"])
    off = np.full(R + 1 + GUARD, 0xA5A5A5A5A5A5A5A5, np.uint64)
    pos = np.frombuffer(bytes([FILL]) * ((n + GUARD) * 4), np.uint32).copy()
    baf, pfb = (np.frombuffer(bytes([FILL]) * ((n + GUARD) * 8), np.float64).copy() for _ in range(2))
    rc, got_n = ctx.snp_table_query_raw(table, s, e, off, pos, baf, pfb, n)
    assert rc == 0 and got_n == n, (rc, got_n, n, ctx.last_error())
    for a, k in ((off, R + 1), (pos, n), (baf, n), (pfb, n)):
        assert a[k:].tobytes() == bytes([FILL]) * (GUARD * a.itemsize), "written behind an output"
    return {"snp_off": off[: R + 1], "pos": pos[:n], "baf": baf[:n], "pfb": pfb[:n]}


def _same(got, want, what):
    for f in ("snp_off", "pos", "baf", "pfb"):
        assert got[f].tobytes() == want[f].tobytes(), (what, f)


@pytest.mark.parametrize("kind", ["records", "hits"])
def test_families_equal_the_statement(ctx, kind):
    tables = sti.record_tables() if kind == "records" else sti.hit_tables()
    for name, t in tables.items():
        tab = _make(ctx, kind, t)
        assert tab.n == len(t["pos"])
        s, e = sti.regions_for(t, seed=5)
        want = sti.query_many(kind, t, s, e)
        _same(_query_guarded(ctx, tab, s, e, want), want, (kind, name))
        _same(ctx.snp_table_query(tab, s, e), want, (kind, name))
        tab.free()


@pytest.mark.parametrize("kind", ["records", "hits"])
def test_large_table_and_region_counts(ctx, kind):
    """~70 000 records (several workgroups, long runs among them) with R = 0, 1, 64, 65 and ~5 000 regions."""
    t = sti.random_records(91, sti.BIG_N, span=150_000, dup=0.35) if kind == "records" else sti.random_hits(92, sti.BIG_N, span=150_000)
    tab = _make(ctx, kind, t)
    for R in (0, 1, 64, 65, 5003):
        s, e = sti.random_regions(7 + R, R, 151_000)
        want = sti.query_many(kind, t, s, e)
        _same(_query_guarded(ctx, tab, s, e, want), want, (kind, R))
    s, e = np.asarray([0], np.uint32), np.asarray([sti.POS_MAX], np.uint32)          # the whole table in one region
    want = sti.query_many(kind, t, s, e)
    assert len(want["pos"]) == sti.BIG_N
    _same(_query_guarded(ctx, tab, s, e, want), want, (kind, "whole"))
    tab.free()


def test_one_run_of_equal_positions_several_workgroups(ctx):
    """Hostile input: every record at one position; the flag on one record in the middle, on none, on the last."""
    n = 70_000
    rng = np.random.default_rng(3)
    for flagged in (31_000, None, n - 1):
        has = np.zeros(n, np.uint8)
        if flagged is not None:
            has[flagged] = 1
        t = {"pos": np.full(n, 777, np.uint32), "baf": rng.uniform(0, 1, n), "pfb": rng.uniform(0, 1, n), "has_pfb": has}
        tab = _make(ctx, "records", t)
        s, e = np.asarray([0, 777, 778, 700], np.uint32), np.asarray([776, 777, 900, 800], np.uint32)
        want = sti.query_many("records", t, s, e)
        assert list(want["snp_off"]) == [0, 0, n, n, 2 * n]
        _same(_query_guarded(ctx, tab, s, e, want), want, flagged)
        tab.free()


@pytest.mark.parametrize("kind", ["records", "hits"])
def test_capacity_handshake_writes_nothing(ctx, kind):
    t = sti.record_tables()["n257"] if kind == "records" else sti.hit_tables()["n257"]
    tab = _make(ctx, kind, t)
    s, e = sti.regions_for(t, seed=6)
    want = sti.query_many(kind, t, s, e)
    n = len(want["pos"])
    assert n > 10
    for cap in (0, n - 1):
        off = np.full(len(s) + 1, 0xA5A5A5A5A5A5A5A5, np.uint64)
        pos = np.full(n, 0xA5A5A5A5, np.uint32)
        baf, pfb = (np.frombuffer(bytes([FILL]) * (n * 8), np.float64).copy() for _ in range(2))
        rc, need = ctx.snp_table_query_raw(tab, s, e, off, pos, baf, pfb, cap)
        assert rc == _lib.CSV_ECAPACITY and need == n
        assert all(a.tobytes() == bytes([FILL]) * a.nbytes for a in (off, pos, baf, pfb)), "written despite CSV_ECAPACITY"
    _same(_query_guarded(ctx, tab, s, e, want), want, kind)
    tab.free()


def test_unsorted_input_is_refused_and_the_context_stays_usable(ctx):
    t = sti.random_records(11, 300)
    bad = t["pos"].copy()
    bad[[100, 200]] = bad[[200, 100]]
    assert (np.diff(bad.astype(np.int64)) < 0).any()
    with pytest.raises(CsvError) as ei:
        ctx.snp_table(bad, t["baf"], t["pfb"], t["has_pfb"])
    assert "not ascending" in str(ei.value)
    h = sti.random_hits(12, 300)
    with pytest.raises(CsvError) as ei:
        ctx.snp_table_hits(bad, h["baf"], h["af_pos"], h["af"])
    assert "not ascending" in str(ei.value)
    bad_af = h["af_pos"].copy()
    bad_af[[3, 90]] = bad_af[[90, 3]]
    assert (np.diff(bad_af.astype(np.int64)) < 0).any()
    with pytest.raises(CsvError) as ei:
        ctx.snp_table_hits(h["pos"], h["baf"], bad_af, h["af"])
    assert "af_pos" in str(ei.value) and "not ascending" in str(ei.value)
    with pytest.raises(CsvError) as ei:                                  # the same on the device-pointer form
        ctx.snp_table(torch.from_numpy(bad.view(np.int32)).cuda(), torch.from_numpy(t["baf"]).cuda())
    assert "not ascending" in str(ei.value)
    tab = _make(ctx, "records", t)
    s, e = sti.regions_for(t, seed=8)
    _same(ctx.snp_table_query(tab, s, e), sti.query_many("records", t, s, e), "after the refusals")
    tab.free()


@pytest.mark.parametrize("kind", ["records", "hits"])
def test_device_creators_equal_the_host_ones(ctx, kind):
    dev = lambda a, view=None: None if a is None else torch.from_numpy(np.ascontiguousarray(a) if view is None else np.ascontiguousarray(a).view(view)).cuda()
    cases = [("n0", None), ("n1", None), ("n65", None), ("n257", None), ("big", None)]
    for name, _ in cases:
        if kind == "records":
            t = sti.random_records(93, 20_000, dup=0.3) if name == "big" else sti.record_tables()[name]
            d = ctx.snp_table(dev(t["pos"], np.int32), dev(t["baf"]), dev(t["pfb"]), dev(t["has_pfb"]))
        else:
            t = sti.random_hits(94, 20_000) if name == "big" else sti.hit_tables()[name]
            d = ctx.snp_table_hits(dev(t["pos"], np.int32), dev(t["baf"]), dev(t["af_pos"], np.int32), dev(t["af"]))
        h = _make(ctx, kind, t)
        assert d.n == h.n == len(t["pos"])
        s, e = sti.regions_for(t, seed=9)
        want = sti.query_many(kind, t, s, e)
        _same(ctx.snp_table_query(d, s, e), want, (kind, name, "dev"))
        _same(ctx.snp_table_query(h, s, e), want, (kind, name, "host"))
        d.free(); h.free()
    if kind == "records":                                                # pfb / has_pfb left out on the device form
        t = sti.record_tables()["no_pfb"]
        d = ctx.snp_table(dev(t["pos"], np.int32), dev(t["baf"]))
        s, e = sti.regions_for(t, seed=9)
        _same(ctx.snp_table_query(d, s, e), sti.query_many(kind, t, s, e), "no pfb, dev")
        d.free()


def test_a_table_is_read_from_a_second_context(ctx):
    t, h = sti.random_records(21, 5000), sti.random_hits(22, 5000)
    tabs = [_make(ctx, "records", t), _make(ctx, "hits", h)]
    with cs.Context(0) as other:
        for kind, tab, src in (("records", tabs[0], t), ("hits", tabs[1], h)):
            s, e = sti.random_regions(31, 700, 21_000)
            want = sti.query_many(kind, src, s, e)
            _same(other.snp_table_query(tab, s, e), want, kind)
            _same(ctx.snp_table_query(tab, s, e), want, kind)
    for tab in tabs:
        tab.free()


@pytest.mark.parametrize("kind", ["records", "hits"])
def test_the_second_carve_grows_the_arena(ctx, kind):
    """A context that has never run anything has no arena: the plan's carve (a few regions) allocates a few KiB, the records' carve behind
    the readback (1.4 MB) grows it — a new allocation, so the plan is queued again before the gather reads its tables."""
    t = sti.random_records(95, sti.BIG_N, span=150_000, dup=0.3) if kind == "records" else sti.random_hits(96, sti.BIG_N, span=150_000)
    tab = _make(ctx, kind, t)
    s, e = np.asarray([0, 5, 100_000, 7], np.uint32), np.asarray([sti.POS_MAX, 90_000, 140_000, 3], np.uint32)
    want = sti.query_many(kind, t, s, e)
    assert len(want["pos"]) > sti.BIG_N
    with cs.Context(0) as fresh:
        _same(_query_guarded(fresh, tab, s, e, want), want, kind)
    with cs.Context(0) as fresh:                                         # the arena grown behind a plan it already held
        small = sti.query_many(kind, t, s[3:], e[3:])
        _same(_query_guarded(fresh, tab, s[3:], e[3:], small), small, kind)
        _same(_query_guarded(fresh, tab, s, e, want), want, kind)
    tab.free()


def test_argument_errors(ctx):
    t = sti.record_tables()["n64"]
    tab = _make(ctx, "records", t)
    off = np.zeros(3, np.uint64)
    rc, _ = ctx.snp_table_query_raw(tab, [1, 2], [5, 6], off, None, None, None, 10)       # a capacity without arrays
    assert rc == _lib.CSV_EINVAL and "null array" in ctx.last_error()
    with pytest.raises(ValueError):
        ctx.snp_table(t["pos"], t["baf"][:-1])
    tab.free()
