"""csvgpu_cn_observations_tables_many / csvgpu_cn_decode_tables_many: the copy-number observations with the SNP records looked up in
resident tables on the device, against csvgpu_cn_observations_resident_many / csvgpu_cn_decode_resident_many fed the host's queryFlat
arrays for the same regions — obs_off and all five arrays byte for byte, states and log-likelihoods bit for bit — on the contig of
tests/test_gpu_cnv.py and on every region family of tests/cn_observation_inputs.py; several shards with different tables (one without a
table, one without a region), SNP-driven window counts, the 5087-window limit from either side, the decline that only the device can
decide, and the capacity handshake."""
import ctypes as C

import numpy as np
import pytest

import cn_observation_inputs as cni
import snp_table_inputs as sti
import contextsv_amd as cs
from contextsv_amd import CsvError, _lib, make_hmm
from hmm_params import WGS_HMM
from test_gpu_cnv import CHR_LEN, cnv_setup  # noqa: F401  (cnv_setup: that file's fixture)

pytestmark = pytest.mark.gpu
FIELDS = ("pos", "baf", "pfb", "log2_cov", "is_snp")


def _same(a, b, what, fields=FIELDS):
    assert a is not None, what
    assert a["obs_off"].tobytes() == b["obs_off"].tobytes(), what
    for f in fields:
        assert a[f].tobytes() == b[f].tobytes(), (what, f)


def _flat(regions, tables, kind="records"):
    """The SNP arrays of csv_cn_regions for (table index, start, end) triples, from the host's statement."""
    sp, sb, sf, so = [np.zeros(0, np.uint32)], [np.zeros(0)], [np.zeros(0)], [0]
    for t, s, e in regions:
        if tables[t] is None:
            p, b, f = np.zeros(0, np.uint32), np.zeros(0), np.zeros(0)
        elif kind == "records":
            p, b, f = cni.flat_snps(tables[t], s, e)
        else:
            p, b, f = sti.query("hits", tables[t], s, e)
            b, f = b.view(np.float64), f.view(np.float64)
        sp.append(p); sb.append(b); sf.append(f); so.append(so[-1] + len(p))
    return np.asarray(so, np.uint64), np.concatenate(sp).astype(np.uint32), np.concatenate(sb), np.concatenate(sf)


@pytest.fixture(scope="module")
def fam(ctx):
    """Two shards, the two SNP tables and every region family of cn_observation_inputs: the reference call and the resident tables."""
    reads = cni.build_reads()
    shards = [ctx.upload(reads, cni.CHR_LEN + 1) for _ in range(2)]
    res = [sh.pipeline(eps=0.1, min_pts_pct=0.1) for sh in shards]
    mean_cov = [res[0].mean_cov, 1.7 * res[1].mean_cov]
    tables = cni.build_snps()
    t = cni.device_tables(tables, cni.families(tables))
    ref = ctx.cn_observations(shards, mean_cov, t["reg_off"], t["region_start"], t["region_end"], t["sample_size"], t["snp_off"], t["snp_pos"], t["snp_baf"], t["snp_pfb"])
    dev = [ctx.snp_table(s["pos"], s["baf"], s["pfb"], s["has_pfb"]) for s in tables]
    yield shards, mean_cov, tables, t, ref, dev
    for x in dev + shards:
        x.free()


def test_every_family_equals_the_host_fed_call(ctx, fam):
    shards, mean_cov, tables, t, ref, dev = fam
    n_snps = np.diff(t["snp_off"]).astype(np.int64)
    assert (n_snps > t["sample_size"]).any() and (n_snps == 0).any(), "a region whose SNP count decides the window count, and one without SNPs"
    assert np.maximum(n_snps, t["sample_size"]).max() == cni.MAX_WINDOWS
    got = ctx.cn_observations_tables(shards, dev, mean_cov, t["reg_off"], t["region_start"], t["region_end"], t["sample_size"])
    _same(got, ref, "families")


def test_decode_equals_the_host_fed_decode(ctx, fam):
    shards, mean_cov, tables, t, ref, dev = fam
    hmm = make_hmm(**WGS_HMM)
    want = ctx.cn_decode(hmm, shards, mean_cov, t["reg_off"], t["region_start"], t["region_end"], t["sample_size"], t["snp_off"], t["snp_pos"], t["snp_baf"],
                         t["snp_pfb"], want_observations=True)
    got = ctx.cn_decode_tables(hmm, shards, dev, mean_cov, t["reg_off"], t["region_start"], t["region_end"], t["sample_size"], want_observations=True)
    _same(got, want, "decode", FIELDS + ("states", "loglik"))
    lean = ctx.cn_decode_tables(hmm, shards, dev, mean_cov, t["reg_off"], t["region_start"], t["region_end"], t["sample_size"])
    assert set(lean) == {"obs_off", "pos", "states", "loglik"}
    _same(lean, want, "decode without the arrays", ("pos", "states", "loglik"))


def test_the_cnv_contig(ctx, cnv_setup):
    """tests/test_gpu_cnv.py's contig and SNP table: its query regions and candidate-sized random ones, observations and decode."""
    sh, res, depth, snps = cnv_setup
    rng = np.random.default_rng(41)
    regs = [(70_000, 100_000, 20), (1, 399_999, 20), (205_000, 215_000, 5), (301_000, 305_000, 20), (150_000, 150_009, 20), (50_000, 52_500, 64), (399_000, 400_600, 20)]
    s = rng.integers(1000, CHR_LEN - 60_000, 60)
    regs += [(int(a), int(a + l), 20) for a, l in zip(s, rng.choice([300, 1500, 2500, 8000, 30_000, 55_000], 60))]
    rs, re, ss = (np.asarray([r[k] for r in regs]) for k in range(3))
    so, sp, sb, sf = _flat([(0, a, b) for a, b, _ in regs], [snps])
    args = ([sh], [res.mean_cov], [0, len(regs)], rs, re, ss)
    tab = ctx.snp_table(snps["pos"], snps["baf"], snps["pfb"], snps["has_pfb"])
    _same(ctx.cn_observations_tables([sh], [tab], *args[1:]), ctx.cn_observations(*args, so, sp, sb, sf), "cnv contig")
    hmm = make_hmm(**WGS_HMM)
    _same(ctx.cn_decode_tables(hmm, [sh], [tab], *args[1:]), ctx.cn_decode(hmm, *args, so, sp, sb, sf), "cnv contig, decode", ("pos", "states", "loglik"))
    tab.free()


@pytest.mark.parametrize("n_shards", [2, 3])
def test_several_shards_one_without_a_table_one_without_a_region(ctx, fam, n_shards):
    shards, mean_cov, tables, t, ref, dev = fam
    rng = np.random.default_rng(n_shards)
    regs_a = [(50_000, 150_000, 20), (1, cni.CHR_LEN - 1, 20), (200_000, 230_000, 3)] + [(int(a), int(a) + 4000, 20) for a in rng.integers(1000, 390_000, 70)]
    regs_b = [(10_000, 60_000, 30), (300_500, 305_000, 20)]
    # (shard, its resident table, the same table on the host, its regions): the shard without a region sits between the other two
    layout = [(shards[0], dev[1], tables[1], regs_a), (shards[1], dev[0], tables[0], []), (shards[0], None, None, regs_b)]
    if n_shards == 2:
        layout = [layout[0], (shards[1], None, None, regs_b)]
    use_sh, use_tab, host_tab, per = ([l[k] for l in layout] for k in range(4))
    mc = [mean_cov[0], mean_cov[1], 0.5 * mean_cov[0]][:n_shards]
    reg_off = np.concatenate([[0], np.cumsum([len(p) for p in per])])
    flat = [(c, a, b) for c, p in enumerate(per) for a, b, _ in p]
    rs, re = np.asarray([f[1] for f in flat]), np.asarray([f[2] for f in flat])
    ss = np.asarray([r[2] for p in per for r in p])
    so, sp, sb, sf = _flat(flat, host_tab)
    want = ctx.cn_observations(use_sh, mc, reg_off, rs, re, ss, so, sp, sb, sf)
    _same(ctx.cn_observations_tables(use_sh, use_tab, mc, reg_off, rs, re, ss), want, n_shards)
    assert (np.diff(so)[: len(regs_a)] > ss[: len(regs_a)]).any() and (np.diff(so)[len(regs_a):] == 0).all()


def test_first_hit_tables_feed_the_pass(ctx, fam):
    shards, mean_cov, tables, t, ref, dev = fam
    h = sti.random_hits(51, 900, n_af=300, span=cni.CHR_LEN - 1)
    tab = ctx.snp_table_hits(h["pos"], h["baf"], h["af_pos"], h["af"])
    rng = np.random.default_rng(52)
    regs = [(0, cni.CHR_LEN - 1)] + [(int(a), int(a + l)) for a, l in zip(rng.integers(0, 380_000, 120), rng.choice([0, 50, 900, 4000, 15_000], 120))]
    rs, re = np.asarray([r[0] for r in regs]), np.asarray([r[1] for r in regs])
    ss = np.full(len(regs), 20)
    so, sp, sb, sf = _flat([(0, a, b) for a, b in regs], [h], kind="hits")
    assert (sf.view(np.uint64) != 0).any() and np.isnan(sb).any()
    args = ([shards[0]], [mean_cov[0]], [0, len(regs)], rs, re, ss)
    _same(ctx.cn_observations_tables([shards[0]], [tab], *args[1:]), ctx.cn_observations(*args, so, sp, sb, sf), "hits")
    tab.free()


def test_window_limit_from_both_sides(ctx, fam):
    shards, mean_cov, tables, t, ref, dev = fam
    one = ([shards[0]], [dev[0]], [mean_cov[0]], [0, 1])
    so, sp, sb, sf = _flat([(0, 1000, 90_000)], tables)
    ok = ctx.cn_observations_tables(*one, [1000], [90_000], [cni.MAX_WINDOWS])
    _same(ok, ctx.cn_observations([shards[0]], [mean_cov[0]], [0, 1], [1000], [90_000], [cni.MAX_WINDOWS], so, sp, sb, sf), "5087 windows")
    with pytest.raises(CsvError) as ei:                                    # 5088 from the sample size: the host can see it
        ctx.cn_observations_tables(*one, [1000], [90_000], [cni.MAX_WINDOWS + 1])
    assert ei.value.status == _lib.CSV_EINVAL and "5087" in str(ei.value)


def _raw_tables_call(ctx, shard, tab, mean_cov, rs, re, ss, cap):
    """csvgpu_cn_observations_tables_many into sentinel-filled arrays -> (status, n, arrays)."""
    hs, ts = (C.c_void_p * 1)(shard.h), (C.c_void_p * 1)(tab.h)
    mc, ro = np.asarray([mean_cov], np.float64), np.asarray([0, len(rs)], np.uint64)
    rs, re, ss = np.asarray(rs, np.uint32), np.asarray(re, np.uint32), np.asarray(ss, np.int32)
    t = _lib.csv_cn_table_regions(1, C.cast(hs, C.c_void_p), C.cast(ts, C.c_void_p), mc.ctypes.data, ro.ctypes.data, rs.ctypes.data, re.ctypes.data, ss.ctypes.data)
    arrays = [np.full(len(rs) + 1, 0xA5A5A5A5A5A5A5A5, np.uint64), np.full(max(cap, 1), 0xA5A5A5A5, np.uint32)]
    arrays += [np.frombuffer(b"\xa5" * (max(cap, 1) * 8), np.float64).copy() for _ in range(3)] + [np.full(max(cap, 1), 0xA5, np.uint8)]
    n = C.c_uint64(cap)
    rc = ctx.lib.csvgpu_cn_observations_tables_many(ctx.h, C.byref(t), *[a.ctypes.data for a in arrays], C.byref(n))
    return rc, int(n.value), arrays


def test_a_region_with_5088_snps_is_declined_and_nothing_is_written(ctx, fam):
    """Only the device knows the region's record count: the call declines, the caller's arrays are untouched, the next call works."""
    shards, mean_cov, tables, t, ref, dev = fam
    n = cni.MAX_WINDOWS + 1
    pos = np.arange(2000, 2000 + n, dtype=np.uint32)
    tab = ctx.snp_table(pos, np.full(n, 0.5))
    rc, cnt, arrays = _raw_tables_call(ctx, shards[0], tab, mean_cov[0], [1000, 2000], [1500, 2000 + n - 1], [20, 20], 100_000)
    assert rc == 1 and cnt == 100_000 and "5087" in ctx.last_error()
    assert all(a.tobytes() == b"\xa5" * a.nbytes for a in arrays), "written although declined"
    assert ctx.cn_observations_tables([shards[0]], [tab], [mean_cov[0]], [0, 2], [1000, 2000], [1500, 2000 + n - 1], [20, 20]) is None
    so, sp, sb, sf = _flat([(0, 2000, 2000 + n - 2)], [{"pos": pos, "baf": np.full(n, 0.5), "pfb": np.zeros(n), "has_pfb": np.zeros(n, np.uint8)}])
    ok = ctx.cn_observations_tables([shards[0]], [tab], [mean_cov[0]], [0, 1], [2000], [2000 + n - 2], [20])             # 5087 records: served
    _same(ok, ctx.cn_observations([shards[0]], [mean_cov[0]], [0, 1], [2000], [2000 + n - 2], [20], so, sp, sb, sf), "5087 SNPs")
    tab.free()


def test_capacity_below_the_bound_returns_the_bound(ctx, fam):
    shards, mean_cov, tables, t, ref, dev = fam
    keep = np.arange(0, len(t["region_start"]), 7)
    keep = keep[keep < int(t["reg_off"][1])]                              # regions of the first shard
    rs, re, ss = t["region_start"][keep], t["region_end"][keep], t["sample_size"][keep]
    n_snps = np.diff(t["snp_off"]).astype(np.int64)[keep]
    bound = int(np.maximum(n_snps, ss).sum() + 3 * n_snps.sum())
    args = ([shards[0]], [dev[0]], [mean_cov[0]], [0, len(keep)], rs, re, ss)
    full = ctx.cn_observations_tables(*args)
    assert 0 < len(full["pos"]) <= bound
    for cap in (0, len(full["pos"]), bound - 1):
        rc, need, arrays = _raw_tables_call(ctx, shards[0], dev[0], mean_cov[0], rs, re, ss, cap)
        assert rc == _lib.CSV_ECAPACITY and need == bound, (cap, rc, need)
        assert all(a.tobytes() == b"\xa5" * a.nbytes for a in arrays), "written despite CSV_ECAPACITY"
    with pytest.raises(CsvError) as ei:
        ctx.cn_observations_tables(*args, capacity=bound - 1)
    assert ei.value.status == _lib.CSV_ECAPACITY and ei.value.needed == bound
    _same(ctx.cn_observations_tables(*args, capacity=bound), full, "second call")
    hmm = make_hmm(**WGS_HMM)
    with pytest.raises(CsvError) as ei:
        ctx.cn_decode_tables(hmm, *args, capacity=bound - 1)
    assert ei.value.status == _lib.CSV_ECAPACITY and ei.value.needed == bound


def test_the_second_carve_grows_the_arena(fam):
    """A context that has never run anything has no arena: the plan's carve (three regions) allocates a few KiB, the plan's readback then
    asks for 15 261 windows and the second carve must grow the arena — a new allocation, so the plan is queued again into it before the
    chain reads its tables. Twice over, so that the second context's larger call grows an arena that already holds a plan."""
    shards, mean_cov, tables, t, ref, dev = fam
    hmm = make_hmm(**WGS_HMM)
    rs, re, ss = [1000, 120_000, 250_000], [90_000, 200_000, 399_000], [cni.MAX_WINDOWS] * 3
    so, sp, sb, sf = _flat([(0, a, b) for a, b in zip(rs, re)], tables)
    args = ([shards[0]], [mean_cov[0]], [0, 3], rs, re, ss)
    with cs.Context(0) as first:
        want = first.cn_observations(*args, so, sp, sb, sf)
        want_dec = first.cn_decode(hmm, *args, so, sp, sb, sf)
    for n_regions in (1, 3):                                             # a fresh context each: its first table call grows from nothing
        with cs.Context(0) as fresh:
            a1 = ([shards[0]], [dev[0]], [mean_cov[0]], [0, n_regions], rs[:n_regions], re[:n_regions], ss[:n_regions])
            got = fresh.cn_observations_tables(*a1)
            assert got is not None and len(got["pos"]) >= n_regions * cni.MAX_WINDOWS
            if n_regions == 3:
                _same(got, want, "grown arena")
            else:                                                        # ... and the same context again with three times the windows
                _same(fresh.cn_observations_tables([shards[0]], [dev[0]], *args[1:]), want, "arena grown behind a plan")
    with cs.Context(0) as fresh:
        _same(fresh.cn_decode_tables(hmm, [shards[0]], [dev[0]], *args[1:]), want_dec, "grown arena, decode", ("pos", "states", "loglik"))


def test_no_region_and_argument_errors(ctx, fam):
    shards, mean_cov, tables, t, ref, dev = fam
    empty = ctx.cn_observations_tables(shards, dev, mean_cov, [0, 0, 0], [], [], [])
    assert len(empty["pos"]) == 0 and list(empty["obs_off"]) == [0]
    assert list(ctx.cn_decode_tables(make_hmm(**WGS_HMM), shards, dev, mean_cov, [0, 0, 0], [], [], [])["obs_off"]) == [0]
    one = ([shards[0]], [dev[0]], [mean_cov[0]], [0, 1])
    bad = {"sample_size <= 0": ([1000], [2000], [0]), "start > end": ([2000], [1000], [20]), "2^31": ([2 ** 31 - 100], [2 ** 31 - 1], [20])}
    for what, a in bad.items():
        with pytest.raises(CsvError) as ei:
            ctx.cn_observations_tables(*one, *a)
        assert ei.value.status == _lib.CSV_EINVAL and (what.split()[0] in str(ei.value) or what in str(ei.value)), (what, str(ei.value))
    with pytest.raises(CsvError) as ei:
        ctx.cn_observations_tables(shards, dev, mean_cov, [0, 2, 1], [1000], [2000], [20])
    assert ei.value.status == _lib.CSV_EINVAL and "reg_off" in str(ei.value)
    _same(ctx.cn_observations_tables(shards, dev, mean_cov, t["reg_off"], t["region_start"], t["region_end"], t["sample_size"]), ref, "after the refusals")


OPTIONAL = ("baf", "pfb", "log2_cov", "is_snp")


def _family_regions(ctx, fam, route):
    """The families as the C struct of either route -> (struct, keep-alive, R, the bound windows + 3 records)."""
    shards, mean_cov, tables, t, ref, dev = fam
    common = (mean_cov, t["reg_off"], t["region_start"], t["region_end"], t["sample_size"])
    if route == "host":
        reg, keep, R = ctx._cn_regions(shards, *common, t["snp_off"], t["snp_pos"], t["snp_baf"], t["snp_pfb"], "test")
    else:
        reg, keep, R = ctx._cn_table_regions(shards, dev, *common, "test")
    n_snps = np.diff(t["snp_off"]).astype(np.int64)
    return reg, keep, R, int(np.maximum(n_snps, t["sample_size"]).sum() + 3 * n_snps.sum())


def _raw_decode(ctx, fam, route, want):
    """csvgpu_cn_decode_resident_many ("host") / _tables_many ("tables") with the optional arrays in `want` and null for the others."""
    reg, keep, R, bound = _family_regions(ctx, fam, route)
    hmm = make_hmm(**WGS_HMM)
    out = dict(obs_off=np.zeros(R + 1, np.uint64), pos=np.zeros(bound, np.uint32), states=np.zeros(bound, np.int32), loglik=np.zeros(R, np.float64))
    out.update({f: np.zeros(bound, np.uint8 if f == "is_snp" else np.float64) for f in want})
    n = C.c_uint64(bound)
    fn = ctx.lib.csvgpu_cn_decode_resident_many if route == "host" else ctx.lib.csvgpu_cn_decode_tables_many
    rc = fn(ctx.h, C.byref(reg), C.byref(hmm), *[_lib.ptr(out.get(f)) for f in ("obs_off", "pos", "states", "loglik") + OPTIONAL], C.byref(n))
    assert rc == _lib.CSV_OK, (route, want, rc, ctx.last_error())
    k = int(n.value)
    return {f: (a if f in ("obs_off", "loglik") else a[:k]) for f, a in out.items()}


def test_each_optional_array_alone(ctx, fam):
    """The decode calls take each of baf / pfb / log2_cov / is_snp on its own: a null pointer gets no slot and no copy, and what is asked
    for comes back as in the call that asks for all four. (The wrapper passes all four or none, hence the calls through ctypes.)"""
    for route in ("host", "tables"):
        full = _raw_decode(ctx, fam, route, OPTIONAL)
        assert full["obs_off"].tobytes() == fam[4]["obs_off"].tobytes() and full["pos"].tobytes() == fam[4]["pos"].tobytes(), route
        for f in OPTIONAL:
            got = _raw_decode(ctx, fam, route, (f,))
            assert set(got) == {"obs_off", "pos", "states", "loglik", f}
            for name, a in got.items():
                assert a.tobytes() == full[name].tobytes(), (route, f, name)


def test_host_fed_capacity_leaves_the_arrays_untouched(ctx, fam):
    """csvgpu_cn_observations_resident_many runs with any capacity and reports the exact count afterwards: one short of it is
    CSV_ECAPACITY with that count in *n_obs and nothing written to obs_off or the five arrays; the context serves the next call."""
    shards, mean_cov, tables, t, ref, dev = fam
    reg, keep, R, bound = _family_regions(ctx, fam, "host")
    total = len(ref["pos"])
    cap = total - 1
    arrays = [np.full(R + 1, 0xA5A5A5A5A5A5A5A5, np.uint64), np.full(cap, 0xA5A5A5A5, np.uint32)]
    arrays += [np.frombuffer(b"\xa5" * (cap * 8), np.float64).copy() for _ in range(3)] + [np.full(cap, 0xA5, np.uint8)]
    n = C.c_uint64(cap)
    rc = ctx.lib.csvgpu_cn_observations_resident_many(ctx.h, C.byref(reg), *[_lib.ptr(a) for a in arrays], C.byref(n))
    assert rc == _lib.CSV_ECAPACITY and int(n.value) == total, (rc, int(n.value), total)
    assert all(a.tobytes() == b"\xa5" * a.nbytes for a in arrays), "written despite CSV_ECAPACITY"
    again = ctx.cn_observations(shards, mean_cov, t["reg_off"], t["region_start"], t["region_end"], t["sample_size"], t["snp_off"], t["snp_pos"], t["snp_baf"], t["snp_pfb"])
    _same(again, ref, "after CSV_ECAPACITY")
