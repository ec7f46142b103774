"""The checks and bodies that several entry points of the C-ABI glue (contextsv_amd/csrc/api/) share, reached through every entry point that
uses them: the seg_off check (five sites), the region-table check (three window entry points), the one body behind csvgpu_window_log2 and
csvgpu_window_log2_resident, and the one CIGAR-scan launch of the per-chromosome job (plain stream or a gate's, timed or not).
Every refusal here is a host-side argument check: nothing is launched."""
import ctypes as C

import numpy as np
import pytest

import contextsv_amd as cs
from contextsv_amd._lib import CSV_EINVAL, SPLIT_FIT_DTYPE, ptr

pytestmark = pytest.mark.gpu

M, I, D = 0, 1, 2
DEPTH_TILE = 1 << 14          # common.hpp


def _refused(ctx, rc, message):
    assert rc == CSV_EINVAL
    assert ctx.lib.csvgpu_last_error(ctx.h).decode() == message


def test_decreasing_seg_off_is_refused_at_every_site(ctx):
    lib = ctx.lib
    off = np.array([0, 3, 2], np.uint64)                     # n_seg = 2, the second offset steps back
    u32, i32 = np.array([10, 20], np.uint32), np.array([10, 20], np.int32)
    labels = np.zeros(2, np.int32)
    _refused(ctx, lib.csvgpu_dbscan_iv_batch(ctx.h, ptr(u32), ptr(u32), ptr(off), 2, 0.1, 2, ptr(labels)), "dbscan batch: seg_off not monotone")
    _refused(ctx, lib.csvgpu_dbscan_1d(ctx.h, ptr(i32), ptr(off), 2, 100.0, 2, ptr(labels)), "dbscan1d: seg_off not monotone")
    sgo, go, mem, n = np.zeros(3, np.uint64), np.zeros(3, np.uint64), np.zeros(8, np.uint32), C.c_uint64(8)
    _refused(ctx, lib.csvgpu_split_groups(ctx.h, ptr(i32), ptr(i32), ptr(off), 2, ptr(sgo), ptr(go), ptr(mem), C.byref(n)),
             "split_groups: seg_off not ascending")
    # sf_check, behind csvgpu_split_fits and csvgpu_split_groups_fits
    z = np.zeros(0, np.int32)
    tables = cs.SplitTables(i32, i32 + 5, i32, i32 + 5, np.zeros(2, np.uint8), np.zeros(3, np.uint64), z, z, z, z, np.zeros(0, np.uint8))
    t, fits = tables.c_struct(), np.zeros(2, SPLIT_FIT_DTYPE)
    _refused(ctx, lib.csvgpu_split_fits(ctx.h, C.byref(t), ptr(off), 2, ptr(sgo), ptr(go), ptr(mem), 100.0, 5, ptr(fits)), "split_fits: seg_off not ascending")
    _refused(ctx, lib.csvgpu_split_groups_fits(ctx.h, C.byref(t), ptr(off), 2, 100.0, 5, ptr(sgo), ptr(fits), C.byref(n)), "split_fits: seg_off not ascending")
    # sr_check, behind csvgpu_split_tables_resident and csvgpu_split_resident_fits (the shards are looked at after the offsets)
    refs = cs.SplitRefs(np.zeros(2, np.uint32), np.zeros(3, np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint8))
    f, hs = refs.c_struct(), (C.c_void_p * 2)(None, None)
    _refused(ctx, lib.csvgpu_split_tables_resident(ctx.h, 2, hs, C.byref(f), ptr(off), C.byref(t)), "split_tables_resident: seg_off not ascending")
    _refused(ctx, lib.csvgpu_split_resident_fits(ctx.h, 2, hs, C.byref(f), ptr(off), 100.0, 5, ptr(sgo), ptr(fits), C.byref(n)),
             "split_tables_resident: seg_off not ascending")
    # the context is as usable as before
    again = ctx.dbscan_1d(np.array([10, 11, 12, 13], np.int32), np.array([0, 4], np.uint64), 100.0, 2)
    assert again[0] >= 0 and (again == again[0]).all()


def _depth_shard(ctx, depth_len=4096):
    """32 reads over 300 reference positions each, every 110 positions (the first with a deletion): a depth map of 4096 positions, values 0..3."""
    pos = np.arange(32) * 110
    reads = cs.Reads.from_cigar_lists(pos, np.zeros(32, np.uint16), np.full(32, 60, np.uint8), [[(M, 100), (D, 60), (M, 140)]] + [[(M, 300)]] * 31)
    sh = ctx.upload(reads, depth_len)
    res = sh.pipeline()
    return sh, sh.fetch(res, want_depth=True)["depth"]


def test_window_entry_points_share_the_table_check_and_the_body(ctx):
    lib = ctx.lib
    sh, depth = _depth_shard(ctx)
    try:
        assert len(depth) == 4096 and depth.max() == 3 and depth[3800:].max() == 0
        # a region without windows (sample_size = {3, 0}): refused by all three, with each one's message
        rs, re, ss, wo = np.array([0, 100], np.uint32), np.array([50, 200], np.uint32), np.array([3, 0], np.int32), np.array([0, 3, 3], np.uint64)
        l2, ws, we = np.zeros(3), np.zeros(3, np.uint32), np.zeros(3, np.uint32)
        _refused(ctx, lib.csvgpu_window_log2(ctx.h, ptr(depth), len(depth), ptr(rs), ptr(re), ptr(ss), ptr(wo), 2, 2.0, ptr(l2), ptr(ws), ptr(we)),
                 "window_log2: bad region table")
        _refused(ctx, lib.csvgpu_window_log2_resident(ctx.h, sh.h, ptr(rs), ptr(re), ptr(ss), ptr(wo), 2, 2.0, ptr(l2), ptr(ws), ptr(we)),
                 "window_log2: bad region table")
        one = lambda a: (C.c_void_p * 1)(ptr(a))
        nr, mean = np.array([2], np.uint64), np.array([2.0])
        _refused(ctx, lib.csvgpu_window_log2_resident_many(ctx.h, 1, (C.c_void_p * 1)(sh.h), one(rs), one(re), one(ss), one(wo), ptr(nr), ptr(mean),
                                                           one(l2), one(ws), one(we)), "window_log2_many: bad region table")
        # two regions over the same map: the host-pointer call and the resident call give the same arrays, bit for bit
        rs, re, ss = np.array([100, 2000], np.uint32), np.array([1500, 4000], np.uint32), np.array([7, 13], np.int32)
        h_l2, h_ws, h_we, wo = ctx.window_log2(depth, rs, re, ss, 2.0)
        nw = int(wo[-1])
        l2, ws, we = np.full(nw, -7.0), np.zeros(nw, np.uint32), np.zeros(nw, np.uint32)
        assert lib.csvgpu_window_log2_resident(ctx.h, sh.h, ptr(rs), ptr(re), ptr(ss), ptr(wo), 2, 2.0, ptr(l2), ptr(ws), ptr(we)) == 0
        assert nw == 20 and l2.tobytes() == h_l2.tobytes() and np.array_equal(ws, h_ws) and np.array_equal(we, h_we)
        assert np.isfinite(l2).any() and len(set(ws.tolist())) == nw
        m_l2, m_ws, m_we = np.full(nw, -7.0), np.zeros(nw, np.uint32), np.zeros(nw, np.uint32)
        assert lib.csvgpu_window_log2_resident_many(ctx.h, 1, (C.c_void_p * 1)(sh.h), one(rs), one(re), one(ss), one(wo), ptr(nr), ptr(mean),
                                                    one(m_l2), one(m_ws), one(m_we)) == 0
        assert m_l2.tobytes() == h_l2.tobytes() and np.array_equal(m_ws, h_ws) and np.array_equal(m_we, h_we)
    finally:
        sh.free()


def test_job_scan_launch_on_a_plain_stream_and_behind_a_gate_at_every_timing_level(ctx):
    """One coordinate-sorted shard over three depth tiles (the last holds one position). The scan of the job is one launch whether it runs
    on the context's stream under a timer, or on a gate's stream with or without the pair's events: the calls and labels never change, and
    at level 1 both big groups are counted either way."""
    depth_len = 2 * DEPTH_TILE + 1
    pos = [(i // 4) * 2000 + (i % 4) * 3 for i in range(63)] + [depth_len - 270]                      # (a depth index is pos + 1)
    cig = [[(M, 100), (D, 60 + (i // 4) % 5), (M, 100), (I, 55), (M, 100)] for i in range(63)] + [[(M, 269)]]     # the last read ends on the last position
    reads = cs.Reads.from_cigar_lists(np.array(pos), np.zeros(64, np.uint16), np.full(64, 60, np.uint8), cig)
    sh = ctx.upload(reads, depth_len)
    gate = cs.Gate()
    runs = []
    try:
        for with_gate in (False, True):
            ctx.set_gate(gate if with_gate else None)
            for level in (0, 1, 2):
                ctx.timing_enable(level); ctx.timing_reset()
                res = sh.pipeline(eps=0.1, min_pts_pct=0.1)
                out = sh.fetch(res, want_depth=True)
                t = ctx.timing()
                runs.append((res.n_del, res.n_ins, res.depth_sum, res.min_pts) + tuple(out[k].tobytes() for k in ("sig_del", "sig_ins", "label_del", "label_ins", "depth")))
                if level == 0:
                    assert all(n == 0 for _, n in t.values())
                else:
                    assert t["cigar_scan"][1] == 1 and t["depth"][1] == 1 and t["cigar_scan"][0] > 0 and t["depth"][0] > 0, (with_gate, level, t)
                if level == 2:
                    assert all(n == 0 for k, (_, n) in t.items() if k not in ("cigar_scan", "depth"))
        assert runs[0][:2] == (63, 63) and runs[0][2] == 63 * 300 + 269
        labels = np.frombuffer(runs[0][6], np.int32)
        assert labels.max() >= 0                                     # four reads share every deletion: there are clusters to compare
        assert np.frombuffer(runs[0][-1], np.uint32)[-1] == 1        # the third tile's one position
        for r in runs[1:]:
            assert r == runs[0]
    finally:
        ctx.timing_enable(0)
        ctx.set_gate(None)
        sh.free()
        gate.close()
