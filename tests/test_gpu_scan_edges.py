"""The CIGAR scan (kernels/scan.hip) on the directed inputs of tests/scan_edge_inputs.py — tests/test_scan_edge_inputs.py proves without a
GPU that they reach the seams they are named after — against the oracle, exactly: no tolerance anywhere.

Every case in every form (a wave per read; groups of 16 / 8 lanes; a lane per read), through both entries:
  1. host pointers (ctx.cigar_scan, ctx.aln_intervals, ctx.depth): the unpadded instances, every wave searching its own split points;
  2. resident (upload -> pipeline -> fetch with the depth map, twice on the same shard: counters, bucket counts and tile ranges have to be
     zeroed again between the runs): the padded instances, the 16-bit wave form, scan_split_kernel's table.
The wave form's S, B and R cases also run with packing off (the padded 32-bit instance with the table). Compared: the signatures field by
field in the reference's order, the DEL / INS partition and the three counts, ref_end / q_start / q_end, and the depth map with its sum and
non-zero count — checkpoints and tile ranges show nowhere else. Family S also pins the host-pointer entry's capacity contract.

scan_edge_inputs.split holds below scan_grid's device cap only; the context does not tell its compute-unit count, so no case is skipped by
it: the module keeps every case at 1024 reads or fewer, which stays under the cap of any device with 22 compute units or more."""
import ctypes as C

import numpy as np
import pytest

from contextsv_amd import _lib
import scan_edge_inputs as se

pytestmark = pytest.mark.gpu

_CASES = se.all_cases()
_FIELDS = ("start", "end", "read", "qpos_kind")
_expected = {}


@pytest.fixture(params=se.FORMS, ids=se.FORM_NAMES)
def form(request, ctx):
    ctx.set_tuning(scan_form=request.param)
    ctx.set_cigar_packing(True)
    yield request.param
    ctx.set_cigar_packing(True)
    ctx.set_tuning()


def _want(oracle, case):
    """the oracle's answers, once per case and read-only"""
    name, r, depth_len, min_oplen, min_mapq = case
    if name not in _expected:
        sig = oracle.cigar_scan(r, depth_len, min_oplen, min_mapq)
        iv = [np.asarray(a).astype(np.int32) for a in oracle.aln_intervals(r)]
        od, osum, onz = oracle.depth(r, depth_len)
        for a in [sig, od] + iv:
            a.setflags(write=False)
        _expected[name] = dict(sig=sig, iv=iv, depth=(od, osum, onz))
    return _expected[name]


def _same_sigs(got, want, what):
    assert len(got) == len(want), "%s: %d signatures, want %d" % (what, len(got), len(want))
    for f in _FIELDS:
        if not np.array_equal(got[f], want[f]):
            k = int(np.flatnonzero(got[f] != want[f])[0])
            raise AssertionError("%s: signature %d of %d differs in %s: got %s, want %s" % (what, k, len(want), f, got[k], want[k]))


def _same_intervals(got, want, what):
    for key, g, o in zip(("ref_end", "q_start", "q_end"), got, want):
        if not np.array_equal(np.asarray(g).view(np.uint32), o.view(np.uint32)):
            k = int(np.flatnonzero(np.asarray(g) != o)[0])
            raise AssertionError("%s: %s of read %d: got %d, want %d" % (what, key, k, g[k], o[k]))


def _same_depth(got, want, what):
    d, s, nz = got
    od, osum, onz = want
    if not np.array_equal(d, od):
        bad = np.flatnonzero(d != od)
        raise AssertionError("%s: %d depth positions differ, first %d: got %d, want %d" % (what, len(bad), bad[0], d[bad[0]], od[bad[0]]))
    assert (s, nz) == (osum, onz), what


def _host(ctx, case, want, what):
    name, r, depth_len, min_oplen, min_mapq = case
    _same_sigs(ctx.cigar_scan(r, depth_len, min_oplen, min_mapq), want["sig"], what + " / host pointers")
    _same_intervals(ctx.aln_intervals(r), want["iv"], what + " / host pointers")
    _same_depth(ctx.depth(r, depth_len), want["depth"], what + " / host pointers")


def _resident(ctx, case, want, what, packing=True, packed=None):
    name, r, depth_len, min_oplen, min_mapq = case
    sig = want["sig"]
    is_del = (sig["qpos_kind"] & 3) == se.KIND_DEL
    ctx.set_cigar_packing(packing)
    try:
        sh = ctx.upload(r, depth_len)
    finally:
        ctx.set_cigar_packing(True)
    try:
        if packed is not None:                                   # which form the shard took, as tests/test_gpu_cigar_pack.py tells it
            m, pieces = r.n_cigar, -(-r.n_cigar // se.PIECE_OPS)
            want_bytes = 2 * (pieces * se.PIECE_OPS + 512) + 4 * (pieces + 1) + 8 if packed else 4 * (m + 512)
            assert sh.cigar_bytes() == want_bytes, what
        for run in range(2):
            tag = "%s / resident%s, run %d" % (what, "" if packing else " (packing off)", run)
            res = sh.pipeline(eps=0.1, min_pts_pct=0.1, min_oplen=min_oplen, min_mapq=min_mapq)
            out = sh.fetch(res, want_depth=True)
            assert (res.n_sig, res.n_del, res.n_ins) == (len(sig), int(is_del.sum()), int((~is_del).sum())), tag
            _same_sigs(out["sig_del"], sig[is_del], tag + ", DEL")
            _same_sigs(out["sig_ins"], sig[~is_del], tag + ", INS")
            _same_intervals((out["ref_end"], out["q_start"], out["q_end"]), want["iv"], tag)
            _same_depth((out["depth"], res.depth_sum, res.depth_nonzero), want["depth"], tag)
    finally:
        sh.free()


@pytest.mark.parametrize("case", _CASES, ids=[c[0] for c in _CASES])
def test_both_entries(ctx, oracle, form, case):
    name = case[0]
    want = _want(oracle, case)
    what = "%s, %s form" % (name, se.FORM_NAMES[form])
    _host(ctx, case, want, what)
    family = se.info(name)["family"]
    # only the wave form packs, and there every case does (no escapes in them; every R case must) but the all-empty shard, which has nothing to pack
    assert se.packs(case[1]) or family == "W"
    _resident(ctx, case, want, what, packed=form == 0 and se.packs(case[1]))
    if form == 0 and family in "SBR":
        _resident(ctx, case, want, what, packing=False, packed=False)


_S = [c for c in _CASES if se.info(c[0])["family"] == "S"]
_CANARY = 8


@pytest.mark.parametrize("case", _S, ids=[c[0] for c in _S])
def test_capacity_of_the_host_pointer_entry(ctx, oracle, form, case):
    """A buffer of exactly n_sig signatures is enough — the staged ones and the ones that went straight to HBM count once each. With one
    fewer the call returns CSV_ECAPACITY and the true count, and nothing behind the caller's capacity is written."""
    name, r, depth_len, min_oplen, min_mapq = case
    sig = _want(oracle, case)["sig"]
    n = len(sig)
    assert n > se.SIG_BUF - 2
    rs = r.c_struct()
    for cap in (n, n - 1):
        buf = np.full(n + _CANARY, 0xA5, np.uint8).repeat(16).view(_lib.SIG_DTYPE)
        assert len(buf) == n + _CANARY
        n_out = C.c_uint64(cap)
        rc = ctx.lib.csvgpu_cigar_scan(ctx.h, C.byref(rs), depth_len, min_oplen, min_mapq, buf.ctypes.data, C.byref(n_out))
        assert n_out.value == n, (name, cap)
        assert (buf[cap:].view(np.uint8) == 0xA5).all(), (name, cap)
        if cap == n:
            assert rc == _lib.CSV_OK
            _same_sigs(buf[:n], sig, "%s, capacity n_sig" % name)
        else:
            assert rc == _lib.CSV_ECAPACITY
