"""The depth pass (kernels/depth.hip, and the checkpoints and tile ranges kernels/scan.hip leaves for it) on the directed inputs of
tests/depth_edge_inputs.py — tests/test_depth_edge_inputs.py proves without a GPU that they reach the edges they are named after —
against the oracle AND the module's numpy depth map: depth array, sum and non-zero count, exactly (they are integers).

Three ways in, every form of the walk (a wave per item; groups of 16 / 8 lanes; the lanes scan with groups of 16):
  1. host pointers (ctx.depth): an unpadded arena copy, ranges from the prefix maximum, every tile builds its own list (depth_make_item<3>);
  2. resident (upload -> pipeline -> fetch, twice): padded, depth_items_kernel's lists (depth_make_item<8>) for the first batch, the scan's
     tile ranges when the shard is coordinate-sorted;
  3. wrapped device arrays (twice: the first job does not know yet whether the shard is sorted), the CIGAR array at byte offsets 0, 4, 8
     and 12 of its buffer: offset 0 is unpadded with 16-byte loads allowed, the others are the kernels' vec_ok == 0 branches (dword loads).
Ways 2 and 3 once more behind a gate, where the job launches scan and depth tiles itself on the gate's stream (test_behind_a_gate).
Not covered, because no entry point reaches it: a depth OUTPUT that is not 16-byte aligned (dvec_ok == 0)."""
import ctypes as C

import numpy as np
import pytest

import contextsv_amd as cs
import depth_edge_inputs as de

pytestmark = pytest.mark.gpu

_SMALL = de.small_cases()
_G = de.g_cases()
_WRAPPED = [c for c in _SMALL if c[0] == "A/len%d" % (2 * de.T + 5) or c[0][0] in "CDF"]
_NAMES = {(id(r), depth_len): name for name, r, depth_len in _SMALL + _G}
_expected = {}


@pytest.fixture(params=[0, 1, 2, 3], ids=["wave", "rows16", "rows8", "lanes"])
def form(request, ctx):
    ctx.set_tuning(scan_form=request.param)
    yield request.param
    ctx.set_tuning()


def _want(oracle, reads, depth_len):
    """the oracle's map and numpy's, once per case (they agree: asserted here too, so that a GPU failure is never the expectation's)"""
    name = _NAMES[id(reads), depth_len]
    if name not in _expected:
        od, osum, onz = oracle.depth(reads, depth_len)
        nd, nsum, nnz = de.np_depth(reads, depth_len)
        assert np.array_equal(od, nd) and (osum, onz) == (nsum, nnz)
        od.setflags(write=False)
        _expected[name] = (od, osum, onz)
    return _expected[name]


def _same(got, want, what):
    d, s, nz = got
    od, osum, onz = want
    if not np.array_equal(d, od):
        bad = np.flatnonzero(d != od)
        raise AssertionError("%s: %d positions differ, first %d (tile %d + %d): got %d, want %d" % (
            what, len(bad), bad[0], bad[0] >> de.DEPTH_TILE_SHIFT, bad[0] & (de.T - 1), d[bad[0]], od[bad[0]]))
    assert (s, nz) == (osum, onz), what


def _resident_twice(sh, want, what):
    for rep in range(2):
        res = sh.pipeline(eps=0.1, min_pts_pct=0.1)
        out = sh.fetch(res, want_depth=True)
        _same((out["depth"], res.depth_sum, res.depth_nonzero), want, "%s, run %d" % (what, rep))


def _check(ctx, oracle, reads, depth_len, paths):
    name, want = _NAMES[id(reads), depth_len], _want(oracle, reads, depth_len)
    if "host" in paths:
        _same(ctx.depth(reads, depth_len), want, name + " / host pointers")
    if "resident" in paths:
        sh = ctx.upload(reads, depth_len)
        try:
            _resident_twice(sh, want, name + " / resident")
        finally:
            sh.free()
    if "wrapped" in paths:
        hip = C.CDLL("libamdhip64.so")                         # the runtime the library itself is linked against
        hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        hip.hipFree.argtypes = [C.c_void_p]
        held, shards = [], []

        def to_device(a, shift=0):
            a = np.ascontiguousarray(a)
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), a.nbytes + 16) == 0
            held.append(p)
            assert hip.hipMemcpy(p.value + shift, a.ctypes.data, a.nbytes, 1) == 0          # hipMemcpyHostToDevice
            return p.value + shift

        try:
            d_pos, d_flag, d_mapq, d_off = (to_device(a) for a in (reads.pos, reads.flag, reads.mapq, reads.cigar_off))
            for shift in (0, 4, 8, 12):
                d_cig = to_device(reads.cigar, shift)
                assert d_cig % 16 == shift
                sh = ctx.wrap_device_ptrs(reads.n_reads, reads.n_cigar, d_pos, d_flag, d_mapq, d_off, d_cig, depth_len)
                shards.append(sh)
                _resident_twice(sh, want, "%s / wrapped, CIGAR array at byte offset %d" % (name, shift))
        finally:
            for sh in shards:
                sh.free()
            ctx.synchronize()
            for p in held:
                hip.hipFree(p)


@pytest.mark.parametrize("case", _SMALL, ids=[c[0] for c in _SMALL])
def test_host_and_resident(ctx, oracle, form, case):
    name, reads, depth_len = case
    _check(ctx, oracle, reads, depth_len, ("host", "resident"))


@pytest.mark.parametrize("case", _WRAPPED, ids=[c[0] for c in _WRAPPED])
def test_wrapped_at_every_alignment(ctx, oracle, form, case):
    name, reads, depth_len = case
    _check(ctx, oracle, reads, depth_len, ("wrapped",))


_GATED = [c for c in _WRAPPED if c[0] in ("A/len%d" % (2 * de.T + 5), "D/tail1")]


@pytest.mark.parametrize("case", _GATED, ids=[c[0] for c in _GATED])
def test_behind_a_gate(ctx, oracle, form, case):
    """The job's other caller of the two launchers: behind a gate a coordinate-sorted shard's scan and depth tiles go straight onto the
    gate's stream, with no chain between. Resident (padded; the wave form at 16 bits and, with packing off, at 32) and wrapped (unpadded,
    every alignment; the first job of a wrapped shard does not know its order yet and still takes the chain)."""
    name, reads, depth_len = case
    assert np.all(np.diff(reads.pos.astype(np.int64)) >= 0)           # or the gate would not take it
    gate = cs.Gate()
    ctx.set_gate(gate)
    try:
        _check(ctx, oracle, reads, depth_len, ("resident", "wrapped"))
        if form == 0:
            ctx.set_cigar_packing(False)
            _check(ctx, oracle, reads, depth_len, ("resident",))
    finally:
        ctx.set_cigar_packing(True)
        ctx.set_gate(None)
        gate.close()


@pytest.mark.parametrize("scan_form", [0, 1], ids=["wave", "rows16"])
@pytest.mark.parametrize("case", _G, ids=[c[0] for c in _G])
def test_fast_threshold(ctx, oracle, case, scan_form):
    """2^20 - 1 candidates in a full tile: the 32-bit partial sums of the fast write-out; 2^20: the 64-bit path. One workgroup walks them
    in 2048 batches."""
    name, reads, depth_len = case
    ctx.set_tuning(scan_form=scan_form)
    try:
        _check(ctx, oracle, reads, depth_len, ("host", "resident"))
    finally:
        ctx.set_tuning()
