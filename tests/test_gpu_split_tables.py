"""csvgpu_split_tables_resident / csvgpu_split_resident_fits (Context.split_tables_resident, Context.split_resident_fits): the split-read
pass's member and supplementary tables built on the device from record references into resident shards, against the numpy restatement of
tests/test_split_tables_ref.py fed with the oracle's alignment intervals — field for field — and the groups -> fits chain run on them where
they lie, against csvgpu_split_groups_fits on the returned tables and against the restatements of the groups and the fits — byte for byte."""
import ctypes as C

import numpy as np
import pytest

import contextsv_amd as cs
from contextsv_amd import Reads, host
from contextsv_amd._lib import CSV_EINVAL, SPLIT_FIT_DTYPE, ptr
from test_gpu_split import _make_split_shard
from test_gpu_split_device_groups import _make_dense_shard
from test_split_fits_ref import EPS, MIN_PTS, TABLE_FIELDS, group_set_sizes, reference_fits
from test_split_groups_host import reference_groups
from test_split_tables_ref import assert_same_tables, contig_slices, reference_tables

pytestmark = pytest.mark.gpu
M = 0
ST_GRID_CAP = 1024 * 256          # launch_st_tables (kernels/splittables.hip): at most ST_MAX_BLOCKS workgroups of 256 threads; item = member or entry


def _contig_reads(reads, a, b):
    w0, w1 = int(reads.cigar_off[a]), int(reads.cigar_off[b])
    return Reads(reads.pos[a:b].copy(), reads.flag[a:b].copy(), reads.mapq[a:b].copy(), (reads.cigar_off[a:b + 1] - np.uint64(w0)).copy(), reads.cigar[w0:w1].copy())


def _segments(reads, intervals, lo):
    e, qs, qe = intervals
    return [dict(pos=reads.pos[a:b], flag=reads.flag[a:b], ref_end=e[a:b], q_start=qs[a:b], q_end=qe[a:b]) for a, b in zip(lo[:-1], lo[1:])]


class Case:
    """One generated shard, every contig of it uploaded as its own shard and run, with its references and both restated tables."""

    def __init__(self, ctx, oracle, made):
        reads, tid, qn, n_contigs = made
        self.lo = lo = contig_slices(tid, n_contigs)
        self.refs, self.seg_off, _ = host.split_refs(tid, reads.pos, reads.flag, reads.mapq, qn, n_contigs)
        o = oracle.aln_intervals(reads)
        self.want = reference_tables(_segments(reads, o, lo), self.refs, self.seg_off)
        self.want_from_scan = reference_tables(_segments(reads, ctx.aln_intervals(reads), lo), self.refs, self.seg_off)
        self.shards = []
        for a, b in zip(lo[:-1], lo[1:]):
            sh = ctx.upload(_contig_reads(reads, int(a), int(b)), int(o[0][a:b].max()) + 16)
            self.shards.append(sh)
            sh.pipeline()

    def free(self):
        for sh in self.shards:
            sh.free()


CASES = {"split1": lambda: _make_split_shard(1), "split2": lambda: _make_split_shard(2), "split3": lambda: _make_split_shard(3),
         "dense11": lambda: _make_dense_shard(11)}


@pytest.fixture(scope="module")
def cases(ctx, oracle):
    made = {}

    def get(name):
        if name not in made:
            made[name] = Case(ctx, oracle, CASES[name]())
        return made[name]

    yield get
    for c in made.values():
        c.free()


def _same_records(got, want, what):
    assert got.dtype == SPLIT_FIT_DTYPE and len(got) == len(want), (what, len(got), len(want))
    if got.tobytes() != want.tobytes():
        bad = [g for g in range(len(want)) if got[g].tobytes() != want[g].tobytes()]
        raise AssertionError("%s: %d of %d records differ, first %d: got %s, want %s" % (what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]]))


# ---- G1 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_tables_match_the_restatement(ctx, cases, name):
    c = cases(name)
    assert c.refs.n_members > 100 and c.refs.n_supp >= c.refs.n_members
    if name.startswith("split"):
        assert (c.refs.supp_where != 0).any()                 # entries on another tid went through
    T = ctx.split_tables_resident(c.shards, c.refs, c.seg_off)
    assert_same_tables(T, c.want, name + ": oracle's intervals")
    assert_same_tables(T, c.want_from_scan, name + ": csvgpu_aln_intervals")
    other = (T.supp_flags & 2) != 0
    assert np.array_equal(T.supp_flags[other], c.refs.supp_where[other]) and not T.supp_start[other].any() and not T.supp_q_end[other].any()


# ---- G2 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_call_matches_groups_fits_on_the_tables_and_the_restatements(ctx, oracle, cases, name):
    c = cases(name)
    T = ctx.split_tables_resident(c.shards, c.refs, c.seg_off)
    sgo, fits = ctx.split_resident_fits(c.shards, c.refs, c.seg_off)
    sgo2, fits2 = ctx.split_fits(T, c.seg_off)
    assert np.array_equal(sgo, sgo2) and len(fits) > 20
    _same_records(fits, fits2, name + ": csvgpu_split_groups_fits on the returned tables")
    groups = reference_groups(c.want["start"], c.want["end"], c.seg_off)
    assert np.array_equal(sgo, groups[0])
    _same_records(fits, reference_fits(oracle, c.want, c.seg_off, groups), name + ": restatement")


def test_other_eps_and_min_pts(ctx, oracle, cases):
    c = cases("split2")
    groups = reference_groups(c.want["start"], c.want["end"], c.seg_off)
    for eps, min_pts in ((0.0, 1), (25.0, 3), (5000.0, 40)):
        _same_records(ctx.split_resident_fits(c.shards, c.refs, c.seg_off, eps=eps, min_pts=min_pts)[1],
                      reference_fits(oracle, c.want, c.seg_off, groups, eps, min_pts), (eps, min_pts))


def test_empty_segments_no_segments_and_no_entries(ctx, oracle, cases):
    c = cases("split1")
    # an empty segment in the middle (its shard is then never read), one in front and one behind
    s = c.seg_off
    seg_off = np.array([0, 0, s[1], s[1], s[2], s[3], s[3]], np.uint64)
    shards = [c.shards[2], c.shards[0], c.shards[2], c.shards[1], c.shards[2], c.shards[0]]
    T = ctx.split_tables_resident(shards, c.refs, seg_off)
    assert_same_tables(T, c.want, "empty segments")
    sgo, fits = ctx.split_resident_fits(shards, c.refs, seg_off)
    groups = reference_groups(c.want["start"], c.want["end"], seg_off)
    assert np.array_equal(sgo, groups[0]) and sgo[2] == sgo[3] and sgo[0] == sgo[1] == 0 and sgo[5] == sgo[6]
    _same_records(fits, reference_fits(oracle, c.want, seg_off, groups), "empty segments")
    _same_records(fits, ctx.split_fits(T, seg_off)[1], "empty segments, on the tables")
    # nothing at all
    none = cs.SplitRefs([], [0], [], [])
    for shards, seg_off in (([], [0]), (c.shards, [0, 0, 0, 0])):
        T = ctx.split_tables_resident(shards, none, seg_off)
        assert T.n_members == 0 and T.n_supp == 0 and T.supp_off.tolist() == [0]
        sgo, fits = ctx.split_resident_fits(shards, none, seg_off)
        assert sgo.tolist() == [0] * len(seg_off) and len(fits) == 0
    # members, no supplementary entry: the groups are there, sets 2-5 empty
    bare = cs.SplitRefs(c.refs.member_rec, np.zeros(c.refs.n_members + 1, np.uint64), [], [])
    want = reference_tables([dict(pos=np.zeros(0)) for _ in c.shards], cs.SplitRefs([], [0], [], []), [0, 0, 0, 0])
    want.update({k: c.want[k] for k in ("start", "end", "q_start", "q_end", "reverse")}, supp_off=bare.supp_off)
    T = ctx.split_tables_resident(c.shards, bare, c.seg_off)
    assert_same_tables(T, want, "no entries")
    sgo, fits = ctx.split_resident_fits(c.shards, bare, c.seg_off)
    groups = reference_groups(want["start"], want["end"], c.seg_off)
    assert np.array_equal(sgo, groups[0]) and len(fits) > 20 and not fits["size"][:, 2:].any() and fits["size"][:, :2].any()
    _same_records(fits, reference_fits(oracle, want, c.seg_off, groups), "no entries")
    # no segment with two members: no group, nothing launched
    one = cs.SplitRefs(c.refs.member_rec[:1], c.refs.supp_off[:2], c.refs.supp_rec[: int(c.refs.supp_off[1])], c.refs.supp_where[: int(c.refs.supp_off[1])])
    sgo, fits = ctx.split_resident_fits(c.shards[:1], one, [0, 1])
    assert sgo.tolist() == [0, 0] and len(fits) == 0


# ---- G3 --------------------------------------------------------------------------------------------------------------------------------
SENTINEL = 0x5A


class _Raw:
    """The two raw entry points on outputs filled with a sentinel; every call must return CSV_EINVAL and leave them as they were."""

    def __init__(self, ctx, shards, refs, seg_off):
        self.ctx, self.refs, self.seg_off = ctx, refs, np.ascontiguousarray(seg_off, np.uint64)
        self.hs = (C.c_void_p * len(shards))(*[s.h for s in shards])
        self.n_seg = len(shards)

    def refused(self, what, f=None, hs="same", seg_off="same", n_seg=None, eps=EPS, min_pts=MIN_PTS, only_fits=False, null_out=None):
        ctx, lib = self.ctx, self.ctx.lib
        f = f if f is not None else self.refs.c_struct()
        hs = self.hs if isinstance(hs, str) else hs
        so = self.seg_off if isinstance(seg_off, str) else (None if seg_off is None else np.ascontiguousarray(seg_off, np.uint64))
        n_seg = self.n_seg if n_seg is None else n_seg
        nm, ns = self.refs.n_members, self.refs.n_supp
        fp = C.byref(f) if f else None
        if not only_fits:
            i32 = lambda n: np.full(n, SENTINEL, np.int32)
            T = cs.SplitTables(i32(nm), i32(nm), i32(nm), i32(nm), np.full(nm, SENTINEL, np.uint8), np.full(nm + 1, SENTINEL, np.uint64), i32(ns), i32(ns), i32(ns),
                               i32(ns), np.full(ns, SENTINEL, np.uint8))
            t = T.c_struct()
            t.n_members = t.n_supp = SENTINEL
            if null_out == "tables":
                assert lib.csvgpu_split_tables_resident(ctx.h, n_seg, hs, fp, ptr(so), None) == CSV_EINVAL, what
            else:
                if null_out == "supp_flags":
                    t.supp_flags = None
                assert lib.csvgpu_split_tables_resident(ctx.h, n_seg, hs, fp, ptr(so), C.byref(t)) == CSV_EINVAL, what
            assert ctx.lib.csvgpu_last_error(ctx.h), what
            assert (t.n_members, t.n_supp) == (SENTINEL, SENTINEL), what
            assert all((getattr(T, k) == SENTINEL).all() for k in TABLE_FIELDS), what
        if null_out in ("tables", "supp_flags"):
            return
        sgo, out, n = np.full(n_seg + 1, SENTINEL, np.uint64), np.full(max(nm, 1), SENTINEL, np.uint8).repeat(64).view(SPLIT_FIT_DTYPE), C.c_uint64(SENTINEL)
        args = [ptr(sgo), ptr(out), C.byref(n)]
        if null_out is not None:
            args[null_out] = None
        assert lib.csvgpu_split_resident_fits(ctx.h, n_seg, hs, fp, ptr(so), eps, min_pts, *args) == CSV_EINVAL, what
        assert ctx.lib.csvgpu_last_error(ctx.h), what
        assert (sgo == SENTINEL).all() and n.value == SENTINEL and (out.view(np.uint8) == SENTINEL).all(), what


def test_invalid_input_and_the_context_afterwards(ctx, cases):
    c = cases("split1")
    raw = _Raw(ctx, c.shards, c.refs, c.seg_off)
    r, s = c.refs, c.seg_off
    nm, ns = r.n_members, r.n_supp
    n_reads = [sh.n_reads for sh in c.shards]

    def struct(**kw):
        f = r.c_struct()
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    def changed(**kw):
        d = {k: getattr(r, k).copy() for k in ("member_rec", "supp_off", "supp_rec", "supp_where")}
        for k, (i, v) in kw.items():
            d[k][i] = v
        keep = cs.SplitRefs(**d)
        f = keep.c_struct()
        f._keep = keep
        return f

    # null arrays
    raw.refused("null refs", f=False)
    raw.refused("null seg_off", seg_off=None)
    raw.refused("null shards", hs=None)
    for k in ("member_rec", "supp_off", "supp_rec", "supp_where"):
        raw.refused("null " + k, f=struct(**{k: None}))
    raw.refused("null tables", null_out="tables")
    raw.refused("null array in the tables", null_out="supp_flags")
    for k in range(3):
        raw.refused("null output %d" % k, only_fits=True, null_out=k)
    # offsets
    raw.refused("seg_off[0] != 0", seg_off=[1, s[1], s[2], s[3]])
    raw.refused("seg_off not ascending", seg_off=[0, s[2], s[1], s[3]])
    raw.refused("seg_off does not end at the count", seg_off=[0, s[1], s[2], s[3] - 1])
    raw.refused("seg_off beyond the count", seg_off=[0, s[1], s[2], s[3] + 1])
    raw.refused("supp_off[0] != 0", f=changed(supp_off=(0, 1)))
    raw.refused("supp_off not ascending", f=changed(supp_off=(5, int(r.supp_off[4]) - 1)))
    raw.refused("supp_off does not end at the count", f=changed(supp_off=(nm, ns - 1)))
    # shards and record indices
    hs = (C.c_void_p * 3)(c.shards[0].h, None, c.shards[2].h)
    raw.refused("null shard", hs=hs)
    m_last = int(s[1]) - 1                                       # the last member of segment 0
    raw.refused("member beyond its shard", f=changed(member_rec=(m_last, n_reads[0])))
    same = np.flatnonzero(r.supp_where == 0)
    z = int(same[same < int(r.supp_off[int(s[1])])][-1])        # a same-shard entry of segment 0
    raw.refused("entry beyond its shard", f=changed(supp_rec=(z, n_reads[0])))
    for w in (1, 4, 255):
        raw.refused("supp_where %d" % w, f=changed(supp_where=(z, w)))
    # counts
    raw.refused("2^32 - 1 members", f=struct(n_members=0xFFFFFFFF))
    raw.refused("2^32 - 1 entries", f=struct(n_supp=0xFFFFFFFF))
    raw.refused("2^40 entries", f=struct(n_supp=1 << 40))
    # eps / min_pts as csvgpu_dbscan_1d
    for eps, min_pts in ((-1.0, 5), (float("nan"), 5), (100.0, 0)):
        raw.refused((eps, min_pts), eps=eps, min_pts=min_pts, only_fits=True)
    # an entry on another tid may carry any record index
    z = int(np.flatnonzero(r.supp_where != 0)[0])
    other = changed(supp_rec=(z, 0xFFFFFFF0))._keep
    assert_same_tables(ctx.split_tables_resident(c.shards, other, s), c.want, "other-tid record index")
    # a pending split order
    reads = Reads.from_cigar_lists([1, 2, 3], [0, 0, 0x800], [60, 60, 60], [[(0, 10)]] * 3)
    sh = ctx.upload(reads, 100)
    try:
        sh.set_qname_hash(np.array([5, 9, 5], np.uint64))
        one = (C.c_void_p * 1)(sh.h)
        assert ctx.lib.csvgpu_split_order_begin(ctx.h, 1, one, 20) == 0
        try:
            raw.refused("pending split order")
        finally:
            out_rec, out_off = np.zeros(8, np.uint32), np.zeros(2, np.uint64)
            supp = np.array([5], np.uint64)
            assert ctx.lib.csvgpu_split_order_finish(ctx.h, ptr(supp), 1, ptr(out_rec), 8, ptr(out_off)) == 0
    finally:
        sh.free()
    # the context is usable afterwards
    T = ctx.split_tables_resident(c.shards, r, s)
    assert_same_tables(T, c.want, "after the errors")
    _same_records(ctx.split_resident_fits(c.shards, r, s)[1], ctx.split_fits(T, s)[1], "after the errors")


# ---- G4 --------------------------------------------------------------------------------------------------------------------------------
def test_more_items_than_the_capped_grid_and_a_set_beyond_lds(ctx, oracle):
    """Synthetic references that revisit the 2 000 records of one shard (twice: two segments): more members + entries than the kernel's grid has
    threads, so that it strides; the last segment is small and holds one member with 600 entries on its own contig — sets 2 and 3 of its group
    have more than 512 points and take the large-set path of the fits through the new entry point."""
    rng = np.random.default_rng(5)
    n = 2000
    pos = (np.arange(n) // 2) * 10_000 + (np.arange(n) % 2) * 50 + 1000         # records 2i and 2i + 1 overlap each other and nothing else
    flag = np.where(rng.random(n) < 0.4, 0x10, 0).astype(np.uint16)
    reads = Reads.from_cigar_lists(pos, flag, [60] * n, [[(4, int(rng.integers(0, 40))), (M, int(rng.integers(2000, 4000))), (4, int(rng.integers(1, 90)))] for _ in range(n)])
    sh = ctx.upload(reads, int(pos.max()) + 5000)
    try:
        sh.pipeline()
        n_bulk, per, n_small, n_big = 20_000, 14, 6, 600
        member_rec = np.concatenate([rng.integers(0, n, n_bulk), rng.integers(100, 102, n_small)]).astype(np.uint32)
        counts = np.concatenate([np.full(n_bulk, per), [3, n_big, 0, 2, 1, 4]]).astype(np.uint64)
        supp_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        ns = int(supp_off[-1])
        supp_where = rng.choice(np.array([0, 0, 0, 2, 3], np.uint8), ns)
        supp_where[int(supp_off[n_bulk + 1]): int(supp_off[n_bulk + 2])] = 0
        supp_rec = rng.integers(0, n, ns)
        supp_rec[int(supp_off[n_bulk + 1]): int(supp_off[n_bulk + 2])] = rng.integers(500, 502, n_big)        # two places: clusters of hundreds
        refs = cs.SplitRefs(member_rec, supp_off, supp_rec, supp_where)
        seg_off = np.array([0, n_bulk, n_bulk + n_small], np.uint64)
        assert refs.n_supp > ST_GRID_CAP and refs.n_members + refs.n_supp > ST_GRID_CAP + refs.n_supp // 16
        seg = _segments(reads, oracle.aln_intervals(reads), np.array([0, n]))[0]
        want = reference_tables([seg, seg], refs, seg_off)
        T = ctx.split_tables_resident([sh, sh], refs, seg_off)
        assert_same_tables(T, want, "beyond the grid")
        ctx.timing_enable(1)
        try:
            ctx.timing_reset()
            sgo, fits = ctx.split_resident_fits([sh, sh], refs, seg_off)
            tm = ctx.timing()
        finally:
            ctx.timing_enable(0)
        assert tm["misc"][1] == 1 and tm["split_fits"][1] == 2 and tm["dbscan1d"][1] == 0      # (2: the large-set path ran)
        sgo2, fits2 = ctx.split_fits(T, seg_off)
        assert np.array_equal(sgo, sgo2) and int(sgo[1]) >= 900 and int(sgo[2]) == int(sgo[1]) + 1
        _same_records(fits, fits2, "beyond the grid: on the returned tables")
        # the small segment against the restatements
        m0, z0 = n_bulk, int(supp_off[n_bulk])
        sub = {k: (want[k][z0:] if k.startswith("supp_") else want[k][m0:]) for k in TABLE_FIELDS}
        sub["supp_off"] = want["supp_off"][m0:] - np.uint64(z0)
        off = np.array([0, n_small], np.uint64)
        groups = reference_groups(sub["start"], sub["end"], off)
        ref_fits = reference_fits(oracle, sub, off, groups)
        assert len(ref_fits) == 1 and ref_fits["n_members"][0] == n_small and group_set_sizes(sub, off, groups, 0)[2] > 512 and ref_fits["size"][0, 2] > 200
        _same_records(fits[int(sgo[1]):], ref_fits, "the set beyond LDS")
    finally:
        sh.free()


def test_more_segments_than_the_kernel_holds_in_lds(ctx, oracle):
    """1 100 segments that revisit one shard — most of them empty or of one member, some of two or three overlapping ones: beyond ST_SEG_LDS - 1 =
    1 023 segments the kernel searches seg_off in global memory instead of LDS."""
    rng = np.random.default_rng(9)
    n, n_seg = 200, 1100
    pos = (np.arange(n) // 2) * 10_000 + (np.arange(n) % 2) * 50 + 1000         # records 2i and 2i + 1 overlap each other and nothing else
    flag = np.where(rng.random(n) < 0.4, 0x10, 0).astype(np.uint16)
    reads = Reads.from_cigar_lists(pos, flag, [60] * n, [[(4, int(rng.integers(0, 40))), (M, int(rng.integers(2000, 4000))), (4, int(rng.integers(1, 90)))] for _ in range(n)])
    sh = ctx.upload(reads, int(pos.max()) + 5000)
    try:
        sh.pipeline()
        sizes = rng.choice([0, 0, 1, 1, 1, 2, 3], n_seg)
        sizes[[0, 1023, 1024, n_seg - 1]] = [2, 3, 2, 0]
        seg_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        member_rec = np.concatenate([2 * rng.integers(0, n // 2) + rng.integers(0, 2, k) for k in sizes]).astype(np.uint32)
        counts = rng.integers(0, 4, len(member_rec))
        supp_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
        ns = int(supp_off[-1])
        refs = cs.SplitRefs(member_rec, supp_off, rng.integers(0, n, ns), rng.choice(np.array([0, 0, 0, 2, 3], np.uint8), ns))
        seg = _segments(reads, oracle.aln_intervals(reads), np.array([0, n]))[0]
        want = reference_tables([seg] * n_seg, refs, seg_off)
        T = ctx.split_tables_resident([sh] * n_seg, refs, seg_off)
        assert_same_tables(T, want, "1 100 segments")
        sgo, fits = ctx.split_resident_fits([sh] * n_seg, refs, seg_off, eps=100.0, min_pts=2)
        groups = reference_groups(want["start"], want["end"], seg_off)
        assert np.array_equal(sgo, groups[0]) and int(sgo[-1]) == int((sizes >= 2).sum()) and int(sgo[1025]) - int(sgo[1023]) == 2
        _same_records(fits, reference_fits(oracle, want, seg_off, groups, 100.0, 2), "1 100 segments: restatement")
        _same_records(fits, ctx.split_fits(T, seg_off, eps=100.0, min_pts=2)[1], "1 100 segments: on the returned tables")
    finally:
        sh.free()
