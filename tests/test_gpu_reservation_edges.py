"""Every device workspace is reserved by planning its own carve (contextsv_amd/csrc/arena.hpp, layouts.hpp): no slack term hides an
under-count any more. These are the smallest calls at which an exact reservation can still go wrong — counts around a 256-byte line of
4n, 8n, n and n / 64 * 4 + 4 bytes — through the host-pointer entry points, on contexts made for the test: sizes ascending on one (its
arenas start with no memory and grow call by call), then descending on a second (its arenas are reused, with what the larger call left
in them). Every size runs twice in a row. Results are held to what the other tests hold them to: the reference's own dbscan.cpp /
dbscan1d.cpp (`ref`), the restatements of tests/test_split_groups_host.py, test_split_fits_ref.py and test_split_tables_ref.py, and the
host oracle's Viterbi."""
import numpy as np
import pytest

import contextsv_amd as cs
from contextsv_amd import Reads, make_hmm
from hmm_params import WGS_HMM
from test_split_fits_ref import _build, reference_fits
from test_split_groups_host import reference_groups
from test_split_tables_ref import reference_tables

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65)
DBSCAN1D_MAX_SEG, DBSCAN_IV_SMALL_MAX = 512, 2048        # common.hpp: larger segments / sets leave the LDS kernels


def _both_orders(make_ctx, body):
    for order in (SIZES, SIZES[::-1]):
        c = make_ctx()
        try:
            for n in order:
                for _ in range(2):
                    body(c, n)
        finally:
            c.close()


# ---- DBSCAN ----------------------------------------------------------------------------------------------------------------------------
def _intervals(n, seed):
    rng = np.random.default_rng([seed, n])
    c = rng.choice(rng.integers(1000, 200_000, max(1, n // 7 + 1)), n)
    s = np.maximum(1, c + rng.integers(-8, 9, n)).astype(np.uint32)
    e = (s + rng.choice([0, 1, 50, 300, 2000], n)).astype(np.uint32)
    return s, e


def _points(n, seed):
    rng = np.random.default_rng([seed, n])
    return (rng.choice(rng.integers(0, 10**6, 5), n) + rng.integers(-120, 121, n)).astype(np.int32)


def _offsets(parts):
    return np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)


def dbscan_edges(make_ctx, ref):
    """(tests/golden/make_golden.py runs this body too, to record the reference's answers)"""
    def body(c, n):
        s, e = _intervals(n, 1)
        assert np.array_equal(c.dbscan_iv(s, e, 0.1, 2), ref.dbscan_iv(s, e, 0.1, 2)), n
        # batches: n, nothing, n again; at 65 also with a set beyond the LDS kernel (its windowed path reads a flag back while the batch is staged)
        batches = [[_intervals(n, 2), _intervals(0, 2), _intervals(n, 3)]]
        if n == 65:
            batches.append([_intervals(n, 4), _intervals(DBSCAN_IV_SMALL_MAX + 1, 4)])
        for sets in batches:
            off = _offsets([a for a, _ in sets])
            got = c.dbscan_iv_batch(np.concatenate([a for a, _ in sets]), np.concatenate([b for _, b in sets]), off, 0.1, 2)
            for k, (a, b) in enumerate(sets):
                assert np.array_equal(got[int(off[k]): int(off[k + 1])], ref.dbscan_iv(a, b, 0.1, 2)), (n, k, len(a))
        segs = [[_points(n, 5), _points(0, 5), _points(n, 6)]]
        if n == 65:
            segs.append([_points(n, 7), _points(DBSCAN1D_MAX_SEG + 1, 7)])
        for parts in segs:
            off = _offsets(parts)
            got = c.dbscan_1d(np.concatenate(parts), off, 100.0, 2)
            for k, p in enumerate(parts):
                if len(p):
                    assert np.array_equal(got[int(off[k]): int(off[k + 1])], ref.dbscan_1d(p, 100.0, 2)), (n, k, len(p))

    _both_orders(make_ctx, body)


def test_dbscan_entry_points_at_the_rounding_edges(ref):
    dbscan_edges(lambda: cs.Context(0), ref)


# ---- split groups, groups + fits -----------------------------------------------------------------------------------------------------
_SPLIT = {}


def _split_case(oracle, n):
    """n members in one or two segments of overlapping piles -> (tables, seg_off, groups, fits), once per session"""
    if n not in _SPLIT:
        rng = np.random.default_rng([11, n])
        segments = [[(n, {"supps": (0, 3)})]] if n < 4 else [[(n - n // 3, {"supps": (0, 3)})], [(n // 3, {"supps": (1, 2)})]]
        t, off = _build(rng, segments)
        groups = reference_groups(t["start"], t["end"], off)
        _SPLIT[n] = (t, off, groups, reference_fits(oracle, t, off, groups, 100.0, 2))
    return _SPLIT[n]


def test_split_groups_and_fits_at_the_rounding_edges(oracle):
    def body(c, n):
        t, off, groups, want = _split_case(oracle, n)
        assert (len(want) > 0) == (n > 1)
        got = c.split_groups(t["start"], t["end"], off)
        assert all(np.array_equal(a, b) for a, b in zip(got, groups)), n
        sgo, fused = c.split_fits(cs.SplitTables(**t), off, eps=100.0, min_pts=2)
        assert np.array_equal(sgo, groups[0]) and fused.tobytes() == want.tobytes(), n
        assert c.split_fits(cs.SplitTables(**t), off, groups, eps=100.0, min_pts=2)[1].tobytes() == want.tobytes(), n

    _both_orders(lambda: cs.Context(0), body)


# ---- tables from a resident shard -> groups -> fits ----------------------------------------------------------------------------------
_RESIDENT = {}
N_REC = 200


def _resident_reads():
    rng = np.random.default_rng(9)
    pos = (np.arange(N_REC) // 2) * 10_000 + (np.arange(N_REC) % 2) * 50 + 1000      # records 2i and 2i + 1 overlap each other and nothing else
    flag = np.where(rng.random(N_REC) < 0.4, 0x10, 0).astype(np.uint16)
    cig = [[(4, int(rng.integers(0, 40))), (0, int(rng.integers(2000, 4000))), (4, int(rng.integers(1, 90)))] for _ in range(N_REC)]
    return Reads.from_cigar_lists(pos, flag, [60] * N_REC, cig)


def _resident_case(oracle, reads, n):
    """n members that revisit the shard's records, in two segments -> (refs, seg_off, groups, fits), once per session"""
    if n not in _RESIDENT:
        rng = np.random.default_rng([13, n])
        pair = rng.integers(0, 6, n)                                   # few pairs: groups of several members
        member_rec = (2 * pair + rng.integers(0, 2, n)).astype(np.uint32)
        supp_off = np.concatenate([[0], np.cumsum(rng.integers(0, 4, n))]).astype(np.uint64)
        ns = int(supp_off[-1])
        refs = cs.SplitRefs(member_rec, supp_off, rng.integers(0, N_REC, ns), rng.choice(np.array([0, 0, 0, 2, 3], np.uint8), ns))
        seg_off = np.array([0, n - n // 3, n], np.uint64)
        e, qs, qe = oracle.aln_intervals(reads)
        seg = dict(pos=reads.pos, flag=reads.flag, ref_end=e, q_start=qs, q_end=qe)
        want = reference_tables([seg, seg], refs, seg_off)
        groups = reference_groups(want["start"], want["end"], seg_off)
        _RESIDENT[n] = (refs, seg_off, groups, reference_fits(oracle, want, seg_off, groups, 100.0, 2))
    return _RESIDENT[n]


def test_split_resident_fits_at_the_rounding_edges(oracle):
    reads = _resident_reads()
    for order in (SIZES, SIZES[::-1]):
        c = cs.Context(0)
        sh = None
        try:
            sh = c.upload(reads, int(reads.pos.max()) + 5000)
            sh.pipeline()
            for n in order:
                refs, seg_off, groups, want = _resident_case(oracle, reads, n)
                assert (len(want) > 0) == (n > 1)
                for _ in range(2):
                    sgo, fits = c.split_resident_fits([sh, sh], refs, seg_off, eps=100.0, min_pts=2)
                    assert np.array_equal(sgo, groups[0]) and fits.tobytes() == want.tobytes(), n
        finally:
            if sh is not None:
                sh.free()
            c.close()


# ---- Viterbi -------------------------------------------------------------------------------------------------------------------------
def test_viterbi_at_one_and_43_observations(oracle):
    from test_gpu_parity import _obs
    hmm = make_hmm(**WGS_HMM)
    rng = np.random.default_rng(5)
    calls = {}
    for n_obs, off in ((1, [0, 1]), (43, [0, 20, 20, 43])):
        o1, o2, pfb = _obs(rng, n_obs, "del")
        off = np.asarray(off, np.uint64)
        calls[n_obs] = (o1, o2, pfb, off) + tuple(oracle.viterbi(hmm, o1, o2, pfb, off))
    for order in ((1, 43), (43, 1)):
        c = cs.Context(0)
        try:
            for n_obs in order:
                o1, o2, pfb, off, ost, oll = calls[n_obs]
                for _ in range(2):
                    st, ll = c.viterbi(hmm, o1, o2, pfb, off)
                    assert np.array_equal(st, ost), n_obs                        # identical paths
                    np.testing.assert_allclose(ll, oll, rtol=0, atol=1e-6)       # the tolerance of tests/test_gpu_parity.py
        finally:
            c.close()
