"""mergeSVs' representatives chosen on the device (csvgpu_sort_slot, csvgpu_merge_select, csvgpu_chr_merge_select; kernels/mergeselect.hip).
Every expectation comes from the host: host.sort_select_check returns std::sort's own slot, host.sort_select_rounds the partitions the
library's chain takes (it predicts the declines), host.merge_type_with_labels the host's representative rule — never from the device."""
import ctypes as C

import numpy as np
import pytest

import merge_select_inputs as mi
import synth_small as ss
from contextsv_amd import CsvError, _lib, host
from contextsv_amd._lib import ptr

pytestmark = pytest.mark.gpu
CAP = _lib.SORT_SLOT_LDS_CAP
NONE = _lib.SORT_SLOT_NONE


def _check_one_keys_many_slots(ctx, keys, slot_list, tag, max_partitions=0):
    """one segment per slot, all with the same keys, in one call"""
    n, k = len(keys), len(slot_list)
    off = (np.arange(k + 1, dtype=np.uint64) * n)
    idx, declined = ctx.sort_slot(np.tile(keys, k), off, np.asarray(slot_list, np.uint64), max_partitions)
    for j, p in enumerate(slot_list):
        want, rounds = mi.expected_slot(keys, p)
        must_decline = want is None or (max_partitions and rounds > max_partitions)
        assert bool(declined[j]) == bool(must_decline), (tag, n, p, rounds)
        assert int(idx[j]) == (NONE if must_decline else want), (tag, n, p, rounds)


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 18, 33, 100])
def test_sort_slot_every_slot_of_small_segments(ctx, n):
    rng = np.random.default_rng(n)
    for name in mi.PATTERNS:
        _check_one_keys_many_slots(ctx, mi.pattern(name, rng, n), list(range(n)), name)


@pytest.mark.parametrize("name", mi.PATTERNS)
@pytest.mark.parametrize("n", [1000, 4097, CAP - 1, CAP, CAP + 1, 2 * CAP + 3, 200_003])
def test_sort_slot_sampled_slots_of_large_segments(ctx, n, name):
    """the LDS form up to CAP members, the streaming form above it (which drops into LDS once the kept range fits)"""
    rng = np.random.default_rng(n + 7)
    _check_one_keys_many_slots(ctx, mi.pattern(name, rng, n), mi.slots(rng, n), name)


def test_sort_slot_batch_beyond_the_grid_caps(ctx):
    """70 000 segments of 2 .. 20 members: more than any 65 535 cap, both the lane-group and the workgroup form in one call"""
    rng = np.random.default_rng(70)
    sizes = rng.integers(2, 21, 70_000)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    keys = rng.integers(0, 6, int(off[-1])).astype(np.uint32)
    nth = (rng.integers(0, 1 << 30, len(sizes)) % sizes).astype(np.uint64)
    idx, declined = ctx.sort_slot(keys, off, nth)
    assert not declined.any()
    for s in range(len(sizes)):
        assert int(idx[s]) == host.sort_select_check(keys[int(off[s]):int(off[s + 1])], int(nth[s]))[0], (s, int(sizes[s]))


def test_sort_slot_empty_segments_and_empty_batch(ctx):
    idx, declined = ctx.sort_slot(np.zeros(0, np.uint32), np.zeros(1, np.uint64), np.zeros(0, np.uint64))
    assert len(idx) == 0 and len(declined) == 0
    keys = np.array([5, 5, 9, 1, 1, 1], np.uint32)
    off = np.array([0, 0, 2, 2, 2, 6, 6], np.uint64)                # empty, [5 5], empty, empty, [9 1 1 1], empty
    idx, declined = ctx.sort_slot(keys, off, np.array([0, 1, 7, 0, 2, 0], np.uint64))
    assert idx.tolist() == [NONE, 1, NONE, NONE, 2, NONE] and not declined.any()
    idx, declined = ctx.sort_slot(np.zeros(0, np.uint32), np.zeros(4, np.uint64), np.zeros(3, np.uint64))       # nothing but empty segments
    assert idx.tolist() == [NONE] * 3 and not declined.any()
    with pytest.raises(CsvError) as ei:                            # a slot beyond its segment
        ctx.sort_slot(keys, np.array([0, 2, 6], np.uint64), np.array([2, 0], np.uint64))
    assert ei.value.status == _lib.CSV_EINVAL


@pytest.mark.parametrize("max_partitions", [1, 2, 3])
def test_sort_slot_declines_exactly_the_chains_beyond_the_bound(ctx, max_partitions):
    rng = np.random.default_rng(40 + max_partitions)
    sizes = np.concatenate([rng.integers(17, 200, 40), rng.integers(200, 5001, 20), [17, 5000, CAP, CAP + 1], rng.integers(1, 17, 12)])
    parts, nth = [], []
    for k, n in enumerate(sizes):
        parts.append(mi.pattern(mi.PATTERNS[k % len(mi.PATTERNS)], rng, int(n)))
        nth.append(int(rng.integers(0, n)))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    idx, declined = ctx.sort_slot(np.concatenate(parts), off, np.asarray(nth, np.uint64), max_partitions)
    n_declined = 0
    for s, keys in enumerate(parts):
        want, rounds = mi.expected_slot(keys, nth[s])
        must = want is None or rounds > max_partitions
        assert bool(declined[s]) == must, (s, len(keys), rounds)
        assert int(idx[s]) == (NONE if must else want), (s, len(keys), rounds)
        assert not (len(keys) <= 16 and declined[s])
        n_declined += must
    assert 0 < n_declined < len(parts)                               # both sides of the bound ran


# ------------------------------------------------------------------------------------------------ merge_select against the host rule

def _cluster_sigs(rng, sizes_by_label, n_noise=0, lens=(100, 100, 100, 101, 250)):
    """signatures with the given bucket sizes (label -> members), shuffled; lengths tie heavily"""
    labels = np.concatenate([np.full(sz, lab) for lab, sz in sizes_by_label.items()] + [np.full(n_noise, -2)]).astype(np.int32)
    rng.shuffle(labels)
    n = len(labels)
    start = np.sort(rng.integers(1, 2_000_000, n)).astype(np.uint32)
    return mi.make_sigs(start, start + rng.choice(lens, n).astype(np.uint32), rng), labels


def _merge_case(ctx, sig_del, lab_del, sig_ins, lab_ins, max_partitions=0):
    sig, labels = np.concatenate([sig_del, sig_ins]), np.concatenate([lab_del, lab_ins]).astype(np.int32)
    got, counts = ctx.merge_select(sig, labels, len(sig_del), max_partitions)
    want = mi.expected_records(sig, labels, len(sig_del))
    mi.same_records(got, want)
    n_del_rep = len(sig_del) if len(sig_del) < 2 else len(mi.expected_records(sig_del, lab_del, len(sig_del)))
    assert counts["n_rep"] == (n_del_rep, len(want) - n_del_rep) and counts["n_declined"] == (0, 0)
    return got


def test_merge_select_bucket_shapes(ctx):
    rng = np.random.default_rng(11)
    none = (mi.make_sigs([], []), np.zeros(0, np.int32))
    noise = _cluster_sigs(rng, {}, n_noise=300)                                        # all noise: one record, the -2 bucket's
    one = _cluster_sigs(rng, {0: 57})                                                  # one cluster
    mixed = _cluster_sigs(rng, {0: 9, 1: 10, 2: 11, 3: 16, 4: 17, 5: 1, 6: 1, 7: 2, 9: 40}, n_noise=25)       # top goes 1 -> 2 at 10; singletons are dropped; label 8 absent
    got = _merge_case(ctx, *noise, *one)
    assert got["label"].tolist() == [-2, 0] and got["cluster_size"].tolist() == [300, 57]
    got = _merge_case(ctx, *mixed, *noise)
    assert got["label"].tolist() == [-2, 0, 1, 2, 3, 4, 7, 9, -2]
    _merge_case(ctx, *one, *mixed)
    # a type with no and with one signature passes through (status 1, size 0), the other type is merged
    single = (mi.make_sigs([77], [177], rng), np.zeros(1, np.int32))
    for a, b in ((none, mixed), (mixed, none), (single, mixed), (mixed, single), (single, single), (none, single), (single, none), (none, none)):
        got = _merge_case(ctx, *a, *b)
        for side, first in ((a, True), (b, False)):
            if len(side[0]) == 1:
                r = got[0] if first else got[-1]
                assert (r["status"], r["cluster_size"], r["start"], r["end"]) == (1, 0, 77, 177)


def test_merge_select_tie_heavy_set(ctx):
    """the set of tests/test_merge_host.py::test_many_length_ties_follow_std_sort, labels from the device's own DBSCAN"""
    rng = np.random.default_rng(5)
    n = 5000
    s = np.sort(rng.integers(1, 2_000_000, n)).astype(np.uint32)
    e = (s + rng.choice([100, 100, 100, 101, 250], n)).astype(np.uint32)
    labels = ctx.dbscan_iv(s, e, 0.1, 3)
    assert (labels == -2).sum() > CAP and labels.max() >= 0          # the noise bucket streams, the set's few clusters beside it (5000 intervals over 2e6 positions: sparse)
    sig = mi.make_sigs(s, e, rng)
    _merge_case(ctx, sig[:0], labels[:0], sig, labels)
    _merge_case(ctx, sig, labels, sig[:0], labels[:0])


def test_merge_select_random_labels(ctx):
    rng = np.random.default_rng(12)
    for n_clusters in (3, 400):
        n = 3000
        start = np.sort(rng.integers(1, 500_000, n)).astype(np.uint32)
        sig = mi.make_sigs(start, start + rng.integers(50, 60, n).astype(np.uint32), rng)
        labels = rng.integers(-2, n_clusters, n).astype(np.int32)
        _merge_case(ctx, sig[:1200], labels[:1200], sig[1200:], labels[1200:])


def test_merge_select_declines_and_counts_them(ctx):
    rng = np.random.default_rng(13)
    sig, labels = _cluster_sigs(rng, {0: 12, 1: 300, 2: 900, 3: 16}, n_noise=5000)
    got, counts = ctx.merge_select(sig, labels, 0, max_partitions=1)
    want = mi.expected_records(sig, labels, 0)
    assert len(got) == len(want) == 5 and counts["n_rep"] == (0, 5)
    n_declined = 0
    for g, w in zip(got, want):
        lens = (sig["end"] - sig["start"])[labels == w["label"]]
        rounds = host.sort_select_rounds(lens, max(1, int(len(lens) * 0.2)) // 2)
        assert (g["label"], g["cluster_size"]) == (w["label"], w["cluster_size"])
        if rounds > 1 or rounds < 0:
            assert g["status"] == 2
            n_declined += 1
        else:
            assert g.tolist() == w.tolist()
    assert counts["n_declined"] == (0, n_declined) and n_declined >= 2


def test_merge_select_capacity_and_null_outputs(ctx):
    rng = np.random.default_rng(14)
    sig, labels = _cluster_sigs(rng, {k: 5 + k for k in range(20)}, n_noise=100)
    want = mi.expected_records(sig, labels, 8)
    with pytest.raises(CsvError) as ei:
        ctx.merge_select(sig, labels, 8, capacity=len(want) - 1)
    assert ei.value.status == _lib.CSV_ECAPACITY
    n_del_rep = len(mi.expected_records(sig[:8], labels[:8], 8))
    assert ei.value.counts["n_rep"] == (n_del_rep, len(want) - n_del_rep)
    got, _ = ctx.merge_select(sig, labels, 8, capacity=len(want))
    mi.same_records(got, want)
    cnt = _lib.csv_merge_counts()
    rep = np.zeros(64, _lib.MERGE_REP_DTYPE)
    lib = ctx.lib
    assert lib.csvgpu_merge_select(ctx.h, ptr(sig), ptr(labels), 8, len(sig) - 8, 0, None, 64, C.byref(cnt)) == _lib.CSV_EINVAL
    assert lib.csvgpu_merge_select(ctx.h, ptr(sig), ptr(labels), 8, len(sig) - 8, 0, ptr(rep), 64, None) == _lib.CSV_EINVAL
    assert lib.csvgpu_merge_select(ctx.h, None, ptr(labels), 8, len(sig) - 8, 0, ptr(rep), 64, C.byref(cnt)) == _lib.CSV_EINVAL
    assert lib.csvgpu_merge_select(ctx.h, ptr(sig), None, 8, len(sig) - 8, 0, ptr(rep), 64, C.byref(cnt)) == _lib.CSV_EINVAL
    bad = labels.copy(); bad[20] = -3
    assert lib.csvgpu_merge_select(ctx.h, ptr(sig), ptr(bad), 8, len(sig) - 8, 0, ptr(rep), 64, C.byref(cnt)) == _lib.CSV_EINVAL
    got, _ = ctx.merge_select(sig, labels, 8)                        # the context is usable afterwards
    mi.same_records(got, want)


# ------------------------------------------------------------------------------------------------ behind a shard's pipeline

SHARDS = {
    "ont_like": dict(seed=301, n_reads=400, mean_ops=60, big_frac=0.08),
    "hifi_like": dict(seed=302, n_reads=700, mean_ops=12, big_frac=0.03, all_ops=False),
    "clip_end": dict(seed=303, n_reads=200, clip_end=True),
    "no_signatures": dict(seed=304, n_reads=50, mean_ops=3, big_frac=0.0, all_ops=False),
}


@pytest.mark.parametrize("kind", sorted(SHARDS))
def test_chain_select_equals_fetch_and_host_merge(ctx, kind):
    """Shard.pipeline() + Shard.merge_select == fetch + the host rule; with the select not called, a pipeline launches nothing of it."""
    reads, depth_len = ss.random_shard(**SHARDS[kind])
    if kind == "no_signatures":
        reads.cigar[:] = (reads.cigar & 0xF) | (np.minimum(reads.cigar >> 4, 30) << 4)       # no op reaches the 50 of a signature
    sh = ctx.upload(reads, depth_len)
    try:
        ctx.timing_enable(1)
        ctx.timing_reset()
        res = sh.pipeline()
        assert ctx.timing()["misc"][1] == 0                           # off is untouched: no launch of this feature in a pipeline
        got, counts = sh.merge_select(res)
        assert ctx.timing()["misc"][1] == (1 if res.n_sig else 0)
        ctx.timing_enable(0)
        f = sh.fetch(res)
        sig, labels = np.concatenate([f["sig_del"], f["sig_ins"]]), np.concatenate([f["label_del"], f["label_ins"]]).astype(np.int32)
        assert (res.n_sig == 0) == (kind == "no_signatures")
        want = mi.expected_records(sig, labels, res.n_del)
        mi.same_records(got, want)
        assert sum(counts["n_rep"]) == len(want) and counts["n_declined"] == (0, 0)
        # one record too few: CSV_ECAPACITY with the counts, the results still on the shard for the second call
        if len(want):
            with pytest.raises(CsvError) as ei:
                sh.merge_select(res, capacity=len(want) - 1)
            assert ei.value.status == _lib.CSV_ECAPACITY and ei.value.counts == counts
            again, _ = sh.merge_select(res, capacity=len(want))
            mi.same_records(again, want)
        # the pipeline's own results are untouched by the select
        f2 = sh.fetch(res)
        assert all(np.array_equal(f[k], f2[k]) for k in ("sig_del", "sig_ins", "label_del", "label_ins"))
    finally:
        ctx.timing_enable(0)
        sh.free()
