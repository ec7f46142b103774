"""csvgpu_split_groups (Context.split_groups): the overlap groups of the split-read pass computed on the device — member order by a
stable sort, the tree's pre-order from nearest-smaller-rank links, seeds per connected component, one sort for every group's member
order — against the literal restatement of the reference kept in tests/test_split_groups_host.py, and at size against
host.split_groups_host, which that file pins. Every comparison is exact, order included."""
import numpy as np
import pytest

import contextsv_amd as cs
from contextsv_amd import host
from test_split_groups_host import FAMILIES, assert_same, make, mixed_batch, one_segment, reference_groups

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("family", sorted(FAMILIES))
def test_families_match_reference(ctx, family):
    for n in (2, 3, 9, 63, 64, 65, 257, 700):
        for seed in (1, 2):
            s, e, off = one_segment(*make(family, seed, n))
            assert_same(ctx.split_groups(s, e, off), reference_groups(s, e, off))


def test_empty_and_single_member_segments(ctx):
    z = np.zeros(0, dtype=np.int32)
    sgo, go, mem = ctx.split_groups(z, z, np.zeros(1, dtype=np.uint64))
    assert sgo.tolist() == [0] and go.tolist() == [0] and len(mem) == 0
    sgo, go, mem = ctx.split_groups(z, z, np.zeros(4, dtype=np.uint64))
    assert sgo.tolist() == [0, 0, 0, 0] and go.tolist() == [0] and len(mem) == 0
    s, e = np.array([5, 5, 7], dtype=np.int32), np.array([9, 9, 8], dtype=np.int32)
    off = np.array([0, 1, 1, 2, 3], dtype=np.uint64)
    assert_same(ctx.split_groups(s, e, off), reference_groups(s, e, off))
    # empty segments in front of, between and behind segments that have groups
    s, e = np.array([5, 6, 1, 2, 3], dtype=np.int32), np.array([9, 9, 8, 2, 4], dtype=np.int32)
    off = np.array([0, 0, 2, 2, 5, 5], dtype=np.uint64)
    want = reference_groups(s, e, off)
    assert want[0].tolist() == [0, 0, 1, 1, 2, 2]
    assert_same(ctx.split_groups(s, e, off), want)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_24_mixed_segments_in_one_call(ctx, seed):
    s, e, off = mixed_batch(seed)
    assert_same(ctx.split_groups(s, e, off), reference_groups(s, e, off))


def test_group_sizes_1_to_500(ctx):
    """Segment k is one pile of k mutually overlapping members (k = 1 .. 500) in a shuffled order: one group of k members (none for k = 1)."""
    rng = np.random.default_rng(7)
    ss, ee, off = [], [], [0]
    for k in range(1, 501):
        s = rng.integers(0, 1000, k)
        ss.append(s)
        ee.append(rng.integers(1000, 2000, k))
        off.append(off[-1] + k)
    s, e, off = np.concatenate(ss).astype(np.int32), np.concatenate(ee).astype(np.int32), np.asarray(off, dtype=np.uint64)
    got = ctx.split_groups(s, e, off)
    assert np.diff(got[1].astype(np.int64)).tolist() == list(range(2, 501))
    assert_same(got, reference_groups(s, e, off))


@pytest.mark.parametrize("family", ["staircase", "staircase_shuffled"])
def test_600_member_staircase(ctx, family):
    """Ascending staircase: member r overlaps r - 1 and r + 1 only, so every second member is a seed and each depends on the one before
    (about 300 dependent rounds); shuffled ranks break the chain into short ones."""
    s, e, off = one_segment(*make(family, 3, 600))
    want = reference_groups(s, e, off)
    if family == "staircase":
        assert len(want[1]) - 1 == 300
    assert_same(ctx.split_groups(s, e, off), want)


def test_pile_of_5000(ctx):
    rng = np.random.default_rng(11)
    s = rng.integers(0, 50_000, 5000).astype(np.int32)
    e = (60_000 + rng.integers(0, 50_000, 5000)).astype(np.int32)
    s2, e2, off = one_segment(s, e)
    want = reference_groups(s2, e2, off)
    assert want[1].tolist() == [0, 5000]
    assert_same(ctx.split_groups(s2, e2, off), want)


def test_large_components_by_both_seeding_forms(ctx):
    """Components of more than 512 members are seeded out of global memory: by a cursor through the ranks when the component's ranks lie close
    together (here: a segment that is one chain of 3 000 members), by rounds over the whole component when they are scattered (here: a chain
    of 700 members whose ranks are spread over a segment of 20 000)."""
    def one_chain(s, e):                                 # start-sorted: every member starts at or before the furthest end so far
        return bool((s[1:] <= np.maximum.accumulate(e)[:-1]).all())

    rng = np.random.default_rng(31)
    s = np.sort(rng.integers(0, 60_000, 3000))
    e = s + rng.integers(200, 400, 3000)
    assert one_chain(s, e)
    p = rng.permutation(3000)
    s1, e1, off = one_segment(s[p].astype(np.int32), e[p].astype(np.int32))
    want = reference_groups(s1, e1, off)
    assert len(want[1]) > 80
    assert_same(ctx.split_groups(s1, e1, off), want)
    chain_s = np.sort(rng.integers(0, 14_000, 700))
    chain_e = chain_s + rng.integers(200, 400, 700)
    assert one_chain(chain_s, chain_e)
    singles = 1_000_000 + np.arange(19_300) * 1000
    s = np.concatenate([chain_s, singles])
    e = np.concatenate([chain_e, singles + 10])
    p = rng.permutation(len(s))
    s2, e2, off = one_segment(s[p].astype(np.int32), e[p].astype(np.int32))
    want = reference_groups(s2, e2, off)
    assert len(want[1]) > 15
    assert_same(ctx.split_groups(s2, e2, off), want)


def _adversary(k=300, L=40):
    """k short disjoint seeds under L long intervals, the seeds first in rank order: k groups of L + 1 members."""
    s = np.concatenate([np.arange(k) * 100 + 1000, np.zeros(L, dtype=np.int64)]).astype(np.int32)
    e = np.concatenate([np.arange(k) * 100 + 1010, np.full(L, 1_000_000)]).astype(np.int32)
    return one_segment(s, e)


def test_capacity_protocol(ctx):
    s, e, off = _adversary()
    want = reference_groups(s, e, off)
    total = 300 * 41
    assert len(want[2]) == total
    # the raw entry point reports the exact count and writes nothing else
    import ctypes as C
    from contextsv_amd._lib import CSV_ECAPACITY, ptr
    sgo, go, mem = np.zeros(2, np.uint64), np.zeros(len(s) + 1, np.uint64), np.zeros(100, np.uint32)
    n = C.c_uint64(100)
    rc = ctx.lib.csvgpu_split_groups(ctx.h, ptr(s), ptr(e), ptr(off), 1, ptr(sgo), ptr(go), ptr(mem), C.byref(n))
    assert rc == CSV_ECAPACITY and n.value == total and not mem.any()
    # the default capacity (2 n) is too small: the binding retries with the reported count
    assert 2 * len(s) < total
    assert_same(ctx.split_groups(s, e, off), want)
    assert_same(ctx.split_groups(s, e, off, capacity=total), want)
    with pytest.raises(cs.CsvError) as ei:
        ctx.split_groups(s, e, off, capacity=total - 1)
    assert ei.value.status == CSV_ECAPACITY
    assert_same(ctx.split_groups(s, e, off), want)                              # the context is usable afterwards


def test_invalid_input(ctx):
    from contextsv_amd._lib import CSV_EINVAL
    s, e = np.array([5, 9, 3], dtype=np.int32), np.array([6, 8, 4], dtype=np.int32)
    with pytest.raises(cs.CsvError) as ei:
        ctx.split_groups(s, e, np.array([0, 3], dtype=np.uint64))               # end < start
    assert ei.value.status == CSV_EINVAL
    with pytest.raises(cs.CsvError) as ei:
        ctx.split_groups(s, s, np.array([0, 2, 1, 3], dtype=np.uint64))          # offsets not ascending
    assert ei.value.status == CSV_EINVAL
    s2, e2, off = one_segment(*make("random", 1, 50))
    assert_same(ctx.split_groups(s2, e2, off), reference_groups(s2, e2, off))


def hifi_like_segment(rng, n, span):
    """n survivors of one contig drawn like HiFi primaries with a supplementary record: events of 20-80 reads whose ends pile up at a
    breakpoint, and background singles; ends = start + 10-25 kb. Returned in an order like the qname map's: roughly descending start
    (a coordinate-sorted file), shuffled locally."""
    starts = []
    left = n - n // 5                                   # four fifths of the members belong to events
    while left > 0:
        k = int(min(left, rng.integers(20, 81)))
        bp = int(rng.integers(30_000, span - 30_000))
        starts.append(bp - rng.integers(10_000, 25_000, k) + rng.integers(-5, 6, k))
        left -= k
    starts.append(rng.integers(1, span - 30_000, n - sum(len(x) for x in starts)))
    s = np.concatenate(starts).astype(np.int64)
    e = s + rng.integers(10_000, 25_001, len(s))
    order = np.argsort(-s + rng.integers(-40_000, 40_001, len(s)), kind="stable")
    return s[order].astype(np.int32), e[order].astype(np.int32)


def test_at_size_24_segments_of_1e5_members(ctx):
    rng = np.random.default_rng(2024)
    sizes = rng.multinomial(100_000, np.linspace(2.0, 0.3, 24) / np.linspace(2.0, 0.3, 24).sum())
    ss, ee, off = [], [], [0]
    for n in sizes:
        s, e = hifi_like_segment(rng, int(n), 60_000 * int(n) + 1_000_000)
        ss.append(s)
        ee.append(e)
        off.append(off[-1] + len(s))
    s, e, off = np.concatenate(ss), np.concatenate(ee), np.asarray(off, dtype=np.uint64)
    assert len(s) == 100_000 and len(off) == 25
    want = host.split_groups_host(s, e, off)
    assert len(want[1]) > 1000 and np.diff(want[1].astype(np.int64)).max() >= 20
    assert_same(ctx.split_groups(s, e, off), want)


def test_at_size_one_segment_of_2e5_members(ctx):
    rng = np.random.default_rng(2025)
    s, e = hifi_like_segment(rng, 200_000, 240_000_000)
    s, e, off = one_segment(s, e)
    want = host.split_groups_host(s, e, off)
    assert len(want[1]) > 1000
    assert_same(ctx.split_groups(s, e, off), want)


def test_three_launch_radix_passes_give_the_same_groups(ctx):
    s, e, off = mixed_batch(4)
    want = reference_groups(s, e, off)
    ctx.set_tuning(sort_three_launch=True)
    try:
        assert_same(ctx.split_groups(s, e, off), want)
    finally:
        ctx.set_tuning()
