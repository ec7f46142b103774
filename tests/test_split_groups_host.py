"""host.split_groups_host (the host tree of host/split_caller.cpp behind csvhost_split_groups_host) against a literal restatement of
the reference's overlap grouping: node-by-node insertion into the unbalanced interval tree (sv_caller.cpp:964-980), findOverlaps with
its left-subtree pruning (:948-962) and the greedy seeding loop with the `processed` set (:215-238). No GPU is needed.

The restatement (`reference_groups`) and the input families (`FAMILIES`, `mixed_batch`) are also what tests/test_gpu_split_groups.py
checks the device form against."""
import numpy as np
import pytest

I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


# ---- the reference's behaviour, one node and one call at a time ---------------------------------------------------------------------
def _segment_groups(start, end):
    """Groups (lists of member indices, more than one member each) of ONE segment whose members are given in map iteration order."""
    n = len(start)
    left, right, max_end = [-1] * n, [-1] * n, [int(e) for e in end]
    root = -1
    for m in range(n):                                   # insert(root, region, qname), iteration order
        if root < 0:
            root = m
            continue
        x = root
        while True:                                      # (the recursion, unrolled: a spine of 1e5 nodes is the normal shape)
            if max_end[x] < end[m]:
                max_end[x] = int(end[m])                 # `root->max_end = max(root->max_end, region.end)` on the way back up
            if start[m] < start[x]:
                if left[x] < 0:
                    left[x] = m
                    break
                x = left[x]
            else:
                if right[x] < 0:
                    right[x] = m
                    break
                x = right[x]
    groups, processed = [], set()
    for m in range(n):
        if m in processed:
            continue
        qs, qe = start[m], end[m]
        found, stack = [], [root]
        while stack:                                     # findOverlaps: node, left if it may overlap, always right
            x = stack.pop()
            if x < 0:
                continue
            if qs <= end[x] and qe >= start[x]:
                found.append(x)
            stack.append(right[x])
            if left[x] >= 0 and max_end[left[x]] >= qs:
                stack.append(left[x])
        processed.update(found)
        if len(found) > 1:
            groups.append(found)
    return groups


def reference_groups(start, end, seg_off):
    start = [int(x) for x in start]
    end = [int(x) for x in end]
    seg_group_off, group_off, members = [0], [0], []
    for c in range(len(seg_off) - 1):
        a, b = int(seg_off[c]), int(seg_off[c + 1])
        for g in _segment_groups(start[a:b], end[a:b]):
            members.extend(g)
            group_off.append(len(members))
        seg_group_off.append(len(group_off) - 1)
    return (np.asarray(seg_group_off, dtype=np.uint64), np.asarray(group_off, dtype=np.uint64), np.asarray(members, dtype=np.uint32))


def assert_same(got, want):
    sgo, go, mem = got
    wsgo, wgo, wmem = want
    assert np.array_equal(np.asarray(sgo, dtype=np.uint64), wsgo)
    assert np.array_equal(np.asarray(go, dtype=np.uint64), wgo)
    assert np.array_equal(np.asarray(mem, dtype=np.uint32), wmem)


# ---- input families: name -> f(rng, n) -> (start, end), int32, start <= end ------------------------------------------------------------
def _random(rng, n):
    s = rng.integers(0, max(4 * n, 8), n)
    return s, s + rng.integers(0, 12, n)


def _equal_starts(rng, n):
    s = rng.integers(0, max(n // 8, 2), n) * 50
    return s, s + rng.integers(0, 120, n)


def _identical(rng, n):
    s = rng.integers(0, max(n // 6, 2), n) * 10
    return s, s + 15


def _nested(rng, n):
    k = rng.permutation(n)
    return 1000 + k, 1000 + 2 * n + 5 - k


def _descending(rng, n):
    s = np.sort(rng.integers(0, 6 * n + 8, n))[::-1]
    return s, s + rng.integers(0, 30, n)


def _staircase(rng, n):
    s = np.arange(n) * 10
    return s, s + 12


def _staircase_shuffled(rng, n):
    s, e = _staircase(rng, n)
    p = rng.permutation(n)
    return s[p], e[p]


def _points(rng, n):
    s = rng.integers(0, max(n // 2, 2), n)
    return s, s.copy()


def _extremes(rng, n):
    pool = np.array([I32_MIN, I32_MIN + 1, -1, 0, 1, I32_MAX - 1, I32_MAX], dtype=np.int64)
    a, b = pool[rng.integers(0, len(pool), n)], pool[rng.integers(0, len(pool), n)]
    return np.minimum(a, b), np.maximum(a, b)


FAMILIES = {"random": _random, "equal_starts": _equal_starts, "identical": _identical, "nested": _nested, "descending": _descending,
            "staircase": _staircase, "staircase_shuffled": _staircase_shuffled, "points": _points, "extremes": _extremes}


def make(family, seed, n):
    s, e = FAMILIES[family](np.random.default_rng(seed), n)
    return np.ascontiguousarray(s, dtype=np.int32), np.ascontiguousarray(e, dtype=np.int32)


def mixed_batch(seed, sizes=(0, 1, 2, 3, 5, 0, 17, 64, 65, 1, 128, 200, 33, 0, 7, 300, 2, 90, 1, 63, 450, 11, 0, 129)):
    """24 segments of mixed sizes and families in one call (empty and one-member segments among them)."""
    names = sorted(FAMILIES)
    ss, ee, off = [], [], [0]
    for k, n in enumerate(sizes):
        s, e = make(names[(k + seed) % len(names)], seed * 100 + k, n)
        ss.append(s)
        ee.append(e)
        off.append(off[-1] + n)
    return np.concatenate(ss).astype(np.int32), np.concatenate(ee).astype(np.int32), np.asarray(off, dtype=np.uint64)


def one_segment(s, e):
    return s, e, np.asarray([0, len(s)], dtype=np.uint64)


# ---- the tests ------------------------------------------------------------------------------------------------------------------------
def test_restatement_on_a_hand_example():
    # iteration order: [10,20] [5,12] [30,40] [11,31] [50,60]; tree: 0 root, 1 left of 0, 2 right of 0, 3 left of 2, 4 right of 2
    s, e, off = one_segment(np.array([10, 5, 30, 11, 50], dtype=np.int32), np.array([20, 12, 40, 31, 60], dtype=np.int32))
    sgo, go, mem = reference_groups(s, e, off)
    # seed 0 overlaps 0, 1, 3 (pre-order: 0, 1, then the right subtree 2 -> 3); seed 2 overlaps 2, 3; seed 4 is alone (dropped)
    assert mem.tolist() == [0, 1, 3, 2, 3] and go.tolist() == [0, 3, 5] and sgo.tolist() == [0, 2]


@pytest.mark.parametrize("family", sorted(FAMILIES))
@pytest.mark.parametrize("n", [2, 3, 9, 64, 257, 700])
def test_host_groups_match_reference(family, n):
    from contextsv_amd import host
    for seed in (1, 2):
        s, e, off = one_segment(*make(family, seed, n))
        assert_same(host.split_groups_host(s, e, off), reference_groups(s, e, off))


def test_empty_and_single_member_segments():
    from contextsv_amd import host
    z = np.zeros(0, dtype=np.int32)
    sgo, go, mem = host.split_groups_host(z, z, np.zeros(1, dtype=np.uint64))                       # n_seg == 0
    assert sgo.tolist() == [0] and go.tolist() == [0] and len(mem) == 0
    sgo, go, mem = host.split_groups_host(z, z, np.zeros(4, dtype=np.uint64))                       # three empty segments
    assert sgo.tolist() == [0, 0, 0, 0] and go.tolist() == [0] and len(mem) == 0
    s, e = np.array([5, 5, 7], dtype=np.int32), np.array([9, 9, 8], dtype=np.int32)
    off = np.array([0, 1, 1, 2, 3], dtype=np.uint64)                                                # one member each: no group has two
    assert_same(host.split_groups_host(s, e, off), reference_groups(s, e, off))
    assert host.split_groups_host(s, e, off)[0].tolist() == [0, 0, 0, 0, 0]


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_24_mixed_segments_in_one_call(seed):
    from contextsv_amd import host
    s, e, off = mixed_batch(seed)
    assert len(off) == 25
    want = reference_groups(s, e, off)
    assert want[1][-1] > 0
    assert_same(host.split_groups_host(s, e, off), want)


def test_invalid_input_is_refused():
    from contextsv_amd import host
    s, e = np.array([5, 9], dtype=np.int32), np.array([6, 8], dtype=np.int32)
    with pytest.raises(ValueError):
        host.split_groups_host(s, e, np.array([0, 2], dtype=np.uint64))                             # end < start
    with pytest.raises(ValueError):
        host.split_groups_host(s, s, np.array([0, 2, 1], dtype=np.uint64))                          # offsets not ascending
