"""What the reference derives from an overlap group of split reads before it makes calls (sv_caller.cpp:248-416): the strand vote, the six
point sets, six DBSCAN1D(100, 5) fits, getLargestCluster and the medians — restated literally (`reference_fits`) on the tables of
include/csvgpu.h (csv_split_tables), with the clustering itself taken from oracle.dbscan_1d / oracle.largest_cluster, which
tests/test_oracle_golden.py pins to the reference. No GPU is needed here.

The restatement, checked below on hand-derived cases, and the input families (`FAMILIES`, `family`) are what
tests/test_gpu_split_fits.py checks csvgpu_split_fits and csvgpu_split_groups_fits against, record for record."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_split_groups_host import reference_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS, MIN_PTS = 100.0, 5
FIT_DTYPE = np.dtype([("median", "<i4", (6,)), ("size", "<u4", (6,)), ("n_members", "<u4"), ("n_opposite", "<u4"), ("reserved", "<u4", (2,))])
TABLE_FIELDS = ("start", "end", "q_start", "q_end", "reverse", "supp_off", "supp_start", "supp_end", "supp_q_start", "supp_q_end", "supp_flags")


# ---- the reference's behaviour, one group at a time ------------------------------------------------------------------------------------
def group_sets(t, base, members):
    """The six point sets of one group (members: indices within the segment that starts at member `base`, findOverlaps order) and the
    number of members with a same-tid supplementary record on the other strand."""
    sets = [[] for _ in range(6)]
    n_opposite = 0
    for q in members:                                             # :251-264
        m = base + int(q)
        has_opposite = False
        for z in range(int(t["supp_off"][m]), int(t["supp_off"][m + 1])):
            f = int(t["supp_flags"][z])
            if not (f & 2) and (f & 1) != int(t["reverse"][m]):
                has_opposite = True
        n_opposite += has_opposite
    for q in members:                                             # :275-280
        m = base + int(q)
        sets[0].append(int(t["start"][m]))
        sets[1].append(int(t["end"][m]))
    for q in members:                                             # :302-356
        m = base + int(q)
        p_start, p_end, p_qs, p_qe = (int(t[k][m]) for k in ("start", "end", "q_start", "q_end"))
        for z in range(int(t["supp_off"][m]), int(t["supp_off"][m + 1])):
            f = int(t["supp_flags"][z])
            if f & 2:                                             # another chromosome
                continue
            s_start, s_end, s_qs, s_qe = (int(t[k][z]) for k in ("supp_start", "supp_end", "supp_q_start", "supp_q_end"))
            sets[2].append(s_start)
            sets[3].append(s_end)
            if (f & 1) != int(t["reverse"][m]):
                continue
            primary_5p = p_start < s_start
            read_distance = max(0, max(s_qs, p_qs) - min(s_qe, p_qe))
            ref_distance = max(0, max(s_start, p_start) - min(s_end, p_end))
            if not primary_5p:
                read_distance = -read_distance
            sets[4].append(read_distance)
            sets[5].append(ref_distance)
    return sets, n_opposite


def largest_sorted(oracle, pts, eps=EPS, min_pts=MIN_PTS, ref=None):
    """fit + getLargestCluster + std::sort of one set -> the sorted largest cluster (may be empty)."""
    if not pts:
        return []
    labels = oracle.dbscan_1d(pts, eps, min_pts)
    cl = oracle.largest_cluster(pts, labels).tolist()
    if ref is not None:
        assert ref.largest(pts, eps, min_pts).tolist() == cl
    return sorted(cl)


def reference_fits(oracle, t, seg_off, groups, eps=EPS, min_pts=MIN_PTS, ref=None):
    seg_group_off, group_off, members = groups
    out = np.zeros(int(seg_group_off[-1]), FIT_DTYPE)
    for c in range(len(seg_off) - 1):
        for g in range(int(seg_group_off[c]), int(seg_group_off[c + 1])):
            mem = members[int(group_off[g]):int(group_off[g + 1])]
            sets, n_opposite = group_sets(t, int(seg_off[c]), mem)
            for s in range(6):
                cl = largest_sorted(oracle, sets[s], eps, min_pts, ref)
                out["size"][g, s] = len(cl)
                out["median"][g, s] = cl[len(cl) // 2] if cl else 0
            out["n_members"][g] = len(mem)
            out["n_opposite"][g] = n_opposite
    return out


def is_inversion(fit):
    return float(fit["n_opposite"]) / float(fit["n_members"]) > 0.5        # :265


# ---- tables from explicit members ------------------------------------------------------------------------------------------------------
def tables_of(members):
    """members: list of (start, end, q_start, q_end, reverse, [(start, end, q_start, q_end, flags), ...]) -> dict of the table arrays."""
    t = {k: [] for k in TABLE_FIELDS}
    t["supp_off"].append(0)
    for (s, e, qs, qe, rev, supps) in members:
        t["start"].append(s); t["end"].append(e); t["q_start"].append(qs); t["q_end"].append(qe); t["reverse"].append(rev)
        for (ss, se, sqs, sqe, f) in supps:
            t["supp_start"].append(ss); t["supp_end"].append(se); t["supp_q_start"].append(sqs); t["supp_q_end"].append(sqe); t["supp_flags"].append(f)
        t["supp_off"].append(len(t["supp_start"]))
    dt = {"reverse": np.uint8, "supp_flags": np.uint8, "supp_off": np.uint64}
    return {k: np.asarray(v, dtype=dt.get(k, np.int32)) for k, v in t.items()}


def one_group(members):
    """All members in one segment and one group, in the order given."""
    n = len(members)
    return (tables_of(members), np.array([0, n], np.uint64),
            (np.array([0, 1], np.uint64), np.array([0, n], np.uint64), np.arange(n, dtype=np.uint32)))


def _fit_of(oracle, members):
    t, off, groups = one_group(members)
    return reference_fits(oracle, t, off, groups)[0]


def _plain(start, end=None, supps=()):
    return (start, start + 5000 if end is None else end, 0, 4000, 0, list(supps))


# ---- hand-derived cases ----------------------------------------------------------------------------------------------------------------
def test_two_clusters_of_equal_size_the_lower_id_wins(oracle):
    # cluster ids follow the first visit: the five starts near 1000 come first, so they are cluster 0, and 5 > 5 is false for cluster 1
    f = _fit_of(oracle, [_plain(s) for s in (1000, 1001, 1002, 1003, 1004, 0, 1, 2, 3, 4)])
    assert f["size"][0] == 5 and f["median"][0] == 1002
    f = _fit_of(oracle, [_plain(s) for s in (0, 1, 2, 3, 4, 1000, 1001, 1002, 1003, 1004)])
    assert f["size"][0] == 5 and f["median"][0] == 2
    assert f["n_members"] == 10 and f["n_opposite"] == 0 and not f["reserved"].any()


def test_border_points_count_in_the_size(oracle):
    # only 100 has five points within 100 (itself included): one core point, four border points, one cluster of five
    f = _fit_of(oracle, [_plain(s, 9000) for s in (0, 50, 100, 150, 200)])
    assert f["size"][0] == 5 and f["median"][0] == 100
    assert f["size"][1] == 5 and f["median"][1] == 9000


def test_even_sized_cluster_takes_the_upper_middle(oracle):
    f = _fit_of(oracle, [_plain(s) for s in (60, 10, 50, 20, 40, 30)])
    assert f["size"][0] == 6 and f["median"][0] == 40


def test_all_noise_set_has_no_cluster(oracle):
    f = _fit_of(oracle, [_plain(s, 9000) for s in (0, 1000, 2000, 3000, 4000)])
    assert f["size"][0] == 0 and f["median"][0] == 0
    assert f["size"][1] == 5 and f["median"][1] == 9000


def test_opposite_strands_leave_the_distance_sets_empty(oracle):
    mem = [(100 + i, 5000, 0, 4000, 0, [(20000 + i, 23000, 4100, 7000, 1)]) for i in range(6)]
    f = _fit_of(oracle, mem)
    assert f["size"].tolist() == [6, 6, 6, 6, 0, 0] and f["median"].tolist() == [103, 5000, 20003, 23000, 0, 0]
    assert f["n_opposite"] == 6 and is_inversion(f)


def test_translocated_record_counts_nowhere(oracle):
    # every member: one record on another tid (flags bit 1; its opposite strand bit must not vote) and, for five of six, one on the same tid
    mem = [(100 + i, 5000, 0, 4000, 0, [(7, 0, 0, 0, 3)] + ([(20000 + i, 23000, 4100, 7000, 0)] if i else [])) for i in range(6)]
    f = _fit_of(oracle, mem)
    assert f["size"].tolist() == [6, 6, 5, 5, 5, 5] and f["n_opposite"] == 0
    assert f["median"][2] == 20003 and f["median"][4] == 100 and f["median"][5] == 15003      # 4100 - 4000; 20003 - 5000


def test_negative_read_distances(oracle):
    # the supplementary record lies in front of the primary on the reference: the read distance is negated, the reference distance is not
    mem = [(20000 + i, 25000, 0, 4000, 1, [(1000, 3000 + i, 4250, 7000, 1)]) for i in range(5)]
    f = _fit_of(oracle, mem)
    assert f["size"][4] == 5 and f["median"][4] == -250
    assert f["size"][5] == 5 and f["median"][5] == 20002 - 3002       # start - supplementary end, third of five
    assert f["n_opposite"] == 0


def test_vote_at_exactly_one_half_is_not_an_inversion(oracle):
    mem = [(100 + i, 5000, 0, 4000, 0, [(20000, 23000, 4100, 7000, 1 if i < 3 else 0)]) for i in range(6)]
    f = _fit_of(oracle, mem)
    assert f["n_opposite"] == 3 and f["n_members"] == 6 and not is_inversion(f)
    mem.append((106, 5000, 0, 4000, 0, [(20000, 23000, 4100, 7000, 1)]))
    assert is_inversion(_fit_of(oracle, mem))


# ---- input families --------------------------------------------------------------------------------------------------------------------
# A segment is a list of piles; a pile is k mutually overlapping members (one overlap group) around its own base. Options of a pile:
#   supps     how many supplementary records a member has: an int, or (lo, hi) drawn per member
#   other     probability that a record lies on another tid
#   opposite  probability that a same-tid record lies on the other strand
#   behind    probability that a same-tid record lies in front of the primary (negative read distance)
#   tight     probability that a coordinate belongs to the pile's cluster (the rest is scattered by thousands)
#   dup       coordinates drawn from this many distinct values (0: free)
def _pile(rng, base, k, supps=1, other=0.05, opposite=0.1, behind=0.2, tight=0.85, dup=0):
    def near(centre, n=None):
        j = rng.integers(-40, 41, n) if not dup else rng.integers(0, dup, n) * 7
        far = rng.integers(-4000, 4001, n) if not dup else rng.integers(0, dup, n) * 900
        return centre + np.where(rng.random(n) < tight, j, far)
    out = []
    starts, ends = near(base + 5000, k), near(base + 16000, k)       # starts <= base + 9000 < base + 12000 <= ends: all overlap
    for i in range(k):
        rev = int(rng.random() < 0.5)
        a = int(rng.integers(3000, 9000))
        n_s = supps if isinstance(supps, int) else int(rng.integers(supps[0], supps[1] + 1))
        recs = []
        for _ in range(n_s):
            if rng.random() < other:
                recs.append((int(rng.integers(0, 1000)), 0, 0, 0, 2 | int(rng.random() < 0.5)))
                continue
            srev = rev ^ int(rng.random() < opposite)
            gap = int(near(300))
            if rng.random() < behind:
                ss = int(near(base - 30000)); se = ss + int(rng.integers(2000, 6000))
            else:
                ss = int(near(base + 40000)); se = int(near(base + 46000))
            recs.append((ss, max(se, ss), a + max(gap, -a), a + 3000 + max(gap, -a), srev))
        out.append((int(starts[i]), int(ends[i]), 0, a, rev, recs))
    return out


def _build(rng, segments):
    members, seg_off = [], [0]
    for piles in segments:
        seg = []
        for j, (k, opts) in enumerate(piles):
            seg += _pile(rng, 100_000 + 1_000_000 * j, k, **opts)
        order = rng.permutation(len(seg))
        members += [seg[i] for i in order]
        seg_off.append(len(members))
    return tables_of(members), np.asarray(seg_off, np.uint64)


def _sizes_2_500(rng):
    sizes = [2, 3, 4, 5, 6, 7, 9, 17, 33, 63, 64, 65, 100, 128, 129, 200, 257, 300, 400, 500]
    return [[(k, {"supps": 0} if k == 17 else {})] for k in sizes] + [[(40, {}), (2, {}), (11, {"opposite": 0.9})]]


def _oversize(rng):
    return [[(513, {})], [(600, {"supps": (1, 2)})], [(3000, {})], [(2, {}), (40, {}), (3, {"supps": 0})], [(60, {})]]


def _no_same_tid(rng):
    return [[(30, {"other": 1.0}), (25, {}), (8, {"supps": 0})], [(50, {"other": 1.0, "supps": 2})], [(12, {}), (90, {"other": 0.5})], [(3, {})]]


def _multi_supp(rng):
    return [[(200, {"supps": 3}), (20, {"supps": (0, 4)})], [(70, {"supps": (1, 3), "opposite": 0.6})], [(4, {"supps": 0}), (150, {"supps": 4, "behind": 0.7})],
            [(9, {"supps": (0, 2)})]]


def _duplicates(rng):
    return [[(40, {"dup": 1}), (30, {"dup": 2})], [(100, {"dup": 3, "supps": 2})], [(3, {"dup": 1}), (12, {"dup": 1, "tight": 0.5})], [(6, {"dup": 4, "supps": 0})]]


def _mixed24(rng):
    sizes = (0, 1, 2, 3, 5, 0, 17, 64, 65, 1, 128, 200, 33, 0, 7, 300, 2, 90, 1, 63, 450, 11, 0, 129)
    segs = []
    for n in sizes:
        piles, left = [], n
        while left > 0:
            k = int(min(left, rng.choice([1, 2, 3, 8, 30, 80, 200])))
            piles.append((k, {"supps": (0, 3), "opposite": float(rng.choice([0.1, 0.5, 0.9]))}))
            left -= k
        segs.append(piles)
    return segs


FAMILIES = {"sizes_2_500": _sizes_2_500, "oversize": _oversize, "no_same_tid": _no_same_tid, "multi_supp": _multi_supp,
            "duplicates": _duplicates, "mixed24": _mixed24}


def family(name, seed=1):
    """-> (tables as a dict of arrays, seg_off)"""
    rng = np.random.default_rng([seed, sorted(FAMILIES).index(name)])
    return _build(rng, FAMILIES[name](rng))


_WANT = {}


def expected(oracle, name, seed=1):
    """(tables, seg_off, groups, reference_fits) of a family, computed once per session"""
    if (name, seed) not in _WANT:
        import oracle_lib
        t, off = family(name, seed)
        groups = reference_groups(t["start"], t["end"], off)
        # where the reference's own dbscan1d.cpp is built (oracle/_ref), every set's largest cluster is also taken from it and must agree
        _WANT[(name, seed)] = (t, off, groups, reference_fits(oracle, t, off, groups, ref=oracle_lib.load_ref()))
    return _WANT[(name, seed)]


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_families_are_not_vacuous(oracle, name):
    t, off, groups, want = expected(oracle, name)
    n_groups = len(want)
    assert n_groups >= 4 and n_groups == int(groups[0][-1])
    for s in range(6):
        assert (want["size"][:, s] > 0).sum() * 10 >= n_groups, (name, s)          # a largest cluster in at least a tenth of the groups
        assert (want["size"][:, s] == 0).any(), (name, s)                           # and at least one group without
    assert (want["n_members"] >= 2).all()
    if name == "oversize":
        assert sorted(want["n_members"].tolist())[-3:] == [513, 600, 3000]
    if name == "sizes_2_500":
        assert {2, 3, 4, 5, 500} <= set(want["n_members"].tolist())
    if name == "mixed24":
        assert len(off) == 25 and (np.diff(off.astype(np.int64)) == 0).sum() == 4
    if name == "multi_supp":                                                         # a small group whose supplementary sets are oversize
        k = int(np.argmax(want["n_members"] == 200))
        assert want["n_members"][k] == 200 and group_set_sizes(t, off, groups, k)[2] > 512


def group_set_sizes(t, seg_off, groups, g):
    c = int(np.searchsorted(groups[0], g, side="right")) - 1
    sets, _ = group_sets(t, int(seg_off[c]), groups[2][int(groups[1][g]):int(groups[1][g + 1])])
    return [len(x) for x in sets]


def test_host_tree_gives_the_restatements_groups_on_the_families():
    from contextsv_amd import host
    for name in sorted(FAMILIES):
        t, off = family(name)
        got, want = host.split_groups_host(t["start"], t["end"], off), reference_groups(t["start"], t["end"], off)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), name


# ---- the ABI ---------------------------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(ROOT, "include", "csvgpu.h")).read()


def _struct_fields(name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(?:const\s+)?(\w+)\s+(.*)$", decl, flags=re.S)
        for item in m.group(2).split(","):
            im = re.match(r"\s*(\*?)\s*(\w+)\s*(?:\[(\d+)\])?\s*$", item)
            fields.append((im.group(2), m.group(1), bool(im.group(1)), int(im.group(3) or 1)))
    return fields                                                                    # (name, type, pointer, count)


def test_entry_points_declared_exported_and_bound():
    from contextsv_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    lib = _lib.load()
    for name in ("csvgpu_split_fits", "csvgpu_split_groups_fits"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert hasattr(lib, name) and name in _lib.ABI
    assert len(_lib.ABI["csvgpu_split_fits"][1]) == 10 and len(_lib.ABI["csvgpu_split_groups_fits"][1]) == 9
    assert _lib.KERNEL_NAMES[10] == "split_fits" and _lib.K_SPLIT_FITS == 10 and _lib.K_COUNT == 11
    assert re.search(r"CSV_K_SPLIT_FITS\s*=\s*10\b", text) and re.search(r"CSV_K_COUNT\s*=\s*11\b", text)
    assert re.search(r"#define\s+CSVGPU_ABI_VERSION\s+4\b", text)


def test_fit_record_is_64_bytes_in_the_headers_field_order():
    from contextsv_amd import _lib
    fields = _struct_fields("csv_split_fit")
    assert [(n, ty, k) for n, ty, p, k in fields] == [("median", "int32_t", 6), ("size", "uint32_t", 6), ("n_members", "uint32_t", 1),
                                                      ("n_opposite", "uint32_t", 1), ("reserved", "uint32_t", 2)]
    assert sum(4 * k for _, _, _, k in fields) == 64
    for dt in (_lib.SPLIT_FIT_DTYPE, FIT_DTYPE):
        assert dt.itemsize == 64 and list(dt.names) == [n for n, _, _, _ in fields]
        assert [dt.fields[n][1] for n, _, _, _ in fields] == [0, 24, 48, 52, 56]
        assert [dt.fields[n][0].base.str for n, _, _, _ in fields] == ["<i4", "<u4", "<u4", "<u4", "<u4"]


def test_tables_struct_matches_the_header():
    from contextsv_amd import _lib
    fields = _struct_fields("csv_split_tables")
    assert [n for n, _, _, _ in fields] == ["n_members", "n_supp"] + list(TABLE_FIELDS) == [n for n, _ in _lib.csv_split_tables._fields_]
    for (n, ty, pointer, _), (_, ct) in zip(fields, _lib.csv_split_tables._fields_):
        assert (ct is C.c_void_p) == pointer and (pointer or (ty == "uint64_t" and ct is C.c_uint64)), n
    want = {"reverse": "uint8_t", "supp_flags": "uint8_t", "supp_off": "uint64_t"}
    assert all(ty == want.get(n, "int32_t") for n, ty, pointer, _ in fields if pointer)
    assert C.sizeof(_lib.csv_split_tables) == 8 * 13
