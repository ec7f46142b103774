"""The inputs of tests/depth_edge_inputs.py hold what they claim (no GPU): the module's constants are the kernels', its numpy depth map
and its model of the tile kernel's decisions equal the oracle on every case, each family's structural claim — what makes it reach an
edge of kernels/depth.hip or of the scan's tile ranges — follows from the model under BOTH producers of the candidate ranges, and the
model with one comparison or mask the wrong way round gives another map than the oracle on the case aimed at it (so a kernel with that
mistake turns tests/test_gpu_depth_edges.py red)."""
import functools
import os
import re

import numpy as np
import pytest

import depth_edge_inputs as de

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "contextsv_amd", "csrc")
T = de.T

_SMALL = de.small_cases()
_G = de.g_cases()


def _int(pattern, text):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1))


def _case(name):
    return next(c for c in _SMALL + _G if c[0] == name)


def _sorted(reads):
    return not (np.diff(reads.pos.astype(np.int64)) < 0).any()


@functools.lru_cache(maxsize=None)
def _items(name, producer):
    _, r, depth_len = _case(name)
    return de.tile_items(r, depth_len, de.candidate_ranges(r, depth_len, producer))


def _per_tile(name, producer):
    _, r, depth_len = _case(name)
    lo, hi, _ = de.candidate_ranges(r, depth_len, producer)
    n_items = np.zeros(de.n_tiles_of(depth_len), np.int64)
    for it in _items(name, producer):
        n_items[it["tile"]] += it["item"]
    return hi - lo, n_items


def test_constants_are_the_kernels():
    """a retune of the tile, the checkpoint grid, the batch sizes, the ring or the slots has to move the module's edges with it"""
    depth = open(os.path.join(CSRC, "kernels", "depth.hip")).read()
    scan = open(os.path.join(CSRC, "kernels", "scan.hip")).read()
    common = open(os.path.join(CSRC, "common.hpp")).read()
    assert _int(r"constexpr int DEPTH_TILE_SHIFT = (\d+),", common) == de.DEPTH_TILE_SHIFT
    assert _int(r"constexpr int CKPT_SHIFT = (\d+),", common) == de.CKPT_SHIFT
    assert _int(r"constexpr int DEPTH_THREADS = (\d+);", depth) == de.DEPTH_THREADS
    assert _int(r"constexpr int WL_CAP = (\d+);", depth) == de.WL_CAP
    assert _int(r"constexpr int WL_SPEC = (\d+);", depth) == de.WL_SPEC
    assert _int(r"constexpr int DEPTH_PF = (\d+);", depth) == de.DEPTH_PF
    assert 1 << _int(r"\(k_hi - k_lo\) < \(1ull << (\d+)\)", depth) == de.FAST_MAX_CANDIDATES
    assert re.search(r"constexpr int WPL = 4;", depth) and _int(r"constexpr int WAVE = (\d+);", common) * 4 == de.CW
    assert _int(r"constexpr uint32_t TR_SLOTS = (\d+);", scan) == de.TR_SLOTS
    assert _int(r"constexpr uint32_t RS_MIN_READS = (\d+);", scan) == de.RS_MIN_READS
    assert _int(r"constexpr int RS_THREADS = (\d+);", scan) == de.RS_THREADS
    assert [_int(r"t1 - t0 >= (\d+)u", s) for s in scan.split("const bool wide")[1:]] == [de.WIDE_TILES] * 2      # rows and lanes kernels
    # the cases sit where these constants put the edges
    assert {de.WL_SPEC - 1, de.WL_SPEC, de.WL_SPEC + 1, de.WL_CAP - 1, de.WL_CAP, de.WL_CAP + 1, 2 * de.WL_CAP - 1, 2 * de.WL_CAP,
            2 * de.WL_CAP + 1, 0, 1} <= set(de.B_COUNTS)
    for gl in (16, 8):
        ngrp = de.DEPTH_THREADS // gl
        assert {ngrp - 1, ngrp, ngrp + 1} <= set(de.B_COUNTS)
    assert set(de.D_NCHUNKS) == {1, 2, de.NS - 1, de.NS, de.NS + 1, 2 * de.NS, 2 * de.NS + 1}
    assert set(de.D_NREM) == {de.CW - 1, de.CW, de.CW + 1, de.NS * de.CW - 1, de.NS * de.CW, de.NS * de.CW + 1}
    assert set(de.A_DEPTH_LENS) == {1, 3, T - 1, T, T + 1, 2 * T + 5, 3 * T}
    assert de.H_TILES == 2 * de.TR_SLOTS + 2


def test_case_names_are_unique_and_coordinates_small():
    names = [c[0] for c in _SMALL + _G]
    assert len(set(names)) == len(names)
    for name, r, depth_len in _SMALL + _G:
        assert _sorted(r) == (not name.startswith("U/")), name
        assert (r.mapq == 60).all() and int(np.abs(r.pos.astype(np.int64)).max()) + int(de.ref_len(r).max()) < 2**31, name
        assert de.n_tiles_of(depth_len) <= 131, name


@pytest.mark.parametrize("case", _SMALL + _G, ids=[c[0] for c in _SMALL + _G])
def test_numpy_depth_and_model_equal_the_oracle(oracle, case):
    name, r, depth_len = case
    od, osum, onz = oracle.depth(r, depth_len)
    d, s, nz = de.np_depth(r, depth_len)
    assert np.array_equal(d, od) and (s, nz) == (osum, onz)
    if name.startswith("G/"):
        return                                   # (2^20 items in pure Python: the model's ranges are checked in the family's own test)
    for producer in ("pmax", "scan") if _sorted(r) else ("pmax",):
        d, s, nz = de.model_depth(r, depth_len, producer)
        assert np.array_equal(d, od) and (s, nz) == (osum, onz), producer


def test_a_reads_sit_on_every_tile_and_map_edge():
    r = _case("A/len%d" % (3 * T))[1]
    p1, last, tags = de.p1_of(r), de.p1_of(r) + de.ref_len(r) - 1, r.tags
    for B in (T, 2 * T):
        got = {(int(p1[i]) - B, int(last[i]) - B) for i in tags["edge"]}
        assert {(a, b) for a in range(-2, 2) for b in range(a, 2)} <= got
    owner, op, ln, rl, cs, before = de._words(r)
    gap = de._GAP[op] & (ln > 0)
    starts, ends = (p1[owner] + before)[gap], (p1[owner] + before + ln)[gap]
    for B in (T, 2 * T):
        assert B in starts and B in ends                                        # a D / N that starts on B, one whose next base is B
        zero = (ln == 0) & de._REF[op] & (p1[owner] + before == B)
        assert zero.any()
    assert (T, 2 * T) in set(zip(starts.tolist(), ends.tolist())) and (T - 1, 2 * T + 1) in set(zip(starts.tolist(), ends.tolist()))
    assert int(r.pos.min()) == -1
    for L in de.A_DEPTH_LENS:
        assert {x for x in (L - 2, L - 1, L, L + 1) if x >= 0} <= set(last[tags["map_end"]].tolist())
        assert (p1[tags["beyond"]] > L).any()
    assert (de.ref_len(r)[tags["no_ref"]] == 0).all() and (np.diff(r.cigar_off.astype(np.int64))[tags["empty"]] == 0).all()
    assert {int(f) & de.DEPTH_FILTER for f in r.flag[tags["filtered"]]} >= {de.F_UNMAP, de.F_SECONDARY, de.F_QCFAIL, de.F_DUP}
    assert (r.flag[tags["counted"]] & de.DEPTH_FILTER == 0).all() and (r.flag[tags["counted"]] != 0).all()


def test_b_candidate_and_item_counts_per_tile():
    for producer in ("pmax", "scan"):
        cand, items = _per_tile("B/items_eq_candidates", producer)
        assert cand.tolist() == list(de.B_COUNTS) and items.tolist() == list(de.B_COUNTS), producer
        cand, items = _per_tile("B/every_7th_filtered", producer)
        want = [n - sum(de.b_filtered(k, n) for k in range(n)) for n in de.B_COUNTS]
        assert cand.tolist() == list(de.B_COUNTS) and items.tolist() == want, producer
        assert all(w < n for w, n in zip(want, de.B_COUNTS) if n > 4)             # n_pre < k_n
        assert want[de.B_COUNTS.index(de.WL_CAP + 1)] < de.WL_CAP and want[de.B_COUNTS.index(de.WL_SPEC + 1)] < de.WL_SPEC
        cand, items = _per_tile("B/candidates_without_items", producer)
        assert cand[2] == de.WL_CAP + 1 and 0 < items[2] < de.WL_SPEC and items[2] == 2, producer
        assert ((cand > 0) & (items == 0)).any(), producer
    cand, items = _per_tile("B/candidates_without_items", "pmax")
    assert cand[4] == 6 and items[4] == 0                                         # the filtered long read and the short ones behind it
    cand, items = _per_tile("B/candidates_without_items", "scan")
    assert cand[5] == 3 and items[5] == 0                                         # reads of the last tile that start beyond the map


def test_c_checkpoint_searches_reach_their_edges():
    name, r, depth_len = _case("C/checkpoints")
    tags = r.tags
    for producer in ("pmax", "scan"):
        its = [it for it in _items(name, producer) if "nb" in it]
        live = [it for it in its if it["item"]]
        for delta, key in ((0, "on_T0"), (-1, "on_T1m1"), (0, "on_T1")):
            for c0rel in (37, 63):
                rd = tags["ckpt%+d/c0rel%d" % (delta, c0rel)][0]
                assert any(it["read"] == rd and it[key] for it in live), (producer, key, c0rel)
        # one short of each edge, and one past T0 (what the flipped T0 comparison would take)
        ck, p1, off = de.checkpoints(r), de.p1_of(r), r.cigar_off.astype(np.int64)
        for delta in (-2, -1, 0, 1):
            rd = tags["ckpt%+d/c0rel37" % delta][0]
            g = (int(off[rd]) >> de.CKPT_SHIFT) + 10
            assert int(p1[rd]) + int(ck[g]) == 2 * T + delta
        assert any(it["read"] == tags["nb0"][0] and it["nb"] == 0 for it in live)
        assert len({it["tile"] for it in live if it["read"] == tags["nb0"][0]}) == 2          # across a tile edge
        assert any(it["read"] == tags["nb1"][0] and it["nb"] == 1 for it in live)
        assert {37, 63} <= {it["c0rel"] for it in live}
        assert any(it["nb"] > 0 and not it["want1"] and it["want0"] for it in live)           # ends inside the tile it entered
        assert any(it["nb"] > 0 and it["e_lo"] == 1 and it["nrem"] == de.CKPT_WORDS for it in live)      # first boundary already right of the tile
        for key in ("miss0", "miss1"):
            assert any(it[key][8] for it in live), (producer, key)
            assert all(it[key][3] for it in live if it[key][8])                               # (NP = 8 open implies NP = 3 open)
        # ... and by more than the probes' reach, at both ends of the bracket: the answer is the first boundary (skip in front) and
        # the last (skip behind)
        for tag, search, answer in (("skip_first", "lo", 1), ("skip_first", "e_lo", 1), ("skip_last", "lo", None), ("skip_last", "e_lo", None)):
            hit = [it for it in live if it["read"] == tags[tag][0] and it["miss0" if search == "lo" else "miss1"][8]
                   and it[search] == (it["nb"] + 1 if answer is None else answer)]
            assert hit and all(abs(it["gs0" if search == "lo" else "gs1"] - it[search]) > 8 for it in hit), (tag, search)
        cl = [it for it in live if it["read"] == tags["clamps"][0]]
        assert any(it["want0"] and min(de.probes(it["gs0"], it["nb"], 8)) == 1 and it["gs0"] - 3 < 1 for it in cl)
        assert any(it["want1"] and max(de.probes(it["gs1"], it["nb"], 8)) == it["nb"] and it["gs1"] + 4 > it["nb"] for it in cl)
        assert all(it["nb"] >= 9 for it in cl)
    # a candidate whose start is at or right of T1: only the scan's ranges hold one (the pmax range ends in front of it)
    assert any(it["why"] == "right_of_tile" and it["read"] == tags["beyond"][0] for it in _items(name, "scan"))
    assert not any(it["why"] == "right_of_tile" for it in _items(name, "pmax"))


def test_d_chunk_counts_and_neighbours():
    for m in (0, 1, 2, 3):
        name, r, depth_len = _case("D/tail%d" % m)
        assert r.n_cigar % 4 == m and r.n_cigar % de.CW != 0
        assert int(r.cigar_off[-1]) - int(r.cigar_off[-2]) > de.CW                # the last read's last chunk is the array's partial one
        owner, op, ln, rl, cs, before = de._words(r)
        for producer in ("pmax", "scan"):
            live = [it for it in _items(name, producer) if it["item"]]
            named = [it for it in live if it["read"] in r.tags["item"]]
            assert {it["n_chunks"] for it in live} >= set(de.D_NCHUNKS)
            assert {(it["nrem"], it["c0rel"]) for it in named} >= {(a, b) for a in de.D_NREM for b in de.D_C0REL}
            assert len(named) == len(r.tags["item"])                                 # each of them lies in one tile
            for it in named:
                a, b = it["chunk"] + it["c0rel"] - 1, it["chunk"] + it["nrem"]      # the words next to its first and last valid word
                assert rl[a] >= 1000 and rl[b] >= 1000 and owner[a] != it["read"] and owner[b] != it["read"]
            row = [it for it in live if it["read"] in r.tags["row"]]
            assert len(row) == 20 and all(it["n_chunks"] == 1 for it in row) and len({it["tile"] for it in row}) == 1
            assert np.array_equal(np.diff(sorted(it["read"] for it in row)), np.ones(19, np.int64))


def test_e_chunks_on_both_sides_of_the_in_tile_test():
    name, r, depth_len = _case("E/paths")
    for producer in ("pmax", "scan"):
        chunks = []
        for it in _items(name, producer):
            if it["item"]:
                TW = min((it["tile"] + 1) * T, depth_len) - it["tile"] * T
                chunks += [(b, b + tot - TW, gaps, zero, tot) for b, tot, gaps, zero in de.item_chunks(r, it, depth_len)]
        assert {-1, 0, 1} <= {c[0] for c in chunks} and {-1, 0, 1} <= {c[1] for c in chunks}
        assert any(c[0] >= 0 and c[1] <= 0 for c in chunks) and any(c[0] < 0 for c in chunks) and any(c[1] > 0 for c in chunks)
        assert any(c[2] == de.CW and c[4] > 0 for c in chunks)                      # 256 gap words and nothing else
        assert any(c[3] and c[4] == 0 for c in chunks)                              # 256 zero-length words
    owner, op, ln, rl, cs, before = de._words(r)
    p1 = de.p1_of(r)
    a = (p1[owner] + before)[de._GAP[op]]
    b = a + ln[de._GAP[op]]
    edges = np.arange(1, de.n_tiles_of(depth_len)) * T
    assert any(((a < B) & (b > B) & (b - a < T)).any() for B in edges)              # a gap that straddles T0 of one tile = T1 of the other
    assert ((b - a > T) & (a % T != 0)).any()                                       # one that covers a whole tile and more


def test_f_window_grid_is_complete():
    name, r, depth_len = _case("F/windows")
    n_w = np.diff(r.cigar_off.astype(np.int64))
    assert {int(n_w[i]) for i in r.tags["item"]} == set(de.F_VALID)
    for producer in ("pmax", "scan"):
        live = [it for it in _items(name, producer) if it["item"] and it["read"] in r.tags["item"]]
        assert {de.group_windows(it) for it in live} >= {(m, w) for m in range(4) for w in (1, 2, 3)}
        got = {(int(r.cigar_off[it["read"]]) & 3, int(n_w[it["read"]])) for it in live if it["nrem"] - it["c0rel"] == n_w[it["read"]]}
        assert got == {(m, n) for m in range(4) for n in de.F_VALID}


def test_g_middle_tile_sits_on_the_fast_threshold():
    for (name, r, depth_len), want in zip(_G, (de.FAST_MAX_CANDIDATES - 1, de.FAST_MAX_CANDIDATES)):
        assert depth_len == 3 * T                                                   # the middle tile is a full one
        for producer in ("pmax", "scan"):
            lo, hi, _ = de.candidate_ranges(r, depth_len, producer)
            assert (hi - lo).tolist() == [1, want, 1], (name, producer)
        p1, last = de.p1_of(r)[1:-1], (de.p1_of(r) + de.ref_len(r) - 1)[1:-1]
        assert p1.min() >= T and last.max() < 2 * T and (np.diff(r.cigar_off.astype(np.int64)) == 1).all()
        assert set(np.unique(r.cigar[1:-1] >> 4).tolist()) == set(range(1, 41))


def test_h_one_workgroup_more_tiles_than_slots():
    name, r, depth_len = _case("H/scan_tile_ranges")
    assert r.n_reads <= (de.RS_THREADS // 64) * de.RS_MIN_READS                     # scan_grid: ceil(n / (waves x RS_MIN_READS)) = 1 workgroup (rows; lanes take more)
    first = de.p1_of(r) >> de.DEPTH_TILE_SHIFT
    last = (de.p1_of(r) + de.ref_len(r) - 1) >> de.DEPTH_TILE_SHIFT
    tbase = int(first[0])
    assert tbase == 0 and len(set(first.tolist())) == de.H_TILES - len(de.H_SKIP) and int(first.max()) == de.H_TILES - 1 > 2 * de.TR_SLOTS
    per_tile = np.bincount(first)
    assert set(per_tile.tolist()) == {0, 1, 2} and all(per_tile[t] == 2 for t in de.H_DOUBLE)
    reach = (last - first).tolist()
    assert {de.WIDE_TILES - 1, de.WIDE_TILES} <= set(reach)
    assert {de.TR_SLOTS - 1, de.TR_SLOTS} <= {int(t) - tbase for t in first}
    wide_across = [(int(a), int(b)) for a, b in zip(first, last) if b - a >= de.WIDE_TILES and a - tbase < de.TR_SLOTS <= b - tbase]
    assert wide_across                                                              # a wide read whose tiles lie on both sides of the slots' end
    lo, hi, _ = de.candidate_ranges(r, depth_len, "scan")
    assert np.flatnonzero(hi - lo == 0).tolist() == list(de.H_SKIP)                 # (tiles without a read keep the all-zero range)
    assert all((hi - lo)[a + 1:b + 1].min() >= 2 for a, b in wide_across)           # the reaching read and the tile's own


def test_u_twins_are_unsorted_permutations():
    for name, r, depth_len in _SMALL:
        if not name.startswith("U/"):
            continue
        src = "B/items_eq_candidates" if name == "U/B/equal_pos_runs" else name[2:]
        _, s, s_len = _case(src)
        assert s_len == depth_len and not _sorted(r) and r.n_reads == s.n_reads and r.n_cigar == s.n_cigar

        def key(x, with_pos):
            off = x.cigar_off.astype(np.int64)
            return sorted(((int(x.pos[i]) if with_pos else 0), int(x.flag[i]), x.cigar[off[i]:off[i + 1]].tobytes()) for i in range(x.n_reads))
        assert key(r, name != "U/B/equal_pos_runs") == key(s, name != "U/B/equal_pos_runs")
    r = _case("U/B/equal_pos_runs")[1]
    assert np.bincount(r.pos - r.pos.min()).max() >= 8                              # runs of equal pos


@pytest.mark.parametrize("flip,case_name,producer", [
    ("ckpt_t0", "C/checkpoints", "pmax"), ("ckpt_t0", "C/checkpoints", "scan"),
    ("ckpt_t1", "C/checkpoints", "pmax"), ("ckpt_t1", "C/checkpoints", "scan"),
    ("mask", "D/tail0", "pmax"), ("mask", "D/tail1", "scan"),
    ("range_end", "A/len%d" % (2 * T + 5), "pmax"),
])
def test_a_flipped_comparison_changes_the_map(oracle, flip, case_name, producer):
    """The unflipped model equals the oracle (above). One comparison or mask the wrong way round does not, on the case aimed at it:
    a checkpoint one position right of T0 taken as the walk's start loses position T0 (the direction that matters: `<` for `<=` only starts
    a boundary earlier), `<` for `<=` at T1 - 1 drops the words from a boundary on T1 - 1 on, unmasked neighbour words move the cursor and
    count, and a range that ends at pos >= T1 - 2 loses the read whose first base is the tile's last position."""
    name, r, depth_len = _case(case_name)
    od, osum, onz = oracle.depth(r, depth_len)
    d, s, nz = de.model_depth(r, depth_len, producer, flip=flip)
    assert not np.array_equal(d, od)
    if flip.startswith("ckpt"):
        # ... and exactly where the case puts it: at the tile edge the flipped comparison concerns, one read short
        bad = np.flatnonzero(d != od)
        assert (bad % T == (0 if flip == "ckpt_t0" else T - 1)).all() and (od[bad] - d[bad] == 1).all()
