"""The inputs of tests/scan_edge_inputs.py hold what they claim (no GPU): the module's constants are the kernels', its op-by-op scan equals
the oracle on every case (signatures as a sorted set, the three per-read intervals), and each family's structural claim — what makes a case
reach a seam of kernels/scan.hip — follows from the module's model of the work split, the ring, the staging buffer and the lane stage."""
import functools
import os
import re

import numpy as np
import pytest

import scan_edge_inputs as se

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "contextsv_amd", "csrc")

_CASES = se.all_cases()
_BY_NAME = {c[0]: c for c in _CASES}


def _int(pattern, text):
    m = re.search(pattern, text)
    assert m, pattern
    return int(m.group(1), 0)


def _family(f):
    return [c for c in _CASES if se.info(c[0])["family"] == f]


@functools.lru_cache(maxsize=None)
def _scan(name):
    _, r, depth_len, min_oplen, min_mapq = _BY_NAME[name]
    return se.np_scan(r, depth_len, min_oplen, min_mapq)


def _n_words(r):
    return np.diff(r.cigar_off.astype(np.int64))


def test_constants_are_the_kernels():
    """a retune of the staging buffer, the ring, the stage or the grids has to move the module's edges with it"""
    scan = open(os.path.join(CSRC, "kernels", "scan.hip")).read()
    common = open(os.path.join(CSRC, "common.hpp")).read()
    pack = open(os.path.join(CSRC, "cigar_pack_core.hpp")).read()
    wave = _int(r"constexpr int WAVE = (\d+);", common)
    assert wave == se.WAVE
    for form in ("SCAN", "RS", "LN"):
        assert re.search(r"constexpr int %s_WAVES = %s_THREADS / WAVE;" % (form, form), scan)
        assert _int(r"constexpr int %s_THREADS = (\d+);" % form, scan) // wave == se.SCAN_WAVES
    assert _int(r"constexpr uint32_t SIG_BUF = (\d+);", scan) == se.SIG_BUF
    assert _int(r"constexpr int RING_D = (\d+);", scan) == se.RING_D
    assert _int(r"constexpr int CHUNK_WORDS = (\d+) \* WAVE;", scan) * wave == se.CHUNK_WORDS
    assert _int(r"constexpr uint32_t LN_STAGE = (\d+);", scan) == se.LN_STAGE
    assert _int(r"constexpr uint32_t RS_MIN_READS = (\d+);", scan) == se.RS_MIN_READS
    assert _int(r"form == SCAN_FORM_LANES \? (\d+) : RS_MIN_READS", scan) == se.LN_READS_PER_WAVE
    assert re.search(r"const uint64_t want = \(n_reads \+ SCAN_WAVES - 1\) / SCAN_WAVES;", scan)                 # the wave form: a read per wave
    assert _int(r"constexpr uint32_t BK_BITS = (\d+),", common) == se.BK_BITS
    assert _int(r"BK_LOCAL_MAX = (\d+);", common) == se.BK_LOCAL_MAX
    assert 1 << _int(r"constexpr uint32_t PIECE_SHIFT = (\d+),", pack) == se.PIECE_OPS == 2 * se.CHUNK_WORDS
    assert _int(r"constexpr uint32_t ESC_LEN = (0x[0-9A-Fa-f]+)u;", pack) == se.ESC_LEN
    assert _int(r"constexpr uint64_t MAX_ESC_DENOM = (\d+);", pack) == se.MAX_ESC_DENOM
    # the cases sit where these constants put the edges
    assert [3 * 128 + x for x in se.S_COUNT_LAST] == [se.SIG_BUF - 1, se.SIG_BUF, se.SIG_BUF + 1]
    assert se.S_DENSE_READS * se.S_DENSE_SIGS // 2 > 2 * se.SIG_BUF
    assert se.L_PER_READ * se.WAVE == se.LN_STAGE and min(se.L_BIG) == se.LN_STAGE + 1
    assert set(se.R_SINGLE) >= {k * se.CHUNK_WORDS + d for k in range(1, 6) for d in (-1, 0, 1)} | {1, 2049}
    assert se.READS_PER_WG == {0: 4, 1: 128, 2: 128, 3: 512}


def test_names_positions_and_sizes():
    names = [c[0] for c in _CASES]
    assert len(set(names)) == len(names)
    bases = sorted(se.info(n)["pos_base"] for n in names)
    assert len(set(bases)) == len(bases) and min(np.diff(bases)) >= 1000
    for name, r, depth_len, min_oplen, min_mapq in _CASES:
        assert 1 <= r.n_reads <= se.MAX_READS, name
        assert not (np.diff(r.pos.astype(np.int64)) < 0).any(), name                  # coordinate-sorted: the resident entry takes the scan's tile ranges
        assert int(r.pos[0]) == se.info(name)["pos_base"] and depth_len < 2**20, name
        assert r.n_cigar <= 40_000 and min_oplen in (1, 50), name
    assert {se.info(n)["family"] for n in names} == set("SBRWL")


@pytest.mark.parametrize("case", _CASES, ids=[c[0] for c in _CASES])
def test_numpy_scan_equals_the_oracle(oracle, case):
    name, r, depth_len, min_oplen, min_mapq = case
    got = _scan(name)
    sig = oracle.cigar_scan(r, depth_len, min_oplen, min_mapq)
    want = sorted(zip(sig["start"].tolist(), sig["end"].tolist(), sig["read"].tolist(), sig["qpos_kind"].tolist()))
    assert len(got["emitted"]) == len(got["sig"]) == len(want)                         # (no two signatures of these cases are equal)
    assert sorted(got["sig"]) == want
    for key, o in zip(("ref_end", "q_start", "q_end"), oracle.aln_intervals(r)):
        assert np.array_equal(got[key], np.asarray(o).astype(np.int64)), key


# ------------------------------------------------------------------------------------------------------------------- the split itself
def test_split_model_is_a_partition_in_every_form():
    for name, r, *_ in _CASES:
        for form in se.FORMS:
            sp = se.split(r, form)
            assert sp["grid"] == -(-r.n_reads // se.READS_PER_WG[form]) and sp["n_waves"] == 4 * sp["grid"]
            assert sp["r_begin"][0] == 0 and sp["r_end"][-1] == r.n_reads and np.array_equal(sp["r_begin"][1:], sp["r_end"][:-1])
            assert (sp["reads_per_wave"] >= 0).all() and int(sp["reads_per_wave"].sum()) == r.n_reads
            assert sp["share"] * sp["n_waves"] >= r.n_cigar > (sp["share"] - 1) * sp["n_waves"] or r.n_cigar == 0
            off = r.cigar_off.astype(np.int64)
            for g in range(sp["n_waves"] - 1):                                         # every read's first word lies in its wave's share
                rd = np.arange(sp["r_begin"][g], sp["r_end"][g])
                assert ((off[rd] >= g * sp["share"]) & (off[rd] < (g + 1) * sp["share"])).all(), (name, form, g)


# ------------------------------------------------------------------------------------------------------------------- S
def test_s_workgroups_sit_on_the_staging_edge():
    totals = []
    for last in se.S_COUNT_LAST:
        name, r, *_ = _BY_NAME["S/count_%d" % (3 * 128 + last)]
        em = _scan(name)["emitted"]
        assert np.bincount([e[2] for e in em]).tolist() == [128, 128, 128, last]
        for form in se.FORMS:
            assert se.sigs_per_workgroup(r, form, em).tolist() == [3 * 128 + last], (name, form)        # one workgroup in every form
        totals.append(len(em))
    assert totals == [se.SIG_BUF - 1, se.SIG_BUF, se.SIG_BUF + 1]
    for name, at_50 in (("S/dense_oplen50", True), ("S/dense_oplen1", False)):
        _, r, depth_len, min_oplen, _ = _BY_NAME[name]
        em = _scan(name)["emitted"]
        assert (_n_words(r) == se.S_DENSE_WORDS).all() and r.n_reads == se.S_DENSE_READS
        per_read = np.bincount([e[2] for e in em])
        if at_50:
            assert per_read.tolist() == [se.S_DENSE_SIGS] * (se.S_DENSE_READS - 1) + [se.S_DENSE_SIGS - 1]      # (the last read's clip at the contig's end is skipped)
            assert se.sigs_per_workgroup(r, 0, em).tolist() == [1200, 1199]
            for form in (1, 2, 3):
                assert se.sigs_per_workgroup(r, form, em).tolist() == [2399]
        else:
            assert (per_read > se.S_DENSE_SIGS).all() and (se.sigs_per_workgroup(r, 0, em) > 2 * se.SIG_BUF).all()
        # the soft clip at the contig's end: its start is exactly depth_len, and an S 60 earlier in the same read does come out
        last = r.n_reads - 1
        assert (r.cigar[-1] & 15, r.cigar[-1] >> 4) == (se.S, 60) and int(_scan(name)["ref_end"][last]) + 1 == depth_len
        assert not any(e[4] == r.n_cigar - 1 for e in em) and any(e[2] == last and e[3] & 3 == se.KIND_CLIP for e in em)


def test_s_bucket_cases_fill_the_buffer_then_overflow_into_one_bucket():
    for name, n_ins in (("S/bucket_over", se.BK_LOCAL_MAX + se.S_BUCKET_EXTRA), ("S/bucket_at", se.BK_LOCAL_MAX)):
        _, r, depth_len, min_oplen, min_mapq = _BY_NAME[name]
        em = _scan(name)["emitted"]
        assert r.n_reads == 1 and se.info(name)["n_ins_at_one_position"] == n_ins
        for form in se.FORMS:
            sp = se.split(r, form)
            assert sp["reads_per_wave"].tolist() == [1, 0, 0, 0]                          # one wave works, three own nothing
            staged, overflow, certain = se.staging_of_single_read(r, form, em)
            # emission order: the SIG_BUF deletions first, filling the buffer exactly at the end of a step of the form ...
            assert certain and len(staged) == se.SIG_BUF and all(e[3] & 3 == se.KIND_DEL for e in staged), (name, form)
            assert [e[4] for e in staged] == list(range(1, 2 * se.SIG_BUF, 2))
            # ... then the insertions, all through the overflow branch and all at one reference position
            ins = [e for e in overflow if e[3] & 3 == se.KIND_INS]
            assert len(ins) == n_ins and len({(e[0], e[1]) for e in ins}) == 1 and len(overflow) - n_ins == (2 if n_ins > se.BK_LOCAL_MAX else 3)
            assert [e[4] for e in ins] == list(range(2 * se.SIG_BUF, 2 * se.SIG_BUF + n_ins))      # nothing reference-consuming between them
            for with_type in (False, True):                                              # the host-pointer entry's keys, the pipeline's
                b_staged = se.bucket_counts(staged, depth_len, with_type)
                b_all = se.bucket_counts(em, depth_len, with_type)
                assert len(b_staged) >= 256 and max(b_staged.values()) <= 4               # spread over many buckets
                assert max(b_all.values()) == n_ins                                      # both counts: BK_LOCAL_MAX + 50, and BK_LOCAL_MAX exactly
                assert sorted(b_all.values())[-2] <= 4                                   # only that bucket, and only the overflow branch sees it
                hot = max(b_all, key=b_all.get)
                assert b_staged.get(hot, 0) == 0
                # ... and it is not the last bucket in use: the overflow branch also emits into higher ones, whose places depend on its count
                b_over = se.bucket_counts(overflow, depth_len, with_type)
                assert max(b_over) > hot, (name, form, with_type)
    assert max(se.bucket_counts(_scan("S/bucket_over")["emitted"], _BY_NAME["S/bucket_over"][2], True).values()) > se.BK_LOCAL_MAX
    assert max(se.bucket_counts(_scan("S/bucket_at")["emitted"], _BY_NAME["S/bucket_at"][2], True).values()) == se.BK_LOCAL_MAX


def test_s_kinds_are_mixed_and_n_del_differs_per_case():
    n_del = {}
    for name, *_ in _family("S"):
        kinds = np.bincount([e[3] & 3 for e in _scan(name)["emitted"]], minlength=3)
        assert kinds[se.KIND_DEL] > 0 and kinds[se.KIND_INS] > 0 and kinds[se.KIND_CLIP] > 0, name
        n_del[name] = int(kinds[se.KIND_DEL])
    assert len(set(n_del.values())) == len(n_del) and min(n_del.values()) > 0, n_del


# ------------------------------------------------------------------------------------------------------------------- B
def test_b_waves_own_more_than_a_batch():
    seen = set()
    for name, r, *_ in _family("B"):
        per_wave = se.split(r, 0)["reads_per_wave"]
        seen |= set(per_wave.tolist())
        assert per_wave.max() > se.WAVE or name.endswith("_64"), name
        want = se.info(name)["want"]
        if want:
            assert (want in per_wave.tolist()) if want < 190 else per_wave.max() >= 190, (name, per_wave.max())
        assert (per_wave == 0).any(), name                                                # (waves inside the long read own nothing)
    assert {64, 65, 128, 129} <= seen and max(seen) >= 190
    # mirrors: the tiny reads come first, so it is the FIRST wave whose batches run on
    for want in se.B_FRONT:
        assert se.split(_BY_NAME["B/mirror_%d" % want][1], 0)["reads_per_wave"][0] >= want
    assert se.split(_BY_NAME["B/mirror_190"][1], 0)["reads_per_wave"][0] == 190


def test_b_signatures_come_from_every_batch():
    for name in ("B/front_65_sigs", "B/front_129_sigs"):
        _, r, *_ = _BY_NAME[name]
        sp = se.split(r, 0)
        per_read = np.bincount([e[2] for e in _scan(name)["emitted"]], minlength=r.n_reads)
        g = int(np.argmax(sp["reads_per_wave"]))
        assert sp["reads_per_wave"][g] == se.info(name)["want"]
        for rb in range(int(sp["r_begin"][g]), int(sp["r_end"][g]), se.WAVE):              # the batches of that wave
            assert per_read[rb:min(rb + se.WAVE, int(sp["r_end"][g]))].sum() > 0, (name, rb)
        assert (sp["r_end"][g] - sp["r_begin"][g] - 1) // se.WAVE >= 1


def test_b_empty_reads_at_a_batchs_64th_and_65th_slot():
    name, r, *_ = _BY_NAME["B/empty_at_slots_63_64"]
    a, b = se.info(name)["empties"]
    sp = se.split(r, 0)
    g = int(np.flatnonzero((sp["r_begin"] <= a) & (a < sp["r_end"]))[0])
    assert (a - sp["r_begin"][g], b - sp["r_begin"][g]) == (se.WAVE - 1, se.WAVE) and sp["r_end"][g] > b + 1      # last of one batch, first of the next
    nw = _n_words(r)
    assert nw[a] == 0 and nw[b] == 0 and nw[a - 1] == 1 and nw[b + 1] == 1
    assert (int(r.flag[a]), int(r.flag[b])) == (se.F_UNMAP, 0)                            # unmapped, and mapped with an empty CIGAR
    assert int(_scan(name)["ref_end"][a]) == int(r.pos[a]) + 1 and int(_scan(name)["ref_end"][b]) == int(r.pos[b]) + 1


def test_b_run_of_empty_reads_goes_to_one_wave():
    name, r, *_ = _BY_NAME["B/run_of_70_empty"]
    a, b = se.info(name)["run"]
    assert b - a == 70 and (_n_words(r)[a:b] == 0).all() and _n_words(r)[a - 1] == 1 and _n_words(r)[b] == 1
    sp = se.split(r, 0)
    g = np.flatnonzero((sp["r_begin"] <= a) & (a < sp["r_end"]))
    assert len(g) == 1 and sp["r_end"][g[0]] >= b and sp["reads_per_wave"][g[0]] > se.WAVE
    assert {int(f) for f in r.flag[a:b]} == {0, se.F_UNMAP}


# ------------------------------------------------------------------------------------------------------------------- R
def test_r_streams_of_every_length_and_start():
    pieces32, pieces16, tails = set(), set(), set()
    for n in se.R_SINGLE:
        name, r, *_ = _BY_NAME["R/single_%d" % n]
        assert r.n_reads == 1 and r.n_cigar == n
        sp = se.split(r, 0)
        assert sp["reads_per_wave"].tolist() == [1, 0, 0, 0] and (sp["w_begin"][0], sp["w_end"][0]) == (0, n)
        p32, p16 = se.ring_pieces(sp, se.CHUNK_WORDS), se.ring_pieces(sp, se.PIECE_OPS)
        assert p32.tolist() == [-(-n // 256), 0, 0, 0] and p16.tolist() == [-(-n // 512), 0, 0, 0]
        pieces32.add(int(p32[0])); pieces16.add(int(p16[0])); tails.add(n % se.CHUNK_WORDS)
        # signature-sized ops in the first and last word of every chunk, and they come out
        words = {e[4] for e in _scan(name)["emitted"]}
        edge = {k for k in range(n) if k % se.CHUNK_WORDS in (0, se.CHUNK_WORDS - 1)} | {0, n - 1}
        assert words == edge, name
    # 1 .. RING_D + 2 pieces at both widths: the prologue alone (< RING_D), the first top-up (RING_D), steady waits and the drain
    assert set(range(1, se.RING_D + 3)) <= pieces32 and set(range(1, se.RING_D + 3)) <= pieces16
    assert tails >= {0, 1, se.CHUNK_WORDS - 1}                                            # the array ends on a chunk (all LDS-DMA) or past it (register path)
    res32, res16, j0_odd = set(), set(), False
    for name, want_off in se.R_STARTS.items():
        _, r, *_ = _BY_NAME[name]
        assert tuple(r.cigar_off.tolist()) == want_off
        sp = se.split(r, 0)
        assert sp["reads_per_wave"].tolist() == [1, 1, 1, 1]                              # a read per wave: every stream but the first starts mid-chunk
        res32 |= {int(w) % se.CHUNK_WORDS for w in sp["w_begin"][1:]}
        res16 |= {int(w) % se.PIECE_OPS for w in sp["w_begin"][1:]}
        j0_odd |= any((int(w) % se.PIECE_OPS) >= se.CHUNK_WORDS for w in sp["w_begin"][1:])
        assert (se.ring_pieces(sp, se.PIECE_OPS) >= 2).all()                              # ... and is counted in pieces
    assert {1, se.CHUNK_WORDS - 1} <= res32 and {255, 256, 257, 511} <= res16 and j0_odd
    name, r, *_ = _BY_NAME["R/three_reads_one_chunk"]
    sp = se.split(r, 0)
    assert sp["reads_per_wave"].tolist()[:2] == [2, 1] and int(r.cigar_off[3]) <= se.CHUNK_WORDS      # reads 0, 1, 2 in chunk 0, waves 0 and 1
    assert sp["w_begin"][1] % se.CHUNK_WORDS != 0


def test_r_cases_pack():
    for name, r, *_ in _family("R"):
        assert se.n_escapes(r) == 0 and int((r.cigar >> 4).max()) < se.ESC_LEN and se.packs(r), name


# ------------------------------------------------------------------------------------------------------------------- W
def test_w_split_targets_and_idle_waves():
    name, r, *_ = _BY_NAME["W/empty_run_on_target"]
    sp = se.split(r, 0)
    off, nw = r.cigar_off.astype(np.int64), _n_words(r)
    hit = [g for g in range(sp["n_waves"]) if sp["reads_per_wave"][g] and nw[sp["r_begin"][g]] == 0 and off[sp["r_begin"][g]] == g * sp["share"]]
    assert hit                                                                            # a run of empty reads lies on a split target ...
    for g in hit:
        rb = int(sp["r_begin"][g])
        run = rb
        while nw[run] == 0:
            run += 1
        assert sp["r_end"][g] > run and (rb == 0 or nw[rb - 1] > 0)                        # ... and the wave takes the whole run and the read behind it
    assert any(int(sp["r_end"][g]) - int(sp["r_begin"][g]) >= 4 for g in hit)
    name, r, *_ = _BY_NAME["W/trailing_empty"]
    for form in se.FORMS:
        sp = se.split(r, form)
        assert (_n_words(r)[-3:] == 0).all() and sp["r_begin"][-1] <= r.n_reads - 3 and sp["r_end"][-1] == r.n_reads      # the last wave takes them
    name, r, *_ = _BY_NAME["W/all_empty"]
    assert r.n_reads == 200 and r.n_cigar == 0
    for form in se.FORMS:
        sp = se.split(r, form)
        assert sp["share"] == 0 and sp["reads_per_wave"].tolist() == [0] * (sp["n_waves"] - 1) + [200]
    assert se.split(r, 0)["n_waves"] == 200                                               # 199 idle waves, one with four batches
    name, r, *_ = _BY_NAME["W/lopsided"]
    assert r.n_reads == 5 and _n_words(r).max() >= 0.99 * r.n_cigar
    sp = se.split(r, 0)
    assert sp["n_waves"] == 8 and int((sp["reads_per_wave"] == 0).sum()) >= 5
    em = _scan(name)["emitted"]
    assert {e[2] for e in em} == {0, 1, 4}                                                # the duplicate and the mapq 19 read are filtered
    assert sorted(int(np.diff(_BY_NAME["W/one_word_reads_%d" % n][1].cigar_off.astype(np.int64)).sum()) for n in se.W_ONE_WORD_READS) == [1, 4, 5, 257]
    assert [se.split(_BY_NAME["W/one_word_reads_%d" % n][1], 0)["grid"] for n in se.W_ONE_WORD_READS] == [1, 1, 2, 65]
    sp = se.split(_BY_NAME["W/one_word_reads_1"][1], 0)
    assert sp["reads_per_wave"].tolist() == [1, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------------------- L
def test_l_batches_by_the_fits_rule():
    b = se.lane_batches(_BY_NAME["L/full_batch"][1])
    assert b == [[(64 * g, 64, False)] for g in range(4)]                                 # 3072 words: one full batch per wave
    b = se.lane_batches(_BY_NAME["L/batch_cut_at_63"][1])
    assert b[0] == [(0, 63, False), (63, 1, False)]                                       # one word more: cut at 63
    b = se.lane_batches(_BY_NAME["L/stage_sized_aligned"][1])
    assert b[0] == [(0, 1, False), (1, 1, False)] and int(_BY_NAME["L/stage_sized_aligned"][1].cigar_off[1]) % 4 == 0
    b = se.lane_batches(_BY_NAME["L/stage_sized_unaligned"][1])
    assert b[0] == [(0, 1, False), (1, 1, True)] and int(_BY_NAME["L/stage_sized_unaligned"][1].cigar_off[1]) % 4 == 1
    for big in se.L_BIG:
        name, r, *_ = _BY_NAME["L/direct_%d" % big]
        flat = [x for w in se.lane_batches(r) for x in w]
        direct = [x[0] for x in flat if x[2]]
        assert direct == [0, r.n_reads // 2, r.n_reads - 1]                               # the first, a middle and the last read
        assert all(x[1] == 1 for x in flat if x[2]) and any(x[1] > 1 for x in flat if not x[2])
        words = {e[4] for e in _scan(name)["emitted"]}
        off = r.cigar_off.astype(np.int64)
        assert all(int(off[d + 1]) - 1 in words for d in direct)                          # a signature in the last word of a direct read
    name, r, *_ = _BY_NAME["L/full_batch"]
    assert {e[4] for e in _scan(name)["emitted"]} >= {se.LN_STAGE * g + se.LN_STAGE - 1 for g in range(4)}      # ... and in the last word of the stage
