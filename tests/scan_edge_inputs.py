"""Directed inputs for the CIGAR scan (kernels/scan.hip: the wave form at 32 and at 16 bits, the row forms, the lane form, and the split
table of resident shards), and a plain model of what those kernels DECIDE — which reads a wave owns, where its load stream starts and how
many ring pieces it has, how many signatures a workgroup emits and which of them no longer fit its staging buffer, which reads a lane-form
batch takes — so that tests/test_scan_edge_inputs.py can prove, without a GPU, that every case reaches the seam it is named after, and
tests/test_gpu_scan_edges.py can run the kernels on them against the oracle. numpy only; nothing here models HOW the kernels search.

Each case is (name, Reads, depth_len, min_oplen, min_mapq). Families:
  S  signature staging (SIG_BUF per workgroup, the overflow branch's bucket counts)      B  more than 64 reads in one wave
  R  the wave form's LDS ring (pieces per stream, where a stream starts, the array's end)  W  the work split
  L  the lane form's stage (LN_STAGE words per batch, the direct walk)

The split formulas below are scan_grid's only while the grid stays under its device cap (two rounds of resident workgroups): every case
has at most 1024 reads, so the wave form asks for at most 256 workgroups and the short-read forms for at most 8 — under the cap of any
device with 22 compute units or more. The context does not tell its compute-unit count, so the GPU test cannot skip by it and does not.

Positions: every case's reads start at a base of its own, POS_STEP apart from the previous case's, so a read the kernel skipped cannot
pass on the output an earlier case left in the reused arena. Every coordinate is far below 2^31.

What the entry points turn away by design: nothing of what these families need. A shard whose reads are all empty has n_cigar == 0 and a
word array of no elements; check_reads asks for a word pointer only when n_cigar != 0, and the oracle never dereferences it, so the
all-empty shard of family W goes through both entries as it is."""
import numpy as np

from contextsv_amd import Reads

M, I, D, N, S, H, P, EQ, X = range(9)

# ---- the kernels' constants (tests/test_scan_edge_inputs.py reads them back from the sources) -----------------------------------------
WAVE = 64
SCAN_WAVES = 4                       # waves per workgroup, every form
SIG_BUF = 512                        # signatures staged per workgroup
RING_D = 4                           # ring slots per wave
CHUNK_WORDS = 256                    # words per visit of the wave form; a ring piece at 32 bits
PIECE_OPS = 512                      # cigar_pack_core: ops per ring piece at 16 bits
LN_STAGE = 3072                      # words a lane-form batch can stage
LN_READS_PER_WAVE = 128              # scan_grid: reads a lane-form wave wants
RS_MIN_READS = 32                    # ... a row-form wave
BK_BITS = 14
BK_LOCAL_MAX = 2048                  # a bucket above this sends the ordering pass to the radix path
ESC_LEN = 0xFFF                      # lengths from here on are escapes of the 16-bit form
MAX_ESC_DENOM = 64

FORMS = (0, 1, 2, 3)                 # wave, rows16, rows8, lanes
FORM_NAMES = ("wave", "rows16", "rows8", "lanes")
READS_PER_WG = {0: SCAN_WAVES, 1: SCAN_WAVES * RS_MIN_READS, 2: SCAN_WAVES * RS_MIN_READS, 3: SCAN_WAVES * LN_READS_PER_WAVE}
MAX_READS = 1024
POS_STEP = 1500

F_UNMAP, F_SECONDARY, F_QCFAIL, F_DUP, F_SUPP = 0x4, 0x100, 0x200, 0x400, 0x800
SCAN_FILTER = F_SECONDARY | F_UNMAP | F_DUP | F_QCFAIL | F_SUPP
KIND_INS, KIND_DEL, KIND_CLIP = 0, 1, 2
_REF_OPS = (M, D, N, EQ, X)
_QRY_OPS = (M, I, S, EQ, X)
_QST_OPS = (M, I, EQ, X)
_M32 = 0xffffffff


# ======================================================================================================================= the model
def np_scan(reads, depth_len, min_oplen, min_mapq):
    """The reference's loop, op by op (findCIGARSVs / processCIGARRecord, getAlignmentReadPositions, bam_endpos): a second reference beside
    the oracle. -> dict(sig: set of (start, end, read, qpos_kind); emitted: the same as a list in op order with the op's word index as a
    fifth field; ref_end, q_start, q_end: int64 arrays holding the int32 values)."""
    off = reads.cigar_off.astype(np.int64)
    n = reads.n_reads
    emitted = []
    ref_end, q_start, q_end = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
    cig = reads.cigar.tolist()
    for r in range(n):
        fl = int(reads.flag[r])
        emit_ok = not (fl & SCAN_FILTER) and int(reads.mapq[r]) >= min_mapq
        pos = int(reads.pos[r]) & _M32                 # the signatures' cursor, in uint32
        qpos = 0                                       # ... their query cursor: a skipped clip does not move it
        qs, qe, rlen = -1, 0, 0                        # the intervals' cursors: every op moves them
        for i in range(int(off[r]), int(off[r + 1])):
            op, ln = cig[i] & 15, cig[i] >> 4
            if qs < 0 and op in _QST_OPS:
                qs = qe
            if op in _QRY_OPS:
                qe += ln
            if op in _REF_OPS:
                rlen += ln
            if emit_ok and ln >= min_oplen and op in (I, S, D):
                start = (pos + 1) & _M32
                if op == S and start >= depth_len:
                    continue                           # at or beyond the contig's end: no call, and neither cursor moves
                end = (start + ln - 1) & _M32
                if start <= end:                       # addSVCall turns start > end away
                    kind = KIND_INS if op == I else (KIND_DEL if op == D else KIND_CLIP)
                    emitted.append((start, end, r, ((qpos << 2) & _M32) | kind, i))
            if op in _REF_OPS:
                pos = (pos + ln) & _M32
            if op in _QRY_OPS:
                qpos = (qpos + ln) & _M32
        if fl & F_UNMAP:
            rlen = 0
        ref_end[r] = int(reads.pos[r]) + (rlen if rlen else 1)
        q_start[r] = qs if qs >= 0 else 0
        q_end[r] = qe
    return dict(sig={e[:4] for e in emitted}, emitted=emitted, ref_end=ref_end, q_start=q_start, q_end=q_end)


def grid_of(n_reads, form):
    """scan_grid below its device cap"""
    return -(-n_reads // READS_PER_WG[form])


def split(reads, form):
    """The work split of `form`: wave g owns the reads [r_begin[g], r_end[g]) whose first word falls into its share of the word array,
    lb(t) being the first r in [0, n_reads] with cigar_off[r] >= t, and the last wave owns up to n_reads. w_begin / w_end: cigar_off at
    the two (what scan_split_kernel's table holds beside them), wg: the wave's workgroup."""
    off = reads.cigar_off.astype(np.int64)
    n, m = reads.n_reads, reads.n_cigar
    assert 1 <= n <= MAX_READS
    grid = grid_of(n, form)
    n_waves = SCAN_WAVES * grid
    share = -(-m // n_waves)
    g = np.arange(n_waves + 1, dtype=np.int64)
    b = np.searchsorted(off, g * share, side="left")           # lb over [0, n_reads] (off has n + 1 entries, the last is >= every target but ...)
    b = np.minimum(b, n)
    b[n_waves] = n                                             # ... the last wave's end is n_reads whatever the offsets say
    return dict(grid=grid, n_waves=n_waves, share=share, r_begin=b[:-1], r_end=b[1:], w_begin=off[b[:-1]], w_end=off[b[1:]],
                wg=g[:-1] // SCAN_WAVES, reads_per_wave=b[1:] - b[:-1])


def ring_pieces(sp, piece):
    """pieces of `piece` ops in every wave's load stream: it starts at w_begin rounded down to a piece and ends at w_end; 0 for a wave
    that owns no read"""
    base = sp["w_begin"] & ~np.int64(piece - 1)
    return np.where(sp["reads_per_wave"] > 0, (sp["w_end"] - base + piece - 1) // piece, 0)


def sigs_per_workgroup(reads, form, emitted):
    sp = split(reads, form)
    per_read = np.bincount([e[2] for e in emitted], minlength=reads.n_reads) if emitted else np.zeros(reads.n_reads, np.int64)
    cs = np.concatenate(([0], np.cumsum(per_read)))
    per_wave = cs[sp["r_end"]] - cs[sp["r_begin"]]
    return np.bincount(sp["wg"], weights=per_wave, minlength=sp["grid"]).astype(np.int64)


def lane_batches(reads):
    """The lane form's batches, per wave: [(first read, reads taken, direct)]. A batch takes the leading run of a wave's next (up to 64)
    reads that end within LN_STAGE words of the first one's first word rounded down to 16 bytes; when not even the first one does, that
    read alone is walked straight from global memory."""
    off = reads.cigar_off.astype(np.int64)
    sp = split(reads, 3)
    out = []
    for g in range(sp["n_waves"]):
        rb, r_end, mine = int(sp["r_begin"][g]), int(sp["r_end"][g]), []
        while rb < r_end:
            avail = min(WAVE, r_end - rb)
            base = int(off[rb]) & ~3
            nb = 0
            while nb < avail and int(off[rb + nb + 1]) - base <= LN_STAGE:
                nb += 1
            direct = nb == 0
            nb = max(nb, 1)
            mine.append((rb, nb, direct))
            rb += nb
        out.append(mine)
    return out


def emission_steps(reads, r, form):
    """The word ranges of read r in the order a form works through them; the signatures of one step reserve their slots together, in no
    order the model relies on: 256-word chunks of the array (wave), 64-word windows from the read's first word rounded down to 4 (rows),
    single ops (lanes)."""
    c0, c1 = int(reads.cigar_off[r]), int(reads.cigar_off[r + 1])
    if form == 3:
        return [(i, i + 1) for i in range(c0, c1)]
    step, a = (CHUNK_WORDS, c0 & ~(CHUNK_WORDS - 1)) if form == 0 else (64, c0 & ~3)
    return [(max(x, c0), min(x + step, c1)) for x in range(a, c1, step)]


def staging_of_single_read(reads, form, emitted):
    """A shard of one read (one wave, one workgroup): -> (staged, overflow, certain). The first SIG_BUF signatures in emission order are
    staged in LDS, the rest go straight to HBM through the overflow branch; `certain`: the buffer fills exactly at the end of a step, so
    that which signatures overflow does not depend on the order inside one."""
    assert reads.n_reads == 1
    by_word = {e[4]: e for e in emitted}
    staged, overflow, certain = [], [], True
    for a, b in emission_steps(reads, 0, form):
        here = [by_word[i] for i in range(a, b) if i in by_word]
        room = max(0, SIG_BUF - len(staged) - len(overflow))       # (a slot is the count of everything emitted before)
        if 0 < room < len(here):
            certain = False
        staged.extend(here[:room])
        overflow.extend(here[room:])
    return staged, overflow, certain


def key_layout(depth_len, with_type):
    """api/reads.hip key_layout without the overflow flag -> (type_pos, bucket_shift)"""
    limit_bits = max(int(depth_len).bit_length(), 8)           # scan_start_limit = 1 << this (below 2^32)
    start_bits = max(1, limit_bits)
    key_bits = start_bits + (1 if with_type else 0)
    return (start_bits if with_type else -1), max(0, key_bits - BK_BITS)


def bucket_counts(sigs, depth_len, with_type):
    """bk_bucket over a list of signatures -> {bucket: count}"""
    type_pos, shift = key_layout(depth_len, with_type)
    out = {}
    for e in sigs:
        k = e[0]
        if type_pos >= 0 and (e[3] & 3) != KIND_DEL:
            k |= 1 << type_pos
        b = min(k >> shift, (1 << BK_BITS) - 1)
        out[b] = out.get(b, 0) + 1
    return out


def n_escapes(reads):
    return int(np.count_nonzero((reads.cigar >> 4) >= ESC_LEN))


def packs(reads):
    return reads.n_cigar > 0 and n_escapes(reads) * MAX_ESC_DENOM <= reads.n_cigar


# ======================================================================================================================= builders
_cases, _info = [], {}


def _add(name, cigs, flags=None, mapqs=None, min_oplen=50, min_mapq=20, depth_len=None, pos_step=1, **info):
    """One case: reads from op lists, positions growing by pos_step from the case's own base."""
    k = len(_cases)
    n = len(cigs)
    assert 1 <= n <= MAX_READS and name not in _info, name
    pos = POS_STEP * (k + 1) + pos_step * np.arange(n, dtype=np.int64)
    r = Reads.from_cigar_lists(pos.astype(np.int32), np.asarray(flags if flags is not None else [0] * n, np.uint16),
                               np.asarray(mapqs if mapqs is not None else [60] * n, np.uint8), cigs)
    if depth_len is None:
        ref = sum(ln for c in cigs for op, ln in c if op in _REF_OPS)
        depth_len = int(pos[-1]) + ref + 64
    info["pos_base"] = int(pos[0])
    _info[name] = info
    _cases.append((name, r, int(depth_len), min_oplen, min_mapq))


def _sig_op(k, salt, period):
    """the k-th signature-sized op of a read: mostly D 60, an I 60 every `period`-th, one S 60"""
    if k == 5:
        return (S, 60)
    return (I, 60) if (k + salt) % period == 0 else (D, 60)


def _pairs(n_sig, salt=0, period=3):
    """n_sig pairs M 10 / <signature-sized op>"""
    return [op for k in range(n_sig) for op in ((M, 10), _sig_op(k, salt, period))]


def _filler(n, mark_chunks_from=None):
    """n words no form emits at min_oplen 50: M 7 / I 1 / M 5 / D 2 ...; mark_chunks_from = c0: the words that are the first or the last of
    a 256-word chunk of the array (the read starting at word c0), and the read's own first and last, become D 60 / I 60 alternately"""
    ops = [((M, 7), (I, 1), (M, 5), (D, 2))[k % 4] for k in range(n)]
    if mark_chunks_from is not None and n:
        marks = sorted({0, n - 1} | {k for k in range(n) if (mark_chunks_from + k) % CHUNK_WORDS in (0, CHUNK_WORDS - 1)})
        for j, k in enumerate(marks):
            ops[k] = (D, 60) if j % 2 == 0 else (I, 60)
    return ops


def _marked_reads(lengths):
    """reads of these lengths, laid out one behind the other, each marked at its ends and at the array's chunk edges"""
    out, c0 = [], 0
    for n in lengths:
        out.append(_filler(n, c0))
        c0 += n
    return out


# ------------------------------------------------------------------------------------------------------------------- S
S_COUNT_LAST = (127, 128, 129)
S_DENSE_READS, S_DENSE_WORDS, S_DENSE_SIGS = 8, 600, 300
S_BUCKET_EXTRA = 50


def _s_cases():
    for j, last in enumerate(S_COUNT_LAST):
        _add("S/count_%d" % (3 * 128 + last), [_pairs(128, salt=r, period=3 + j) for r in range(3)] + [_pairs(last, salt=3, period=3 + j)],
             family="S", total=3 * 128 + last)
    # the dense shard: 300 signature-sized ops among 600 words; a few short gaps so that min_oplen 1 sees more of them. Its last read ends
    # in a soft clip at the contig's end (the reference's `continue`), behind an S 60 that is not at the end
    dense = []
    for r in range(S_DENSE_READS):
        ops = _pairs(S_DENSE_SIGS, salt=r, period=4)
        for k in range(0, 40 + 4 * r, 4):
            ops[2 * k] = (D, 3) if k % 8 == 0 else (I, 2)
        dense.append(ops)
    dense[-1][-1] = (S, 60)
    ref_last = sum(ln for op, ln in dense[-1] if op in _REF_OPS)
    k = len(_cases)
    end_last = (S_DENSE_READS - 1) + ref_last + 1                            # the trailing clip's start (pos + 1), relative to the case's base
    _add("S/dense_oplen50", dense, depth_len=POS_STEP * (k + 1) + end_last, family="S", clip_at_end=True)
    _add("S/dense_oplen1", dense, min_oplen=1, depth_len=POS_STEP * (k + 2) + end_last, family="S", clip_at_end=True)
    # the bucket cases: SIG_BUF staged deletions spread over the buckets, then insertions at ONE reference position, which only the overflow
    # branch counts: BK_LOCAL_MAX + 50 of them (the radix path is required) and exactly BK_LOCAL_MAX (the bucket path still is)
    # Behind them a few more signatures in HIGHER buckets, also through the overflow branch: with the insertions' bucket count missing, the
    # bucket path would put these where the insertions belong (were the insertions' bucket the last one in use, a missing count would
    # leave the order right by accident: the last bucket's end is the signature count, not a sum of counts)
    for name, n_ins in (("S/bucket_over", BK_LOCAL_MAX + S_BUCKET_EXTRA), ("S/bucket_at", BK_LOCAL_MAX)):
        tail = [(M, 30), (D, 80), (M, 5), (S, 60)] if n_ins > BK_LOCAL_MAX else [(M, 30), (D, 70), (M, 40), (D, 71), (M, 5), (S, 60)]
        ops = [op for _ in range(SIG_BUF) for op in ((M, 10), (D, 60))] + [(I, 60)] * n_ins + tail
        _add(name, [ops], family="S", n_ins_at_one_position=n_ins)


# ------------------------------------------------------------------------------------------------------------------- B
# (G, K): one read of G words and K one-word reads — 256 reads, 256 waves of the wave form, share = ceil((G + K) / 256)
B_FRONT = {64: (16128, 255), 65: (16385, 255), 128: (32512, 255), 129: (32637, 255)}
B_MIRROR_190 = (38500, 200)                                                   # 201 reads, 204 waves, share 190: the first wave owns 190 reads


def _tiny(k, with_sig):
    return [(D, 60)] if with_sig else [((M, 9), (EQ, 4), (X, 2), (I, 3))[k % 4]]


def _b_cases():
    for want, (G, K) in B_FRONT.items():
        big = _filler(G, 0)
        _add("B/front_%d" % want, [big] + [_tiny(k, False) for k in range(K)], family="B", want=want)
        _add("B/mirror_%d" % want, [_tiny(k, False) for k in range(K)] + [_filler(G, K)], family="B", want=None)
    G, K = B_MIRROR_190
    _add("B/mirror_190", [_tiny(k, k % 7 == 0) for k in range(K)] + [_filler(G, K)], family="B", want=190)
    # every tiny read carries a signature: signatures from every batch of a wave
    G, K = B_FRONT[65]
    _add("B/front_65_sigs", [_filler(G, 0)] + [_tiny(k, True) for k in range(K)], family="B", want=65, sigs_every_batch=True)
    G, K = B_FRONT[129]
    _add("B/front_129_sigs", [_filler(G, 0)] + [_tiny(k, True) for k in range(K)], family="B", want=129, sigs_every_batch=True)
    # reads of no words at a batch's 64th and 65th slot: an unmapped one (flag 4) and a mapped one with an empty CIGAR. In B/front_65 the
    # wave that owns the words from 65 * 253 on starts at read 61, so its slots 63 and 64 are reads 124 and 125
    G, K = B_FRONT[65]
    cigs = [_filler(G, 0)] + [_tiny(k, True) for k in range(K)]
    flags = [0] * (K + 1)
    cigs[124], cigs[125], flags[124] = [], [], F_UNMAP
    _add("B/empty_at_slots_63_64", cigs, flags=flags, family="B", want=None, empties=(124, 125))
    # 70 reads of no words in mid-shard: they share one offset, so one wave takes the whole run
    cigs = [_filler(G, 0)] + [_tiny(k, True) for k in range(100)] + [[] for _ in range(70)] + [_tiny(k, True) for k in range(K - 170)]
    flags = [0] * len(cigs)
    for r in range(101, 171, 3):
        flags[r] = F_UNMAP
    _add("B/run_of_70_empty", cigs, flags=flags, family="B", want=None, run=(101, 171))


# ------------------------------------------------------------------------------------------------------------------- R
R_SINGLE = (1, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 1279, 1280, 1281, 2047, 2048, 2049, 2561, 3072, 3073)
# (2047 .. 3073: nine chunks at 32 bits are only five pieces at 16; these reach RING_D + 2 pieces there too)
# four reads, one per wave (offsets chosen against share = ceil(n / 4)): first words at these residues
R_STARTS = {"R/starts_a": (0, 1023, 2303, 3328, 4092), "R/starts_b": (0, 1281, 2815, 3841, 5120)}
R_SHARED = (60, 60, 120, 240)                                                 # three reads in chunk 0, owned by two waves


def _r_cases():
    for n in R_SINGLE:
        _add("R/single_%d" % n, [_filler(n, 0)], family="R", n=n)
    for name, off in R_STARTS.items():
        _add(name, _marked_reads(np.diff(off).tolist()), family="R", offsets=off)
    _add("R/three_reads_one_chunk", _marked_reads(R_SHARED), family="R")


# ------------------------------------------------------------------------------------------------------------------- W
W_ON_TARGET = (8, 0, 0, 0, 8, 8, 24, 0, 8, 8, 8, 8, 24, 8, 8, 8)            # 16 reads, 128 words, 16 waves of the wave form: share 8
W_TRAILING = (5, 5, 5, 0, 0, 0)
W_LOPSIDED = (2, 1000, 2, 3, 3)
W_ONE_WORD_READS = (1, 4, 5, 257)


def _w_cases():
    _add("W/empty_run_on_target", _marked_reads(W_ON_TARGET), family="W")
    _add("W/trailing_empty", _marked_reads(W_TRAILING), flags=[0, 0, 0, 0, F_UNMAP, 0], family="W")
    _add("W/all_empty", [[] for _ in range(200)], flags=[F_UNMAP if r % 3 == 0 else 0 for r in range(200)], family="W")
    # one read holds 99 % of the words; a duplicate and a low-mapq read whose D 60 must not come out
    _add("W/lopsided", _marked_reads(W_LOPSIDED), flags=[0, 0, F_DUP, 0, 0], mapqs=[60, 60, 60, 19, 20], family="W")
    for n in W_ONE_WORD_READS:
        _add("W/one_word_reads_%d" % n, [_tiny(k, k % 5 == 0) for k in range(n)], family="W", n=n)


# ------------------------------------------------------------------------------------------------------------------- L
L_PER_READ = 48                                                               # 64 reads of 48 words fill the stage exactly
L_BIG = (3073, 10000)
L_SHORT = (10, 30)                                                            # reads between the long ones: how many, how long


def _l_cases():
    n = SCAN_WAVES * WAVE                                                     # 256 reads: one lane-form workgroup, 64 reads per wave
    _add("L/full_batch", _marked_reads([L_PER_READ] * n), family="L")
    lens = [L_PER_READ] * n
    lens[WAVE - 1] += 1                                                       # the first wave's 64th read ends one word behind the stage
    _add("L/batch_cut_at_63", _marked_reads(lens), family="L")
    _add("L/stage_sized_aligned", _marked_reads([4, LN_STAGE]), family="L", c0_mod4=0)
    _add("L/stage_sized_unaligned", _marked_reads([5, LN_STAGE]), family="L", c0_mod4=1)
    for big in L_BIG:
        k, w = L_SHORT
        _add("L/direct_%d" % big, _marked_reads([big] + [w] * k + [big] + [w] * k + [big]), family="L", big=big)


_s_cases(); _b_cases(); _r_cases(); _w_cases(); _l_cases()


def all_cases():
    return list(_cases)


def info(name):
    return _info[name]
