"""Directed inputs for the depth pass (kernels/depth.hip and the tile ranges kernels/scan.hip leaves for it), and a plain model of what
those kernels DECIDE — which reads are a tile's candidates, which (tile, read) pairs become work-list items and with which fields, which
words of an item's chunks are its own — so that tests/test_depth_edge_inputs.py can prove, without a GPU, that every case reaches the
edge it is named after, and tests/test_gpu_depth_edges.py can run the kernels on them against the oracle. numpy only; nothing here
models HOW the kernels search (probes, rings, lane groups), only the answers they must arrive at.

Families (each case is (name, Reads, depth_len); positions sorted, mapq 60, flag 0 unless the family says otherwise):
  A  tile and map edges          B  candidates / items per tile      C  checkpoint searches        D  the chunk stream
  E  in-tile against clipped     F  group-form windows               G  the write-out's `fast` threshold
  H  tile ranges of the short-read scans                              U  unsorted twins of A, B, C, D

Not reachable through any entry point, and therefore not here: a depth output that is not 16-byte aligned (dvec_ok == 0 in
depth_tile_kernel — the shard's map and the arena's are both aligned). Reads whose reference span wraps uint32 stay out by decision
(DESIGN.md); every coordinate below is far under 2^31."""
import numpy as np

from contextsv_amd import Reads

M, I, D, N, S, H, P, EQ, X = range(9)

# ---- the kernels' constants (tests/test_depth_edge_inputs.py reads them back from the sources) ----------------------------------------
DEPTH_TILE_SHIFT = 14
CKPT_SHIFT = 6
WL_CAP = 512
WL_SPEC = 256
DEPTH_PF = 5
DEPTH_THREADS = 1024
FAST_MAX_CANDIDATES = 1 << 20        # depth_tile_kernel: `fast` needs fewer candidates than this
TR_SLOTS = 64
WIDE_TILES = 8                       # a read with t1 - t0 >= 8 is marked by the whole wave
RS_MIN_READS = 32
RS_THREADS = 256

T = 1 << DEPTH_TILE_SHIFT
CKPT_WORDS = 1 << CKPT_SHIFT
CW = 256                             # words per chunk of the wave form: four per lane
NS = DEPTH_PF + 1                    # ring slots of the chunk stream
F_UNMAP, F_SECONDARY, F_QCFAIL, F_DUP = 0x4, 0x100, 0x200, 0x400
DEPTH_FILTER = F_UNMAP | F_SECONDARY | F_QCFAIL | F_DUP
_REF = np.zeros(16, bool); _REF[[M, D, N, EQ, X]] = True
_ALN = np.zeros(16, bool); _ALN[[M, EQ, X]] = True
_GAP = _REF & ~_ALN


# ======================================================================================================================= the model
def _words(reads):
    """per word: owning read, op, length, reference offset of the owning read in front of the word"""
    off = reads.cigar_off.astype(np.int64)
    n_w = np.diff(off)
    owner = np.repeat(np.arange(reads.n_reads, dtype=np.int64), n_w)
    op = (reads.cigar & 15).astype(np.int64)
    ln = (reads.cigar >> 4).astype(np.int64)
    rl = np.where(_REF[op], ln, 0)
    cs = np.concatenate(([0], np.cumsum(rl)))                     # cs[w]: reference bases of all words in front of word w
    before = cs[:-1] - cs[off[owner]] if len(owner) else np.zeros(0, np.int64)
    return owner, op, ln, rl, cs, before


def ref_len(reads):
    off = reads.cigar_off.astype(np.int64)
    cs = _words(reads)[4]
    return cs[off[1:]] - cs[off[:-1]]


def ref_end(reads):
    """scan.hip's ref_end: pos + reference length, a length of 0 (or an unmapped read) counting as 1 — htslib's bam_endpos, int32"""
    rlen = np.where(reads.flag.astype(np.int64) & F_UNMAP, 0, ref_len(reads))
    rlen = np.where(rlen == 0, 1, rlen)
    return ((reads.pos.astype(np.int64) + rlen) & 0xffffffff).astype(np.uint32).view(np.int32).astype(np.int64)


def p1_of(reads):
    """the 1-based first reference position, in uint32 as the reference computes it (pos -1 wraps to 0)"""
    return (reads.pos.astype(np.int64) + 1) & 0xffffffff


def np_depth(reads, depth_len):
    """Difference-array depth map, its sum and non-zero count, by the reference's rules as oracle/csv_oracle.c orc_depth states them:
    reads with an UNMAP / SECONDARY / QCFAIL / DUP flag do not count, the cursor starts at pos + 1 in uint32, every base of an M / = / X
    op counts, bases at or beyond depth_len are dropped."""
    owner, op, ln, rl, cs, before = _words(reads)
    keep = _ALN[op] & (ln > 0) & ((reads.flag.astype(np.int64)[owner] & DEPTH_FILTER) == 0)
    a = (p1_of(reads)[owner[keep]] + before[keep]) & 0xffffffff
    b = a + ln[keep]
    assert (b < (1 << 32)).all(), "a run that wraps uint32: out of this module's range by decision"
    a = np.minimum(a, depth_len); b = np.minimum(b, depth_len)
    diff = np.bincount(a, minlength=depth_len + 1).astype(np.int64) - np.bincount(b, minlength=depth_len + 1).astype(np.int64)
    depth = np.cumsum(diff[:depth_len]).astype(np.uint32)
    return depth, int(depth.astype(np.uint64).sum()), int(np.count_nonzero(depth))


def checkpoints(reads):
    """ckpt[g]: reference offset of the owning read at global word 64 g, for every boundary strictly inside a read (0 elsewhere) — what
    every form of the scan writes"""
    off = reads.cigar_off.astype(np.int64)
    owner, op, ln, rl, cs, before = _words(reads)
    ck = np.zeros((reads.n_cigar >> CKPT_SHIFT) + 2, np.int64)
    w = np.arange(CKPT_WORDS, reads.n_cigar, CKPT_WORDS, dtype=np.int64)
    inside = off[owner[w]] != w
    ck[w[inside] >> CKPT_SHIFT] = before[w[inside]]
    return ck


def n_tiles_of(depth_len):
    return (depth_len + T - 1) // T


def candidate_ranges(reads, depth_len, producer, range_end_shift=0):
    """-> (lo[t], hi[t], ord): tile t's candidates are ord[lo[t] : hi[t]] (ord None: the reads themselves).
    "pmax" (depth_ranges_kernel, reads in position order): from the first read whose prefix maximum of ref_end is >= T0 up to the first
    read with pos >= T1 - 1. "scan" (the scan's tile_range, coordinate-sorted shards): from the first to the last read that passes the
    depth filter, has a reference length above 0 and reaches the tile.
    range_end_shift: the "pmax" end taken at pos >= T1 - 1 - shift (the sensitivity test's flipped comparison)."""
    nt = n_tiles_of(depth_len)
    pos = reads.pos.astype(np.int64)
    t0s = np.arange(nt, dtype=np.int64) * T
    t1s = np.minimum(t0s + T, depth_len)
    if producer == "pmax":
        order = None
        end = ref_end(reads)
        if (np.diff(pos) < 0).any():
            order = np.argsort(pos, kind="stable")
            pos, end = pos[order], end[order]
        pm = np.maximum.accumulate(end) if len(end) else end
        lo = np.searchsorted(pm, t0s, side="left")
        hi = np.searchsorted(pos, t1s - 1 - range_end_shift, side="left")
        return lo, np.maximum(lo, hi), order
    assert producer == "scan" and not (np.diff(pos) < 0).any()
    rl = ref_len(reads)
    first = p1_of(reads)
    last = (first + rl - 1) & 0xffffffff
    ok = ((reads.flag.astype(np.int64) & DEPTH_FILTER) == 0) & (rl != 0) & ((first >> DEPTH_TILE_SHIFT) < nt) & (last >= first)
    big = np.int64(1) << 62
    lo = np.full(nt, big, np.int64); hi = np.zeros(nt, np.int64)
    idx = np.flatnonzero(ok)
    a, b = first[idx] >> DEPTH_TILE_SHIFT, np.minimum(last[idx] >> DEPTH_TILE_SHIFT, nt - 1)
    np.minimum.at(lo, a, idx)                                      # (the first tile of every read; the others below)
    np.maximum.at(hi, a, idx + 1)
    for r, ta, tb in zip(idx[b > a], a[b > a], b[b > a]):
        lo[ta:tb + 1] = np.minimum(lo[ta:tb + 1], r)
        hi[ta:tb + 1] = np.maximum(hi[ta:tb + 1], r + 1)
    lo = np.where(lo == big, 0, lo)
    return lo, np.maximum(lo, hi), None


def _f32_guess(d, nb, rlen):
    """depth_make_item's interpolated boundary for a target d positions right of the read's start, in float32 as the kernel computes it"""
    per_pos = np.float32(nb) / np.float32(rlen if rlen else 1)
    return int(min(max(1 + int(np.float32(d & 0xffffffff) * per_pos), 1), nb))


def probes(guess, nb, NP):
    """the NP boundaries depth_make_item<NP> looks at around a guess (clamped into [1, nb])"""
    return [min(max(guess + i, 1 + (NP // 2 - 1)) - (NP // 2 - 1), nb) for i in range(NP)]


def _bracket_open(answer, guess, nb, NP):
    """True when the NP probes leave the bracket open (the bisection loop has to run): answer = the first boundary that fails the test"""
    lo, hi = 1, nb + 1
    for q in probes(guess, nb, NP):
        if q < answer:
            lo = max(lo, q + 1)
        else:
            hi = min(hi, q)
    return lo < hi


def tile_items(reads, depth_len, ranges, t0_slack=0, t1_strict=False):
    """Every (tile, candidate) pair as a dict: tile, read, item (bool) and why not ("filtered", "right_of_tile"), and for items nb, lo,
    e_lo, c0rel, nrem, n_chunks, start, chunk (first word of the walk), want0 / want1, on_T0 / on_T1m1 / on_T1 (a checkpoint of the read
    exactly there), gs0 / gs1 and miss0 / miss1 = {3: bool, 8: bool} (the probes of depth_make_item<NP> leave that search open).
    t0_slack / t1_strict: the two checkpoint comparisons off by one (the sensitivity test's flipped variants)."""
    lo_t, hi_t, order = ranges
    off = reads.cigar_off.astype(np.int64)
    fl = reads.flag.astype(np.int64)
    end, p1s, ck = ref_end(reads), p1_of(reads), checkpoints(reads)
    out = []
    for t in range(n_tiles_of(depth_len)):
        T0 = t * T
        T1 = min(T0 + T, depth_len)
        X1 = T1 - 1
        for k in range(int(lo_t[t]), int(hi_t[t])):
            r = int(order[k]) if order is not None else k
            c0, c1, p1, r_end = int(off[r]), int(off[r + 1]), int(p1s[r]), int(end[r])
            rec = dict(tile=t, read=r, item=False, why=None)
            out.append(rec)
            if not (r_end >= T0 and not (fl[r] & DEPTH_FILTER) and c1 > c0):
                rec["why"] = "filtered"
                continue
            g0 = c0 >> CKPT_SHIFT
            nb = ((c1 - 1) >> CKPT_SHIFT) - g0
            ckr = ck[g0:g0 + nb + 1]                                   # ckr[1 .. nb]
            at = p1 + ckr[1:]
            want0 = nb > 0 and p1 <= T0
            want1 = nb > 0 and p1 <= X1 and r_end >= T1
            lo = 1 + int(np.count_nonzero(at <= T0 + t0_slack)) if nb else 1
            if want1:
                e_lo = 1 + int(np.count_nonzero(at < X1 if t1_strict else at <= X1))
            else:
                e_lo = nb + 1 if p1 <= X1 else 1
            chunk, carry = c0 & ~(CKPT_WORDS - 1), 0
            if lo > 1:
                chunk, carry = (g0 + lo - 1) << CKPT_SHIFT, int(ckr[lo - 1])
            rec.update(nb=nb, lo=lo, e_lo=e_lo, want0=want0, want1=want1, on_T0=bool((at == T0).any()), on_T1m1=bool((at == X1).any()),
                       on_T1=bool((at == T1).any()))
            if not (p1 + carry < T1):
                rec["why"] = "right_of_tile"
                continue
            b0 = lo - 1 if lo > 1 else 0
            nrem = c1 - chunk
            if e_lo <= nb:
                nrem = min(nrem, (e_lo - b0) << CKPT_SHIFT)
            rlen = (r_end - p1 + 1) & 0xffffffff
            gs0 = _f32_guess(T0 - p1, nb, rlen) if want0 else 0
            gs1 = _f32_guess(X1 - p1, nb, rlen) if want1 else 0
            rec.update(item=True, chunk=chunk, c0rel=c0 - chunk if c0 > chunk else 0, nrem=nrem, n_chunks=(nrem + CW - 1) // CW,
                       start=p1 - T0 + carry, gs0=gs0, gs1=gs1,
                       miss0={NP: bool(want0 and _bracket_open(lo, gs0, nb, NP)) for NP in (3, 8)},
                       miss1={NP: bool(want1 and _bracket_open(e_lo, gs1, nb, NP)) for NP in (3, 8)})
    return out


def item_chunks(reads, item, depth_len, unmasked=False):
    """The wave form's chunks of one item: (base_rel, total, n_gap_words, all_zero_length) per 256-word chunk — total is what the chunk's
    own words add to the reference cursor, base_rel the cursor (relative to the tile) at its first word.
    unmasked: the neighbouring reads' words in the first and last chunk count too (the sensitivity test's flipped mask)."""
    owner, op, ln, rl, cs, before = _words(reads)
    res, base = [], item["start"]
    for j in range(item["n_chunks"]):
        a = item["chunk"] + j * CW
        w = np.arange(a, min(a + CW, reads.n_cigar))
        mine = np.ones(len(w), bool) if unmasked else ((w >= item["chunk"] + item["c0rel"]) & (w < item["chunk"] + item["nrem"]))
        total = int(rl[w][mine].sum())
        res.append((base, total, int(np.count_nonzero(_GAP[op[w]] & mine)), bool(mine.any() and (ln[w][mine] == 0).all())))
        base += total
    return res


def model_depth(reads, depth_len, producer="pmax", flip=None):
    """The depth map as the tile kernel's DECISIONS give it: per tile, the candidates of `producer`, their items, and for every item
    the aligned bases of its own words from the walk's start, clipped to the tile. flip: None, or one comparison / mask the wrong way —
    "ckpt_t0" (a boundary one position right of T0 still counts as left of the tile), "ckpt_t1" (a boundary on T1 - 1 already counts as
    right of the tile), "mask" (neighbouring reads' words of the first and last chunk are not masked), "range_end" (the pmax range ends
    at the first read with pos >= T1 - 2)."""
    ranges = candidate_ranges(reads, depth_len, producer, range_end_shift=1 if flip == "range_end" else 0)
    items = tile_items(reads, depth_len, ranges, t0_slack=1 if flip == "ckpt_t0" else 0, t1_strict=flip == "ckpt_t1")
    owner, op, ln, rl, cs, before = _words(reads)
    diff = np.zeros(n_tiles_of(depth_len) * T + 1, np.int64)
    for it in items:
        if not it["item"]:
            continue
        T0 = it["tile"] * T
        TW = min(T0 + T, depth_len) - T0
        if flip == "mask":
            w = np.arange(it["chunk"], min(it["chunk"] + it["n_chunks"] * CW, reads.n_cigar))
        else:
            w = np.arange(it["chunk"] + it["c0rel"], it["chunk"] + it["nrem"])
        cur = it["start"] + np.concatenate(([0], np.cumsum(rl[w])))[:-1]
        sel = _ALN[op[w]]
        a = np.clip(cur[sel], 0, TW) + T0
        b = np.clip(cur[sel] + ln[w][sel], 0, TW) + T0
        np.add.at(diff, a, 1)
        np.add.at(diff, b, -1)
    depth = np.cumsum(diff[:depth_len]).astype(np.uint32)
    return depth, int(depth.astype(np.uint64).sum()), int(np.count_nonzero(depth))


def group_windows(item):
    """(first valid word mod 4, 64-word windows) of an item in the group forms: windows start at the first valid word rounded down to 4"""
    fv = item["chunk"] + item["c0rel"]
    nval = item["nrem"] - item["c0rel"]
    return fv & 3, max(1, ((fv & 3) + nval + 63) >> 6)


# ======================================================================================================================= builders
class _Shard:
    """reads appended in array order; pos must not decrease unless the family says so"""

    def __init__(self):
        self.pos, self.flag, self.cig, self.n_words, self.tags = [], [], [], 0, {}

    def add(self, pos, ops, flag=0, tag=None):
        self.pos.append(int(pos)); self.flag.append(int(flag)); self.cig.append(list(ops))
        self.n_words += len(ops)
        if tag is not None:
            self.tags.setdefault(tag, []).append(len(self.pos) - 1)
        return len(self.pos) - 1

    def align(self, pos, residue, modulus=CKPT_WORDS, edge=(I, 1), always=False):
        """a filler read so that the next read's first word sits at `residue` modulo `modulus`; its first and last words are `edge`"""
        k = (residue - self.n_words) % modulus
        if k == 0 and always:
            k = modulus
        if k:
            ops = [(I, 1)] * k
            ops[0] = edge; ops[-1] = edge
            self.add(pos, ops, tag="filler")

    def reads(self, sort=True):
        pos = np.asarray(self.pos, np.int64)
        order = np.argsort(pos, kind="stable") if sort else np.arange(len(pos))
        r = Reads.from_cigar_lists(pos[order], np.asarray(self.flag, np.uint16)[order], np.full(len(pos), 60, np.uint8),
                                   [self.cig[i] for i in order])
        where = np.empty(len(pos), np.int64)
        where[order] = np.arange(len(pos))
        r.tags = {k: [int(where[i]) for i in v] for k, v in self.tags.items()}      # tag -> read indices of the finished shard
        return r


def alt(n_words, a, other=(I, 1)):
    """n_words words alternating M a / `other`: the reference offset in front of word w is a * ceil(w / 2) (other = I)"""
    return [(M, a) if k % 2 == 0 else other for k in range(n_words)]


def permute(reads, perm):
    off = reads.cigar_off.astype(np.int64)
    n_w = np.diff(off)[perm]
    new_off = np.concatenate(([0], np.cumsum(n_w))).astype(np.uint64)
    cig = np.concatenate([reads.cigar[off[r]:off[r + 1]] for r in perm]) if len(perm) else reads.cigar[:0]
    return Reads(reads.pos[perm], reads.flag[perm], reads.mapq[perm], new_off, cig)


# ------------------------------------------------------------------------------------------------------------------- A
A_DEPTH_LENS = (1, 3, T - 1, T, T + 1, 2 * T + 5, 3 * T)


def _a_shard():
    s = _Shard()
    s.add(-1, [(M, 10)], tag="pos-1")                                           # pos + 1 wraps to 0 in uint32
    for B in (T, 2 * T):
        for fb in range(B - 2, B + 2):
            for lb in range(fb, B + 2):
                n = lb - fb + 1
                ops = [(M, n)] if (fb + lb) % 3 == 0 else ([(S, 3), (M, n)] if (fb + lb) % 3 == 1 else [(H, 2), (EQ, n), (I, 2)])
                s.add(fb - 1, ops, tag="edge")
        for gap in (D, N):
            s.add(B - 11, [(M, 10), (gap, 7), (M, 5)], tag="gap")               # the gap starts exactly on B
            s.add(B - 11, [(M, 3), (gap, 7), (X, 5)], tag="gap")                # ... ends exactly in front of B
            s.add(B - 8, [(gap, 7), (M, 5)], tag="gap")                         # a read that opens with the gap, next base on B
        s.add(B - 4, [(M, 3), (M, 0), (D, 0), (N, 0), (M, 4)], tag="zero")      # zero-length ops on B
        s.add(B - 1, [(M, 0), (D, 0)], tag="zero")                              # a read of nothing but those
    s.add(T - 6, [(M, 5), (N, T), (M, 5)], tag="skip")                          # N covers exactly [T, 2T)
    s.add(T - 7, [(M, 5), (N, T + 2), (M, 5)], tag="skip")                      # N covers [T - 1, 2T + 1)
    for L in A_DEPTH_LENS:
        for lb in range(L - 2, L + 2):
            if lb >= 0:
                fb = max(lb - 3, 0)
                s.add(fb - 1, [(M, lb - fb + 1)], tag="map_end")
        s.add(L + 2, [(M, 5)], tag="beyond")                                    # wholly beyond a map of L positions
    s.add(T - 2, [(S, 5), (I, 3), (H, 2), (P, 1)], tag="no_ref")
    s.add(T, [], tag="empty"); s.add(2 * T - 1, [], tag="empty")
    for f in (F_UNMAP, F_SECONDARY, F_QCFAIL, F_DUP, F_DUP | F_SECONDARY):
        s.add(T - 20, [(M, 50)], flag=f, tag="filtered")
    s.add(T - 20, [(M, 50)], flag=0x800 | 0x10 | 0x1, tag="counted")            # supplementary, reverse, paired: these count
    return s.reads()


def a_cases():
    r = _a_shard()
    return [("A/len%d" % L, r, L) for L in A_DEPTH_LENS]


# ------------------------------------------------------------------------------------------------------------------- B
B_COUNTS = (0, 1, WL_SPEC - 1, WL_SPEC, WL_SPEC + 1, WL_CAP - 1, WL_CAP, WL_CAP + 1, 2 * WL_CAP - 1, 2 * WL_CAP, 2 * WL_CAP + 1,
            63, 64, 65, 127, 128, 129)
B_STEP = 8                                                                      # positions between two reads of a tile
B3_J = WL_CAP - 1                                                               # short reads behind the long one (third variant)


def _b_short(k):
    return [(M, 20), (D, 3), (M, 17)] if k % 2 else [(M, 33), (I, 4), (EQ, 2)]


def b_filtered(k, n):
    """second variant: every 7th read of a tile is a duplicate — never the tile's last, so that the scan's range keeps its end"""
    return k % 7 == 3 and k != n - 1


def b_cases():
    assert 64 + B_STEP * max(B_COUNTS) + 50 < T
    out = []
    for name, filt in (("B/items_eq_candidates", False), ("B/every_7th_filtered", True)):
        s = _Shard()
        for t, n in enumerate(B_COUNTS):
            for k in range(n):
                s.add(t * T + 64 + k * B_STEP, _b_short(k), flag=F_DUP if filt and b_filtered(k, n) else 0)
        out.append((name, s.reads(), len(B_COUNTS) * T))
    # third: a long read across tiles 1 and 2, then B3_J short reads that end left of tile 2, then one read inside tile 2: tile 2 has
    # WL_CAP + 1 candidates under both producers and 2 items. A duplicate-flagged long read into tile 4 followed by short reads left of it:
    # under "pmax" tile 4 has candidates and no item. Reads that start in the last (partial) tile beyond the map's end: under "scan" that
    # tile has candidates and no item.
    s = _Shard()
    s.add(T + 100, [(M, T)], tag="long")
    for k in range(B3_J):
        s.add(T + 200 + k * B_STEP, _b_short(k))
    s.add(2 * T + 300, _b_short(0), tag="own")
    s.add(3 * T + 10, [(M, T + 50)], flag=F_DUP, tag="long_filtered")
    for k in range(5):
        s.add(3 * T + 100 + k * B_STEP, _b_short(k))
    for k in range(3):
        s.add(5 * T + 20 + k, [(M, 30)], tag="beyond")
    out.append(("B/candidates_without_items", s.reads(), 5 * T + 10))
    return out


# ------------------------------------------------------------------------------------------------------------------- C
C_A = 5                                                                          # the alternating reads' M length
C_WORDS = 40 * CKPT_WORDS


def _c_offset_at_boundary(c0rel, j):
    """reference offset of an alt(.., C_A) read that starts c0rel words behind a checkpoint boundary, at its j-th boundary (j >= 1)"""
    return C_A * ((j * CKPT_WORDS - c0rel + 1) // 2)


def c_cases():
    s = _Shard()
    B = 2 * T
    # checkpoints of the read exactly on B - 2, B - 1, B, B + 1: B is T0 of the tile right of it and T1 of the tile left of it
    for c0rel in (37, 63):
        for delta in (-2, -1, 0, 1):
            pos = B + delta - _c_offset_at_boundary(c0rel, 10) - 1
            s.align(pos, c0rel, always=True)
            s.add(pos, alt(C_WORDS, C_A), tag="ckpt%+d/c0rel%d" % (delta, c0rel))
        B += 2 * T
    # nb == 0 across a tile edge; nb == 1; (every read above ends inside the tile it entered: want1 false there)
    s.align(B - 500, 5)
    s.add(B - 500, [(M, 100)] * 10, tag="nb0")
    s.align(B - 400, 10)
    s.add(B - 400, alt(70, 20), tag="nb1")
    B += 2 * T
    # interpolation misses: a skip of three tiles in front of 40 x 64 short words, and behind them
    s.align(B + 9, 37)
    s.add(B + 9, [(N, 3 * T)] + alt(C_WORDS, C_A), tag="skip_first")
    B += 5 * T
    s.align(B + 9, 37)
    s.add(B + 9, alt(C_WORDS, C_A) + [(N, 3 * T), (M, 5)], tag="skip_last")
    B += 5 * T
    # ten boundaries, from just left of a tile to just right of the next: the probe window clamps at 1 (first search of the tile it
    # covers) and at nb (second search)
    s.align(B - 101, 20)
    s.add(B - 101, alt(10 * CKPT_WORDS, 52), tag="clamps")
    s.add(B - 101, [(M, 7)] * 3)
    B += 2 * T
    depth_len = B + 100
    s.add(depth_len + 200 - 1, alt(100, 3), tag="beyond")        # in the last tile, right of the map's end: a candidate of the scan's range only
    return [("C/checkpoints", s.reads(), depth_len)]


# ------------------------------------------------------------------------------------------------------------------- D
D_NREM = (255, 256, 257, NS * CW - 1, NS * CW, NS * CW + 1)
D_C0REL = (0, 1, 3, 4, 63)
D_NCHUNKS = (1, 2, NS - 1, NS, NS + 1, 2 * NS, 2 * NS + 1)
D_BIG = 5000


def _d_shard(tail):
    """tail: n_cigar mod 4 of the finished shard (its last read ends the array)"""
    s = _Shard()
    t = 0

    def item(nrem, c0rel):
        nonlocal t
        t += 1
        pos = t * T + 50
        s.align(pos, c0rel, edge=(M, D_BIG), always=True)                 # the neighbour in front: its last word is M 5000
        s.add(pos, alt(nrem - c0rel, 1), tag="item")
        s.add(pos, [(M, D_BIG)], tag="after")                               # ... and the one behind opens with it

    for nrem in D_NREM:
        for c0rel in D_C0REL:
            item(nrem, c0rel)
    for nc in D_NCHUNKS:
        item(nc * CW - 100, 7)
    t += 1
    for k in range(20):                                                     # twenty one-chunk items in a row
        s.add(t * T + 50 + 10 * k, [(M, 1200)] + alt(28, 1) + [(M, 1200)], tag="row")
    t += 1
    n_last = 300
    while (s.n_words + n_last) % 4 != tail or (s.n_words + n_last) % CW == 0:
        n_last += 1
    s.add(t * T + 50, alt(n_last, 2, other=(D, 1)), tag="last")
    return s.reads(), (t + 1) * T


def d_cases():
    return [("D/tail%d" % m,) + _d_shard(m) for m in (0, 1, 2, 3)]


# ------------------------------------------------------------------------------------------------------------------- E
def e_cases():
    s = _Shard()
    B = T
    one = [(M, 50), (D, 5), (M, 50)]                                        # total 105, one chunk
    for br in (-1, 0, 1):                                                   # base_rel of tile B / T
        s.align(B + br - 1, 0)
        s.add(B + br - 1, one, tag="base_rel")
    B += 2 * T
    for e in (-1, 0, 1):                                                    # base_rel + total - TW of tile B / T - 1
        s.align(B - 105 + e - 1, 0)
        s.add(B - 105 + e - 1, one, tag="end")
    B += 2 * T
    s.add(B - 21, [(M, 10), (D, 20), (M, 10)], tag="straddle")              # D over [B - 10, B + 10): T1 of one tile, T0 of the next
    s.add(B - 21, [(M, 10), (N, 20), (M, 10)], tag="straddle")
    B += 2 * T
    s.add(B - 51, [(M, 5), (D, T + 100), (M, 5)], tag="cover")              # a D over a whole tile and more
    B += 3 * T
    s.align(B + 99, 0)
    s.add(B + 99, [(M, 1)] * CW + [(D, 1), (N, 2)] * (CW // 2) + [(M, 1)] * 88, tag="gap_chunk")
    s.align(B + 99, 0)
    s.add(B + 99, [(M, 1)] * CW + [(M, 0), (D, 0), (I, 0), (N, 0)] * (CW // 4) + [(M, 1)] * 88, tag="zero_chunk")
    return [("E/paths", s.reads(), B + T)]


# ------------------------------------------------------------------------------------------------------------------- F
F_VALID = (60, 61, 64, 65, 128, 129)


def f_cases():
    s = _Shard()
    p = T - 1500                                                            # the later reads cross into, or start in, the second tile
    for m in range(4):
        for n in F_VALID:
            s.align(p, m, modulus=4, edge=(M, 900))
            s.add(p, [((M, 4), (D, 1), (I, 2))[k % 3] for k in range(n)], tag="item")
            p += 97
    s.add(p, [(M, 900)])
    return [("F/windows", s.reads(), 2 * T)]


# ------------------------------------------------------------------------------------------------------------------- G
def g_cases():
    out = []
    for name, n in (("G/below", FAST_MAX_CANDIDATES - 1), ("G/at", FAST_MAX_CANDIDATES)):
        i = np.arange(n, dtype=np.int64)
        pos = np.concatenate(([100], T + (i * (T - 60)) // n, [2 * T + 100])).astype(np.int32)
        ln = np.concatenate(([30], 1 + i % 40, [30])).astype(np.uint32)
        out.append((name, Reads(pos, np.zeros(n + 2, np.uint16), np.full(n + 2, 60, np.uint8), np.arange(n + 3, dtype=np.uint64), (ln << 4) | M),
                    3 * T))
    return out


# ------------------------------------------------------------------------------------------------------------------- H
H_TILES = 2 * TR_SLOTS + 2
H_SKIP, H_DOUBLE = (20, 40, 100, 120), (TR_SLOTS - 1, TR_SLOTS)
H_REACH = {10: WIDE_TILES - 1, 30: WIDE_TILES, TR_SLOTS - 4: 10}            # first tile -> t1 - t0: not wide, wide, wide across the slots' end


def h_cases():
    s = _Shard()
    for t in range(H_TILES):
        if t in H_SKIP:
            continue
        for k in range(2 if t in H_DOUBLE else 1):
            ops = [(M, 40), (I, 3), (M, 25)]
            if t in H_REACH and k == 0:
                ops = [(M, 40), (N, H_REACH[t] * T), (M, 25)]
            s.add(t * T + 300 + 7 * k, ops)
    return [("H/scan_tile_ranges", s.reads(), H_TILES * T)]


# ------------------------------------------------------------------------------------------------------------------- U
def u_cases():
    out = []
    src = [next(c for c in a_cases() if c[2] == 2 * T + 5), b_cases()[0], c_cases()[0], d_cases()[0]]
    for name, r, depth_len in src:
        perm = np.random.default_rng(0xD0 + len(name)).permutation(r.n_reads)
        out.append(("U/" + name, permute(r, perm), depth_len))
    # runs of equal pos: the first B variant with positions rounded down to multiples of 64, permuted
    name, r, depth_len = b_cases()[0]
    q = Reads((r.pos // 64) * 64, r.flag, r.mapq, r.cigar_off, r.cigar)
    out.append(("U/B/equal_pos_runs", permute(q, np.random.default_rng(0xE0).permutation(q.n_reads)), depth_len))
    return out


def small_cases():
    """every family but G"""
    return a_cases() + b_cases() + c_cases() + d_cases() + e_cases() + f_cases() + h_cases() + u_cases()
