"""Inputs of the device inflate's checks, shared by the CPU check of the decode core (tests/test_inflate_core.py writes them to a corpus
file for tools/fuzz/inflate_core_check.cpp) and the GPU tests (tests/test_gpu_bgzf_inflate.py): zlib-made streams of every block kind,
hand-built streams for the corners zlib never produces, and damaged variants. Everything is seeded: both sides see the same bytes."""
import heapq
import struct
import zlib
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name comp data")          # comp: a raw DEFLATE stream; data: what it decodes to

BLOCK_DTYPE = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("in_len", "<u4"), ("out_len", "<u4"), ("crc32", "<u4"), ("reserved", "<u4")])
GUARD = 0xEE
STRATEGIES = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FIXED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FILTERED)
LEVELS = (0, 1, 3, 6, 9)


def crc(data):
    return zlib.crc32(data) & 0xFFFFFFFF


# ---- the generators of tests/test_fast_inflate.py -----------------------------------------------------------------------------------------
def deflate(data, level, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(data) + c.flush()


def datasets():
    rng = np.random.default_rng(1)
    out = []
    for n in (0, 1, 2, 5, 17, 100, 1000, 20_000, 65_280):
        out.append(bytes(rng.integers(0, 256, n, dtype=np.uint8)))            # incompressible: stored / literal-only blocks
        out.append(bytes(rng.integers(0, 4, n, dtype=np.uint8)))              # short codes
        out.append(b"A" * n)                                                   # distance-1 runs
        out.append((b"abcdefgh" * (n // 8 + 1))[:n])                           # distance-8 matches
        out.append((b"xyz" * (n // 3 + 1))[:n])                                # overlapping copies, distance < 8
        w = rng.integers(1, 400, max(n // 4, 1)).astype(np.uint32) << 4 | rng.choice([0, 1, 2, 4], max(n // 4, 1)).astype(np.uint32)
        out.append(w.tobytes()[:n])                                            # CIGAR words
    return out


def zlib_cases():
    """(a): every data set x level x strategy. A member holds at most 64 KiB of input: the level-0 (stored) form of the longest data
    sets is 5 bytes per stored block longer than the data and still fits."""
    out = []
    for i, data in enumerate(datasets()):
        for level in LEVELS:
            for strategy in STRATEGIES:
                comp = deflate(data, level, strategy)
                assert len(comp) <= 65536
                out.append(Case(f"zlib d{i} n{len(data)} l{level} s{strategy}", comp, data))
    return out


# ---- a small DEFLATE encoder for the streams zlib never writes ------------------------------------------------------------------------------
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
PRE_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):                     # a number, least significant bit first
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, n):                  # a Huffman code, most significant bit first
        self.bits(int(format(code, f"0{n}b")[::-1], 2), n)

    def align(self):
        if self.n:
            self.out.append(self.acc & 255)
            self.acc, self.n = 0, 0

    def done(self):
        self.align()
        return bytes(self.out)


def _len_sym(l):
    return 28 if l == 258 else max(s for s in range(28) if LEN_BASE[s] <= l)


def _dist_sym(d):
    return max(s for s in range(30) if DIST_BASE[s] <= d)


def canonical(lengths):
    """symbol -> (code, bits) of the canonical Huffman code with these code lengths"""
    out, code = {}, 0
    for l in range(1, 16):
        for s, sl in enumerate(lengths):
            if sl == l:
                out[s] = (code, l)
                code += 1
        code <<= 1
    return out


def huff_lengths(freq, n_sym):
    """code lengths of a Huffman code for the symbols with freq > 0 (at least two of them)"""
    heap = [(f, s, (s,)) for s, f in sorted(freq.items()) if f > 0]
    assert len(heap) >= 2
    heapq.heapify(heap)
    lengths = [0] * n_sym
    while len(heap) > 1:
        fa, ka, a = heapq.heappop(heap)
        fb, kb, b = heapq.heappop(heap)
        for s in a + b:
            lengths[s] += 1
        heapq.heappush(heap, (fa + fb, min(ka, kb), a + b))
    assert max(lengths) <= 15
    return lengths


def _put_tokens(bw, tokens, lit_code, dist_code):
    for t in tokens:
        if isinstance(t, int):
            bw.code(*lit_code[t])
        else:
            l, d = t
            s = _len_sym(l)
            bw.code(*lit_code[257 + s])
            bw.bits(l - LEN_BASE[s], LEN_EXTRA[s])
            ds = _dist_sym(d)
            bw.code(*dist_code[ds])
            bw.bits(d - DIST_BASE[ds], DIST_EXTRA[ds])
    bw.code(*lit_code[256])


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = {s: (s, 5) for s in range(30)}


def fixed_block(bw, tokens, final):
    bw.bits(1 if final else 0, 1)
    bw.bits(1, 2)
    _put_tokens(bw, tokens, FIXED_LIT, FIXED_DIST)


def stored_block(bw, data, final):
    assert len(data) <= 65535
    bw.bits(1 if final else 0, 1)
    bw.bits(0, 2)
    bw.align()
    bw.out += struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data


def dynamic_block(bw, tokens, final):
    """A dynamic block whose distance code is what the tokens need and no more: no code at all (HDIST 1, length 0) without a match, ONE code
    of one bit for a single distance symbol (the incomplete code RFC 1951 allows), a Huffman code otherwise. The code lengths go out one by
    one under a code-length code of sixteen 4-bit codes (no repeat symbols)."""
    freq, dfreq = {256: 1}, {}
    for t in tokens:
        if isinstance(t, int):
            freq[t] = freq.get(t, 0) + 1
        else:
            freq[257 + _len_sym(t[0])] = freq.get(257 + _len_sym(t[0]), 0) + 1
            dfreq[_dist_sym(t[1])] = dfreq.get(_dist_sym(t[1]), 0) + 1
    ll = huff_lengths(freq, 286)
    if len(dfreq) == 0:
        dl = [0]
    elif len(dfreq) == 1:
        dl = [0] * 30
        dl[next(iter(dfreq))] = 1
    else:
        dl = huff_lengths(dfreq, 30)
    hlit = max(257, max(s for s, l in enumerate(ll) if l) + 1)
    hdist = max(1, max([s for s, l in enumerate(dl) if l], default=0) + 1)
    bw.bits(1 if final else 0, 1)
    bw.bits(2, 2)
    bw.bits(hlit - 257, 5)
    bw.bits(hdist - 1, 5)
    bw.bits(19 - 4, 4)
    for s in PRE_ORDER:
        bw.bits(0 if s >= 16 else 4, 3)
    for l in ll[:hlit] + dl[:hdist]:
        bw.code(l, 4)
    _put_tokens(bw, tokens, canonical(ll), canonical(dl))


def expand(tokens):
    out = bytearray()
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        else:
            l, d = t
            assert 1 <= d <= len(out)
            for _ in range(l):
                out.append(out[-d])
    return bytes(out)


def _one(name, block, tokens):
    bw = BitWriter()
    block(bw, tokens, True)
    comp, data = bw.done(), expand(tokens)
    assert zlib.decompress(comp, -15) == data, name           # zlib is the reference of every hand-built stream
    assert len(comp) <= 65536 and len(data) <= 65536
    return Case(name, comp, data)


OVERLAP_LENGTHS = (3, 64, 65, 258)


def overlap_cases():
    """(b) 4: every distance 1..70 with lengths 3, 64, 65 and 258: either side of the wave width, and dist < len"""
    rng = np.random.default_rng(11)
    out = []
    for dist in range(1, 71):
        for length in OVERLAP_LENGTHS:
            lits = [int(x) for x in rng.integers(0, 256, dist + int(rng.integers(0, 5)))]
            out.append(_one(f"overlap d{dist} l{length}", fixed_block, lits + [(length, dist)] + [int(x) for x in rng.integers(0, 256, 2)]))
    return out


def fibonacci_data():
    """symbol i occurs fib(i) times: the Huffman tree is a chain, zlib caps the code lengths at 15"""
    fib = [1, 1]
    while sum(fib) + fib[-1] + fib[-2] <= 65_280:
        fib.append(fib[-1] + fib[-2])
    data = np.concatenate([np.full(f, 33 + i, np.uint8) for i, f in enumerate(fib)])
    np.random.default_rng(13).shuffle(data)
    return bytes(data)


def edge_cases():
    """(b) 1-9, each a whole member"""
    rng = np.random.default_rng(7)
    out = []
    # 1. several DEFLATE blocks per member: empty stored blocks (the flushes) between Huffman blocks
    text = (b"ACGTTGCA" * 40 + bytes(rng.integers(0, 256, 300, dtype=np.uint8))) * 6
    for level in (1, 6):
        c = zlib.compressobj(level, zlib.DEFLATED, -15)
        comp = c.compress(text[:1000]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(text[1000:2500]) + c.flush(zlib.Z_SYNC_FLUSH) + c.compress(text[2500:]) + c.flush()
        out.append(Case(f"flushes l{level}", comp, text))
    bw = BitWriter()
    stored_block(bw, b"", False)
    fixed_block(bw, [65, 66, 67, (5, 3)], False)
    stored_block(bw, b"stored in the middle", False)
    dynamic_block(bw, [1, 2, 3, 1, 2, 3, (9, 6), 4], False)
    stored_block(bw, b"", True)
    comp = bw.done()
    out.append(Case("mixed block kinds", comp, zlib.decompress(comp, -15)))
    # 2. a match of length 258 at distance 32768 that ends exactly at out_len
    lits = [int(x) for x in rng.integers(0, 256, 32768)]
    out.append(_one("len 258 dist 32768 at the end", fixed_block, lits + [(258, 32768)]))
    # 3. length-3 matches
    toks = [int(x) for x in rng.integers(0, 256, 5)]
    for k in range(300):
        toks += [(3, 1 + k % 5), int(rng.integers(0, 256))]
    out.append(_one("length-3 matches, fixed", fixed_block, toks))
    out.append(_one("length-3 matches, dynamic", dynamic_block, toks))
    # 5. code lengths of 15 bits
    fibd = fibonacci_data()
    for strategy in (zlib.Z_HUFFMAN_ONLY, zlib.Z_DEFAULT_STRATEGY):
        out.append(Case(f"15-bit codes s{strategy}", deflate(fibd, 6, strategy), fibd))
    # 6. a dynamic block with a single distance code (one code of one bit: incomplete, allowed)
    toks = [int(x) for x in rng.integers(0, 256, 40)] + [(20, 17), 7, (30, 18), 9, (258, 19), (3, 20)]
    assert len({_dist_sym(t[1]) for t in toks if not isinstance(t, int)}) == 1
    out.append(_one("single distance code", dynamic_block, toks))
    # 7. a dynamic block with no distance code: zlib's Z_HUFFMAN_ONLY (which still sends two unused codes) and one with none at all
    lit = bytes(rng.integers(0, 7, 3000, dtype=np.uint8))
    out.append(Case("huffman only", deflate(lit, 6, zlib.Z_HUFFMAN_ONLY), lit))
    out.append(_one("no distance code at all", dynamic_block, list(lit[:500])))
    # 8. the BGZF EOF member
    out.append(Case("EOF member", b"\x03\x00", b""))
    # 9. out_len 65536
    full = (bytes(rng.integers(0, 16, 4096, dtype=np.uint8)) * 16)[:65536]
    out.append(Case("out_len 65536", deflate(full, 6), full))
    assert len(out[-1].data) == 65536 and len(out[-1].comp) <= 65536
    return out


CRC_LENGTHS = list(range(0, 301)) + [511, 512, 513, 4095, 4096, 65_535]


def crc_cases():
    """(b) 12: stored blocks of every length 0..300 and 511/512/513/4095/4096/65535. A stored block of 65 535 bytes is 65 540 bytes of input,
    more than a member (and the entry point) allows: that length is one stored block of 60 000 bytes and a fixed block of 5 535 more."""
    rng = np.random.default_rng(17)
    buf = bytes(rng.integers(0, 256, 65_535, dtype=np.uint8))
    out = []
    for n in CRC_LENGTHS:
        bw = BitWriter()
        if n <= 65_531:
            stored_block(bw, buf[:n], True)
            data = buf[:n]
        else:
            stored_block(bw, buf[:60_000], False)
            toks = [0] + [(258, 1)] * ((n - 60_001) // 258)
            toks += [int(x) for x in buf[: n - 60_000 - len(expand(toks))]]
            fixed_block(bw, toks, True)
            data = buf[:60_000] + expand(toks)
        comp = bw.done()
        assert len(data) == n and len(comp) <= 65536 and zlib.decompress(comp, -15) == data
        out.append(Case(f"crc n{n}", comp, data))
    return out


def small_cases(n=5000):
    """(b) 11: many small members"""
    rng = np.random.default_rng(19)
    pool = [bytes(rng.integers(0, 8, int(k), dtype=np.uint8)) for k in rng.integers(0, 40, 64)]
    comps = [deflate(d, 6) for d in pool]
    return [Case(f"small {i}", comps[i % 64], pool[i % 64]) for i in range(n)]


def damaged_cases(n=300):
    """(d): the garbage of tests/test_fast_inflate.py — one to three bytes of a level-6 stream changed, three in ten cut short —, the
    data still the original's. Whoever decodes one declines it, or (the damage fell on bits that do not matter) gets the original."""
    rng = np.random.default_rng(5)
    data = datasets()[-1]
    comp = deflate(data, 6)
    out = []
    for k in range(n):
        b = bytearray(comp)
        for _ in range(int(rng.integers(1, 4))):
            b[int(rng.integers(0, len(b)))] ^= int(rng.integers(1, 256))
        if rng.random() < 0.3:
            b = b[: int(rng.integers(0, len(b)))]
        out.append(Case(f"damaged {k}", bytes(b), data))
    for k, junk in enumerate((b"", b"\x00", b"\xff" * 40, bytes(rng.integers(0, 256, 300, dtype=np.uint8)))):
        out.append(Case(f"junk {k}", junk, data[:48]))
    return out


def intact_cases():
    return zlib_cases() + edge_cases() + overlap_cases() + crc_cases()


def write_corpus(path, intact=None, damaged=None):
    """the file tools/fuzz/inflate_core_check.cpp reads"""
    intact = intact_cases() if intact is None else intact
    damaged = damaged_cases() if damaged is None else damaged
    with open(path, "wb") as f:
        f.write(b"ICC1" + struct.pack("<I", len(intact) + len(damaged)))
        for flag, cases in ((1, intact), (0, damaged)):
            for c in cases:
                f.write(struct.pack("<IIII", flag, len(c.comp), len(c.data), crc(c.data)) + c.comp + c.data)
    return len(intact), len(damaged)


def layout(cases, out_lens=None, crcs=None):
    """One call's buffers: the streams packed with gaps of 1, 2, 3, 5, ... bytes (in_off and out_off odd, and no multiples of 4 or 16, most
    of the time), the outputs with GUARD bytes before, between and behind. Returns comp, blocks, out (filled with GUARD), the output slices."""
    gaps = (1, 2, 3, 5, 7, 9, 13, 17, 19)
    comp = bytearray(b"\x5a" * 3)
    blocks = np.zeros(len(cases), BLOCK_DTYPE)
    o = 5
    for i, c in enumerate(cases):
        n_out = len(c.data) if out_lens is None else out_lens[i]
        blocks[i] = (len(comp), o, len(c.comp), n_out, crc(c.data) if crcs is None else crcs[i], 0)
        comp += c.comp + b"\x5a" * gaps[i % len(gaps)]
        o += n_out + gaps[(i + 4) % len(gaps)]
    out = np.full(o + 32, GUARD, np.uint8)
    return np.frombuffer(bytes(comp), np.uint8), blocks, out


def guards_intact(out, blocks):
    mask = np.ones(len(out), bool)
    for b in blocks:
        mask[int(b["out_off"]): int(b["out_off"]) + int(b["out_len"])] = False
    return bool((out[mask] == GUARD).all())
