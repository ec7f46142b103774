// cigar_pack_core.hpp — the 16-bit form of a resident long-read shard's CIGAR array: the rule that packs a 32-bit word, the escape for
// the words that do not fit, and the look-up that brings an escaped word back. The same text compiles for the device (kernels/cigarpack.hip,
// scan.hip, depth.hip) and for the host with g++ (tools/fuzz/cigar_pack_core_check.cpp, under the sanitizers): no HIP construct in it.
//
// A CIGAR word is len << 4 | op with 28 bits of length. Op i of a packed shard is the halfword
//     h[i] = len << 4 | op        when len < 0xFFF   (zero-extended, h IS the 32-bit word of the same op)
//     h[i] = 0xFFF0 | op          otherwise (an ESCAPE), and the full word sits in a side table.
// The table holds one 64-bit entry per escape, sorted by op index: word << 32 | (uint32_t)i. The array is cut into PIECES of 512 ops (1 KiB
// of halfwords, one LDS-DMA instruction of the scan), and piece[p] is the number of escapes in front of piece p (piece[n_pieces] = all of
// them): the entries of op i's piece are tab[piece[i >> 9] .. piece[(i >> 9) + 1]). Inside one piece the low 32 bits of the op indices
// grow strictly (a piece is aligned to 512 ops, so they cannot wrap), which is all the look-up needs: op indices may exceed 2^32.
// The look-up bisects the piece's entries (at most 512, nine steps; an ONT piece has none or one).
#pragma once
#include <stdint.h>

#ifndef CPK_HD
#define CPK_HD
#endif

namespace cigar_pack_core {

constexpr uint32_t PIECE_SHIFT = 9, PIECE_OPS = 1u << PIECE_SHIFT;       // ops per piece
constexpr uint32_t ESC_LEN = 0xFFFu;                                     // the length field of an escape: lengths >= this do not fit
constexpr uint32_t ESC_MIN = ESC_LEN << 4;                               // a halfword is an escape iff it is >= this
constexpr uint64_t MAX_ESC_DENOM = 64;                                   // a shard with more than n_ops / 64 escapes stays at 32 bits

CPK_HD inline uint64_t n_pieces(uint64_t n_ops) { return (n_ops + PIECE_OPS - 1) >> PIECE_SHIFT; }
CPK_HD inline bool is_escape_word(uint32_t w) { return (w >> 4) >= ESC_LEN; }             // of a 32-bit word: must it be escaped?
CPK_HD inline bool is_escape(uint32_t h) { return h >= ESC_MIN; }                         // of a (zero-extended) halfword: is it one?
CPK_HD inline uint16_t pack(uint32_t w) { return (uint16_t)(is_escape_word(w) ? (ESC_MIN | (w & 15u)) : w); }
CPK_HD inline uint64_t entry(uint64_t i, uint32_t w) { return ((uint64_t)w << 32) | (uint64_t)(uint32_t)i; }
CPK_HD inline bool packs(uint64_t n_ops, uint64_t n_esc) { return n_esc * MAX_ESC_DENOM <= n_ops; }

// the full word of the escaped op i; `h` (its halfword) comes back for an op the table does not hold (never for a table made by the rule above)
CPK_HD inline uint32_t lookup(const uint32_t *piece, const uint64_t *tab, uint64_t i, uint32_t h)
{
    const uint64_t p = i >> PIECE_SHIFT;
    uint32_t a = piece[p];
    const uint32_t end = piece[p + 1];
    uint32_t b = end;
    const uint32_t key = (uint32_t)i;
    while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        if ((uint32_t)tab[mid] < key) a = mid + 1; else b = mid;
    }
    if (a < end) {
        const uint64_t e = tab[a];
        if ((uint32_t)e == key) return (uint32_t)(e >> 32);
    }
    return h;
}

CPK_HD inline uint32_t unpack(const uint16_t *half, const uint32_t *piece, const uint64_t *tab, uint64_t i)
{
    const uint32_t h = half[i];
    return is_escape(h) ? lookup(piece, tab, i, h) : h;
}

// The whole array on one thread: what the device's three steps (count per piece, exclusive sum, fill) compute together.
// piece: [n_pieces + 1]; half: [n_pieces * 512] (the last piece's tail is zeroed); tab: [return value of count_escapes].
CPK_HD inline uint64_t count_escapes(const uint32_t *w, uint64_t n_ops)
{
    uint64_t n = 0;
    for (uint64_t i = 0; i < n_ops; i++) n += is_escape_word(w[i]) ? 1u : 0u;
    return n;
}
CPK_HD inline void pack_array(const uint32_t *w, uint64_t n_ops, uint16_t *half, uint32_t *piece, uint64_t *tab)
{
    const uint64_t np = n_pieces(n_ops);
    uint32_t n = 0;
    for (uint64_t p = 0; p < np; p++) {
        piece[p] = n;
        for (uint64_t i = p << PIECE_SHIFT; i < ((p + 1) << PIECE_SHIFT); i++) {
            const uint32_t x = i < n_ops ? w[i] : 0u;
            half[i] = pack(x);
            if (is_escape_word(x)) tab[n++] = entry(i, x);
        }
    }
    piece[np] = n;
}

}  // namespace cigar_pack_core
