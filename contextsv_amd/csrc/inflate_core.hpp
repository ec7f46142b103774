// inflate_core.hpp — the sequential core of the device's raw-DEFLATE decoder (RFC 1951) for BGZF members: bit reader, code-length decoding,
// canonical Huffman table build (primary table + sub-tables for the longer codes) and the decode of one symbol to a token. The same text
// compiles for the device (kernels/inflate.hip, every lane of a wave runs it on the same values) and for the host with g++
// (tools/fuzz/inflate_core_check.cpp, under the sanitizers): no HIP construct in it, no array on the stack that is indexed at run time
// (all of those live in `Work`, which the kernel places in LDS), no table in constant memory (the base / extra-bit tables are formulas).
// Contract, the one of host/fast_inflate.h: decline anything unusual. The caller decodes a declined block with zlib, and every block is
// CRC-checked either way, so the result never depends on this file being right about a corner of the format.
// What it guarantees whatever the input: every token it hands out has been checked against the output (a literal or a copy fits the
// bytes left, a distance reaches no further back than the bytes written), the input is only read through In::get32 (which pads with
// zeros past the end; running past the end is detected on the next token), no table entry is written past its table, and every loop
// consumes at least one input bit or produces an output byte per iteration.
#pragma once
#include <stdint.h>

#ifndef IC_HD
#define IC_HD
#endif
// IC_UNIFORM(x): x, a 32-bit value every lane of the wave holds alike (it came out of LDS or memory). The kernel defines it as a read of the
// first lane, so that the value itself sits in a scalar register; here, and on the host, it is x. It is a hint and no more: in the kernel as
// hipcc builds it today the decoder's state still lives in vector registers and the token loop is compiled with exec-mask branches
//  — the reads bought a few per cent, not a scalar decode loop.
#ifndef IC_UNIFORM
#define IC_UNIFORM(x) (x)
#endif

namespace inflate_core {

constexpr int LITLEN_BITS = 10, DIST_BITS = 8, PRE_BITS = 7;
// primary table + room for the sub-tables. Sized as zlib sizes its own (a sub-table only as deep as the codes behind its prefix): 1332
// entries at most for 286 symbols and 10 root bits; a code set that needs more is declined, not overrun.
constexpr int LITLEN_CAP = 2048, DIST_CAP = 768, PRE_CAP = 1 << PRE_BITS;
constexpr uint32_t MAX_BLOCK = 65536;          // a BGZF member holds at most 64 KiB, compressed and decoded

// table entry: bits 0-7 codeword bits to consume | 8-12 extra bits (or sub-table index bits) | 13-15 kind | 16-31 value
enum : uint32_t { K_INVALID = 0, K_LITERAL = 1, K_LENGTH = 2, K_END = 3, K_SUB = 4, K_DIST = 5 };
IC_HD inline uint32_t mk(uint32_t kind, uint32_t value, uint32_t extra) { return (value << 16) | (kind << 13) | (extra << 8); }
IC_HD inline uint32_t e_bits(uint32_t e) { return e & 0xff; }
IC_HD inline uint32_t e_extra(uint32_t e) { return (e >> 8) & 0x1f; }
IC_HD inline uint32_t e_kind(uint32_t e) { return (e >> 13) & 7; }
IC_HD inline uint32_t e_value(uint32_t e) { return e >> 16; }

enum : int { TK_LITLEN = 0, TK_DIST = 1, TK_PRE = 2 };

// RFC 1951 §3.2.5 as formulas: length codes 257..285 (s = code - 257), distance codes 0..29
IC_HD inline uint32_t len_extra(uint32_t s) { return (s < 8 || s == 28) ? 0 : (s >> 2) - 1; }
IC_HD inline uint32_t len_base(uint32_t s) { return s < 8 ? 3 + s : s == 28 ? 258 : 3 + ((4 + (s & 3)) << len_extra(s)); }
IC_HD inline uint32_t dist_extra(uint32_t d) { return d < 4 ? 0 : (d >> 1) - 1; }
IC_HD inline uint32_t dist_base(uint32_t d) { return d < 4 ? d + 1 : 1 + ((2 + (d & 1)) << dist_extra(d)); }
// the order the code-length code's lengths come in: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, five bits each
IC_HD inline uint32_t pre_order(uint32_t i)
{
    const uint64_t lo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    const uint64_t hi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    return (uint32_t)((i < 12 ? lo >> (5 * i) : hi >> (5 * (i - 12))) & 31);
}

IC_HD inline uint32_t entry_of(int kind, uint32_t sym)
{
    if (kind == TK_PRE) return mk(K_LITERAL, sym, 0);
    if (kind == TK_DIST) return sym < 30 ? mk(K_DIST, dist_base(sym), dist_extra(sym)) : mk(K_INVALID, 0, 0);
    if (sym < 256) return mk(K_LITERAL, sym, 0);
    if (sym == 256) return mk(K_END, 0, 0);
    if (sym <= 285) return mk(K_LENGTH, len_base(sym - 257), len_extra(sym - 257));
    return mk(K_INVALID, 0, 0);                       // 286, 287 take part in the fixed code but may not occur
}

IC_HD inline uint32_t reverse_bits(uint32_t code, int len)
{
    uint32_t r = 0;
    for (int i = 0; i < len; i++) { r = (r << 1) | (code & 1); code >>= 1; }
    return r;
}

// Everything the decoder indexes at run time. ~12.6 KiB: in LDS on the device, one per decoding wave.
struct Work {
    uint32_t litlen[LITLEN_CAP];
    uint32_t dist[DIST_CAP];
    uint32_t pre[PRE_CAP];
    uint16_t sorted[288];          // symbols by (length, symbol)
    uint16_t count[16], offs[17], at[17];
    uint8_t  lens[288 + 32];       // literal/length code lengths, then the distance code lengths
    uint8_t  pre_lens[19];
};

// Canonical Huffman code -> look-up table indexed by the next `tb` stream bits (LSB first), with sub-tables for longer codes; a sub-table
// is as deep as the codes that share its prefix need (the codes of one prefix are consecutive in canonical order). A complete code is
// required, except for the one-symbol code RFC 1951 allows (a single distance code of one bit). Over-subscribed and incomplete sets are
// refused before the first entry is written; a sub-table that does not fit `cap` is refused before it is written. lens[s] <= 15.
IC_HD inline bool build_table(const uint8_t *lens, int n_sym, int tb, uint32_t *table, int cap, int kind, Work &w)
{
    for (int l = 0; l < 16; l++) w.count[l] = 0;
    for (int s = 0; s < n_sym; s++) w.count[IC_UNIFORM((uint32_t)lens[s]) & 15]++;
    const int used = n_sym - (int)IC_UNIFORM((uint32_t)w.count[0]);
    if (used == 0) return false;
    int left = 1;
    for (int l = 1; l <= 15; l++) { left = left * 2 - (int)IC_UNIFORM((uint32_t)w.count[l]); if (left < 0) return false; }
    if (left > 0 && !(used == 1 && IC_UNIFORM((uint32_t)w.count[1]) == 1)) return false;
    w.offs[1] = 0;
    for (int l = 1; l <= 15; l++) w.offs[l + 1] = (uint16_t)(w.offs[l] + w.count[l]);
    for (int l = 1; l <= 16; l++) w.at[l] = w.offs[l];
    for (int s = 0; s < n_sym; s++) { const int l = (int)(IC_UNIFORM((uint32_t)lens[s]) & 15); if (l) w.sorted[w.at[l]++] = (uint16_t)s; }      // at most n_sym <= 288 entries
    const uint32_t primary = 1u << tb;
    for (uint32_t i = 0; i < primary; i++) table[i] = mk(K_INVALID, 0, 0);
    uint32_t next_free = primary, code = 0, cur_prefix = 0xffffffffu, sub_base = 0, sub_bits = 0;
    for (int l = 1; l <= 15; l++) {
        const uint32_t k_end = IC_UNIFORM((uint32_t)w.offs[l + 1]);
        for (uint32_t k = IC_UNIFORM((uint32_t)w.offs[l]); k < k_end; k++, code++) {
            const uint32_t rev = reverse_bits(code, l);
            const uint32_t e = entry_of(kind, IC_UNIFORM((uint32_t)w.sorted[k]));
            if (l <= tb) {
                for (uint32_t i = rev; i < primary; i += 1u << l) table[i] = e | (uint32_t)l;
                continue;
            }
            const uint32_t prefix = rev & (primary - 1);
            if (prefix != cur_prefix) {
                // open the sub-table of this prefix: deepen it until the codes from here on fill it (zlib's inftrees.c sizes its own so)
                uint32_t sb = (uint32_t)(l - tb);
                int room = (1 << sb) - (int)(k_end - k);
                for (int ll = l; room > 0 && ll < 15;) { ll++; sb++; room = room * 2 - (int)IC_UNIFORM((uint32_t)w.count[ll]); }
                if (next_free + (1u << sb) > (uint32_t)cap) return false;
                table[prefix] = mk(K_SUB, next_free, sb) | (uint32_t)tb;
                for (uint32_t i = 0; i < (1u << sb); i++) table[next_free + i] = mk(K_INVALID, 0, 0);
                sub_base = next_free; sub_bits = sb; cur_prefix = prefix;
                next_free += 1u << sb;
            }
            if ((uint32_t)(l - tb) > sub_bits) return false;
            for (uint32_t i = rev >> tb; i < (1u << sub_bits); i += 1u << (l - tb)) table[sub_base + i] = e | (uint32_t)(l - tb);
        }
        code <<= 1;
    }
    return true;
}

enum : uint32_t { T_LITERAL = 0, T_MATCH = 1, T_STORED = 2, T_DONE = 3, T_DECLINE = 4 };
struct Token {
    uint32_t kind;
    uint32_t a;        // T_LITERAL: the byte; T_MATCH: length; T_STORED: length (> 0)
    uint32_t b;        // T_MATCH: distance; T_STORED: offset of the bytes in the input
};

// In: uint32_t get32(uint32_t pos) — the four input bytes at byte offset pos, little-endian, zeros for the bytes at and past in_len
// (a block header is read to its end before the overrun is looked at, so pos can pass in_len by a few hundred bytes); void seek(uint32_t pos) — the next get32 will be at pos or later (a hint, after a stored block).
// The decoder owns the output position: a token it returns has already been counted, the caller only moves the bytes.
template <class In>
struct Decoder {
    In &in;
    Work &w;
    uint32_t in_len, out_len;
    uint32_t out_pos = 0;
    uint64_t buf = 0;
    uint32_t cnt = 0;              // valid bits in buf
    uint32_t p = 0;                // next input byte to fetch
    bool in_block = false, last = false;

    IC_HD Decoder(In &in_, Work &w_, uint32_t in_len_, uint32_t out_len_) : in(in_), w(w_), in_len(in_len_), out_len(out_len_) {}

    IC_HD void refill() { if (cnt < 32) { buf |= (uint64_t)IC_UNIFORM(in.get32(p)) << cnt; p += 4; cnt += 32; } }      // afterwards cnt >= 32
    IC_HD uint32_t peek(uint32_t n) const { return (uint32_t)(buf & ((1ull << n) - 1)); }
    IC_HD void drop(uint32_t n) { if (n > cnt) n = cnt; buf >>= n; cnt -= n; }
    IC_HD uint32_t take(uint32_t n) { const uint32_t v = peek(n); drop(n); return v; }
    IC_HD uint64_t consumed_bits() const { return (uint64_t)p * 8 - cnt; }
    IC_HD bool over() const { return consumed_bits() > (uint64_t)in_len * 8; }      // bits were taken from the zero padding

    // block header, and for a Huffman block its tables. false: decline. Sets in_block, or leaves a stored run in `t` (kind T_STORED), or
    // neither (an empty stored block).
    IC_HD bool begin_block(Token &t)
    {
        refill();
        last = take(1) != 0;
        const uint32_t btype = take(2);
        if (btype == 0) {                               // stored: back to a byte boundary, LEN, ~LEN, bytes
            drop(cnt & 7);
            refill();
            const uint32_t len = take(16), nlen = take(16);
            if ((len ^ nlen) != 0xffffu) return false;
            p -= cnt >> 3;                              // hand the whole bytes still in the bit buffer back to the input (p >= 4 here)
            buf = 0; cnt = 0;
            if (p > in_len || in_len - p < len || out_len - out_pos < len) return false;
            if (len) { t.kind = T_STORED; t.a = len; t.b = p; out_pos += len; }
            p += len;
            in.seek(p);
            return true;
        }
        if (btype == 3) return false;
        if (btype == 1) {
            for (int i = 0; i < 144; i++) w.lens[i] = 8;
            for (int i = 144; i < 256; i++) w.lens[i] = 9;
            for (int i = 256; i < 280; i++) w.lens[i] = 7;
            for (int i = 280; i < 288; i++) w.lens[i] = 8;
            for (int i = 0; i < 32; i++) w.lens[288 + i] = 5;
            if (!build_table(w.lens, 288, LITLEN_BITS, w.litlen, LITLEN_CAP, TK_LITLEN, w)) return false;
            if (!build_table(w.lens + 288, 32, DIST_BITS, w.dist, DIST_CAP, TK_DIST, w)) return false;
            in_block = true;
            return true;
        }
        refill();
        const uint32_t hlit = take(5) + 257, hdist = take(5) + 1, hclen = take(4) + 4;
        if (hlit > 286 || hdist > 30) return false;
        for (int i = 0; i < 19; i++) w.pre_lens[i] = 0;
        for (uint32_t i = 0; i < hclen; i++) {
            refill();
            w.pre_lens[pre_order(i)] = (uint8_t)take(3);
        }
        if (over()) return false;
        if (!build_table(w.pre_lens, 19, PRE_BITS, w.pre, PRE_CAP, TK_PRE, w)) return false;
        const uint32_t total = hlit + hdist;            // <= 316: fits w.lens
        uint32_t n = 0;
        while (n < total) {                             // every iteration adds at least one length
            refill();
            const uint32_t e = IC_UNIFORM(w.pre[peek(PRE_BITS)]);
            if (e_kind(e) != K_LITERAL) return false;
            drop(e_bits(e));
            const uint32_t sym = e_value(e);
            if (sym < 16) { w.lens[n++] = (uint8_t)sym; continue; }
            uint32_t rep, val = 0;
            if (sym == 16) { if (n == 0) return false; val = IC_UNIFORM((uint32_t)w.lens[n - 1]); rep = 3 + take(2); }
            else if (sym == 17) rep = 3 + take(3);
            else if (sym == 18) rep = 11 + take(7);
            else return false;
            if (n + rep > total) return false;
            for (uint32_t i = 0; i < rep; i++) w.lens[n + i] = (uint8_t)val;
            n += rep;
        }
        if (over() || IC_UNIFORM((uint32_t)w.lens[256]) == 0) return false;   // no end-of-block code: not decodable
        if (!build_table(w.lens, (int)hlit, LITLEN_BITS, w.litlen, LITLEN_CAP, TK_LITLEN, w)) return false;
        if (!build_table(w.lens + hlit, (int)hdist, DIST_BITS, w.dist, DIST_CAP, TK_DIST, w)) {
            // a block without matches may carry no usable distance code at all: decodable as long as no length code occurs
            bool any = false;
            for (uint32_t i = 0; i < hdist; i++) any |= IC_UNIFORM((uint32_t)w.lens[hlit + i]) != 0;
            if (any) return false;
            for (int i = 0; i < (1 << DIST_BITS); i++) w.dist[i] = mk(K_INVALID, 0, 0);
        }
        in_block = true;
        return true;
    }

    // The next token. Every call consumes at least one input bit or ends the member, and gives up once bits came from past the input's
    // end: at most 8 * in_len + 1 calls return anything but T_DECLINE.
    IC_HD Token next()
    {
        Token t;
        t.kind = T_DECLINE; t.a = 0; t.b = 0;
        for (;;) {
            if (over()) return t;
            if (!in_block) {
                if (last) {
                    // exactly the announced output, and nothing but the padding of the last byte left in the input
                    if (out_pos == out_len && (consumed_bits() + 7) / 8 == in_len) t.kind = T_DONE;
                    return t;
                }
                if (!begin_block(t) || over()) { t.kind = T_DECLINE; return t; }
                if (t.kind == T_STORED) return t;
                continue;                               // a Huffman block opened, or an empty stored block passed: >= 3 bits consumed
            }
            refill();
            uint32_t e = IC_UNIFORM(w.litlen[peek(LITLEN_BITS)]);
            if (e_kind(e) == K_SUB) {
                drop(e_bits(e));
                e = IC_UNIFORM(w.litlen[e_value(e) + peek(e_extra(e))]);          // inside the sub-table build_table reserved: value + 2^extra <= cap
            }
            const uint32_t kind = e_kind(e);
            if (kind == K_LITERAL) {
                drop(e_bits(e));
                if (out_pos >= out_len) return t;
                out_pos++;
                t.kind = T_LITERAL; t.a = e_value(e);
                return t;
            }
            if (kind == K_END) { drop(e_bits(e)); in_block = false; continue; }
            if (kind != K_LENGTH) return t;
            drop(e_bits(e));
            const uint32_t len = e_value(e) + take(e_extra(e));
            refill();
            uint32_t d = IC_UNIFORM(w.dist[peek(DIST_BITS)]);
            if (e_kind(d) == K_SUB) {
                drop(e_bits(d));
                d = IC_UNIFORM(w.dist[e_value(d) + peek(e_extra(d))]);
            }
            if (e_kind(d) != K_DIST) return t;
            drop(e_bits(d));
            const uint32_t dist = e_value(d) + take(e_extra(d));
            if (over()) return t;
            if (dist > out_pos || len > out_len - out_pos) return t;
            out_pos += len;
            t.kind = T_MATCH; t.a = len; t.b = dist;
            return t;
        }
    }
};

// ---- CRC-32 (gzip polynomial, reflected) in slices ---------------------------------------------------------------------------------------
// A register c that takes in n more bytes becomes c * x^(8n) + (the register that starts at 0 and takes in the same bytes), all mod P: the
// update is linear. So 64 lanes take consecutive slices — lane 0's register starts at 0xffffffff, the others' at 0 —, each multiplies its
// register by x^(8 * bytes behind its slice), and the XOR of the 64 products, inverted, is the CRC-32 of the whole.
constexpr uint32_t CRC_POLY = 0xedb88320u;
IC_HD inline uint32_t crc_byte(uint32_t c, uint32_t b)
{
    c ^= b;
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (CRC_POLY & (0u - (c & 1)));
    return c;
}
// a * b mod P, both in the reflected representation (bit 31 = x^0)
IC_HD inline uint32_t gf2_mulmod(uint32_t a, uint32_t b)
{
    uint32_t prod = 0;
    for (int i = 0; i < 32; i++) {
        prod ^= b & (0u - ((a >> (31 - i)) & 1));
        b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1)));
    }
    return prod;
}
// x^(8n) mod P
IC_HD inline uint32_t crc_x8n(uint32_t n)
{
    uint32_t r = 0x80000000u, base = 0x00800000u;          // x^0, x^8
    for (; n; n >>= 1) { if (n & 1) r = gf2_mulmod(r, base); base = gf2_mulmod(base, base); }
    return r;
}
// bytes per lane when 64 lanes share n bytes: whole 32-bit words, an odd number of them (consecutive lanes then start on different LDS banks)
IC_HD inline uint32_t crc_slice_bytes(uint32_t n) { return (((n + 255) / 256) | 1) * 4; }

}  // namespace inflate_core
