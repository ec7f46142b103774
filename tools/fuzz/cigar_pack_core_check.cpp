// cigar_pack_core_check.cpp — the 16-bit form of a shard's CIGAR array (contextsv_amd/csrc/cigar_pack_core.hpp) on the CPU, under
// AddressSanitizer + UBSan: pack -> unpack round trips, and the escape look-up held against a linear search of the table, on 1e6 random ops
// at escape rates 0, 1e-5, 1e-2 and 1, and on the edge positions (array start and end, the 256-op chunk and 512-op piece edges, runs of
// escapes, shards of 1, 3 and 513 ops, op indices beyond 2^32). Every array lives in a heap block of exactly its size.
// A program of its own: `make -C contextsv_amd/csrc cigar-pack-check`, driven by tests/test_cigar_pack_core.py.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <vector>

#include "../../contextsv_amd/csrc/cigar_pack_core.hpp"

namespace cpk = cigar_pack_core;

static uint64_t n_cases = 0, n_escapes = 0, n_fail = 0;

static void fail(const char *what, uint64_t i)
{
    if (n_fail++ < 20) fprintf(stderr, "FAIL %s at op %llu\n", what, (unsigned long long)i);
}

// the table searched from its first entry to its last: what lookup() must agree with
static uint32_t linear(const uint64_t *tab, uint64_t n_esc, uint64_t i, uint32_t h)
{
    for (uint64_t e = 0; e < n_esc; e++) if ((uint32_t)tab[e] == (uint32_t)i) return (uint32_t)(tab[e] >> 32);
    return h;
}

// one array: packed, every op unpacked and compared; `linear_too`: every escape's look-up against the linear search (quadratic: small arrays)
static void check(const std::vector<uint32_t> &w, bool linear_too)
{
    const uint64_t m = w.size(), np = cpk::n_pieces(m);
    const uint64_t n_esc = cpk::count_escapes(w.data(), m);
    uint16_t *half = new uint16_t[np * cpk::PIECE_OPS];
    uint32_t *piece = new uint32_t[np + 1];
    uint64_t *tab = new uint64_t[n_esc];
    cpk::pack_array(w.data(), m, half, piece, tab);
    n_cases++; n_escapes += n_esc;
    if (piece[0] != 0 || piece[np] != n_esc) fail("piece index ends", np);
    for (uint64_t p = 0; p < np; p++) if (piece[p] > piece[p + 1]) fail("piece index decreases", p);
    for (uint64_t e = 1; e < n_esc; e++)
        if (!((uint32_t)tab[e - 1] < (uint32_t)tab[e])) fail("table not sorted by op index", e);          // (arrays below 2^32 ops here)
    for (uint64_t i = 0; i < m; i++) {
        const uint32_t h = half[i];
        if (cpk::is_escape(h) != cpk::is_escape_word(w[i])) fail("escape mark", i);
        if ((h & 15u) != (w[i] & 15u)) fail("op field", i);
        if (!cpk::is_escape(h) && h != w[i]) fail("halfword is not the word", i);
        if (cpk::unpack(half, piece, tab, i) != w[i]) fail("round trip", i);
        if (linear_too && cpk::is_escape(h) && cpk::lookup(piece, tab, i, h) != linear(tab, n_esc, i, h)) fail("lookup vs linear search", i);
    }
    for (uint64_t i = m; i < np * cpk::PIECE_OPS; i++) if (half[i] != 0) fail("tail of the last piece not zero", i);
    delete[] half; delete[] piece; delete[] tab;
}

static uint32_t cg(uint32_t op, uint32_t len) { return (len << 4) | op; }

int main()
{
    std::mt19937_64 g(0xC16A5EEDull);
    // ---- random arrays of 1e6 ops at the four escape rates
    const double rates[4] = {0.0, 1e-5, 1e-2, 1.0};
    for (double rate : rates) {
        std::vector<uint32_t> w(1000000);
        std::uniform_real_distribution<double> u(0.0, 1.0);
        for (auto &x : w) {
            const uint32_t op = (uint32_t)(g() % 9);
            const bool esc = u(g) < rate;
            const uint32_t len = esc ? 0xFFFu + (uint32_t)(g() % (0x0FFFFFFFu - 0xFFFu + 1)) : (uint32_t)(g() % 0xFFFu);
            x = cg(op, len);
        }
        check(w, rate <= 1e-2);
    }
    // ---- the lengths at the edge of the 12-bit field, every op code
    {
        std::vector<uint32_t> w;
        for (uint32_t len : {0u, 1u, 4093u, 4094u, 4095u, 4096u, 65535u, 65536u, 300000u, (1u << 28) - 1u})
            for (uint32_t op = 0; op < 16; op++) w.push_back(cg(op, len));
        check(w, true);
    }
    // ---- one escape at every edge position of small arrays, and runs of escapes across them
    for (uint64_t m : {1ull, 3ull, 255ull, 256ull, 257ull, 511ull, 512ull, 513ull, 1023ull, 1024ull, 1025ull, 1537ull}) {
        for (uint64_t at : {0ull, 1ull, 63ull, 64ull, 65ull, 255ull, 256ull, 257ull, 511ull, 512ull, 513ull, 1023ull, 1024ull, 1536ull}) {
            if (at >= m) continue;
            std::vector<uint32_t> w(m, cg(0, 20));
            w[at] = cg(2, 70000); check(w, true);
            w[m - 1] = cg(4, (1u << 28) - 1u); check(w, true);
            for (uint64_t run : {2ull, 4ull, 64ull, 300ull, 600ull}) {
                std::vector<uint32_t> v(m, cg(0, 20));
                for (uint64_t i = at; i < m && i < at + run; i++) v[i] = cg((uint32_t)(1 + i % 4), 4095u + (uint32_t)i);
                check(v, true);
            }
        }
        std::vector<uint32_t> all(m);
        for (uint64_t i = 0; i < m; i++) all[i] = cg((uint32_t)(i % 9), 5000u + (uint32_t)i);
        check(all, true);
    }
    // ---- op indices beyond 2^32: the look-up keys on the low 32 bits inside one piece, so five escapes in the three pieces behind op
    // 2^32 + 1024 are found through a per-piece index that really is that long (8 Mi entries, zero in front of them)
    {
        const uint64_t base = (1ull << 32) + 1024, p0 = base >> cpk::PIECE_SHIFT, np = p0 + 3;
        std::vector<uint32_t> piece(np + 1, 0u);
        uint64_t *tab = new uint64_t[5];
        const uint64_t idx[5] = {base + 0, base + 511, base + 512, base + 700, base + 1535};
        const uint32_t val[5] = {cg(2, 4095), cg(3, 70000), cg(4, 4096), cg(1, 99999), cg(5, (1u << 28) - 1u)};
        piece[p0] = 0; piece[p0 + 1] = 2; piece[p0 + 2] = 4; piece[p0 + 3] = 5;
        for (int e = 0; e < 5; e++) tab[e] = cpk::entry(idx[e], val[e]);
        for (int e = 0; e < 5; e++) {
            if (cpk::lookup(piece.data(), tab, idx[e], 0xFFF0u) != val[e]) fail("lookup beyond 2^32", idx[e]);
            n_cases++;
        }
        // an op the table does not hold comes back as its halfword; so does any op of a piece without entries
        if (cpk::lookup(piece.data(), tab, base + 5, 0xFFF3u) != 0xFFF3u || cpk::lookup(piece.data(), tab, base + 1534, 0xFFF1u) != 0xFFF1u ||
            cpk::lookup(piece.data(), tab, 700, 0xFFF2u) != 0xFFF2u) fail("missing entry", base);
        delete[] tab;
    }
    // ---- the threshold: at most one op in 64 may be an escape
    if (!cpk::packs(6400, 100) || cpk::packs(6400, 101) || !cpk::packs(64, 1) || cpk::packs(63, 1) || !cpk::packs(1, 0)) fail("threshold", 0);

    printf("cigar_pack_core_check: %llu cases, %llu escapes, %llu failures\n", (unsigned long long)n_cases, (unsigned long long)n_escapes, (unsigned long long)n_fail);
    return n_fail ? 1 : 0;
}
