// inflate_core_check.cpp — contextsv_amd/csrc/inflate_core.hpp (the sequential core of the device's DEFLATE decoder) on the CPU, under
// AddressSanitizer + UBSan. A program of its own, no GPU: built by `make -C contextsv_amd/csrc inflate-check`, driven by
// tests/test_inflate_core.py, which writes the corpus of tests/inflate_inputs.py to a file.
//   usage: inflate_core_check CORPUS
//   corpus: "ICC1", u32 count, then per record: u32 flags, u32 in_len, u32 out_len, u32 crc32, in bytes, out bytes (the original data)
//           flags bit 0: a stream zlib (or the helper's own encoder) made — it must decode, equal zlib's bytes and CRC, and be declined with
//           out_len one less or one more; clear: a damaged stream — declined, or decoded to exactly the original bytes.
// The core runs as the kernel runs it — tokens from Decoder::next, a plain scalar copy loop for the matches (the kernel's replicated
// pattern: src = pos - dist + i mod dist), the CRC-32 in 64 slices combined by x^(8n) — with the input and the output in heap blocks of
// exactly in_len and out_len bytes, so that the sanitizer sees any byte outside them; the work area is a heap block too.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <zlib.h>

#include <memory>
#include <vector>

#include "../../contextsv_amd/csrc/inflate_core.hpp"

namespace ic = inflate_core;

struct HostIn {
    const uint8_t *p;
    uint32_t n;
    uint32_t get32(uint32_t pos) const
    {
        uint32_t v = 0;
        for (uint32_t b = 0; b < 4; b++) if (pos + b < n) v |= (uint32_t)p[pos + b] << (8 * b);
        return v;
    }
    void seek(uint32_t) {}
};

// the kernel's CRC: 64 slices of whole words, each lane's register moved to the end by x^(8 * bytes behind it)
static uint32_t crc_sliced(const uint8_t *d, uint32_t n)
{
    const uint32_t L = ic::crc_slice_bytes(n);
    uint32_t acc = 0;
    for (uint32_t lane = 0; lane < 64; lane++) {
        const uint64_t b0 = (uint64_t)lane * L;
        const uint32_t lo = (uint32_t)(b0 < n ? b0 : n), hi = (uint32_t)(b0 + L < n ? b0 + L : n);
        uint32_t c = lane == 0 ? 0xffffffffu : 0;
        for (uint32_t i = lo; i < hi; i++) c = ic::crc_byte(c, d[i]);
        acc ^= ic::gf2_mulmod(c, ic::crc_x8n(n - hi));
    }
    return ~acc;
}

// 0: decoded exactly out_len bytes, stream consumed, CRC equal; 1: declined
static int decode(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_len, uint32_t want_crc, long &n_tokens)
{
    std::unique_ptr<ic::Work> w(new ic::Work);
    memset(w.get(), 0xA5, sizeof(ic::Work));               // nothing in the work area may be read before the decoder wrote it
    HostIn src{in, in_len};
    ic::Decoder<HostIn> dec(src, *w, in_len, out_len);
    uint32_t pos = 0;
    long budget = (long)in_len * 8 + 2;                    // every token but the last consumes at least one input bit
    for (;;) {
        const ic::Token t = dec.next();
        n_tokens++;
        if (--budget < 0) { fprintf(stderr, "FAIL: more tokens than input bits\n"); exit(1); }
        if (t.kind == ic::T_DECLINE) return 1;
        if (t.kind == ic::T_DONE) break;
        if (t.kind == ic::T_LITERAL) { out[pos++] = (uint8_t)t.a; continue; }
        if (t.kind == ic::T_STORED) { for (uint32_t i = 0; i < t.a; i++) out[pos + i] = in[t.b + i]; pos += t.a; continue; }
        const uint32_t len = t.a, dist = t.b;
        for (uint32_t i = 0; i < len; i++) out[pos + i] = out[pos - dist + (dist < len ? i % dist : i)];
        pos += len;
    }
    if (pos != out_len || dec.out_pos != out_len) { fprintf(stderr, "FAIL: T_DONE at %u of %u bytes\n", pos, out_len); exit(1); }
    return crc_sliced(out, out_len) == want_crc ? 0 : 1;
}

static std::vector<uint8_t> zlib_inflate(const uint8_t *in, uint32_t in_len, uint32_t cap)
{
    std::vector<uint8_t> out(cap + 1);
    z_stream zs;
    memset(&zs, 0, sizeof zs);
    if (inflateInit2(&zs, -15) != Z_OK) { fprintf(stderr, "inflateInit2 failed\n"); exit(2); }
    zs.next_in = const_cast<Bytef *>(in); zs.avail_in = in_len;
    zs.next_out = out.data(); zs.avail_out = (uInt)out.size();
    const int rc = inflate(&zs, Z_FINISH);
    const size_t n = zs.total_out;
    inflateEnd(&zs);
    if (rc != Z_STREAM_END) { fprintf(stderr, "FAIL: zlib does not decode an intact record (rc %d)\n", rc); exit(1); }
    out.resize(n);
    return out;
}

int main(int argc, char **argv)
{
    // the formulas against RFC 1951's tables, and the sliced CRC against zlib at every small length
    static const uint16_t len_base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const uint8_t len_extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    static const uint16_t dist_base[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577};
    static const uint8_t dist_extra[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};
    static const uint8_t pre_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    int fail = 0;
    for (uint32_t s = 0; s < 29; s++) if (ic::len_base(s) != len_base[s] || ic::len_extra(s) != len_extra[s]) { fprintf(stderr, "FAIL: length code %u\n", s); fail++; }
    for (uint32_t d = 0; d < 30; d++) if (ic::dist_base(d) != dist_base[d] || ic::dist_extra(d) != dist_extra[d]) { fprintf(stderr, "FAIL: distance code %u\n", d); fail++; }
    for (uint32_t i = 0; i < 19; i++) if (ic::pre_order(i) != pre_order[i]) { fprintf(stderr, "FAIL: code-length order %u\n", i); fail++; }
    {
        std::vector<uint8_t> buf(70000);
        uint32_t x = 12345;
        for (auto &b : buf) { x = x * 1664525u + 1013904223u; b = (uint8_t)(x >> 24); }
        for (uint32_t n = 0; n <= 70000; n += (n < 1100 ? 1 : 997)) {
            std::unique_ptr<uint8_t[]> d(new uint8_t[n ? n : 1]);
            memcpy(d.get(), buf.data(), n);
            if (crc_sliced(d.get(), n) != (uint32_t)crc32(crc32(0L, Z_NULL, 0), d.get(), n)) { fprintf(stderr, "FAIL: sliced CRC at %u bytes\n", n); fail++; }
        }
    }
    if (argc < 2) { fprintf(stderr, "usage: %s CORPUS\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char magic[4];
    uint32_t count = 0;
    if (fread(magic, 1, 4, f) != 4 || memcmp(magic, "ICC1", 4) != 0 || fread(&count, 4, 1, f) != 1) { fprintf(stderr, "bad corpus header\n"); return 2; }
    long n_intact = 0, n_damaged = 0, n_declined_damaged = 0, n_tokens = 0;
    for (uint32_t r = 0; r < count; r++) {
        uint32_t h[4];
        if (fread(h, 4, 4, f) != 4) { fprintf(stderr, "corpus truncated at record %u\n", r); return 2; }
        const uint32_t flags = h[0], in_len = h[1], out_len = h[2], crc = h[3];
        if (in_len > ic::MAX_BLOCK || out_len > ic::MAX_BLOCK) { fprintf(stderr, "record %u larger than a BGZF member\n", r); return 2; }
        // exact-size heap blocks: one byte outside either is a sanitizer report
        std::unique_ptr<uint8_t[]> in(new uint8_t[in_len ? in_len : 1]), want(new uint8_t[out_len ? out_len : 1]);
        if ((in_len && fread(in.get(), 1, in_len, f) != in_len) || (out_len && fread(want.get(), 1, out_len, f) != out_len)) { fprintf(stderr, "corpus truncated in record %u\n", r); return 2; }
        std::unique_ptr<uint8_t[]> out(new uint8_t[out_len ? out_len : 1]);
        memset(out.get(), 0xEE, out_len ? out_len : 1);
        const int st = decode(in.get(), in_len, out.get(), out_len, crc, n_tokens);
        if (flags & 1) {
            n_intact++;
            const std::vector<uint8_t> z = zlib_inflate(in.get(), in_len, out_len);
            const uint32_t zcrc = (uint32_t)crc32(crc32(0L, Z_NULL, 0), z.data(), (uInt)z.size());
            if (z.size() != out_len || memcmp(z.data(), want.get(), out_len) != 0 || zcrc != crc) { fprintf(stderr, "FAIL: record %u: the corpus disagrees with zlib\n", r); fail++; continue; }
            if (st != 0) { fprintf(stderr, "FAIL: record %u (in %u, out %u): an intact stream was declined\n", r, in_len, out_len); fail++; continue; }
            if (memcmp(out.get(), z.data(), out_len) != 0) { fprintf(stderr, "FAIL: record %u: bytes differ from zlib's\n", r); fail++; continue; }
            // the announced size must be exact
            for (int d = -1; d <= 1; d += 2) {
                if ((d < 0 && out_len == 0) || (d > 0 && out_len == ic::MAX_BLOCK)) continue;
                const uint32_t n2 = out_len + d;
                std::unique_ptr<uint8_t[]> o2(new uint8_t[n2 ? n2 : 1]);
                const uint32_t crc2 = (uint32_t)crc32(crc32(0L, Z_NULL, 0), want.get(), d < 0 ? n2 : out_len);
                if (decode(in.get(), in_len, o2.get(), n2, crc2, n_tokens) == 0) { fprintf(stderr, "FAIL: record %u: accepted with out_len %+d\n", r, d); fail++; }
            }
        } else {
            n_damaged++;
            if (st != 0) n_declined_damaged++;
            else if (memcmp(out.get(), want.get(), out_len) != 0) { fprintf(stderr, "FAIL: record %u: a damaged stream was accepted with other bytes\n", r); fail++; }
        }
    }
    fclose(f);
    printf("inflate_core_check: %ld intact, %ld damaged (%ld declined), %ld tokens, %d failures\n", n_intact, n_damaged, n_declined_damaged, n_tokens, fail);
    return fail ? 1 : 0;
}
