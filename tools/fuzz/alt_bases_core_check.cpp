// alt_bases_core_check — the per-base rule of the device's ALT strings (contextsv_amd/csrc/alt_bases_core.hpp) on the CPU, held against a
// literal copy of the host loop (SVCaller::toSVCall, host/sv_caller.cpp:47-62) on edge and random inputs. A program of its own, built by
// `make -C contextsv_amd/csrc alt-check` with g++ under AddressSanitizer + UBSan; the packed sequence of every case lies in a heap block of
// exactly its size, so a byte read past the host's bound is an error here. Driven by tests/test_alt_bases_core.py.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "../../contextsv_amd/csrc/alt_bases_core.hpp"

namespace abc = alt_bases_core;

// the host loop, as it stands in SVCaller::toSVCall: p = the record's packed sequence, n_bytes = seq_off[read + 1] - seq_off[read]
static std::string host_alt(const uint8_t *p, uint64_t n_bytes, uint32_t q0, uint32_t op_len)
{
    std::string alt;
    alt.assign(op_len, 'N');
    if (((uint64_t)q0 + op_len + 1) / 2 <= n_bytes) {
        static const char nt16[] = "=ACMGRSVTWYHKDBN";
        for (uint32_t j = 0; j < op_len; j++) {
            const uint32_t q = q0 + j;
            const char b = nt16[(p[q >> 1] >> ((~q & 1u) << 2)) & 0xf];
            switch (b) {
                case 'R': case 'Y': case 'K': case 'M': case 'S': case 'W': case 'B': case 'D': case 'H': case 'V': alt[j] = 'N'; break;
                default: alt[j] = b;
            }
        }
    }
    return alt;
}

// what a lane per character makes of the same item with the header
static std::string core_alt(const uint8_t *p, uint64_t n_bytes, uint32_t q0, uint64_t len)
{
    std::string alt((size_t)len, '?');
    const bool in = abc::inside(q0, len, n_bytes);
    for (uint64_t j = 0; j < len; j++) {
        char c = 'N';
        if (in) {
            const uint32_t q = q0 + (uint32_t)j;
            c = abc::base(p[abc::byte_of(q)], q);
        }
        alt[(size_t)j] = c;
    }
    return alt;
}

static uint64_t n_cases = 0, n_inside = 0, n_outside = 0, n_fail = 0;

static void one(const std::vector<uint8_t> &seq, uint32_t q0, uint32_t len)
{
    // a heap block of exactly the sequence's bytes (none for an empty one: the pointer must not be read then)
    uint8_t *p = seq.empty() ? nullptr : new uint8_t[seq.size()];
    if (p) memcpy(p, seq.data(), seq.size());
    const std::string want = host_alt(p, seq.size(), q0, len), got = core_alt(p, seq.size(), q0, len);
    n_cases++;
    (abc::inside(q0, len, seq.size()) ? n_inside : n_outside)++;
    if (want != got) {
        if (n_fail++ < 10) printf("MISMATCH: %zu bytes, qpos %u, len %u: host '%s' core '%s'\n", seq.size(), q0, len, want.c_str(), got.c_str());
    }
    delete[] p;
}

int main()
{
    std::mt19937_64 rng(20240611);
    // all sixteen codes at both nibble positions
    std::vector<uint8_t> all;
    for (int hi = 0; hi < 16; hi++) for (int lo = 0; lo < 16; lo++) all.push_back((uint8_t)((hi << 4) | lo));
    for (uint32_t q = 0; q < 512; q++) for (uint32_t len : {1u, 2u, 49u, 50u, 51u}) one(all, q, len);
    // the bound: qpos + len at l_seq - 1, l_seq, l_seq + 1, l_seq + 2 for odd and even l_seq, a non-zero pad nibble, l_seq = 0
    for (uint32_t l_seq : {0u, 1u, 2u, 49u, 50u, 51u, 99u, 100u, 101u, 200u, 201u}) {
        std::vector<uint8_t> seq((l_seq + 1) / 2);
        for (auto &b : seq) b = (uint8_t)rng();
        for (uint32_t len : {0u, 1u, 49u, 50u, 51u, 64u, 65u, 200u}) {
            for (int d = -2; d <= 3; d++) {
                const int64_t q = (int64_t)l_seq + d - (int64_t)len;
                if (q >= 0) one(seq, (uint32_t)q, len);
            }
            one(seq, 0, len);
        }
        one(seq, 1u << 30, 50);
        one(seq, 0xffffffffu, 50);              // (the host's 64-bit sum: far outside, no wrap)
        one(seq, 0xffffffffu, 0);
    }
    // random
    for (int it = 0; it < 200000; it++) {
        const uint32_t l_seq = (uint32_t)(rng() % 300);
        std::vector<uint8_t> seq((l_seq + 1) / 2);
        for (auto &b : seq) b = (uint8_t)rng();
        const uint32_t len = (uint32_t)(rng() % 210), q = (uint32_t)(rng() % (l_seq + 8));
        one(seq, q, len);
    }
    // lengths only the device's 64-bit item can have: outside, without the sum wrapping
    for (uint64_t len : {(uint64_t)1 << 32, (uint64_t)1 << 62, ~(uint64_t)0, ~(uint64_t)0 - (uint64_t)0xffffffffu})
        for (uint32_t q : {0u, 1u, 0xffffffffu}) {
            n_cases++;
            if (abc::inside(q, len, 150)) { n_fail++; printf("MISMATCH: len %llu qpos %u counted as inside 150 bytes\n", (unsigned long long)len, q); }
        }
    printf("alt_bases_core_check: %llu cases, %llu inside, %llu outside, %llu failures\n", (unsigned long long)n_cases, (unsigned long long)n_inside,
           (unsigned long long)n_outside, (unsigned long long)n_fail);
    return n_fail ? 1 : 0;
}
