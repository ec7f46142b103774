// alt_bases_core.hpp — the per-base rule of the 50-base ALT strings cut on the device (kernels/shardbuild.hip, csvgpu_alt_bases_resident):
// whether an item's bases lie inside its record's packed sequence, and which character a 4-bit code becomes. The same text compiles for the
// device (a lane runs it on a base of its own) and for the host with g++ (tools/fuzz/alt_bases_core_check.cpp, under the sanitizers, against
// a literal copy of the host loop): no HIP construct in it.
// It replaces the base loop of SVCaller::toSVCall (host/sv_caller.cpp:47-62; the reference's sv_caller.cpp:572-590, :607-625), character
// for character.
#pragma once
#include <stdint.h>

#ifndef ABC_HD
#define ABC_HD
#endif

namespace alt_bases_core {

// The host's test `((uint64_t)qpos + len + 1) / 2 <= seq_off[read + 1] - seq_off[read]`: a bound on BYTES, so for an odd l_seq the pad
// nibble of the last byte is inside it. The host's len is 32 bits wide; one of 2^62 or more (no sequence has that many bytes) is outside
// without the sum being formed.
ABC_HD inline bool inside(uint32_t qpos, uint64_t len, uint64_t seq_bytes)
{
    if (len >> 62) return false;
    return ((uint64_t)qpos + len + 1) / 2 <= seq_bytes;
}

// Base q of a record whose packed sequence is p[]: the byte it lies in, and the character of its nibble (high nibble first) — the BAM code
// table "=ACMGRSVTWYHKDBN" (SAM spec §4.2.3) with the ten ambiguity codes R Y K M S W B D H V already turned into N.
ABC_HD inline uint64_t byte_of(uint32_t q) { return q >> 1; }
ABC_HD inline char base(uint8_t byte, uint32_t q)
{
    const uint32_t nib = (byte >> ((~q & 1u) << 2)) & 0xfu;
    // "=ACNGNNN" and "TNNNNNNN", the first character in the lowest byte
    const uint64_t lo = 0x4e4e4e474e43413dull, hi = 0x4e4e4e4e4e4e4e54ull;
    return (char)(((nib & 8u) ? hi : lo) >> ((nib & 7u) << 3));
}

}  // namespace alt_bases_core
