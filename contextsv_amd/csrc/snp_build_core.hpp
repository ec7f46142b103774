// snp_build_core.hpp — the rules of the SNP table builder (kernels/snpbuild.hip, api/snp_build.hip), in a form that compiles with g++ and
// with hipcc: no allocation, no libc. What they replace is the `keep` lambda and the merge loop of SNPFile::load (host/snp_io.cpp), which
// find a record's contig with a memcmp per record and append it to that contig's vectors in file order. The stand-alone check
// (tools/fuzz/snp_build_core_check.cpp) runs the same functions against that loop.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SNPB_HD __host__ __device__
#else
#define SNPB_HD
#endif

namespace snpbuild {

constexpr uint32_t ID_LIMIT = 1u << 16;          // contig ids are below this
constexpr uint64_t KEY_LIMIT = 1ull << 48;       // order keys (text_base + line_off) are below this
// a record's `run` word: the global run number of a device-appended record, or HOST_TAG | contig id of a host-appended one
constexpr uint32_t HOST_TAG = 0x80000000u;

// Two CHROM fields of one text differ: another length or another byte. Byte loads only, all inside [off, off + len) of a field, so
// nothing outside the text is touched whatever its alignment (the parser's promise of the aligned 16-byte pieces holds trivially).
SNPB_HD inline bool chrom_differs(const uint8_t *text, uint32_t off_a, uint32_t len_a, uint32_t off_b, uint32_t len_b)
{
    if (len_a != len_b) return true;
    for (uint32_t i = 0; i < len_a; i++)
        if (text[off_a + i] != text[off_b + i]) return true;
    return false;
}

// Kept record k of a call starts a run: the first kept record, or a CHROM other than kept record k - 1's. Lines between two kept records
// (skipped, deferred) are not looked at.
SNPB_HD inline bool starts_run(const uint8_t *text, const uint32_t *line_off, const uint32_t *chrom_len, uint32_t k)
{
    return k == 0 || chrom_differs(text, line_off[k], chrom_len[k], line_off[k - 1], chrom_len[k - 1]);
}

// the bits that hold every value up to and including v (0 for 0)
SNPB_HD inline int bits_for(uint64_t v)
{
    int b = 0;
    while (v) { b++; v >>= 1; }
    return b;
}

// The one sort key of finish: the contig id above the order key. `shift` = bits_for(the largest order key of the builder) <= 48, so that
// the digits above are constant and the sort need not visit them; with shift == 48 this is the fixed packing id << 48 | key.
SNPB_HD inline uint64_t pack_key(uint32_t id, uint64_t key, int shift) { return ((uint64_t)id << shift) | key; }
SNPB_HD inline uint32_t id_of(uint64_t packed, int shift) { return (uint32_t)(packed >> shift); }

SNPB_HD inline uint32_t contig_of(uint32_t run_word, const uint32_t *run_contig)
{
    return (run_word & HOST_TAG) ? (run_word & ~HOST_TAG) : run_contig[run_word];
}

}  // namespace snpbuild
