// snp_table_core.hpp — the per-region rules of a resident SNP table (csv_snp_table; kernels/snptable.hip), free of HIP calls: the kernels
// use them as they stand and the CPU check (tools/fuzz/snp_table_core_check.cpp) holds them against the host mirror's two SNPSource forms.
//
// A table is one contig's records by ascending position. What SNPSource::queryFlat appends for a region [start, end]:
//   range     the records from lower_bound(pos, start) up to the first pos > end (nothing when start > end)
//   baf       every member of a run of equal positions carries the baf of the run's LAST member (the reference's hash map keeps the
//             later write)
//   pfb       per-record kind (SNPTable): the pfb of the run's last member that has one, else 0.0. A run never straddles a region boundary,
//             so baf and pfb do not depend on the query: they are resolved once, when the table is created.
//             first-hit kind (SNPFileTable through the default queryFlat): with lo / hi the region's first and last record position and
//             g = lower_bound(af_pos, lo): if g < n_af and af_pos[g] <= hi, the records at af_pos[g] get af[g]; every other record 0.0.
//   windows   a region has max(sample_size, records) windows.
// Values travel as their 64 bits: a NaN stays that NaN.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SNPCORE_HD __host__ __device__ __forceinline__
#else
#define SNPCORE_HD static inline
#endif

namespace snpcore {

constexpr uint32_t NO_HIT = 0xffffffffu;

// first index in [lo, n] with a[i] >= key (a ascending)
SNPCORE_HD uint32_t first_ge(const uint32_t *a, uint32_t lo, uint32_t n, uint32_t key)
{
    uint32_t hi = n;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (a[mid] < key) lo = mid + 1; else hi = mid; }
    return lo;
}
// first index in [lo, n] with a[i] > key
SNPCORE_HD uint32_t first_gt(const uint32_t *a, uint32_t lo, uint32_t n, uint32_t key)
{
    uint32_t hi = n;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (a[mid] <= key) lo = mid + 1; else hi = mid; }
    return lo;
}

// the records of [start, end]: [first, first + count)
SNPCORE_HD void range(const uint32_t *pos, uint32_t n, uint32_t start, uint32_t end, uint32_t &first, uint32_t &count)
{
    first = 0; count = 0;
    if (start > end || n == 0) return;
    first = first_ge(pos, 0, n, start);
    count = first_gt(pos, first, n, end) - first;
}

// last member of the run of equal positions that record i belongs to
SNPCORE_HD uint32_t run_last(const uint32_t *pos, uint32_t n, uint32_t i) { return first_gt(pos, i, n, pos[i]) - 1u; }

// The pfb of a run is found with an inclusive prefix maximum over mark(i, has_pfb[i]): at the run's last member j the maximum names the
// last flagged record at or in front of j, which belongs to the run exactly when it has the run's position. The marks are compared as
// signed 32-bit numbers (the prefix maximum's type): index + 1 with the top bit flipped, so that any n below 2^32 - 1 keeps its order.
SNPCORE_HD int32_t mark(uint32_t i, bool flagged) { return (int32_t)((flagged ? i + 1u : 0u) ^ 0x80000000u); }
SNPCORE_HD uint64_t resolved_pfb_bits(const uint32_t *pos, const uint64_t *pfb_bits, uint32_t i, int32_t prefix_max_at_run_last)
{
    const uint32_t u = (uint32_t)prefix_max_at_run_last ^ 0x80000000u;      // last flagged index + 1, or 0
    if (u == 0 || pos[u - 1u] != pos[i]) return 0;                            // +0.0
    return pfb_bits ? pfb_bits[u - 1u] : 0;
}

// first-hit kind: the AF record a region's records [first, first + count) select, or NO_HIT
SNPCORE_HD uint32_t first_hit(const uint32_t *pos, uint32_t first, uint32_t count, const uint32_t *af_pos, uint32_t n_af)
{
    if (count == 0 || n_af == 0) return NO_HIT;
    const uint32_t lo = pos[first], hi = pos[first + count - 1u];
    const uint32_t g = first_ge(af_pos, 0, n_af, lo);
    return g < n_af && af_pos[g] <= hi ? g : NO_HIT;
}
SNPCORE_HD uint64_t hit_pfb_bits(uint32_t p, uint32_t hit, const uint32_t *af_pos, const uint64_t *af_bits)
{
    return hit != NO_HIT && af_pos[hit] == p ? af_bits[hit] : 0;
}

SNPCORE_HD uint32_t window_count(int32_t sample_size, uint32_t count) { return (uint32_t)sample_size > count ? (uint32_t)sample_size : count; }

}  // namespace snpcore
