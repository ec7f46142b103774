// sort_select_core.hpp — the slot replay of host/sort_select.h ("which element does libstdc++'s std::sort, by length descending, leave at
// slot nth?") stated for lanes: every step of a round is a map over the range, a prefix count or a scatter, so a workgroup runs it
// (kernels/mergeselect.hip) and a loop over "virtual lanes" runs it on the CPU (tools/fuzz/sort_select_core_check.cpp, under the sanitizers,
// against std::sort and against lib_unguarded_partition). The same text compiles with hipcc and with g++: no HIP construct in it.
// It replaces the representative choice of mergeSVs (the reference's sv_object.cpp:190-230; host/sv_caller.cpp mergeSignaturesWithLabels).
//
// One bucket of sz >= 2 members in input order, slot nth, entries x[0 .. sz):
//   limit = 2 * floor(log2 sz)                                   (depth_limit; a caller's bound may lower it)
//   while hi - lo > SMALL:
//       limit == 0: DECLINED (the library heap-sorts here; that is not replayed)          else --limit
//       median_to_first(x, lo, hi)                                one lane
//       pv = len(x[lo]); over p in [lo + 1, hi):                  a map and two prefix counts
//           a(p) = len(x[p]) <= pv      the library's left scan stops here   (!comp(x, pivot))
//           b(p) = len(x[p]) >= pv      the library's right scan stops here  (!comp(pivot, x))
//           a_before(p) = #{q < p : a(q)},  b_after(p) = #{q > p : b(q)}
//       With A the a-positions ascending and B the b-positions descending, the library swaps x[A[k]] <-> x[B[k]] for the K leading k with
//       A[k] < B[k] and nothing else. Position p = A[k] has k = a_before(p) and A[k] < B[k] <=> b_after(p) > k; likewise for q = B[k],
//       k = b_after(q), A[k] < B[k] <=> a_before(q) > k. So every position decides for itself (swaps_a / swaps_b), the swapped ones scatter
//       their position to list_a[k] / list_b[k], and lane k < K swaps the pair. No position is in two pairs.
//       cut = min(A[K], B[K - 1]) = the lowest position that is an UNswapped a-position or a swapped b-position (cut_candidate); none: hi
//       nth >= cut ? lo = cut : hi = cut
//   closing segment [lo, hi), at most SMALL long: the library's final insertion sort is stable inside it, so the member at nth is the one
//   with closing_rank == nth - lo.
#pragma once
#include <stdint.h>

#ifndef SSC_HD
#define SSC_HD
#endif

namespace sort_select_core {

typedef uint64_t Ent;                              // (length << 32) | index in the caller's array: 8 bytes
constexpr uint32_t SMALL = 16;                     // libstdc++'s _S_threshold: ranges up to here are left to the insertion sort
constexpr uint32_t LDS_CAP = 4096;                 // the largest range a workgroup replays in LDS (kernels/mergeselect.hip)
constexpr uint32_t NONE = 0xffffffffu;             // idx_out of a declined or empty segment

SSC_HD inline Ent make_ent(uint32_t len, uint32_t idx) { return ((Ent)len << 32) | idx; }
SSC_HD inline uint32_t len_of(Ent e) { return (uint32_t)(e >> 32); }
SSC_HD inline uint32_t idx_of(Ent e) { return (uint32_t)e; }
SSC_HD inline bool comp(Ent x, Ent y) { return len_of(x) > len_of(y); }       // the comparator: length descending, nothing else

// mergeSVs' slot: top = max(1, (int)(sz * 0.2)) in double precision as the reference writes it, the member at [top / 2]
SSC_HD inline uint32_t top_of(uint64_t sz)
{
    const int t = (int)((double)sz * 0.2);
    return (uint32_t)(t > 1 ? t : 1);
}
SSC_HD inline uint32_t nth_of(uint64_t sz) { return top_of(sz) / 2; }

// std::sort's depth limit, 2 * std::__lg(sz); max_partitions > 0: the caller's own bound where it is lower
SSC_HD inline uint32_t depth_limit(uint64_t sz, uint32_t max_partitions)
{
    uint32_t lg = 0;
    for (uint64_t k = sz; k > 1; k >>= 1) lg++;
    const uint32_t lim = 2 * lg;
    return max_partitions && max_partitions < lim ? max_partitions : lim;
}

// lib_move_median_to_first(lo, lo + 1, lo + (hi - lo) / 2, hi - 1), the library's decision tree verbatim; one lane's work
template <class P>
SSC_HD inline void median_to_first(P x, uint32_t lo, uint32_t hi)
{
    const uint32_t a = lo + 1, b = lo + (hi - lo) / 2, c = hi - 1;
    const Ent va = x[a], vb = x[b], vc = x[c];
    uint32_t m;
    if (comp(va, vb)) {
        if (comp(vb, vc)) m = b;
        else if (comp(va, vc)) m = c;
        else m = a;
    } else if (comp(va, vc)) m = a;
    else if (comp(vb, vc)) m = c;
    else m = b;
    const Ent t = x[lo]; x[lo] = x[m]; x[m] = t;
}

SSC_HD inline bool in_a(uint32_t len, uint32_t pv) { return len <= pv; }
SSC_HD inline bool in_b(uint32_t len, uint32_t pv) { return len >= pv; }
// position p with a_before a-positions below it and b_after b-positions above it
SSC_HD inline bool swaps_a(bool a, uint32_t a_before, uint32_t b_after) { return a && b_after > a_before; }     // it is A[a_before], paired with B[a_before]
SSC_HD inline bool swaps_b(bool b, uint32_t a_before, uint32_t b_after) { return b && a_before > b_after; }     // it is B[b_after], paired with A[b_after]
SSC_HD inline bool cut_candidate(bool a, bool b, uint32_t a_before, uint32_t b_after)
{
    return (a && !swaps_a(a, a_before, b_after)) || swaps_b(b, a_before, b_after);
}
// which side of the cut holds nth
SSC_HD inline void keep_side(uint32_t &lo, uint32_t &hi, uint32_t cut, uint32_t nth) { if (nth >= cut) lo = cut; else hi = cut; }

// The closing segment [lo, hi), hi - lo <= SMALL: where the stable insertion sort puts member i
template <class P>
SSC_HD inline uint32_t closing_rank(P x, uint32_t lo, uint32_t hi, uint32_t i)
{
    const uint32_t li = len_of(x[i]);
    uint32_t r = 0;
    for (uint32_t j = lo; j < hi; j++) {
        const uint32_t lj = len_of(x[j]);
        r += (lj > li) || (lj == li && j < i);
    }
    return r;
}

}  // namespace sort_select_core
