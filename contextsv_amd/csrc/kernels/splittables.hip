// splittables.hip — kernel #10: the member and supplementary tables of the split-read pass, built from the resident shards (gfx950).
//
// Replaces the interval gather, membersOf and the flattening of fitsOnDevice (host/split_caller.cpp) in front of the groups -> fits chain:
// everything csv_split_tables holds — pos, flag and the scan's ref_end / q_start / q_end of the records that take part — already lies in HBM
// in the shards, and which records go where is known when SplitPass::prepare() ends. The call's references (csv_split_refs: a record index
// per member, a record index or an "other tid" byte per supplementary entry) come up, one launch writes the eleven arrays where the chain
// reads them.
//
// One thread per member and one per supplementary entry, all segments (contigs) of the call in one launch: items [0, n_members) are the
// members, [n_members, n_members + n_supp) the entries. A gather, bound by latency: every thread issues its five loads at once. A member finds
// its segment by a search over seg_off (the last c with seg_off[c] <= m: empty segments repeat a value, the last of them owns the member), an
// entry first finds its member the same way over supp_off. seg_off sits in LDS when the call has at most ST_SEG_LDS - 1 segments (every run:
// a contig per segment); beyond that the same search reads it from global memory. The grid is capped and strides.
//
// The kernel also checks the fits' domain (csvgpu.h: every coordinate >= 0, end >= start, for members and same-tid entries), since no host
// loop sees these tables: a violation ORs `err_bit` into *err, which travels in a readback the caller makes anyway.
#include <algorithm>

#include "../common.hpp"

namespace csv {

constexpr int ST_THREADS = 256;
constexpr uint32_t ST_SEG_LDS = 1024;      // seg_off entries held in LDS (8 KiB)

// the last c in [0, n) with off[c] <= x (off[0] == 0 <= x)
__device__ __forceinline__ uint64_t st_owner(const uint64_t *off, uint64_t n, uint64_t x)
{
    uint64_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

struct StRow { int32_t start, end, q_start, q_end; uint32_t reverse; };

__device__ __forceinline__ StRow st_row(const SplitTabSeg &S, uint32_t r)
{
    StRow o;
    const int32_t pos = S.pos[r], ref_end = S.ref_end[r], qs = S.q_start[r], qe = S.q_end[r];
    const uint32_t flag = S.flag[r];
    o.start = (int32_t)((uint32_t)pos + 1u);
    o.end = ref_end; o.q_start = qs; o.q_end = qe;
    o.reverse = (flag & 0x10u) ? 1u : 0u;
    return o;
}

__device__ __forceinline__ bool st_outside(const StRow &o) { return o.start < 0 || o.q_start < 0 || o.q_end < 0 || o.end < o.start; }

__global__ __launch_bounds__(ST_THREADS) void st_tables_kernel(SplitTablesIn in, SplitTablesOut out)
{
    __shared__ uint64_t s_seg[ST_SEG_LDS];
    const bool in_lds = in.n_seg + 1 <= (uint64_t)ST_SEG_LDS;
    if (in_lds) {
        for (uint32_t i = threadIdx.x; i <= (uint32_t)in.n_seg; i += ST_THREADS) s_seg[i] = in.seg_off[i];
        __syncthreads();
    }
    const uint64_t *seg_off = in_lds ? s_seg : in.seg_off;
    const uint64_t n_items = (uint64_t)in.n_members + in.n_supp, stride = (uint64_t)gridDim.x * ST_THREADS;
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x; i < n_items; i += stride) {
        if (i < in.n_members) {
            const SplitTabSeg S = in.seg[st_owner(seg_off, in.n_seg, i)];
            const StRow o = st_row(S, in.member_rec[i]);
            out.start[i] = o.start; out.end[i] = o.end; out.q_start[i] = o.q_start; out.q_end[i] = o.q_end;
            out.reverse[i] = (uint8_t)o.reverse;
            bad |= st_outside(o);
            continue;
        }
        const uint64_t z = i - in.n_members;
        const uint32_t where = in.supp_where[z];
        StRow o{0, 0, 0, 0, where};
        if (where == 0) {
            const uint64_t m = st_owner(in.supp_off, in.n_members, z);
            const SplitTabSeg S = in.seg[st_owner(seg_off, in.n_seg, m)];
            o = st_row(S, in.supp_rec[z]);
            bad |= st_outside(o);
        }
        out.supp_start[z] = o.start; out.supp_end[z] = o.end; out.supp_q_start[z] = o.q_start; out.supp_q_end[z] = o.q_end;
        out.supp_flags[z] = (uint8_t)o.reverse;
    }
    if (bad) atomicOr(out.err, out.err_bit);
}

void launch_st_tables(hipStream_t s, const SplitTablesIn &in, const SplitTablesOut &out)
{
    const uint64_t n_items = (uint64_t)in.n_members + in.n_supp;
    if (!n_items) return;
    const uint64_t blocks = std::min<uint64_t>((n_items + ST_THREADS - 1) / ST_THREADS, ST_MAX_BLOCKS);
    hipLaunchKernelGGL(st_tables_kernel, dim3((uint32_t)blocks), dim3(ST_THREADS), 0, s, in, out);
}

}  // namespace csv
