// snptable.hip — kernel #17: a contig's SNP records resident in HBM, and the copy-number pass's tables derived from them (gfx950).
//
// Replaces, for a caller that holds a csv_snp_table, SNPSource::queryFlat per region on the host (host/cnv_caller.cpp) and everything
// cn_run (api/copynumber.hip) builds from the regions' record counts. The rules are snp_table_core.hpp's; the kernels only deal them out:
//   resolve   once per table: a lane per record finds its run's last member by binary search (a run of n equal positions costs log n
//             probes per lane like any other), the run's pfb comes from an inclusive prefix maximum over the flagged indices
//   plan      a lane per region: two binary searches over the table (dependent loads: latency-bound by construction), the first-hit
//             kind's third search, the window count; the lists of the two kernel forms by wave-aggregated appends; the totals
//   offsets   exclusive sums (sort.hip) over the window counts and the record counts; the per-shard relative offsets by subtraction
//   gather    a lane per record of the compact layout: its region by binary search over the offsets
#include <algorithm>

#include "../common.hpp"
#include "../devutil.hpp"
#include "../snp_table_core.hpp"

namespace csv {

constexpr int SNP_THREADS = 256;
static inline uint32_t snp_blocks(uint64_t items) { return (uint32_t)std::min<uint64_t>((items + SNP_THREADS - 1) / SNP_THREADS, ST_MAX_BLOCKS); }

// ---- resolve ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SNP_THREADS) void snp_mark_kernel(const uint8_t *__restrict__ has_pfb, uint32_t n, int32_t *__restrict__ marks)
{
    const uint32_t stride = gridDim.x * SNP_THREADS;
    for (uint64_t i = blockIdx.x * SNP_THREADS + threadIdx.x; i < n; i += stride) marks[i] = snpcore::mark((uint32_t)i, has_pfb[i] != 0);
}

__global__ __launch_bounds__(SNP_THREADS) void snp_resolve_kernel(const uint32_t *__restrict__ pos, const uint64_t *__restrict__ baf, const uint64_t *__restrict__ pfb,
                                                                  const int32_t *__restrict__ pm, uint32_t n, uint64_t *__restrict__ baf_out,
                                                                  uint64_t *__restrict__ pfb_out)
{
    const uint32_t stride = gridDim.x * SNP_THREADS;
    for (uint64_t i64 = blockIdx.x * SNP_THREADS + threadIdx.x; i64 < n; i64 += stride) {
        const uint32_t i = (uint32_t)i64, j = snpcore::run_last(pos, n, i);
        baf_out[i] = baf[j];
        if (pfb_out) pfb_out[i] = pm ? snpcore::resolved_pfb_bits(pos, pfb, i, pm[j]) : 0;
    }
}

void launch_snp_resolve(hipStream_t s, const uint32_t *pos, const uint64_t *baf, const uint64_t *pfb, const uint8_t *has_pfb, uint32_t n, int32_t *marks, int32_t *pm,
                        void *pm_tmp, uint64_t *baf_out, uint64_t *pfb_out)
{
    if (n == 0) return;
    const bool flagged = pfb_out && has_pfb;
    if (flagged) {
        hipLaunchKernelGGL(snp_mark_kernel, dim3(snp_blocks(n)), dim3(SNP_THREADS), 0, s, has_pfb, n, marks);
        launch_prefix_max(s, marks, pm, n, pm_tmp);
    }
    hipLaunchKernelGGL(snp_resolve_kernel, dim3(snp_blocks(n)), dim3(SNP_THREADS), 0, s, pos, baf, pfb, flagged ? pm : nullptr, n, baf_out, pfb_out);
}

// ---- plan ------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// this lane's slot in a list that every flagged lane of the wave appends to: one atomic per wave
__device__ __forceinline__ uint32_t wave_append(bool flag, uint32_t *counter)
{
    const unsigned long long m = __ballot(flag);
    const int lane = lane_id();
    uint32_t base = 0;
    if (lane == 0 && m) base = atomicAdd(counter, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, 0, 64);
    return base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

__global__ __launch_bounds__(SNP_THREADS) void cn_plan_kernel(CnPlan p, uint32_t R)
{
    const uint32_t stride = gridDim.x * SNP_THREADS;
    unsigned long long W = 0, S = 0;
    bool over = false;
    for (uint64_t base = (uint64_t)blockIdx.x * SNP_THREADS; base < R; base += stride) {         // (whole waves stay in the loop: the ballots)
        const uint64_t r64 = base + threadIdx.x;
        const bool valid = r64 < R;
        const uint32_t r = (uint32_t)r64;
        uint32_t nw = 0;
        if (valid) {
            const SnpTabDev t = p.tabs[p.rsh ? p.rsh[r] : 0u];
            uint32_t first, count;
            snpcore::range(t.pos, t.n, p.rs[r], p.re[r], first, count);
            p.sfirst[r] = first; p.soff[r] = count;
            p.hit[r] = t.n_af ? snpcore::first_hit(t.pos, first, count, t.af_pos, t.n_af) : snpcore::NO_HIT;
            nw = snpcore::window_count(p.ssf ? p.ssf[r] : 1, count);
            if (nw > CN_MAX_WINDOWS) { over = true; nw = CN_MAX_WINDOWS; }             // (the caller declines: nothing behind the flag is used)
            p.ss[r] = (int32_t)nw; p.wbase[r] = nw;
            W += nw; S += count;
        }
        const bool is_small = valid && nw <= CN_SMALL_MAX, is_big = valid && nw > CN_SMALL_MAX;
        const uint32_t a = wave_append(is_small, &p.head->n_small), b = wave_append(is_big, &p.head->n_big);
        if (is_small) p.small[a] = r;
        if (is_big) p.big[b] = r;
    }
    W = wave_sum_u64(W); S = wave_sum_u64(S);
    if (lane_id() == 0) {
        if (W) atomicAdd(&p.head->W, W);
        if (S) atomicAdd(&p.head->S, S);
    }
    if (over) atomicOr(&p.head->flags, (uint32_t)CN_PLAN_OVER_WINDOWS);
    if (blockIdx.x == 0 && threadIdx.x == 0) { p.wbase[R] = 0; p.soff[R] = 0; }
}

// behind the two exclusive sums: the offsets relative to each shard's first window, and every shard's first window for the readback
__global__ __launch_bounds__(SNP_THREADS) void cn_plan_offsets_kernel(CnPlan p, uint32_t R, uint32_t n_shards)
{
    const uint32_t stride = gridDim.x * SNP_THREADS, first = blockIdx.x * SNP_THREADS + threadIdx.x;
    for (uint64_t r64 = first; r64 < R; r64 += stride) {
        const uint32_t r = (uint32_t)r64, s = p.rsh ? p.rsh[r] : 0u;
        const uint32_t w0 = p.wbase[p.reg_off[s]];
        p.wo[(uint64_t)r + s] = p.wbase[r] - w0;
        if (r + 1u == p.reg_off[s + 1u]) p.wo[(uint64_t)r + 1u + s] = p.wbase[r + 1u] - w0;
    }
    for (uint64_t s = first; s <= n_shards; s += stride) p.shard_w0[s] = p.wbase[p.reg_off[s]];
}

void launch_cn_plan(hipStream_t s, const CnPlan &p, uint32_t R, uint32_t n_shards)
{
    (void)hipMemsetAsync(p.head, 0, CN_PLAN_HEAD_BYTES, s);
    hipLaunchKernelGGL(cn_plan_kernel, dim3(snp_blocks(R)), dim3(SNP_THREADS), 0, s, p, R);
    launch_exclusive_sum_u32(s, p.wbase, (uint64_t)R + 1, p.es_tmp);
    launch_exclusive_sum_u32(s, p.soff, (uint64_t)R + 1, p.es_tmp);
    hipLaunchKernelGGL(cn_plan_offsets_kernel, dim3(snp_blocks(std::max<uint64_t>(R, (uint64_t)n_shards + 1))), dim3(SNP_THREADS), 0, s, p, R, n_shards);
}

// ---- gather ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SNP_THREADS) void snp_gather_kernel(CnPlan p, uint32_t R, uint32_t S, uint32_t *__restrict__ spos, uint64_t *__restrict__ sbaf,
                                                                 uint64_t *__restrict__ spfb)
{
    const uint32_t stride = gridDim.x * SNP_THREADS;
    for (uint64_t k64 = blockIdx.x * SNP_THREADS + threadIdx.x; k64 < S; k64 += stride) {
        const uint32_t k = (uint32_t)k64;
        const uint32_t r = snpcore::first_gt(p.soff, 0, R + 1u, k) - 1u;             // soff[r] <= k < soff[r + 1]: soff[0] = 0, soff[R] = S > k
        const SnpTabDev t = p.tabs[p.rsh ? p.rsh[r] : 0u];
        const uint32_t i = p.sfirst[r] + (k - p.soff[r]);
        const uint32_t x = t.pos[i];
        spos[k] = x; sbaf[k] = t.baf[i];
        spfb[k] = t.pfb ? t.pfb[i] : snpcore::hit_pfb_bits(x, p.hit[r], t.af_pos, t.af);
    }
}

void launch_snp_gather(hipStream_t s, const CnPlan &p, uint32_t R, uint32_t S, uint32_t *spos, uint64_t *sbaf, uint64_t *spfb)
{
    if (S) hipLaunchKernelGGL(snp_gather_kernel, dim3(snp_blocks(S)), dim3(SNP_THREADS), 0, s, p, R, S, spos, sbaf, spfb);
}

}  // namespace csv
