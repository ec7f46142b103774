// snpbuild.hip — kernel #19: the kept records of VCF text batches cut by contig on the device (gfx950); csvgpu_snp_builder_* / _columns_*.
//
// Replaces the `keep` lambda and the merge loop of SNPFile::load (host/snp_io.cpp: a memcmp and a push_back per record on one thread) and
// the `sorted` copy of SNPFile::table. The rules are snp_build_core.hpp's; the kernels only deal them out, a lane per record, striding
// over a capped grid:
//   flags     kept record k starts a CHROM run (compared through the text, byte loads inside the two fields only)
//   append    behind the exclusive sum of the flags (sort.hip): the run table of the call, and every record at the builder's tail with
//             its global run number and its order key
//   keys      finish: (contig id, order key) packed into one sort key, the record's index as the value
//   columns   behind the radix sort (sort.hip): pos / baf gathered into the order, every contig's first and last slot, its descents, and
//             whether two neighbours share a key
// Every kernel is bound by the latency of a few dependent loads per lane; none holds more than a handful of registers.
#include <algorithm>

#include "../common.hpp"
#include "../devutil.hpp"
#include "../snp_build_core.hpp"

namespace csv {

constexpr int SB_THREADS = 256;
static inline uint32_t sb_blocks(uint64_t items) { return (uint32_t)std::min<uint64_t>((items + SB_THREADS - 1) / SB_THREADS, SB_MAX_BLOCKS); }

// flags[k] = 1 where kept record k starts a run, flags[n] = 0 (the slot that holds the total once the sums are made)
__global__ __launch_bounds__(SB_THREADS) void sb_flags_kernel(const uint8_t *__restrict__ text, const uint32_t *__restrict__ line_off,
                                                              const uint32_t *__restrict__ chrom_len, uint32_t n, uint32_t *__restrict__ flags)
{
    const uint32_t stride = gridDim.x * SB_THREADS;
    for (uint64_t k = blockIdx.x * SB_THREADS + threadIdx.x; k <= n; k += stride)
        flags[k] = k < n && snpbuild::starts_run(text, line_off, chrom_len, (uint32_t)k) ? 1u : 0u;
}

// ridx: the exclusive sums of the flags, [n + 1]. Record k belongs to run ridx[k + 1] - 1 of the call and starts it where ridx[k + 1] != ridx[k].
__global__ __launch_bounds__(SB_THREADS) void sb_append_kernel(SnpAppendArgs a)
{
    const uint32_t stride = gridDim.x * SB_THREADS;
    for (uint64_t k = blockIdx.x * SB_THREADS + threadIdx.x; k < a.n; k += stride) {
        const uint32_t before = a.ridx[k], r = a.ridx[k + 1] - 1, off = a.line_off[k];
        if (before == r) { a.run_first[r] = (uint32_t)k; a.run_line_off[r] = off; a.run_chrom_len[r] = a.chrom_len[k]; }
        const uint64_t at = a.tail + k;
        a.pos[at] = a.rec_pos[k];
        a.baf[at] = a.rec_baf[k];
        a.run[at] = a.run_base + r;
        a.key[at] = a.text_base + off;
    }
}

__global__ __launch_bounds__(SB_THREADS) void sb_keys_kernel(const uint32_t *__restrict__ run, const uint64_t *__restrict__ key, const uint32_t *__restrict__ run_contig,
                                                             uint32_t n, int shift, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint32_t stride = gridDim.x * SB_THREADS;
    for (uint64_t i = blockIdx.x * SB_THREADS + threadIdx.x; i < n; i += stride) {
        keys[i] = snpbuild::pack_key(snpbuild::contig_of(run[i], run_contig), key[i], shift);
        vals[i] = (uint32_t)i;
    }
}

// first / end: a contig's records are one stretch of the order, so each word has one writer; desc / dup: every writer stores the same 1
__global__ __launch_bounds__(SB_THREADS) void sb_columns_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, const uint32_t *__restrict__ pos_in,
                                                                const uint64_t *__restrict__ baf_in, uint32_t n, int shift, uint32_t *__restrict__ pos_out,
                                                                uint64_t *__restrict__ baf_out, uint32_t *__restrict__ first, uint32_t *__restrict__ end,
                                                                uint32_t *__restrict__ desc, uint32_t *__restrict__ dup)
{
    const uint32_t stride = gridDim.x * SB_THREADS;
    for (uint64_t i = blockIdx.x * SB_THREADS + threadIdx.x; i < n; i += stride) {
        const uint64_t k = keys[i];
        const uint32_t v = vals[i], id = snpbuild::id_of(k, shift), p = pos_in[v];
        pos_out[i] = p;
        baf_out[i] = baf_in[v];
        if (i == 0) first[id] = 0;
        else {
            const uint64_t kp = keys[i - 1];
            const uint32_t idp = snpbuild::id_of(kp, shift);
            if (idp != id) { first[id] = (uint32_t)i; end[idp] = (uint32_t)i; }
            else {
                if (kp == k) *dup = 1;
                if (p < pos_in[vals[i - 1]]) desc[id] = 1;
            }
        }
        if (i == n - 1) end[id] = n;
    }
}

void launch_snp_run_flags(hipStream_t s, const uint8_t *text, const uint32_t *line_off, const uint32_t *chrom_len, uint32_t n, uint32_t *flags, void *es_tmp)
{
    hipLaunchKernelGGL(sb_flags_kernel, dim3(sb_blocks((uint64_t)n + 1)), dim3(SB_THREADS), 0, s, text, line_off, chrom_len, n, flags);
    launch_exclusive_sum_u32(s, flags, (uint64_t)n + 1, es_tmp);
}

void launch_snp_append(hipStream_t s, const SnpAppendArgs &a)
{
    if (a.n) hipLaunchKernelGGL(sb_append_kernel, dim3(sb_blocks(a.n)), dim3(SB_THREADS), 0, s, a);
}

void launch_snp_keys(hipStream_t s, const uint32_t *run, const uint64_t *key, const uint32_t *run_contig, uint32_t n, int shift, uint64_t *keys, uint32_t *vals)
{
    if (n) hipLaunchKernelGGL(sb_keys_kernel, dim3(sb_blocks(n)), dim3(SB_THREADS), 0, s, run, key, run_contig, n, shift, keys, vals);
}

void launch_snp_columns(hipStream_t s, const uint64_t *keys, const uint32_t *vals, const uint32_t *pos_in, const uint64_t *baf_in, uint32_t n, int shift,
                        uint32_t *pos_out, uint64_t *baf_out, uint32_t *first, uint32_t *end, uint32_t *desc, uint32_t *dup)
{
    if (n) hipLaunchKernelGGL(sb_columns_kernel, dim3(sb_blocks(n)), dim3(SB_THREADS), 0, s, keys, vals, pos_in, baf_in, n, shift, pos_out, baf_out, first, end, desc, dup);
}

}  // namespace csv
