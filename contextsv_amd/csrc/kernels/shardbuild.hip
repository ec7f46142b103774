// shardbuild.hip — the small kernels of a resident shard built on the device (api/shard_build.hip): the sortedness of the appended
// positions, the rebase of a host batch's offsets, and the 50-base ALT strings cut from the shard's packed sequences
// (csvgpu_alt_bases_resident: the base loop of SVCaller::toSVCall, host/sv_caller.cpp:47-62, through alt_bases_core.hpp).
#include "../common.hpp"

#define ABC_HD __host__ __device__
#include "../alt_bases_core.hpp"

namespace csv {

namespace abc = alt_bases_core;

namespace {

constexpr int SB_THREADS = 256;
constexpr unsigned SB_MAX_BLOCKS = 2048;      // larger calls stride

unsigned sb_grid(uint64_t items) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + SB_THREADS - 1) / SB_THREADS, SB_MAX_BLOCKS)); }

// *unsorted |= pos[i] < pos[i - 1] for i in [first, first + n), i > 0: the first appended record is held against the previous tail
__global__ __launch_bounds__(SB_THREADS) void sb_unsorted_kernel(const int32_t *__restrict__ pos, uint64_t first, uint64_t n, uint32_t *__restrict__ unsorted)
{
    bool bad = false;
    for (uint64_t k = (uint64_t)blockIdx.x * SB_THREADS + threadIdx.x; k < n; k += (uint64_t)gridDim.x * SB_THREADS) {
        const uint64_t i = first + k;
        if (i > 0 && pos[i] < pos[i - 1]) bad = true;
    }
    if (__any(bad) && (threadIdx.x & (WAVE - 1)) == 0) atomicOr(unsorted, 1u);
}

// off[i] += delta for i in [0, n)
__global__ __launch_bounds__(SB_THREADS) void sb_add_kernel(uint64_t *__restrict__ off, uint64_t n, uint64_t delta)
{
    for (uint64_t i = (uint64_t)blockIdx.x * SB_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * SB_THREADS) off[i] += delta;
}

// One wave per item, the waves striding over the items; a lane per output character. Byte loads: a record's sequence starts anywhere.
__global__ __launch_bounds__(SB_THREADS) void sb_alt_bases_kernel(const uint64_t *__restrict__ seq_off, const uint8_t *__restrict__ seq, const uint32_t *__restrict__ read,
                                                                  const uint32_t *__restrict__ qpos, const uint64_t *__restrict__ out_off, uint64_t n,
                                                                  uint8_t *__restrict__ out)
{
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    const uint64_t waves = (uint64_t)gridDim.x * (SB_THREADS / WAVE);
    for (uint64_t it = (uint64_t)blockIdx.x * (SB_THREADS / WAVE) + threadIdx.x / WAVE; it < n; it += waves) {
        const uint64_t o0 = out_off[it], len = out_off[it + 1] - o0;
        if (len == 0) continue;
        const uint32_t r = read[it], q0 = qpos[it];
        const uint64_t s0 = seq_off[r], bytes = seq_off[r + 1] - s0;
        const bool in = abc::inside(q0, len, bytes);
        for (uint64_t j = lane; j < len; j += WAVE) {
            char c = 'N';
            if (in) {
                const uint32_t q = q0 + (uint32_t)j;
                c = abc::base(seq[s0 + abc::byte_of(q)], q);
            }
            out[o0 + j] = (uint8_t)c;
        }
    }
}

}  // namespace

void launch_sb_unsorted(hipStream_t s, const int32_t *pos, uint64_t first, uint64_t n, uint32_t *unsorted)
{
    if (n) hipLaunchKernelGGL(sb_unsorted_kernel, dim3(sb_grid(n)), dim3(SB_THREADS), 0, s, pos, first, n, unsorted);
}

void launch_sb_add(hipStream_t s, uint64_t *off, uint64_t n, uint64_t delta)
{
    if (n && delta) hipLaunchKernelGGL(sb_add_kernel, dim3(sb_grid(n)), dim3(SB_THREADS), 0, s, off, n, delta);
}

void launch_alt_bases(hipStream_t s, const uint64_t *seq_off, const uint8_t *seq, const uint32_t *read, const uint32_t *qpos, const uint64_t *out_off, uint64_t n,
                      uint8_t *out)
{
    if (n) hipLaunchKernelGGL(sb_alt_bases_kernel, dim3(sb_grid(n * WAVE)), dim3(SB_THREADS), 0, s, seq_off, seq, read, qpos, out_off, n, out);
}

}  // namespace csv
