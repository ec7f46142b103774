// cigarpack.hip — the 16-bit form of a resident long-read shard's CIGAR array, made and undone on the device (gfx950).
//
// The rule is cigar_pack_core.hpp's (the CPU check runs the same text). Three steps per upload, one streaming pass each over the words:
//   1. cigar_esc_count_kernel: the escapes of every 512-op piece;
//   2. the exclusive sum of the counts (sort.hip's), which is the per-piece index of the table and whose last entry sizes it;
//   3. cigar_pack_kernel: the halfwords, and the table's entries at their rank (the piece's exclusive sum + the op's rank inside the piece).
// One workgroup of 256 threads per piece, two consecutive ops per thread: a thread's two halfwords are one 32-bit store, and the ranks grow
// with the thread index, so the table comes out sorted by op index.
// cigar_unpack_kernel gives the 32-bit words back (csvgpu_shard_fetch_reads).
#include "../common.hpp"
#include "../devutil.hpp"

#define CPK_HD __host__ __device__
#include "../cigar_pack_core.hpp"

namespace csv {

namespace cpk = cigar_pack_core;
constexpr int CPK_THREADS = cpk::PIECE_OPS / 2;
static_assert(CPK_THREADS == 256, "a piece is walked by four waves, two ops per lane");

__global__ __launch_bounds__(CPK_THREADS) void cigar_esc_count_kernel(const uint32_t *__restrict__ cigar, uint64_t n_cigar, uint32_t *__restrict__ piece)
{
    __shared__ uint32_t wcnt[CPK_THREADS / WAVE];
    const uint64_t i = ((uint64_t)blockIdx.x << cpk::PIECE_SHIFT) + 2u * threadIdx.x;
    const uint32_t a = i < n_cigar ? cigar[i] : 0u, b = i + 1 < n_cigar ? cigar[i + 1] : 0u;
    const uint32_t n = (uint32_t)__popcll(__ballot(cpk::is_escape_word(a))) + (uint32_t)__popcll(__ballot(cpk::is_escape_word(b)));
    if (lane_id() == 0) wcnt[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
        piece[blockIdx.x] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        if (blockIdx.x == 0) piece[gridDim.x] = 0u;
    }
}

__global__ __launch_bounds__(CPK_THREADS) void cigar_pack_kernel(const uint32_t *__restrict__ cigar, uint64_t n_cigar, const uint32_t *__restrict__ piece,
                                                                 uint16_t *__restrict__ half, uint64_t *__restrict__ tab)
{
    __shared__ uint32_t wcnt[CPK_THREADS / WAVE];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    const uint64_t i = ((uint64_t)blockIdx.x << cpk::PIECE_SHIFT) + 2u * threadIdx.x;      // (the halfword array reaches the end of the last piece)
    const uint32_t a = i < n_cigar ? cigar[i] : 0u, b = i + 1 < n_cigar ? cigar[i + 1] : 0u;
    *reinterpret_cast<uint32_t *>(half + i) = (uint32_t)cpk::pack(a) | ((uint32_t)cpk::pack(b) << 16);
    const bool ea = cpk::is_escape_word(a), eb = cpk::is_escape_word(b);
    const uint64_t ma = __ballot(ea), mb = __ballot(eb);
    if (lane == 0) wcnt[wave] = (uint32_t)__popcll(ma) + (uint32_t)__popcll(mb);
    __syncthreads();
    if (!(ea || eb)) return;
    uint32_t rank = piece[blockIdx.x];
    for (int w = 0; w < wave; w++) rank += wcnt[w];
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    rank += (uint32_t)__popcll(ma & below) + (uint32_t)__popcll(mb & below);               // the escapes of the lanes in front of this one
    if (ea) tab[rank++] = cpk::entry(i, a);
    if (eb) tab[rank] = cpk::entry(i + 1, b);
}

__global__ __launch_bounds__(256) void cigar_unpack_kernel(const uint16_t *__restrict__ half, const uint32_t *__restrict__ piece, const uint64_t *__restrict__ tab,
                                                           uint64_t first, uint64_t n, uint32_t *__restrict__ out)
{
    const uint64_t k = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (k < n) out[k] = cpk::unpack(half, piece, tab, first + k);
}

void launch_cigar_esc_count(hipStream_t s, const uint32_t *cigar, uint64_t n_cigar, uint32_t *piece)
{
    const uint64_t np = cpk::n_pieces(n_cigar);
    if (np) hipLaunchKernelGGL(cigar_esc_count_kernel, dim3((unsigned)np), dim3(CPK_THREADS), 0, s, cigar, n_cigar, piece);
}

void launch_cigar_pack(hipStream_t s, const uint32_t *cigar, uint64_t n_cigar, const uint32_t *piece, uint16_t *half, uint64_t *tab)
{
    const uint64_t np = cpk::n_pieces(n_cigar);
    if (np) hipLaunchKernelGGL(cigar_pack_kernel, dim3((unsigned)np), dim3(CPK_THREADS), 0, s, cigar, n_cigar, piece, half, tab);
}

void launch_cigar_unpack(hipStream_t s, const CigarPack &pack, uint64_t first, uint64_t n, uint32_t *out)
{
    if (n) hipLaunchKernelGGL(cigar_unpack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pack.half, pack.piece, pack.tab, first, n, out);
}

}  // namespace csv
