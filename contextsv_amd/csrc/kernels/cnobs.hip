// cnobs.hip — kernel #11: the observation vectors of the copy-number pass, built where the window kernel leaves its windows (gfx950).
//
// Replaces CNVCaller::assembleRegion (host/cnv_caller.cpp; the reference's cnv_caller.cpp:65-164). The reference keys a region's windows
// by the text "ws-we" in an unordered_map<std::string,double>, and the ITERATION ORDER of that libstdc++ container is the order of the
// observations. Window i of a region is [a_i, a_{i+1}] with both ends from one double expression, so ws and we are non-decreasing in i:
//   nodes   equal keys are runs of adjacent windows. A run-head flag and a prefix sum dedupe: node id = rank of the run's head (the first
//           insertion places the node), node value = log2_cov of the run's LAST window (the later write wins). No find.
//   order   the closed form of splitorder.hip: between two rehashes the list at the epoch's end is the nodes sorted by (min t of the node's
//           bucket, descending; t, descending), t = list position when the epoch began, or the insertion index of a node that came later.
//           bucket = hash % B with B from the library's own rehash policy (CnEpochs, filled by the caller) and hash = std::hash<std::string>
//           of the key text: libstdc++'s 64-bit _Hash_bytes (cn_hash_bytes below) over the decimal text (cn_key_hash builds it in registers).
//   join    a region's SNP positions are non-decreasing, so node [ws, we] takes the slice [lower_bound(ws), upper_bound(we)) of them, in list
//           order; both ends inclusive (a SNP can land in up to three nodes: (x,p), (p,p), (p,y)); an empty slice gives the dummy observation.
// cn_order_kernel<T, MAXN> does all of that for one region per workgroup and leaves, per list position, what the fill needs; two forms:
// a wave per region while the region has at most CN_SMALL_MAX windows (a genome pass: ~1e4 regions of ~25 windows), 1024 threads per region
// up to CN_MAX_WINDOWS. An exclusive sum over the regions' totals (sort.hip) gives obs_off, cn_fill_kernel writes the five arrays.
#include <algorithm>

#include "../common.hpp"
#include "../devutil.hpp"

namespace csv {

// ---- std::hash<std::string> of "ws-we" -------------------------------------------------------------------------------------------------
// libstdc++'s _Hash_bytes (the steps of devutil.hpp) of the `len` <= 24 bytes held little-endian in w0, w1, w2 (bytes beyond len are
// zero): whole 8-byte blocks, then the 1..7 tail bytes as one little-endian number.
__device__ __forceinline__ uint64_t cn_hash_bytes(uint64_t w0, uint64_t w1, uint64_t w2, uint32_t len)
{
    uint64_t hash = hb_init(len);
    const uint32_t blocks = len >> 3;
    if (blocks >= 1) hash = hb_block(hash, w0);
    if (blocks >= 2) hash = hb_block(hash, w1);
    if (len & 7u) hash = hb_tail(hash, blocks == 0 ? w0 : (blocks == 1 ? w1 : w2));
    return hb_final(hash);
}

// The key text is built from its last character to its first — a division yields the digits in that order — by shifting the three words
// one byte up and putting the new character at the bottom: no indexed register array, no scratch.
__device__ __forceinline__ uint64_t cn_key_hash(uint32_t ws, uint32_t we)
{
    uint64_t w0 = 0, w1 = 0, w2 = 0;
    uint32_t len = 0;
    auto put = [&](uint32_t c) { w2 = (w2 << 8) | (w1 >> 56); w1 = (w1 << 8) | (w0 >> 56); w0 = (w0 << 8) | c; len++; };
    uint32_t v = we;
    do { put('0' + v % 10u); v /= 10u; } while (v);
    put('-');
    v = ws;
    do { put('0' + v % 10u); v /= 10u; } while (v);
    return cn_hash_bytes(w0, w1, w2, len);
}

// ---- exclusive prefix sum over the items x = tid + i * T (i < PER) of a workgroup, in x order ---------------------------------------------
// part: PER * (T / 64) words of LDS; every thread of the workgroup calls (v = 0 where it has no item). A barrier closes it: `part` is free again.
template <int T, int PER>
__device__ __forceinline__ uint32_t cn_block_scan(uint32_t (&v)[PER], uint32_t *part)
{
    constexpr int NW = T / WAVE;
    const int lane = lane_id(), wave = (int)(threadIdx.x >> 6);
    uint32_t incl[PER];
#pragma unroll
    for (int i = 0; i < PER; i++) {
        incl[i] = wave_incl_sum_dpp(v[i]);
        if (lane == 63) part[i * NW + wave] = incl[i];
    }
    __syncthreads();
    uint32_t acc = 0;
#pragma unroll
    for (int i = 0; i < PER; i++) {
        uint32_t base = 0;
#pragma unroll 1
        for (int w = 0; w < NW; w++) { if (w == wave) base = acc; acc += part[i * NW + w]; }      // (unrolled, its PER * NW loads are all in flight at once: registers)
        v[i] = base + incl[i] - v[i];
    }
    __syncthreads();
    return acc;
}

struct CnOrderIn {                           // device arrays, passed to the kernels by value
    const uint32_t *ws, *we;                 // [W] the window kernel's output, regions back to back
    const uint32_t *win_base;                // [R + 1] first window of each region
    const uint32_t *snp_off;                 // [R + 1]
    const uint32_t *snp_pos;                 // [S] non-decreasing inside a region
    const uint32_t *regions;                 // [n] the regions this launch serves
    uint32_t n;
};

template <int T, int MAXN>
__global__ __launch_bounds__(T) void cn_order_kernel(CnOrderIn in, CnEpochs ep, CnSlots out)
{
    constexpr int PER = (MAXN + T - 1) / T, NW = T / WAVE;
    __shared__ uint16_t FW[MAXN];                       // node -> its run's first window (region-relative)
    __shared__ uint16_t P[MAXN];                        // node -> position in the list (its own index until its first epoch)
    __shared__ uint32_t A1[MAXN], A2[MAXN], A3[MAXN], A4[MAXN];
    __shared__ uint64_t H[MAXN];                        // node -> hash of its key
    __shared__ uint32_t part[PER * NW];
    const int tid = threadIdx.x;
    for (uint32_t q = blockIdx.x; q < in.n; q += gridDim.x) {
        const uint32_t r = in.regions[q];
        const uint32_t w0 = in.win_base[r], ss = in.win_base[r + 1] - w0;             // 1 <= ss <= MAXN (the launcher's split)
        const uint32_t s0 = in.snp_off[r], s1 = in.snp_off[r + 1];
        const uint32_t *__restrict__ const ws = in.ws + w0, *__restrict__ const we = in.we + w0;

        // nodes: the heads of the runs of equal (ws, we)
        uint32_t head[PER], rank[PER];
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const uint32_t x = (uint32_t)tid + (uint32_t)i * T;
            head[i] = x < ss && (x == 0 || ws[x] != ws[x - 1] || we[x] != we[x - 1]) ? 1u : 0u;
            rank[i] = head[i];
        }
        const uint32_t N = cn_block_scan<T, PER>(rank, part);
#pragma unroll
        for (int i = 0; i < PER; i++) if (head[i]) FW[rank[i]] = (uint16_t)((uint32_t)tid + (uint32_t)i * T);
        __syncthreads();
        for (uint32_t x = tid; x < N; x += T) H[x] = cn_key_hash(ws[FW[x]], we[FW[x]]);       // (read by the thread that wrote it: x = tid + i * T)

        // the epochs (the body of so_small_epochs_kernel, the hashes in LDS): A4[p] & 0xffff = the node at list position p
        for (uint32_t k = 0; k < ep.n && ep.first[k] < N; k++) {
            const uint32_t m_old = ep.first[k], B = ep.B[k];
            const uint32_t m = min(N, ep.first[k + 1]);
            const double inv = 1.0 / (double)B;
            for (uint32_t x = m_old + tid; x < m; x += T) P[x] = (uint16_t)x;
            for (uint32_t b = tid; b < B; b += T) A1[b] = 0xffffffffu;
            for (uint32_t t = tid; t < m; t += T) A2[t] = 0;
            __syncthreads();
#pragma unroll
            for (int i = 0; i < PER; i++) {
                const uint32_t x = (uint32_t)tid + (uint32_t)i * T;
                if (x < m) { const uint32_t b = so_mod(H[x], B, inv); A3[x] = b; atomicMin(&A1[b], (uint32_t)P[x]); }      // (A3[x]: this thread's alone)
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < PER; i++) {
                const uint32_t x = (uint32_t)tid + (uint32_t)i * T;
                if (x < m) { const uint32_t w = A1[A3[x]]; atomicAdd(&A2[w], 1u); A3[x] = (w << 16) | (uint32_t)P[x]; }
            }
            __syncthreads();
            {   // A2[w] <- number of nodes with a bucket time above w (blocked layout over the reversed index), A1 <- 0 (the slot counters)
                uint32_t v[PER], tot = 0;
#pragma unroll
                for (int i = 0; i < PER; i++) { const uint32_t rr = (uint32_t)tid * PER + i; v[i] = rr < m ? A2[m - 1 - rr] : 0u; tot += v[i]; }
                const uint32_t incl = wave_incl_sum_dpp(tot);
                if (lane_id() == 63) part[tid >> 6] = incl;
                __syncthreads();
                for (uint32_t b = tid; b < m; b += T) A1[b] = 0;
                uint32_t run = incl - tot;
                for (int w2 = 0; w2 < (tid >> 6); w2++) run += part[w2];
#pragma unroll
                for (int i = 0; i < PER; i++) { const uint32_t rr = (uint32_t)tid * PER + i; if (rr < m) A2[m - 1 - rr] = run; run += v[i]; }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < PER; i++) {
                const uint32_t x = (uint32_t)tid + (uint32_t)i * T;
                if (x < m) { const uint32_t wt = A3[x], w = wt >> 16; A4[A2[w] + atomicAdd(&A1[w], 1u)] = (wt << 16) | x; }          // (t << 16) | node
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < PER; i++) {
                const uint32_t x = (uint32_t)tid + (uint32_t)i * T;
                if (x < m) {
                    const uint32_t wt = A3[x];
                    if ((wt >> 16) == (wt & 0xffffu)) {                     // the bucket's leader orders the bucket: descending own time
                        const uint32_t b0 = A2[wt >> 16], n = A1[wt >> 16];
                        for (uint32_t i1 = 1; i1 < n; i1++) {
                            const uint32_t key = A4[b0 + i1];
                            uint32_t j = i1;
                            while (j > 0 && A4[b0 + j - 1] < key) { A4[b0 + j] = A4[b0 + j - 1]; j--; }
                            A4[b0 + j] = key;
                        }
                    }
                }
            }
            __syncthreads();
            for (uint32_t p = tid; p < m; p += T) P[A4[p] & 0xffffu] = (uint16_t)p;
            __syncthreads();
        }

        // per list position: the node's windows, its slice of the SNPs, max(1, slice length) observations (A1: free after the epochs)
#pragma unroll 1
        for (uint32_t p = tid; p < ss; p += T) {
            const uint32_t g = w0 + p;
            if (p >= N) { out.cnt[g] = CN_SLOT_UNUSED; continue; }
            const uint32_t node = A4[p] & 0xffffu;
            const uint32_t f = FW[node], l = (node + 1 < N ? (uint32_t)FW[node + 1] : ss) - 1u;
            const uint32_t a = ws[f], b = we[f];
            uint32_t lo = s0, hi = s1;
            while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (in.snp_pos[mid] < a) lo = mid + 1; else hi = mid; }     // first position >= ws
            uint32_t ub = lo; hi = s1;
            while (ub < hi) { const uint32_t mid = ub + ((hi - ub) >> 1); if (in.snp_pos[mid] <= b) ub = mid + 1; else hi = mid; }    // first position > we
            out.cnt[g] = ub - lo; out.lo[g] = lo; out.fw[g] = w0 + f; out.lw[g] = w0 + l; out.reg[g] = r;
            A1[p] = max(1u, ub - lo);
        }
        __syncthreads();
        uint32_t off[PER];
#pragma unroll
        for (int i = 0; i < PER; i++) { const uint32_t p = (uint32_t)tid + (uint32_t)i * T; off[i] = p < N ? A1[p] : 0u; }
        const uint32_t total = cn_block_scan<T, PER>(off, part);
#pragma unroll
        for (int i = 0; i < PER; i++) { const uint32_t p = (uint32_t)tid + (uint32_t)i * T; if (p < N) out.off[w0 + p] = off[i]; }
        if (tid == 0) out.tot[r] = total;
    }
}

// ---- the observations ------------------------------------------------------------------------------------------------------------------------
constexpr int CN_FILL_THREADS = 256;
__global__ __launch_bounds__(CN_FILL_THREADS) void cn_fill_kernel(CnSlots sl, uint32_t n_slots, uint32_t n_regions, const uint32_t *__restrict__ obs_off32,
                                                                  const uint32_t *__restrict__ ws, const uint32_t *__restrict__ we,
                                                                  const double *__restrict__ l2, const uint32_t *__restrict__ snp_pos,
                                                                  const double *__restrict__ snp_baf, const double *__restrict__ snp_pfb, CnObs o)
{
    const uint32_t stride = gridDim.x * CN_FILL_THREADS, first = blockIdx.x * CN_FILL_THREADS + threadIdx.x;
    for (uint32_t r = first; r <= n_regions; r += stride) o.obs_off[r] = obs_off32[r];
    for (uint32_t g = first; g < n_slots; g += stride) {
        const uint32_t c = sl.cnt[g];
        if (c == CN_SLOT_UNUSED) continue;
        const uint64_t at = (uint64_t)obs_off32[sl.reg[g]] + sl.off[g];
        const double cov = l2[sl.lw[g]];                                          // the later window's value (cnv_caller.cpp:111-112)
        if (c == 0) {                                                           // dummy observation at the window centre (:144-155)
            const uint32_t f = sl.fw[g];
            o.pos[at] = (ws[f] + we[f]) / 2; o.baf[at] = -1.0; o.pfb[at] = 0.5; o.log2_cov[at] = cov; o.is_snp[at] = 0;
            continue;
        }
        const uint32_t lo = sl.lo[g];
        for (uint32_t k = 0; k < c; k++) {                                       // (:128-143)
            o.pos[at + k] = snp_pos[lo + k]; o.baf[at + k] = snp_baf[lo + k]; o.pfb[at + k] = snp_pfb[lo + k];
            o.log2_cov[at + k] = cov; o.is_snp[at + k] = 1;
        }
    }
}

void launch_cn_order(hipStream_t s, const uint32_t *ws, const uint32_t *we, const uint32_t *win_base, const uint32_t *snp_off, const uint32_t *snp_pos,
                     const uint32_t *regions_small, uint32_t n_small, const uint32_t *regions_big, uint32_t n_big, const CnEpochs &ep, const CnSlots &out)
{
    CnOrderIn in{ws, we, win_base, snp_off, snp_pos, regions_small, n_small};
    if (n_small) hipLaunchKernelGGL((cn_order_kernel<WAVE, (int)CN_SMALL_MAX>), dim3(std::min(n_small, CN_MAX_BLOCKS_SMALL)), dim3(WAVE), 0, s, in, ep, out);
    in.regions = regions_big; in.n = n_big;
    if (n_big) hipLaunchKernelGGL((cn_order_kernel<1024, (int)CN_MAX_WINDOWS>), dim3(std::min(n_big, CN_MAX_BLOCKS_BIG)), dim3(1024), 0, s, in, ep, out);
}

void launch_cn_fill(hipStream_t s, const CnSlots &sl, uint32_t n_slots, uint32_t n_regions, const uint32_t *obs_off32, const uint32_t *ws, const uint32_t *we,
                    const double *l2, const uint32_t *snp_pos, const double *snp_baf, const double *snp_pfb, const CnObs &o)
{
    const uint32_t items = std::max(n_slots, n_regions + 1);
    const uint32_t blocks = std::min<uint32_t>((items + CN_FILL_THREADS - 1) / CN_FILL_THREADS, ST_MAX_BLOCKS);
    hipLaunchKernelGGL(cn_fill_kernel, dim3(blocks), dim3(CN_FILL_THREADS), 0, s, sl, n_slots, n_regions, obs_off32, ws, we, l2, snp_pos, snp_baf, snp_pfb, o);
}

}  // namespace csv
