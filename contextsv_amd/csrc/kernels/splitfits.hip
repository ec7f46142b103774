// splitfits.hip — kernel #9: the evidence of every overlap group of the split-read pass (gfx950).
//
// Replaces what findSplitSVSignatures does with a group before it makes calls (sv_caller.cpp:248-416): the strand vote (:248-265), the six
// point sets (:270-347), six DBSCAN1D fits, getLargestCluster (dbscan1d.cpp:72-90) and the median of each largest cluster. The groups lie
// in device memory (csvgpu_split_groups' chain left them there, or the caller's were staged), the member and supplementary tables beside
// them; one 64-byte csv_split_fit per group goes back.
//
// One 64-lane wave per (group, set), everything in the wave's private LDS slice, no workgroup barrier:
//   build   the set straight from the tables, in the reference's point order (members in the group's order, a member's supplementary
//           records in table order): a wave prefix sum over the members' contribution counts, each lane writes its member's points;
//   label   the four steps of dbscan1d.hip (dbscan1d_lds.hpp), labels kept in LDS;
//   reduce  cluster sizes by LDS atomics, the first strictly largest id (a max over (size, ~id)), and the median as the cluster member
//           whose rank inside the cluster is size / 2 — one prefix sum over the sorted positions that the labelling left in LDS.
// The wave of set 0 also takes the strand vote. Sets of more than DBSCAN1D_MAX_SEG points are only counted here; the glue materialises
// each of them (sf_big_points), labels it by the generic sorted path and reduces it out of global memory (sf_big_reduce).
#include "../common.hpp"
#include "../devutil.hpp"
#include "../dbscan1d_lds.hpp"

namespace csv {

constexpr int SF_THREADS = 128;
constexpr int SF_WAVES = SF_THREADS / WAVE;        // two slices of 18 KiB: eight waves per compute unit's 160 KiB

struct SfLds {
    D1Lds    d;
    int32_t  lab[D1_MAX];      // by original index
    uint32_t sz[D1_MAX];       // by cluster id
};

struct SfGroup { uint64_t base, m0; uint32_t n; };     // first member of the group's segment; the group's slice of members[]

__device__ __forceinline__ SfGroup sf_group(const SplitFitsIn &in, uint32_t g)
{
    // the segment: the last c with seg_group_off[c] <= g (empty segments repeat a value; the last of them owns the group)
    uint64_t lo = 0, hi = in.n_seg;                    // answer in [lo, hi)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (in.seg_group_off[mid] <= (uint64_t)g) lo = mid; else hi = mid;
    }
    SfGroup G;
    G.base = in.seg_off[lo];
    G.m0 = in.group_off[g];
    G.n = (uint32_t)(in.group_off[g + 1] - G.m0);
    return G;
}

// how many points member m gives to the set
__device__ __forceinline__ uint32_t sf_count(const SplitFitsIn &in, uint64_t m, int set)
{
    if (set < 2) return 1u;
    const uint32_t rev = in.reverse[m] & 1u;
    uint32_t c = 0;
    for (uint64_t z = in.supp_off[m], z1 = in.supp_off[m + 1]; z < z1; z++) {
        const uint32_t f = in.supp_flags[z];
        if (f & 2u) continue;                                              // another tid: ignored (:352-354)
        c += set < 4 || (f & 1u) == rev;
    }
    return c;
}

// member m's points, in table order, to dst[at ...]
template <class P>
__device__ __forceinline__ void sf_emit(const SplitFitsIn &in, uint64_t m, int set, P dst, uint32_t at)
{
    if (set == 0) { dst[at] = in.start[m]; return; }
    if (set == 1) { dst[at] = in.end[m]; return; }
    const uint32_t rev = in.reverse[m] & 1u;
    for (uint64_t z = in.supp_off[m], z1 = in.supp_off[m + 1]; z < z1; z++) {
        const uint32_t f = in.supp_flags[z];
        if (f & 2u) continue;
        if (set == 2) { dst[at++] = in.supp_start[z]; continue; }
        if (set == 3) { dst[at++] = in.supp_end[z]; continue; }
        if ((f & 1u) != rev) continue;                                     // opposite strands: no distances (:318-320)
        const int32_t ps = in.start[m], ss = in.supp_start[z];
        if (set == 4) {
            int32_t d = max(0, max(in.supp_q_start[z], in.q_start[m]) - min(in.supp_q_end[z], in.q_end[m]));
            if (!(ps < ss)) d = -d;                                        // :322-325, :343-345
            dst[at++] = d;
        } else {
            dst[at++] = max(0, max(ss, ps) - min(in.supp_end[z], in.end[m]));
        }
    }
}

// the wave's set to dst (LDS or global), n_pts known: prefix sums over 64 members at a time
template <class P>
__device__ __forceinline__ void sf_build(const SplitFitsIn &in, const SfGroup &G, int set, int lane, P dst)
{
    uint32_t carry = 0;
    for (uint32_t k0 = 0; k0 < G.n; k0 += WAVE) {
        const uint32_t k = k0 + (uint32_t)lane;
        const bool have = k < G.n;
        const uint64_t m = have ? G.base + in.members[G.m0 + k] : 0;
        const uint32_t c = have ? sf_count(in, m, set) : 0u;
        const uint32_t incl = wave_incl_sum(c);
        if (c) sf_emit(in, m, set, dst, carry + incl - c);
        carry += __shfl(incl, 63, 64);
    }
}

__device__ __forceinline__ uint32_t sf_set_size(const SplitFitsIn &in, const SfGroup &G, int set, int lane)
{
    if (set < 2) return G.n;
    uint32_t c = 0;
    for (uint32_t k = (uint32_t)lane; k < G.n; k += WAVE) c += sf_count(in, G.base + in.members[G.m0 + k], set);
    return wave_sum(c);
}

__device__ __forceinline__ unsigned long long wave_max64(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long t = __shfl_xor(v, d, 64);
        v = t > v ? t : v;
    }
    return v;
}

__global__ __launch_bounds__(SF_THREADS) void sf_fits_kernel(const SplitFitsIn in, const double eps, const int min_pts, csv_split_fit *__restrict__ out,
                                                            uint32_t *__restrict__ big_n, unsigned long long *big_res)
{
    __shared__ SfLds lds_all[SF_WAVES];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    SfLds &S = lds_all[wave];
    D1Lds &L = S.d;
    const uint64_t n_items = (uint64_t)in.n_groups * 6;
    const uint64_t stride = (uint64_t)gridDim.x * SF_WAVES;

    for (uint64_t w = (uint64_t)blockIdx.x * SF_WAVES + wave; w < n_items; w += stride) {
        const uint32_t g = (uint32_t)(w / 6);
        const int set = (int)(w % 6);
        const SfGroup G = sf_group(in, g);
        csv_split_fit *rec = out + g;

        if (set == 0) {                                                    // the strand vote (:248-265)
            uint32_t opp = 0;
            for (uint32_t k = (uint32_t)lane; k < G.n; k += WAVE) {
                const uint64_t m = G.base + in.members[G.m0 + k];
                const uint32_t rev = in.reverse[m] & 1u;
                bool o = false;
                for (uint64_t z = in.supp_off[m], z1 = in.supp_off[m + 1]; z < z1; z++) {
                    const uint32_t f = in.supp_flags[z];
                    o |= !(f & 2u) && (f & 1u) != rev;
                }
                opp += o;
            }
            opp = wave_sum(opp);
            if (lane == 0) { rec->n_members = G.n; rec->n_opposite = opp; rec->reserved[0] = 0; rec->reserved[1] = 0; }
        }

        const uint32_t n_pts = sf_set_size(in, G, set, lane);
        if (n_pts == 0 || n_pts > (uint32_t)D1_MAX) {
            if (lane == 0) {
                rec->median[set] = 0; rec->size[set] = 0;
                if (n_pts) { big_n[w] = n_pts; atomicAdd(&big_res[0], 1ull); atomicAdd(&big_res[1], (unsigned long long)n_pts); }
            }
            continue;
        }
        const int n = (int)n_pts;
        __builtin_amdgcn_wave_barrier();
        sf_build(in, G, set, lane, L.p);
        for (int i = lane; i < n; i += WAVE) S.sz[i] = 0;
        d1_label_wave(L, n, eps, min_pts, lane, [&](int i, int32_t lab) { S.lab[i] = lab; });
        __builtin_amdgcn_wave_barrier();

        // sizes, then the first strictly largest id: the maximum of (size, ~id)
        for (int i = lane; i < n; i += WAVE) if (S.lab[i] >= 0) atomicAdd(&S.sz[S.lab[i]], 1u);
        __builtin_amdgcn_wave_barrier();
        unsigned long long best = 0;
        for (int c = lane; c < n; c += WAVE) {
            const unsigned long long key = ((unsigned long long)S.sz[c] << 32) | (0xffffffffu - (uint32_t)c);
            best = key > best ? key : best;
        }
        best = wave_max64(best);
        const uint32_t size = (uint32_t)(best >> 32);
        const int32_t id = (int32_t)(0xffffffffu - (uint32_t)best);
        if (size == 0) {
            if (lane == 0) { rec->median[set] = 0; rec->size[set] = 0; }
            continue;
        }
        // the member of the cluster with size / 2 members in front of it in sorted order
        uint32_t carry = 0;
        for (int k0 = 0; k0 < n; k0 += WAVE) {
            const int k = k0 + lane;
            const uint32_t oi = k < n ? L.sidx[k] : 0u;
            const uint32_t f = k < n && S.lab[oi] == id;
            const uint32_t incl = wave_incl_sum(f);
            if (f && carry + incl - 1u == size / 2) { rec->median[set] = L.p[oi]; rec->size[set] = size; }
            carry += __shfl(incl, 63, 64);
        }
    }
}

__global__ __launch_bounds__(WAVE) void sf_big_points_kernel(const SplitFitsIn in, const uint32_t w, int32_t *__restrict__ pts)
{
    const SfGroup G = sf_group(in, w / 6);
    sf_build(in, G, (int)(w % 6), lane_id(), pts);
}

constexpr int SFB_THREADS = 256;

// One workgroup: sizes by global atomics, the first strictly largest id, the median by a prefix over the sorted positions.
__global__ __launch_bounds__(SFB_THREADS) void sf_big_reduce_kernel(const int32_t *__restrict__ pts_sorted, const uint32_t *__restrict__ oid,
                                                                   const int32_t *__restrict__ labels, const uint32_t n, uint32_t *sizes,
                                                                   csv_split_fit *rec, const int set)
{
    __shared__ unsigned long long s_best[SFB_THREADS];
    __shared__ uint32_t s_cnt[SFB_THREADS + 1];
    const uint32_t t = threadIdx.x;
    for (uint32_t i = t; i < n; i += SFB_THREADS) if (labels[i] >= 0) atomicAdd(&sizes[labels[i]], 1u);
    __threadfence();
    __syncthreads();
    unsigned long long best = 0;
    for (uint32_t c = t; c < n; c += SFB_THREADS) {
        const unsigned long long key = ((unsigned long long)__hip_atomic_load(&sizes[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) << 32) | (0xffffffffu - c);
        best = key > best ? key : best;
    }
    s_best[t] = best;
    __syncthreads();
    for (uint32_t d = SFB_THREADS / 2; d > 0; d >>= 1) {
        if (t < d && s_best[t + d] > s_best[t]) s_best[t] = s_best[t + d];
        __syncthreads();
    }
    best = s_best[0];
    const uint32_t size = (uint32_t)(best >> 32);
    const int32_t id = (int32_t)(0xffffffffu - (uint32_t)best);
    if (size == 0) {
        if (t == 0) { rec->median[set] = 0; rec->size[set] = 0; }
        return;
    }
    // thread t owns the sorted positions [t * chunk, (t + 1) * chunk)
    const uint32_t chunk = (n + SFB_THREADS - 1) / SFB_THREADS;
    const uint32_t k0 = min(n, t * chunk), k1 = min(n, k0 + chunk);
    uint32_t c = 0;
    for (uint32_t k = k0; k < k1; k++) c += labels[oid[k]] == id;
    s_cnt[t + 1] = c;
    if (t == 0) s_cnt[0] = 0;
    __syncthreads();
    if (t == 0) for (uint32_t i = 1; i <= SFB_THREADS; i++) s_cnt[i] += s_cnt[i - 1];
    __syncthreads();
    uint32_t r = s_cnt[t];
    for (uint32_t k = k0; k < k1; k++) {
        if (labels[oid[k]] != id) continue;
        if (r == size / 2) { rec->median[set] = pts_sorted[k]; rec->size[set] = size; }
        r++;
    }
}

void launch_sf_fits(hipStream_t s, const SplitFitsIn &in, double eps, int min_pts, csv_split_fit *out, uint32_t *big_n, unsigned long long *big_res)
{
    if (in.n_groups == 0) return;
    uint64_t want = ((uint64_t)in.n_groups * 6 + SF_WAVES - 1) / SF_WAVES;
    if (want > 8192) want = 8192;
    hipLaunchKernelGGL(sf_fits_kernel, dim3((unsigned)want), dim3(SF_THREADS), 0, s, in, eps, min_pts, out, big_n, big_res);
}

void launch_sf_big_points(hipStream_t s, const SplitFitsIn &in, uint32_t w, int32_t *pts)
{
    hipLaunchKernelGGL(sf_big_points_kernel, dim3(1), dim3(WAVE), 0, s, in, w, pts);
}

void launch_sf_big_reduce(hipStream_t s, const int32_t *pts_sorted, const uint32_t *oid, const int32_t *labels, uint32_t n, uint32_t *sizes,
                          csv_split_fit *rec, int set)
{
    hipLaunchKernelGGL(sf_big_reduce_kernel, dim3(1), dim3(SFB_THREADS), 0, s, pts_sorted, oid, labels, n, sizes, rec, set);
}

}  // namespace csv
