// dbscan1d.hip — kernel #3b: batched 1-D DBSCAN, one wavefront per point set (gfx950).
//
// Replaces DBSCAN1D::fit (dbscan1d.cpp:8-70). The reference runs it six times per overlap group of
// split reads on vectors of 5-200 ints (sv_caller.cpp:270-372): tiny sets, huge call count. Here
// every set of a batch is one segment and one 64-lane wave solves it entirely in its private LDS
// slice (no workgroup barrier), with the same order-free labelling as dbscan.hip:
//   1. neighbour counts and the sorted rank of every point by brute force (n <= 512: each lane
//      owns points lane, lane+64, ... and reads the others as LDS broadcasts);
//   2. in sorted order the components of core points are the runs whose consecutive gaps are
//      <= eps (1-D: two cores within eps have every core between them within eps of both), found
//      with two wave max-scans; LDS atomicMin gives each run its smallest ORIGINAL index (= start);
//   3. start flags are prefix-summed in original-index order to the reference's cluster ids;
//   4. cores take their run's id; borders scan their neighbours: largest id among neighbouring
//      start points, else smallest id among neighbouring cores, else -2 (see dbscan.hip).
// Segments longer than DBSCAN1D_MAX_SEG are flagged and solved by the generic sorted-window path.
#include "../common.hpp"
#include "../devutil.hpp"
#include "../dbscan1d_lds.hpp"     // D1Lds and the four labelling steps (shared with splitfits.hip)

namespace csv {

constexpr int D1_THREADS = 256;
constexpr int D1_WAVES = D1_THREADS / WAVE;

__global__ __launch_bounds__(D1_THREADS) void dbscan1d_kernel(const int32_t *__restrict__ pts, const uint64_t *__restrict__ seg_off,
                                                             uint64_t n_seg, double eps, int min_pts,
                                                             int32_t *__restrict__ labels, unsigned int *too_large)
{
    __shared__ D1Lds lds_all[D1_WAVES];
    const int lane = lane_id(), wave = threadIdx.x >> 6;
    D1Lds &L = lds_all[wave];
    const uint64_t wave_gid = (uint64_t)blockIdx.x * D1_WAVES + wave;
    const uint64_t wave_stride = (uint64_t)gridDim.x * D1_WAVES;

    for (uint64_t seg = wave_gid; seg < n_seg; seg += wave_stride) {
        const uint64_t o0 = seg_off[seg], o1 = seg_off[seg + 1];
        const uint64_t n64 = o1 - o0;
        if (n64 == 0) continue;
        if (n64 > (uint64_t)D1_MAX) { if (lane == 0) *too_large = 1u; continue; }
        const int n = (int)n64;
        __builtin_amdgcn_wave_barrier();
        for (int i = lane; i < n; i += WAVE) L.p[i] = pts[o0 + i];
        d1_label_wave(L, n, eps, min_pts, lane, [&](int i, int32_t lab) { labels[o0 + i] = lab; });
    }
}

void launch_dbscan_1d_batched(hipStream_t s, const int32_t *pts, const uint64_t *seg_off, uint64_t n_seg,
                              double eps, int min_pts, int32_t *labels, unsigned int *too_large_flag)
{
    if (n_seg == 0) return;
    uint64_t want = (n_seg + D1_WAVES - 1) / D1_WAVES;
    if (want > 4096) want = 4096;
    hipLaunchKernelGGL(dbscan1d_kernel, dim3((unsigned)want), dim3(D1_THREADS), 0, s, pts, seg_off, n_seg, eps, min_pts,
                       labels, too_large_flag);
}

}  // namespace csv
