// dbscan1d_lds.hpp — the in-LDS labelling of one 1-D point set by one wave (gfx950). Device code only.
//
// Shared by kernels/dbscan1d.hip (labels to global memory) and kernels/splitfits.hip (labels stay in LDS and are reduced there):
// the four steps described at the head of dbscan1d.hip, on a set of at most DBSCAN1D_MAX_SEG points that the caller has put in L.p.
#pragma once
#include "common.hpp"
#include "devutil.hpp"

namespace csv {

constexpr int D1_MAX = (int)DBSCAN1D_MAX_SEG;      // 512
constexpr uint32_t D1_NONE = 0xffffffffu;

struct D1Lds {
    int32_t  p[D1_MAX];        // points, original order
    uint32_t rank[D1_MAX];     // sorted position of original index i
    uint32_t sidx[D1_MAX];     // original index at sorted position k
    uint32_t core[D1_MAX];     // by original index
    uint32_t comp[D1_MAX];     // by sorted position: sorted position of the run head (cores only)
    uint32_t rootmin[D1_MAX];  // by run head position: smallest original index in the run
    uint32_t cid[D1_MAX + 1];  // by original index: start flag -> exclusive prefix sum
};

// L.p[0, n) written by this wave, 0 < n <= D1_MAX; store(i, label) is called once for every original index i by the lane that owns it
// (i % 64). rank and sidx are left valid; store must not write the arrays of L that step 4 reads (p, rank, core, comp, rootmin, cid).
template <class Store>
__device__ __forceinline__ void d1_label_wave(D1Lds &L, const int n, const double eps, const int min_pts, const int lane, Store store)
{
    for (int i = lane; i < n; i += WAVE) { L.rootmin[i] = D1_NONE; L.cid[i] = 0; }
    if (lane == 0) L.cid[n] = 0;
    __builtin_amdgcn_wave_barrier();

    // 1. neighbour count + sorted rank (stable by original index)
    for (int i = lane; i < n; i += WAVE) {
        const int32_t pi = L.p[i];
        int cnt = 0; uint32_t rk = 0;
        for (int j = 0; j < n; j++) {
            const int32_t pj = L.p[j];
            cnt += ((double)abs(pi - pj) <= eps);              // dbscan1d.cpp:68-70
            rk += (pj < pi) || (pj == pi && j < i);
        }
        L.core[i] = cnt >= min_pts;
        L.rank[i] = rk;
        L.sidx[rk] = (uint32_t)i;
    }
    __builtin_amdgcn_wave_barrier();

    // 2. runs of core points in sorted order
    int32_t carry_prev = -1;      // sorted position of the last core seen so far
    int32_t carry_head = -1;      // sorted position of the current run head
    for (int k0 = 0; k0 < n; k0 += WAVE) {
        const int k = k0 + lane;
        const bool in = k < n;
        const uint32_t oi = in ? L.sidx[k] : 0u;
        const bool is_core = in && L.core[oi];
        // previous core position (exclusive max-scan of core positions)
        const int32_t incl_c = wave_incl_max(is_core ? k : -1);
        int32_t prev = __shfl_up(incl_c, 1, 64);
        if (lane == 0) prev = -1;
        prev = max(prev, carry_prev);
        bool head = false;
        if (is_core) {
            head = prev < 0 || !((double)abs(L.p[oi] - L.p[L.sidx[prev]]) <= eps);
        }
        const int32_t incl_h = max(wave_incl_max(head ? k : -1), carry_head);
        if (is_core) {
            L.comp[k] = (uint32_t)incl_h;
            atomicMin(&L.rootmin[incl_h], oi);
        }
        carry_prev = max(carry_prev, __shfl(incl_c, 63, 64));
        carry_head = __shfl(incl_h, 63, 64);
    }
    __builtin_amdgcn_wave_barrier();

    // 3. start points ranked by original index
    for (int i = lane; i < n; i += WAVE)
        if (L.core[i] && L.rootmin[L.comp[L.rank[i]]] == (uint32_t)i) L.cid[i] = 1;
    __builtin_amdgcn_wave_barrier();
    uint32_t carry = 0;
    for (int i0 = 0; i0 <= n; i0 += WAVE) {
        const int i = i0 + lane;
        const uint32_t v = i <= n ? L.cid[i] : 0u;
        const uint32_t incl = wave_incl_sum(v);
        if (i <= n) L.cid[i] = carry + incl - v;
        carry += __shfl(incl, 63, 64);
    }
    __builtin_amdgcn_wave_barrier();

    // 4. labels
    for (int i = lane; i < n; i += WAVE) {
        int32_t lab;
        if (L.core[i]) {
            lab = (int32_t)L.cid[L.rootmin[L.comp[L.rank[i]]]];
        } else {
            const int32_t pi = L.p[i];
            int32_t max_start = -1, min_core = INT32_MAX;
            for (int j = 0; j < n; j++) {
                if (L.core[j] && ((double)abs(pi - L.p[j]) <= eps)) {
                    const uint32_t rj = L.rootmin[L.comp[L.rank[j]]];
                    const int32_t c = (int32_t)L.cid[rj];
                    if (rj == (uint32_t)j) max_start = max(max_start, c); else min_core = min(min_core, c);
                }
            }
            lab = max_start >= 0 ? max_start : (min_core != INT32_MAX ? min_core : -2);
        }
        store(i, lab);
    }
}

}  // namespace csv
