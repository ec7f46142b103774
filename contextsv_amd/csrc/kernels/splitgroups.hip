// splitgroups.hip — the overlap groups of the split-read pass (gfx950): what the reference builds with an unbalanced interval tree and
// a greedy seeding loop (sv_caller.cpp:215-238, insert :964-980, findOverlaps :948-962), for all contigs of a batch side by side.
//
// Segment = one contig's surviving primaries in the iteration order of its qname map; member r (its rank) = the closed interval
// [s_r, e_r]. Three facts make the sequential code parallel without changing a single member's place:
//   1. The tree that BST insertions in rank order produce is the Cartesian tree of the sequence sorted by (start, rank) with the rank
//      as heap priority. A node's place in findOverlaps' pre-order walk is  pre = L + 1 + R:  L = in-order position of the nearest
//      member to its left with a smaller rank (-1: none), R = length of the chain of next-smaller-rank links to its right. That chain
//      is the set of q > p with no smaller rank in [p, q), i.e. of q with nsl(q) < p < q, so R(p) = #{q : nsl(q) < p} - (p + 1): ONE
//      histogram of the nsl values and ONE exclusive sum give every R — no pointer jumping.
//   2. The seeds are the lexicographically first maximal independent set of the overlap graph in rank order. Members of different
//      connected components (start-sorted: a member starts a component when no earlier member of the segment ends at or after its
//      start) never interact: a wave per component repeats "lowest-rank undecided member becomes a seed, what overlaps it dies" — at
//      most one round per member, no waiting for any other wave.
//   3. A seed's group is every member that overlaps it (all inside its component), ordered by pre. The left pruning of :957 never
//      drops an overlap. The fill writes (group, pre) keys; one stable radix sort orders every group of the batch at once.
// Positions of the sorted sequence and member indices of the call share one numbering: segment c owns [seg_off[c], seg_off[c + 1]) in
// both, so "rank" is the member's index in the call (ranks are only ever compared inside a segment, and every member of an earlier
// segment has a smaller index: a search that runs past its segment's first position stops at once).
#include "../common.hpp"
#include "../devutil.hpp"

namespace csv {

constexpr int SG_THREADS = 256;
constexpr int SG_WAVES = SG_THREADS / WAVE;
constexpr uint32_t SG_LDS_CAP = 512;          // members of a component that a wave keeps in LDS (13 bytes each); larger ones: sg_seed_by_cursor, or the same rounds in global memory
constexpr uint64_t SG_NONE = ~0ull;

__device__ __forceinline__ uint32_t sg_wave_min_u32(uint32_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, d, 64));
    return v;
}
__device__ __forceinline__ int32_t sg_wave_max_i32(int32_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ __forceinline__ uint64_t sg_wave_min_u64(uint64_t v)
{
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const uint64_t o = ((uint64_t)(uint32_t)__shfl_xor((int)(v >> 32), d, 64) << 32) | (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int64_t sg_shfl_i64(int64_t v, int j)
{
    return (int64_t)(((uint64_t)(uint32_t)__shfl((int)((uint64_t)v >> 32), j, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)(uint64_t)v, j, 64));
}

// ---- sort keys: segment ‖ biased start, members enumerated in rank order (a stable sort then needs no rank in the key) ---------------
__global__ __launch_bounds__(SG_THREADS) void sg_keys_kernel(const int32_t *__restrict__ start, const uint64_t *__restrict__ seg_off, uint64_t n_seg, uint32_t n,
                                                            uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint32_t i = blockIdx.x * SG_THREADS + threadIdx.x;
    if (i >= n) return;
    uint64_t lo = 0, hi = n_seg;                            // first j in [0, n_seg] with seg_off[j] > i  (seg_off[n_seg] == n > i)
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (seg_off[mid] > i) hi = mid; else lo = mid + 1;
    }
    keys[i] = ((lo - 1) << 32) | ((uint32_t)start[i] ^ 0x80000000u);
    vals[i] = i;
}

// ---- the sorted sequence as arrays, and one summary per 64 positions: smallest rank, largest end ----------------------------------------
__global__ __launch_bounds__(SG_THREADS) void sg_unpack_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, const int32_t *__restrict__ start,
                                                              const int32_t *__restrict__ end, const uint64_t *__restrict__ seg_off, uint32_t n,
                                                              int32_t *__restrict__ ss, int32_t *__restrict__ se, uint32_t *__restrict__ sid, uint32_t *__restrict__ posof,
                                                              uint32_t *__restrict__ plo, uint32_t *__restrict__ blk_min_id, int32_t *__restrict__ blk_max_end)
{
    const uint32_t p = blockIdx.x * SG_THREADS + threadIdx.x;
    const bool valid = p < n;
    uint32_t m = 0xffffffffu;
    int32_t e = INT32_MIN;
    if (valid) {
        m = vals[p];
        e = end[m];
        ss[p] = start[m]; se[p] = e; sid[p] = m; posof[m] = p;
        plo[p] = (uint32_t)seg_off[keys[p] >> 32];
    }
    const uint32_t mn = sg_wave_min_u32(m);
    const int32_t mx = sg_wave_max_i32(e);
    if (lane_id() == 0 && valid) { blk_min_id[p >> 6] = mn; blk_max_end[p >> 6] = mx; }
}

// Nearest position q in [lo, p) whose value is below `thr`, or -1. MODE 0: value = rank (sid), summaries = the blocks' minima; MODE 1:
// value = -end, summaries = -(the blocks' maxima): "ends at or after x" is  -end < -x + 1. A wave owns 64 consecutive positions: its
// own block is settled with lane broadcasts, the blocks to its left 64 summaries at a time (every lane of the wave walks the same
// summaries, so they are loaded once), and only the block that holds the answer is read element by element.
template <int MODE>
__device__ __forceinline__ int64_t sg_value(const void *arr, uint32_t q)
{
    return MODE == 0 ? (int64_t)((const uint32_t *)arr)[q] : -(int64_t)((const int32_t *)arr)[q];
}
template <int MODE>
__device__ __forceinline__ int64_t sg_nearest_left(const void *elem, const void *blk, uint32_t p, uint32_t lo, bool valid, int64_t own, int64_t thr)
{
    const int lane = lane_id();
    const uint32_t base = p - (uint32_t)lane;
    int best = -1;
    for (int j = 0; j < WAVE - 1; j++) {
        const int64_t vj = sg_shfl_i64(own, j);
        if (j < lane && vj < thr) best = j;
    }
    bool done = !valid;
    int64_t res = -1;
    if (!done && best >= 0) { res = (int64_t)base + best; if (res < (int64_t)lo) res = -1; done = true; }
    if (!done && base <= lo) done = true;
    uint32_t cb_hi = base >> 6;                                            // blocks [0, cb_hi) lie to the left of this wave's
    while (cb_hi > 0 && __ballot(!done) != 0) {
        const uint32_t cb = cb_hi > (uint32_t)WAVE ? cb_hi - WAVE : 0u, cn = cb_hi - cb;
        const int64_t bv = (uint32_t)lane < cn ? sg_value<MODE>(blk, cb + (uint32_t)lane) : INT64_MAX;
        int hit = -1;
        for (int j = 0; j < (int)cn; j++) {
            const int64_t vj = sg_shfl_i64(bv, j);
            if (vj < thr) hit = j;
        }
        if (!done) {
            if (hit >= 0) {
                const uint32_t q0 = (cb + (uint32_t)hit) << 6;
                for (int t = WAVE - 1; t >= 0; t--)
                    if (sg_value<MODE>(elem, q0 + (uint32_t)t) < thr) { res = (int64_t)q0 + t; break; }
                if (res < (int64_t)lo) res = -1;
                done = true;
            } else if (((uint64_t)cb << 6) <= lo) done = true;
        }
        cb_hi = cb;
    }
    return res;
}

// ---- per position: L + 1, the histogram of the nearest-smaller-rank links, and whether the position starts a component -------------------
__global__ __launch_bounds__(SG_THREADS) void sg_links_kernel(const int32_t *__restrict__ ss, const int32_t *__restrict__ se, const uint32_t *__restrict__ sid,
                                                             const uint32_t *__restrict__ plo, const uint32_t *__restrict__ blk_min_id,
                                                             const int32_t *__restrict__ blk_max_end, uint32_t n, uint32_t *__restrict__ lp1,
                                                             uint32_t *__restrict__ hist, uint8_t *__restrict__ head)
{
    const uint32_t p = blockIdx.x * SG_THREADS + threadIdx.x;
    const bool valid = p < n;
    const uint32_t lo = valid ? plo[p] : 0u;
    const int64_t rank = valid ? (int64_t)sid[p] : INT64_MAX;
    const int64_t nsl = sg_nearest_left<0>(sid, blk_min_id, p, lo, valid, rank, rank);
    const int64_t neg_end = valid ? -(int64_t)se[p] : INT64_MAX;
    const int64_t reach = sg_nearest_left<1>(se, blk_max_end, p, lo, valid, neg_end, valid ? -(int64_t)ss[p] + 1 : INT64_MIN);
    // hist[nsl + 1] (no link: hist[lo], the slot of position lo - 1 — members of later segments never count it, see the file comment)
    const uint32_t slot = nsl >= 0 ? (uint32_t)nsl + 1u : lo;
    if (valid) {
        lp1[p] = nsl >= 0 ? (uint32_t)nsl - lo + 1u : 0u;
        head[p] = reach < 0 ? 1 : 0;
    }
    // a coordinate-sorted contig's map order is a spine: every link of a wave is the same "none" — one atomic for the wave then
    const uint64_t live = __ballot(valid);
    if (live == 0) return;
    const uint32_t first = (uint32_t)__shfl((int)slot, 0, 64);
    if (__ballot(valid && slot == first) == live) {
        if (lane_id() == 0) atomicAdd(&hist[first], (uint32_t)__popcll(live));
    } else if (valid) {
        atomicAdd(&hist[slot], 1u);
    }
}

// First q in [lo, hi) for which a monotone predicate (false ... false true ... true) holds, or hi: the wave probes 64 places per step.
template <class P>
__device__ __forceinline__ uint32_t sg_first_true(uint32_t lo, uint32_t hi, P pred)
{
    const uint32_t lane = (uint32_t)lane_id();
    for (;;) {
        const uint32_t len = hi - lo;
        if (len == 0) return hi;
        const uint32_t step = (len + WAVE - 1) >> 6;
        const uint64_t off = (uint64_t)(lane + 1) * step;                  // this lane's stretch ends at lo + off (clipped)
        const uint32_t q = off >= len ? hi - 1 : lo + (uint32_t)off - 1;
        const uint64_t bal = __ballot(pred(q));
        if (bal == 0) return hi;
        const uint32_t j = (uint32_t)(__ffsll((unsigned long long)bal) - 1);
        if (step == 1) return lo + j;
        const uint32_t nlo = lo + j * step;
        hi = (uint64_t)nlo + step < hi ? nlo + step : hi;                  // (its last element is true: the next step finds it)
        lo = nlo;
    }
}
__device__ __forceinline__ uint8_t sg_ld_u8(const uint8_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void sg_st_u8(uint8_t *p, uint8_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int32_t sg_ld_i32(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void sg_st_i32(int32_t *p, int32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// A component too large for LDS whose members' ranks lie close together (the map order of a coordinate-sorted contig is nearly its reverse):
// the seeds are taken by a cursor that runs through the ranks once — the lowest-rank undecided member is the next undecided one behind the
// cursor — and a seed only visits the stretch of the component that can overlap it: from the first position whose running maximum of the
// ends reaches its start to the first start beyond its end (two 64-way searches). State bytes and running maxima are written by one lane
// and read by another: agent-scope accesses (past the vector L1).
__device__ __forceinline__ void sg_seed_by_cursor(const int32_t *__restrict__ ss, const int32_t *__restrict__ se, const uint32_t *__restrict__ sid,
                                                  const uint32_t *__restrict__ posof, uint32_t a, uint32_t b, uint32_t rmin, uint32_t rmax, uint8_t *gstate,
                                                  int32_t *pm, uint32_t *__restrict__ cnt, uint32_t *__restrict__ keep, uint32_t *__restrict__ cstart,
                                                  uint32_t *__restrict__ cend, unsigned long long *__restrict__ total)
{
    const uint32_t lane = (uint32_t)lane_id();
    uint64_t cur = rmin;
    while (cur <= rmax) {                                                 // every turn moves the cursor forward
        const uint64_t i = cur + lane;
        uint32_t pi = 0;
        bool ok = false;
        if (i <= rmax) { pi = posof[i]; ok = pi >= a && pi < b && sg_ld_u8(gstate + pi) == 0; }
        const uint64_t bal = __ballot(ok);
        if (bal == 0) { cur += WAVE; continue; }
        const int l = __ffsll((unsigned long long)bal) - 1;
        const uint32_t x = (uint32_t)__shfl((int)pi, l, 64);
        const uint32_t seed = (uint32_t)cur + (uint32_t)l;
        cur = (uint64_t)seed + 1;
        const int32_t xs = ss[x], xe = se[x];
        const uint32_t whi = sg_first_true(x + 1, b, [&](uint32_t q) { return ss[q] > xe; });
        const uint32_t wlo = sg_first_true(a, x + 1, [&](uint32_t q) { return sg_ld_i32(pm + q) >= xs; });
        uint32_t c = 0;
        for (uint32_t q0 = wlo; q0 < whi; q0 += WAVE) {
            const uint32_t q = q0 + lane;
            if (q < whi && xs <= se[q] && xe >= ss[q]) {
                c++;
                if (q == x) sg_st_u8(gstate + q, 1);
                else if (sg_ld_u8(gstate + q) == 0) sg_st_u8(gstate + q, 2);
            }
        }
        c = wave_sum(c);
        if (lane == 0 && c > 1) {
            cnt[seed] = c; keep[seed] = 1u; cstart[seed] = wlo; cend[seed] = whi;   // (the fill only needs the stretch that holds the overlaps)
            atomicAdd(total, (unsigned long long)c);
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");                // this seed's state stores before the cursor's next loads
    }
}

// ---- seeds: a wave per component that starts inside the wave's 64 positions ----------------------------------------------------------------
// cnt[i] / keep[i] / cstart[i] / cend[i] (a stretch of positions that holds every overlap of the seed: its component, or less) are indexed by
// the seed's member index i and only written for groups of more than one member.
__global__ __launch_bounds__(SG_THREADS) void sg_seeds_kernel(const int32_t *__restrict__ ss, const int32_t *__restrict__ se, const uint32_t *__restrict__ sid,
                                                             const uint32_t *__restrict__ posof, const uint8_t *__restrict__ head, uint32_t n,
                                                             uint8_t *gstate /* zeroed */, int32_t *pm,
                                                             uint32_t *__restrict__ cnt, uint32_t *__restrict__ keep, uint32_t *__restrict__ cstart,
                                                             uint32_t *__restrict__ cend, unsigned long long *__restrict__ total, uint32_t *__restrict__ err)
{
    __shared__ int32_t l_s[SG_WAVES][SG_LDS_CAP], l_e[SG_WAVES][SG_LDS_CAP];
    __shared__ uint32_t l_r[SG_WAVES][SG_LDS_CAP];
    __shared__ uint8_t l_st[SG_WAVES][SG_LDS_CAP];
    const int lane = lane_id(), w = threadIdx.x >> 6;
    const uint32_t p = blockIdx.x * SG_THREADS + threadIdx.x;
    const bool valid = p < n;
    // components of one member have no group to report
    const bool starts = valid && head[p] && p + 1 < n && !head[p + 1];
    uint64_t todo = __ballot(starts);
    while (todo) {
        const uint32_t a = uniform32(p - (uint32_t)lane + (uint32_t)(__ffsll((unsigned long long)todo) - 1));
        todo &= todo - 1;
        uint32_t b = n;                                                   // one past the component's last position: the next head
        for (uint32_t q0 = a + 1; q0 < n; q0 += WAVE) {
            const uint32_t q = q0 + (uint32_t)lane;
            const uint64_t hb = __ballot(q >= n || head[q]);
            if (hb) { b = q0 + (uint32_t)(__ffsll((unsigned long long)hb) - 1); break; }
        }
        b = uniform32(min(b, n));
        const uint32_t k = b - a;
        const bool in_lds = k <= SG_LDS_CAP;
        if (!in_lds) {
            // running maximum of the ends and the range of the ranks, one pass
            int32_t carry = INT32_MIN;
            uint32_t rmin = 0xffffffffu, rmax = 0;
            for (uint32_t q0 = 0; q0 < k; q0 += WAVE) {
                const uint32_t q = q0 + (uint32_t)lane;
                int32_t m = wave_incl_max(q < k ? se[a + q] : INT32_MIN);
                m = max(m, carry);
                if (q < k) { sg_st_i32(pm + a + q, m); const uint32_t r = sid[a + q]; rmin = min(rmin, r); rmax = max(rmax, r); }
                carry = __shfl(m, WAVE - 1, 64);
            }
            rmin = uniform32(sg_wave_min_u32(rmin)); rmax = uniform32(wave_max(rmax));
            if ((uint64_t)rmax - rmin < 8ull * k) {
                __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");      // the maxima are read by other lanes from here on
                sg_seed_by_cursor(ss, se, sid, posof, a, b, rmin, rmax, gstate, pm, cnt, keep, cstart, cend, total);
                continue;
            }
        }
        const int32_t *S = ss + a, *E = se + a;
        const uint32_t *R = sid + a;
        uint8_t *st = gstate + a;
        if (in_lds) {
            for (uint32_t q = (uint32_t)lane; q < k; q += WAVE) { l_s[w][q] = ss[a + q]; l_e[w][q] = se[a + q]; l_r[w][q] = sid[a + q]; l_st[w][q] = 0; }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");        // the staging stores before the broadcast reads of a seed's interval
            __builtin_amdgcn_wave_barrier();
            S = l_s[w]; E = l_e[w]; R = l_r[w]; st = l_st[w];
        }
        uint64_t best = SG_NONE;
        for (uint32_t q = (uint32_t)lane; q < k; q += WAVE) { const uint64_t c = ((uint64_t)R[q] << 32) | q; best = c < best ? c : best; }
        best = sg_wave_min_u64(best);
        uint32_t round = 0;
        for (; round < k && best != SG_NONE; round++) {                   // every round settles its seed: k rounds at the most
            const uint32_t x = (uint32_t)best;
            const int32_t xs = S[x], xe = E[x];
            uint32_t c = 0;
            uint64_t next = SG_NONE;
            for (uint32_t q = (uint32_t)lane; q < k; q += WAVE) {         // (a state byte is only ever touched by the lane that owns q)
                const bool ov = xs <= E[q] && xe >= S[q];
                c += ov ? 1u : 0u;
                if (st[q] == 0) {
                    if (ov) st[q] = q == x ? 1 : 2;
                    else { const uint64_t cand = ((uint64_t)R[q] << 32) | q; next = cand < next ? cand : next; }
                }
            }
            c = wave_sum(c);
            if (lane == 0 && c > 1) {
                const uint32_t i = (uint32_t)(best >> 32);
                cnt[i] = c; keep[i] = 1u; cstart[i] = a; cend[i] = b;
                atomicAdd(total, (unsigned long long)c);
            }
            best = sg_wave_min_u64(next);
        }
        if (best != SG_NONE && lane == 0) atomicOr(err, 1u);              // (the word is shared with the table kernel's domain bit) cannot happen; reported (CSV_EHIP), never silently wrong
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");            // this component's LDS reads before the next one's staging stores
        __builtin_amdgcn_wave_barrier();
    }
}

// ---- offsets: group -> seed, group -> first member, segment -> first group; the scalars the host sizes the output with ----------------------
__global__ __launch_bounds__(SG_THREADS) void sg_offsets_kernel(const uint32_t *__restrict__ moff /* [n + 1] exclusive */, const uint32_t *__restrict__ goff /* [n + 1] exclusive */,
                                                               const uint64_t *__restrict__ seg_off, uint64_t n_seg, uint32_t n, const unsigned long long *__restrict__ total,
                                                               const uint32_t *__restrict__ err, const uint32_t *__restrict__ sort_err, uint32_t *__restrict__ seed_of_group,
                                                               uint64_t *__restrict__ group_off, uint64_t *__restrict__ seg_group_off, uint64_t *__restrict__ res)
{
    const uint64_t t = (uint64_t)blockIdx.x * SG_THREADS + threadIdx.x;
    if (t < n) {
        const uint32_t g = goff[t];
        if (goff[t + 1] != g) { seed_of_group[g] = (uint32_t)t; group_off[g] = moff[t]; }
    } else if (t == n) {
        group_off[goff[n]] = *total;
        // (both give-up flags are exactly 1 — sg_seeds ORs 1 into *err, a onesweep pass stores 1 —, so that the value 2 in this word stays the table
        // kernel's domain bit, SG_ERR_DOMAIN in api/split_fits.hip, which sg_wait tells apart)
        res[0] = *total; res[1] = goff[n]; res[2] = (uint64_t)(*err | (sort_err ? *sort_err : 0u));
    } else if (t - n - 1 <= n_seg) {
        const uint64_t c = t - n - 1;
        seg_group_off[c] = goff[seg_off[c]];
    }
}

// ---- fill: a wave per group writes (group ‖ pre, member index within the segment) for every member of the seed's component that overlaps it --
__global__ __launch_bounds__(SG_THREADS) void sg_fill_kernel(const int32_t *__restrict__ ss, const int32_t *__restrict__ se, const uint32_t *__restrict__ sid,
                                                            const uint32_t *__restrict__ posof, const uint32_t *__restrict__ plo, const uint32_t *__restrict__ lp1,
                                                            const uint32_t *__restrict__ lsum /* exclusive sum of the link histogram, [n + 1] */,
                                                            const uint32_t *__restrict__ cstart, const uint32_t *__restrict__ cend, const uint32_t *__restrict__ seed_of_group,
                                                            const uint64_t *__restrict__ group_off, uint32_t n_groups, int pre_bits, uint64_t *__restrict__ keys,
                                                            uint32_t *__restrict__ vals)
{
    const int lane = lane_id();
    const uint32_t g = blockIdx.x * SG_WAVES + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    const uint32_t i = seed_of_group[g], x = posof[i];
    const int32_t xs = ss[x], xe = se[x];
    const uint32_t a = cstart[i], b = cend[i], lo = plo[x];
    uint64_t out = group_off[g];
    const uint64_t lt = lanemask_lt();
    for (uint32_t q0 = a; q0 < b; q0 += WAVE) {
        const uint32_t q = q0 + (uint32_t)lane;
        const bool ov = q < b && xs <= se[q] && xe >= ss[q];
        const uint64_t bal = __ballot(ov);
        if (ov) {
            const uint32_t pre = lp1[q] - 1u + lsum[q + 1] - q;           // L + 1 + R with R = lsum[q + 1] - (q + 1)
            const uint64_t at = out + (uint64_t)__popcll(bal & lt);
            keys[at] = ((uint64_t)g << pre_bits) | pre;
            vals[at] = sid[q] - lo;
        }
        out += (uint64_t)__popcll(bal);
    }
}

// ------------------------------------------------------------------------------------------------------------------------------------
#define SG_GRID(n) dim3((unsigned)(((uint64_t)(n) + SG_THREADS - 1) / SG_THREADS)), dim3(SG_THREADS)

void launch_sg_keys(hipStream_t s, const int32_t *start, const uint64_t *seg_off, uint64_t n_seg, uint32_t n, uint64_t *keys, uint32_t *vals)
{
    if (n) hipLaunchKernelGGL(sg_keys_kernel, SG_GRID(n), 0, s, start, seg_off, n_seg, n, keys, vals);
}

void launch_sg_links(hipStream_t s, const SplitGroupsWs &w, const uint64_t *keys, const uint32_t *vals, const int32_t *start, const int32_t *end,
                     const uint64_t *seg_off, uint32_t n)
{
    if (!n) return;
    hipLaunchKernelGGL(sg_unpack_kernel, SG_GRID(n), 0, s, keys, vals, start, end, seg_off, n, w.ss, w.se, w.sid, w.posof, w.plo, w.blk_min_id, w.blk_max_end);
    hipLaunchKernelGGL(sg_links_kernel, SG_GRID(n), 0, s, w.ss, w.se, w.sid, w.plo, w.blk_min_id, w.blk_max_end, n, w.lp1, w.hist, w.head);
}

void launch_sg_seeds(hipStream_t s, const SplitGroupsWs &w, uint32_t n)
{
    if (n) hipLaunchKernelGGL(sg_seeds_kernel, SG_GRID(n), 0, s, w.ss, w.se, w.sid, w.posof, w.head, n, w.state, w.pm, w.cnt, w.keep, w.cstart, w.cend, w.total, w.err);
}

void launch_sg_offsets(hipStream_t s, const SplitGroupsWs &w, const uint64_t *seg_off, uint64_t n_seg, uint32_t n, const uint32_t *sort_err)
{
    hipLaunchKernelGGL(sg_offsets_kernel, SG_GRID((uint64_t)n + 2 + n_seg), 0, s, w.cnt, w.keep, seg_off, n_seg, n, w.total, w.err, sort_err, w.seed_of_group,
                       w.group_off, w.seg_group_off, w.res);
}

void launch_sg_fill(hipStream_t s, const SplitGroupsWs &w, uint32_t n_groups, int pre_bits, uint64_t *keys, uint32_t *vals)
{
    if (n_groups) hipLaunchKernelGGL(sg_fill_kernel, dim3((n_groups + SG_WAVES - 1) / SG_WAVES), dim3(SG_THREADS), 0, s, w.ss, w.se, w.sid, w.posof, w.plo, w.lp1, w.hist,
                                     w.cstart, w.cend, w.seed_of_group, w.group_off, n_groups, pre_bits, keys, vals);
}

}  // namespace csv
