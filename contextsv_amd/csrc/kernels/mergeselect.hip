// mergeselect.hip — the representative choice of mergeSVs on the device (gfx950): for every bucket of equally labelled signatures, the member
// that libstdc++'s UNSTABLE std::sort by length descending leaves at slot [top / 2] (the reference's sv_object.cpp:190-230; the host form is
// host/sort_select.h). The rule is sort_select_core.hpp: the chain of partitions that decides one slot, each partition a map, two prefix
// counts and a scatter over the range — exact, ties included.
//
// Three forms by segment size, chosen on the device from the offsets:
//   sz <= 16            16 lanes per segment: no partition happens, the member whose stable rank is the slot (ss_small_kernel). The same
//                       kernel marks the kept buckets and appends the larger segments to the two lists below.
//   17 .. LDS_CAP       one workgroup of 256 per segment, entries and pair lists in LDS (49 288 bytes: three workgroups per CU).
//   above LDS_CAP       one workgroup of 1024 per segment that streams the rounds through global memory — the entries are permuted in place,
//                       the pair lists lie in a scratch slice as long as the segment — until the kept range fits LDS, then goes on there.
// A round of a workgroup: lane 0 moves the median of three to the front; every wave walks a contiguous share of the range in coalesced
// 64-entry tiles and counts the two flags with ballots; the waves' totals give every position its two counts on a second walk, where the
// swapped positions scatter themselves into the pair lists and the lowest cut candidate is kept; pair k is swapped by lane k. Four
// barriers a round, at most 2 floor(log2 sz) rounds, a caller's bound where it is lower: a chain that needs more is DECLINED (idx NONE), never
// answered wrong — the library heap-sorts there, which is not replayed.
#include "../layouts.hpp"
#include "../devutil.hpp"
#define SSC_HD __host__ __device__
#include "../sort_select_core.hpp"

namespace csv {

namespace ssc = sort_select_core;
using ssc::Ent;

constexpr int SS_SMALL_THREADS = 256, SS_GROUP = 16;
constexpr int SS_MID_THREADS = 256, SS_BIG_THREADS = 1024;
static_assert(SORT_SLOT_LDS_CAP == ssc::LDS_CAP, "the glue's constant and the core's must agree");

struct SsLds {
    Ent x[ssc::LDS_CAP];
    uint32_t list[ssc::LDS_CAP];         // list_a | list_b, half each: no position is in two pairs
    uint32_t wa[16], wb[16];             // the waves' flag counts
    uint32_t K, cut;                     // pairs of the round, its cut; at the end the answer
};

// One segment replayed by the workgroup: g[0 .. sz) its entries (permuted in place while the range is above LDS_CAP), glist[0 .. sz) scratch.
// Returns the chosen index to every thread, NONE when declined. sz > SMALL.
template <int T>
__device__ uint32_t ss_replay_wg(SsLds &S, Ent *g, uint32_t *glist, uint32_t sz, uint32_t nth, uint32_t max_partitions)
{
    constexpr uint32_t W = T / WAVE;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint64_t lt = lanemask_lt(), le = lt | (1ull << lane);
    uint32_t lo = 0, hi = sz, limit = ssc::depth_limit(sz, max_partitions);
    Ent *x = g;
    uint32_t *la = glist, *lb = glist + sz / 2;
    bool in_lds = false, declined = false;
    while (hi - lo > ssc::SMALL) {
        if (!in_lds && hi - lo <= ssc::LDS_CAP) {
            for (uint32_t i = tid; i < hi - lo; i += T) S.x[i] = g[lo + i];
            nth -= lo; hi -= lo; lo = 0;
            x = S.x; la = S.list; lb = S.list + ssc::LDS_CAP / 2; in_lds = true;
            __syncthreads();
        }
        if (limit == 0) { declined = true; break; }
        --limit;
        if (tid == 0) { ssc::median_to_first(x, lo, hi); S.K = 0; S.cut = hi; }
        __syncthreads();
        const uint32_t pv = ssc::len_of(x[lo]), first = lo + 1, m = hi - first;
        const uint32_t span = (((m + W - 1) / W) + 63u) & ~63u;
        const uint32_t ws = min(first + w * span, hi), we = min(ws + span, hi);      // (ws <= hi: w * span < m + 64 W)
        // the wave's flag counts
        uint32_t ca = 0, cb = 0;
        for (uint32_t t = ws; t < we; t += WAVE) {
            const uint32_t p = t + lane;
            const bool valid = p < we;
            const uint32_t len = valid ? ssc::len_of(x[p]) : 0u;
            ca += (uint32_t)__popcll(__ballot(valid && ssc::in_a(len, pv)));
            cb += (uint32_t)__popcll(__ballot(valid && ssc::in_b(len, pv)));
        }
        if (lane == 0) { S.wa[w] = ca; S.wb[w] = cb; }
        __syncthreads();
        uint32_t run_a = 0, rem_b = cb;                       // a-positions below the tile; b-positions from the tile on
        for (uint32_t k = 0; k < W; k++) { if (k < w) run_a += S.wa[k]; if (k > w) rem_b += S.wb[k]; }
        // every position decides for itself
        uint32_t kw = 0, wcut = ssc::NONE;
        for (uint32_t t = ws; t < we; t += WAVE) {
            const uint32_t p = t + lane;
            const bool valid = p < we;
            const uint32_t len = valid ? ssc::len_of(x[p]) : 0u;
            const bool a = valid && ssc::in_a(len, pv), b = valid && ssc::in_b(len, pv);
            const uint64_t ma = __ballot(a), mb = __ballot(b);
            const uint32_t a_before = run_a + (uint32_t)__popcll(ma & lt), b_after = rem_b - (uint32_t)__popcll(mb & le);
            const bool sa = ssc::swaps_a(a, a_before, b_after), sb = ssc::swaps_b(b, a_before, b_after);
            if (sa) la[a_before] = p;
            if (sb) lb[b_after] = p;
            kw += (uint32_t)__popcll(__ballot(sa));
            const uint64_t mc = __ballot(valid && ssc::cut_candidate(a, b, a_before, b_after));
            if (wcut == ssc::NONE && mc) wcut = t + (uint32_t)__ffsll((unsigned long long)mc) - 1u;      // positions ascend with the lanes and the tiles
            run_a += (uint32_t)__popcll(ma);
            rem_b -= (uint32_t)__popcll(mb);
        }
        if (lane == 0) {
            if (kw) atomicAdd(&S.K, kw);
            if (wcut != ssc::NONE) atomicMin(&S.cut, wcut);
        }
        __syncthreads();
        const uint32_t K = S.K, cut = S.cut;
        for (uint32_t k = tid; k < K; k += T) {
            const uint32_t pa = la[k], pb = lb[k];
            const Ent e = x[pa]; x[pa] = x[pb]; x[pb] = e;
        }
        __syncthreads();
        ssc::keep_side(lo, hi, cut, nth);
    }
    uint32_t res = ssc::NONE;
    if (!declined) {
        // the closing segment: in LDS, or — a streamed range cut straight to SMALL members or fewer — still in global memory, lo != 0
        if (tid < hi - lo && ssc::closing_rank(x, lo, hi, lo + tid) == nth - lo) S.cut = ssc::idx_of(x[lo + tid]);
        __syncthreads();
        res = S.cut;
    }
    __syncthreads();                                          // S is the next segment's
    return res;
}

__device__ __forceinline__ uint32_t ss_slot(const SortSlotArgs &b, uint64_t seg, uint32_t sz) { return b.nth ? b.nth[seg] : ssc::nth_of(sz); }

__global__ __launch_bounds__(SS_SMALL_THREADS) void ss_small_kernel(SortSlotArgs b)
{
    const uint32_t n_seg = *b.n_seg;
    const uint32_t gl = threadIdx.x & (SS_GROUP - 1);
    const uint64_t stride = (uint64_t)gridDim.x * (SS_SMALL_THREADS / SS_GROUP);
    for (uint64_t seg = ((uint64_t)blockIdx.x * SS_SMALL_THREADS + threadIdx.x) / SS_GROUP; seg < n_seg; seg += stride) {
        const uint32_t o0 = b.off[seg], sz = b.off[seg + 1] - o0;
        if (gl == 0 && b.keep) b.keep[seg] = sz >= 2 ? 1u : 0u;
        if (sz > ssc::SMALL) {
            if (gl == 0) {
                const int big = sz > ssc::LDS_CAP;
                const uint32_t k = atomicAdd(&b.cnt[big], 1u);
                (big ? b.big : b.mid)[k] = (uint32_t)seg;
            }
            continue;
        }
        if (sz == 0) { if (gl == 0) b.idx[seg] = ssc::NONE; continue; }
        const Ent *x = (const Ent *)b.ent + o0;
        if (gl < sz && ssc::closing_rank(x, 0u, sz, gl) == ss_slot(b, seg, sz)) b.idx[seg] = ssc::idx_of(x[gl]);
    }
}

template <int T>
__global__ __launch_bounds__(T) void ss_wg_kernel(SortSlotArgs b, int big)
{
    __shared__ SsLds S;
    const uint32_t n_list = b.cnt[big];
    const uint32_t *list = big ? b.big : b.mid;
    for (uint32_t k = blockIdx.x; k < n_list; k += gridDim.x) {
        const uint32_t seg = list[k], o0 = b.off[seg], sz = b.off[seg + 1] - o0;
        const uint32_t res = ss_replay_wg<T>(S, (Ent *)b.ent + o0, b.list + o0, sz, ss_slot(b, seg, sz), b.max_partitions);
        if (threadIdx.x == 0) b.idx[seg] = res;
    }
}

void launch_sort_slot(hipStream_t s, const SortSlotArgs &b, uint64_t n, uint64_t n_seg_bound)
{
    if (n_seg_bound == 0) return;
    (void)hipMemsetAsync(b.cnt, 0, 8, s);                                    // the two lists' counts ([2], the segments in all, is the caller's)
    const uint64_t groups = SS_SMALL_THREADS / SS_GROUP;
    hipLaunchKernelGGL(ss_small_kernel, dim3((unsigned)std::min<uint64_t>((n_seg_bound + groups - 1) / groups, 4096)), dim3(SS_SMALL_THREADS), 0, s, b);
    const uint64_t mid = std::min(n_seg_bound, n / (ssc::SMALL + 1)), big = std::min(n_seg_bound, n / (ssc::LDS_CAP + 1));
    if (mid) hipLaunchKernelGGL(ss_wg_kernel<SS_MID_THREADS>, dim3((unsigned)std::min<uint64_t>(mid, 2048)), dim3(SS_MID_THREADS), 0, s, b, 0);
    if (big) hipLaunchKernelGGL(ss_wg_kernel<SS_BIG_THREADS>, dim3((unsigned)std::min<uint64_t>(big, 256)), dim3(SS_BIG_THREADS), 0, s, b, 1);
}

// ---- the buckets of one type's signatures and the records of their representatives

__global__ void ms_keys_kernel(const int32_t *__restrict__ label, uint32_t n, uint64_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { keys[i] = (uint64_t)((uint32_t)label[i] + 2u); vals[i] = (uint32_t)i; }      // the slot: -2 (noise) first, as the reference's std::map walks
}

// sorted by slot, input order kept inside a slot (the sort is stable): the entries, and a mark on every bucket's first member
__global__ void ms_heads_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ vals, const csv_sig *__restrict__ sig, uint32_t n,
                                uint64_t *__restrict__ ent, uint32_t *__restrict__ head)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const uint32_t v = vals[i];
        ent[i] = ssc::make_ent(sig[v].end - sig[v].start, v);
        head[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
    } else if (i == n) head[n] = 0;
}

// head[] summed: a first member's value is its bucket's number, head[n] the buckets in all
__global__ void ms_offsets_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ head, uint32_t n, uint32_t *__restrict__ off,
                                  uint32_t *__restrict__ n_buckets)
{
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { if (i == 0 || keys[i] != keys[i - 1]) off[head[i]] = (uint32_t)i; }
    else if (i == n) { off[head[n]] = n; *n_buckets = head[n]; }
}

// keep[] summed: a kept bucket's value is its record's place among the type's, keep[n_buckets] the records in all
__global__ void ms_emit_kernel(MergeEmitArgs e)
{
    const uint32_t nb = *e.n_buckets;
    const uint64_t b = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t base = e.type ? e.counts->n_rep[0] : 0;
    if (b == 0) e.counts->n_rep[e.type] = e.keep[nb];
    if (b >= nb) return;
    const uint32_t o0 = e.off[b], sz = e.off[b + 1] - o0;
    if (sz < 2) return;
    const uint32_t pick = e.idx[b];
    if (pick == ssc::NONE) atomicAdd((unsigned long long *)&e.counts->n_declined[e.type], 1ull);
    const uint64_t r = base + e.keep[b];
    if (r >= e.capacity) return;
    csv_merge_rep rec;
    rec.sig = pick == ssc::NONE ? csv_sig{0, 0, 0, 0} : e.sig[pick];
    rec.label = (int32_t)(uint32_t)e.keys[o0] - 2;
    rec.cluster_size = sz;
    rec.status = pick == ssc::NONE ? 2u : 0u;
    rec.reserved = 0;
    e.rep[r] = rec;
}

// a type with fewer than two signatures: they pass through as they are (sv_object.cpp:85-92)
__global__ void ms_pass_kernel(const csv_sig *sig, uint32_t n, int type, csv_merge_counts *counts, csv_merge_rep *rep, uint64_t capacity)
{
    if (threadIdx.x || blockIdx.x) return;
    const uint64_t base = type ? counts->n_rep[0] : 0;
    counts->n_rep[type] = n;
    for (uint32_t i = 0; i < n; i++) {
        if (base + i >= capacity) break;
        csv_merge_rep rec;
        rec.sig = sig[i]; rec.label = -2; rec.cluster_size = 0; rec.status = 1; rec.reserved = 0;
        rep[base + i] = rec;
    }
}

void launch_merge_select_type(hipStream_t s, const MergeSelectWs &w, const csv_sig *sig, const int32_t *label, uint64_t n, int type, int key_bits,
                              uint32_t max_partitions, bool onesweep, csv_merge_counts *counts, csv_merge_rep *rep, uint64_t capacity, const uint32_t **gave_up)
{
    *gave_up = nullptr;
    if (n < 2) { hipLaunchKernelGGL(ms_pass_kernel, dim3(1), dim3(64), 0, s, sig, (uint32_t)n, type, counts, rep, capacity); return; }
    const unsigned threads = 256, grid = (unsigned)((n + 1 + threads - 1) / threads);
    hipLaunchKernelGGL(ms_keys_kernel, dim3(grid), dim3(threads), 0, s, label, (uint32_t)n, w.sw.k0, w.sw.v0);
    const int io = launch_radix_sort_u64(s, w.sw.k0, w.sw.v0, w.sw.k1, w.sw.v1, n, key_bits, w.sw.tmp, onesweep);
    *gave_up = radix_sort_gave_up(w.sw.tmp, n, key_bits, onesweep);
    const uint64_t *keys = io ? w.sw.k1 : w.sw.k0;
    const uint32_t *vals = io ? w.sw.v1 : w.sw.v0;
    hipLaunchKernelGGL(ms_heads_kernel, dim3(grid), dim3(threads), 0, s, keys, vals, sig, (uint32_t)n, w.ss.ent, w.head);
    launch_exclusive_sum_u32(s, w.head, n + 1, w.es_tmp);
    hipLaunchKernelGGL(ms_offsets_kernel, dim3(grid), dim3(threads), 0, s, keys, w.head, (uint32_t)n, w.ss.off, w.ss.cnt + 2);
    (void)hipMemsetAsync(w.keep, 0, (n + 1) * 4, s);
    SortSlotArgs b;
    b.off = w.ss.off; b.n_seg = w.ss.cnt + 2; b.nth = nullptr; b.ent = w.ss.ent; b.list = w.ss.list; b.mid = w.ss.mid; b.big = w.ss.big; b.cnt = w.ss.cnt;
    b.idx = w.ss.idx; b.keep = w.keep; b.max_partitions = max_partitions;
    launch_sort_slot(s, b, n, n);
    launch_exclusive_sum_u32(s, w.keep, n + 1, w.es_tmp);
    MergeEmitArgs e;
    e.off = w.ss.off; e.n_buckets = w.ss.cnt + 2; e.keys = keys; e.idx = w.ss.idx; e.keep = w.keep; e.sig = sig; e.type = type; e.counts = counts; e.rep = rep;
    e.capacity = capacity;
    hipLaunchKernelGGL(ms_emit_kernel, dim3(grid), dim3(threads), 0, s, e);
}

}  // namespace csv
