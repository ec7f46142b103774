// csvgpu.hip — implementation of the C-ABI in include/csvgpu.h: context, staging, kernel chains.
// No CPU fallback lives here: every result is produced by the kernels under kernels/.
#include <atomic>
#include <string.h>

#include <algorithm>
#include <new>

#include "layouts.hpp"
#include <chrono>
#include <unordered_map>

namespace csv {

static std::string g_create_err;
#ifdef CSV_TEST_HOOKS
// csvgpu_test_fail_next_alloc — only in the test build of the library (libcsvgpu_testhooks.so: Makefile), never in libcsvgpu.so
static std::atomic<int> g_fail_alloc{0};
static inline bool csv_test_fail_alloc()
{
    int n = g_fail_alloc.load();
    while (n > 0) if (g_fail_alloc.compare_exchange_weak(n, n - 1)) return true;
    return false;
}
#else
static inline bool csv_test_fail_alloc() { return false; }
#endif

int arena_reserve(csv_ctx *ctx, Arena &a, size_t bytes)
{
    bytes = align_up(bytes + 4096, 4096);
    if (bytes > a.cap) {
        CSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (a.base) CSV_HIP(ctx, hipFree(a.base));
        a.base = nullptr; a.cap = 0;
        size_t want = bytes + bytes / 4;
        if (hipMalloc((void **)&a.base, want) != hipSuccess) {
            (void)hipGetLastError();
            if (hipMalloc((void **)&a.base, bytes) != hipSuccess) { (void)hipGetLastError(); a.base = nullptr; ctx->err = "hipMalloc failed (arena)"; return CSV_ENOMEM; }
            want = bytes;
        }
        a.cap = want;
    }
    a.used = 0;
    return CSV_OK;
}

// Reserve `a` for a layout and carve it: carve(Arena &) -> bool runs on a planning arena (its `used` is the need), then on `a`. The carve
// writes its pointers into a workspace struct of the caller's; the planning pass's values are overwritten by the real pass.
template <class Carve>
static int arena_reserve_for(csv_ctx *ctx, Arena &a, const char *what, Carve &&carve)
{
    const int rc = arena_reserve(ctx, a, arena_plan_bytes(carve));
    if (rc) return rc;
    if (!carve(a)) { ctx->err = std::string("arena exhausted (") + what + ")"; return CSV_ENOMEM; }
    return CSV_OK;
}

int ensure_pinned(csv_ctx *ctx, size_t bytes)
{
    if (bytes <= ctx->pinned_cap) return CSV_OK;
    if (ctx->pinned) CSV_HIP(ctx, hipHostFree(ctx->pinned));
    ctx->pinned = nullptr; ctx->pinned_cap = 0;
    CSV_HIP(ctx, hipHostMalloc(&ctx->pinned, bytes, hipHostMallocDefault));
    ctx->pinned_cap = bytes;
    return CSV_OK;
}

// Host arrays of the host-pointer entry points travel through the context's page-locked block: the runtime stages a pageable
// hipMemcpyAsync itself, in chunks and under a lock that the other contexts' launches also take (seen as millisecond gaps in the lanes'
// big kernels whenever the caller's context copied its observation vectors). in(): bytes copied into the block, the block's address
// returned for the async copy; out(): a slot of the block the device writes to, copied to the caller's array by finish() after the wait;
// slot(): bytes of the block for the caller's own use. Built without a context it plans: the three only advance `used`.
// The block is sized like the arenas, by running the stage: pin_reserve_for plans `stage(PinStage &)`, grows the block once, then runs the
// stage on the real one. Nothing may grow the block while a PinStage over it is live.
struct PinStage {
    csv_ctx *ctx;
    size_t used = 0;
    struct Out { void *dst; const void *src; size_t bytes; };
    std::vector<Out> outs;
    explicit PinStage(csv_ctx *c = nullptr, size_t from = 0) : ctx(c), used(from) {}
    void *slot(size_t bytes) { void *p = ctx ? (char *)ctx->pinned + used : nullptr; used += align_up(bytes, 256); return p; }
    const void *in(const void *src, size_t bytes) { void *p = slot(bytes); if (ctx && bytes) memcpy(p, src, bytes); return p; }
    void *out(void *dst, size_t bytes) { void *p = slot(bytes); if (ctx) outs.push_back(Out{dst, p, bytes}); return p; }
    void finish() { for (const Out &o : outs) if (o.bytes) memcpy(o.dst, o.src, o.bytes); outs.clear(); }
};
template <class Stage>
static int pin_reserve_for(csv_ctx *ctx, PinStage &pin, Stage &&stage)
{
    PinStage plan(nullptr, pin.used);
    stage(plan);
    const int rc = ensure_pinned(ctx, plan.used);
    if (rc) return rc;
    stage(pin);
    return CSV_OK;
}
// the scalars that read_counters, check_reads_dev and dbscan_iv_chain read back through the block's first bytes: a stage whose call runs
// one of them while it is live starts with this slot, so that their ensure_pinned(kPinScalars) cannot grow the block under it
static constexpr size_t kPinScalars = 4096;

static hipEvent_t get_event(csv_ctx *ctx)
{
    if (!ctx->event_pool.empty()) { hipEvent_t e = ctx->event_pool.back(); ctx->event_pool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

bool timer_begin(csv_ctx *ctx, int id, hipStream_t s)
{
    if (!ctx->timing) return false;
    // every recorded event is a barrier packet in the queue (~5 us of idle device each): level 2 keeps them to the two groups a
    // roofline is quoted for
    if (ctx->timing >= 2 && id != CSV_K_CIGAR_SCAN && id != CSV_K_DEPTH) return false;
    Timer t; t.id = id; t.a = get_event(ctx); t.b = get_event(ctx); t.s = s ? s : ctx->stream;
    (void)hipEventRecord(t.a, t.s);
    ctx->timers.push_back(t);
    return true;
}

void timer_end(csv_ctx *ctx)
{
    if (!ctx->timing || ctx->timers.empty()) return;
    (void)hipEventRecord(ctx->timers.back().b, ctx->timers.back().s);
}

static void fold_timers(csv_ctx *ctx)
{
    for (Timer &t : ctx->timers) {
        float ms = 0.f;
        if (hipEventSynchronize(t.b) == hipSuccess && hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess) {
            ctx->t_ms[t.id] += ms; ctx->t_n[t.id]++;
        }
        if (t.own_a) ctx->event_pool.push_back(t.a);
        if (t.own_b) ctx->event_pool.push_back(t.b);
    }
    ctx->timers.clear();
}

// ---------------------------------------------------------------------------------------------
// device-side chains shared by the host- and device-pointer entry points

struct DevReads {
    csv_reads d;
    int32_t *ref_end, *q_start, *q_end;
    uint32_t *ckpt;
    ScanCounters *cnt;
};

static constexpr uint64_t kMaxReadWords = 0x7ffff000ull;       // exclusive bound on one read's CIGAR words
static inline uint32_t *bucket_off(ScanCounters *cnt) { return (uint32_t *)((char *)cnt + 256); }
static inline uint32_t *bucket_cur(ScanCounters *cnt) { return bucket_off(cnt) + BK_N; }

// copy a host shard into its carved slices (carve_reads); returns device views
static int stage_reads(csv_ctx *ctx, const csv_reads *r, const ReadsWs &w, DevReads &o)
{
    const uint64_t n = r->n_reads, m = r->n_cigar;
    hipStream_t s = ctx->stream;
    if (n) {
        CSV_HIP(ctx, hipMemcpyAsync(w.pos, r->pos, n * 4, hipMemcpyHostToDevice, s));
        CSV_HIP(ctx, hipMemcpyAsync(w.flag, r->flag, n * 2, hipMemcpyHostToDevice, s));
        CSV_HIP(ctx, hipMemcpyAsync(w.mapq, r->mapq, n, hipMemcpyHostToDevice, s));
    }
    CSV_HIP(ctx, hipMemcpyAsync(w.coff, r->cigar_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
    if (m) CSV_HIP(ctx, hipMemcpyAsync(w.cig, r->cigar, m * 4, hipMemcpyHostToDevice, s));
    CSV_HIP(ctx, hipMemsetAsync(w.cnt, 0, kCntBytes, s));
    o.ref_end = w.ref_end; o.q_start = w.q_start; o.q_end = w.q_end; o.cnt = w.cnt; o.ckpt = w.ckpt;
    o.d = *r;
    o.d.pos = w.pos; o.d.flag = w.flag; o.d.mapq = w.mapq; o.d.tid = nullptr; o.d.cigar_off = w.coff; o.d.cigar = w.cig;
    return CSV_OK;
}

static int check_reads_ptrs(csv_ctx *ctx, const csv_reads *r)
{
    if (!ctx) return CSV_EINVAL;
    if (!r || !r->cigar_off || (r->n_reads && (!r->pos || !r->flag || !r->mapq)) || (r->n_cigar && !r->cigar)) {
        ctx->err = "csv_reads: null array"; return CSV_EINVAL;
    }
    if (r->n_reads >= 0xffffffffull) { ctx->err = "csv_reads: more than 2^32-2 reads in one shard"; return CSV_EINVAL; }
    return CSV_OK;
}

// Host arrays. The kernels index the word array with cigar_off: nothing reaches the device unless the offsets are monotone and
// inside it (a read's own word count stays far below 2^31: the scan works in 32-bit read-relative indices).
static int check_reads(csv_ctx *ctx, const csv_reads *r)
{
    int rc = check_reads_ptrs(ctx, r);
    if (rc) return rc;
    for (uint64_t i = 0; i < r->n_reads; i++) {
        if (r->cigar_off[i + 1] < r->cigar_off[i]) { ctx->err = "csv_reads: cigar_off not monotone"; return CSV_EINVAL; }
        if (r->cigar_off[i + 1] - r->cigar_off[i] >= kMaxReadWords) { ctx->err = "csv_reads: a read with 2^31 CIGAR words"; return CSV_EINVAL; }
    }
    if (r->cigar_off[r->n_reads] > r->n_cigar) { ctx->err = "csv_reads: cigar_off beyond n_cigar"; return CSV_EINVAL; }
    return CSV_OK;
}

// The same test for arrays that already live in HBM (csvgpu_shard_wrap_dev): one small kernel, once per wrapped shard.
static int check_reads_dev(csv_ctx *ctx, const csv_reads *r)
{
    int rc = check_reads_ptrs(ctx, r);
    if (rc) return rc;
    if ((rc = ensure_pinned(ctx, kPinScalars))) return rc;
    uint32_t *d_bad = nullptr;
    CSV_HIP(ctx, hipMalloc((void **)&d_bad, 256));
    hipError_t e = hipMemsetAsync(d_bad, 0, 4, ctx->stream);
    if (e == hipSuccess) { launch_validate_offsets(ctx->stream, r->cigar_off, r->n_reads, r->n_cigar, kMaxReadWords, d_bad); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->pinned, d_bad, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_bad);
    if (e != hipSuccess) { ctx->err = std::string("csv_reads: offset check failed: ") + hipGetErrorString(e); return CSV_EHIP; }
    if (*(const uint32_t *)ctx->pinned) { ctx->err = "csv_reads: cigar_off not monotone or beyond n_cigar"; return CSV_EINVAL; }
    return CSV_OK;
}

// The waits of the per-chromosome pipeline last a fraction of a millisecond: polling for up to 100 us before blocking
// saves the tens of microseconds a blocked thread takes to be woken, during which the device has nothing queued.
constexpr std::chrono::microseconds kSpinLimit(100);
static hipError_t wait_stream(hipStream_t s)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > kSpinLimit) return hipStreamSynchronize(s);
    }
}
static hipError_t wait_event(hipEvent_t ev)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > kSpinLimit) return hipEventSynchronize(ev);
    }
}

// The scan form of a shard created, or a host-pointer call made, on this context: the forced one (csv_tuning), behind scan_form_for's guard.
static int scan_form(const csv_ctx *ctx, uint64_t n_reads, uint64_t n_cigar)
{
    const int by_rule = scan_form_for(n_reads, n_cigar);
    return (ctx->tuning.scan_form == CSV_FORM_AUTO || n_cigar >= 0xffffffffull) ? by_rule : ctx->tuning.scan_form;
}
static bool onesweep(const csv_ctx *ctx) { return !ctx->tuning.sort_three_launch; }

static int read_counters(csv_ctx *ctx, const ScanCounters *d_cnt, ScanCounters &h)
{
    int rc = ensure_pinned(ctx, kPinScalars);
    if (rc) return rc;
    CSV_HIP(ctx, hipMemcpyAsync(ctx->pinned, d_cnt, sizeof(ScanCounters), hipMemcpyDeviceToHost, ctx->stream));
    CSV_HIP(ctx, wait_stream(ctx->stream));
    memcpy(&h, ctx->pinned, sizeof(ScanCounters));
    return CSV_OK;
}

// sig_raw[0..n) (arbitrary order) -> sig_sorted in the reference's vector order; optional SoA start/end.
// with_type: DEL calls first, then INS calls (per-type subsequences of the vector).
// key layout of the ordering pass: start in the low bits (width from the contig length), the type bit above it
struct KeyLayout { int start_bits, type_pos, key_bits, bucket_shift; };
static KeyLayout key_layout(uint32_t depth_len, bool overflow, bool with_type)
{
    KeyLayout k;
    // starts are < scan_start_limit(depth_len) unless the scan flagged an overflow (then the full 32 bits are sorted)
    k.start_bits = overflow ? 32 : std::max(1, bits_of((uint64_t)scan_start_limit(depth_len) - 1));
    k.type_pos = with_type ? k.start_bits : -1;
    k.key_bits = k.start_bits + (with_type ? 1 : 0);
    k.bucket_shift = std::max(0, k.key_bits - (int)BK_BITS);
    return k;
}

// The ordering pass's bucket counts (and, for shards known to be coordinate-sorted, the depth tiles' candidate ranges) are taken
// by the scan itself: nothing small runs between the scan and the depth pass.
static ScanExtras scan_extras(ScanCounters *cnt, uint32_t depth_len, bool with_type, uint64_t *tile_range)
{
    ScanExtras x;
    const KeyLayout k = key_layout(depth_len, false, with_type);
    x.bucket_hist = bucket_off(cnt); x.type_pos = k.type_pos; x.bucket_shift = k.bucket_shift;
    x.tile_range = tile_range; x.n_tiles = tile_range ? depth_n_tiles(depth_len) : 0;
    return x;
}

static void order_signatures(csv_ctx *ctx, const csv_sig *sig_raw, uint64_t n, uint32_t depth_len, uint32_t overflow, uint32_t max_bucket,
                             ScanCounters *cnt, bool with_type, SortWs &w, csv_sig *sig_sorted, uint32_t *start_out, uint32_t *end_out)
{
    if (!n) return;
    TimerScope ts(ctx, CSV_K_SORT);
    if (!overflow && max_bucket <= BK_LOCAL_MAX) {
        const KeyLayout k = key_layout(depth_len, false, with_type);
        launch_bucket_sort(ctx->stream, sig_raw, n, k.type_pos, k.bucket_shift, bucket_off(cnt), bucket_cur(cnt), w.sig_tmp, sig_sorted, start_out, end_out);
        return;
    }
    const KeyLayout kl = key_layout(depth_len, overflow != 0, with_type);
    const int type_pos = kl.type_pos, key_bits = kl.key_bits;
    launch_sig_make_keys(ctx->stream, sig_raw, n, 0, type_pos, w.k0, w.v0);
    const int in_out = launch_radix_sort_u64(ctx->stream, w.k0, w.v0, w.k1, w.v1, n, key_bits, w.tmp, onesweep(ctx));
    launch_sig_fix_ties_gather(ctx->stream, sig_raw, in_out ? w.k1 : w.k0, in_out ? w.v1 : w.v0, n, sig_sorted, start_out, end_out);
}

// depth chain on device arrays. pmax / ord / range scratch is `ws` (carve_depth); `ranges` != nullptr: the scan already produced the
// tiles' candidate ranges (coordinate-sorted shard) and only the tile kernel remains.
static int depth_chain(csv_ctx *ctx, const DepthWs &ws, const csv_reads &d, const int32_t *ref_end, const uint32_t *ckpt, bool unsorted, uint32_t depth_len,
                       uint32_t *depth, ScanCounters *cnt, const uint64_t *ranges = nullptr, uint32_t cigar_pad = 0, void *items = nullptr,
                       int form = SCAN_FORM_WAVE)
{
    const uint64_t n = d.n_reads;
    TimerScope ts(ctx, CSV_K_DEPTH);
    if (n == 0 || depth_len == 0) {
        if (depth && depth_len) CSV_HIP(ctx, hipMemsetAsync(depth, 0, (size_t)depth_len * 4, ctx->stream));
        return CSV_OK;
    }
    if (ranges && !unsorted) {
        launch_depth_tiles(ctx->stream, d, nullptr, ref_end, ckpt, depth_len, depth, cnt, ranges, cigar_pad, items, form);
        return CSV_OK;
    }
    int32_t *pmax = ws.pmax;
    void *ptmp = ws.ptmp;
    uint64_t *ttmp = ws.ttmp;
    const uint32_t *ord = nullptr;
    const int32_t *pos_s = d.pos;
    const int32_t *end_s = ref_end;
    if (unsorted) {
        // shard not coordinate-sorted: sort the read indices by pos on device and feed the tile search through `ord`
        const SortWs &w = ws.w;
        uint32_t *pos_g = ws.pos_g, *end_g = ws.end_g;
        launch_iota_keys_i32(ctx->stream, d.pos, n, w.k0, w.v0);
        const int io = launch_radix_sort_u64(ctx->stream, w.k0, w.v0, w.k1, w.v1, n, 32, w.tmp, onesweep(ctx));
        const uint32_t *perm = io ? w.v1 : w.v0;
        launch_gather_u32(ctx->stream, (const uint32_t *)d.pos, perm, n, pos_g);
        launch_gather_u32(ctx->stream, (const uint32_t *)ref_end, perm, n, end_g);
        ord = perm; pos_s = (const int32_t *)pos_g; end_s = (const int32_t *)end_g;
    }
    launch_prefix_max(ctx->stream, end_s, pmax, n, ptmp);
    launch_depth_ranges(ctx->stream, pos_s, pmax, n, depth_len, ttmp);
    launch_depth_tiles(ctx->stream, d, ord, ref_end, ckpt, depth_len, depth, cnt, ttmp, cigar_pad, items, form);
    return CSV_OK;
}
// ctx->work for a shard's depth chain: reserved when the job begins (ws == nullptr), carved again — the same carve, the same arguments —
// by whichever later step queues the chain
static int depth_work(csv_ctx *ctx, const csv_shard *sh, DepthWs *ws)
{
    DepthWs w;
    if (!ws) return arena_reserve_for(ctx, ctx->work, "depth", [&](Arena &a) { return carve_depth(a, sh->d.n_reads, sh->depth_len, w); });
    ctx->work.used = 0;
    if (!carve_depth(ctx->work, sh->d.n_reads, sh->depth_len, *ws)) { ctx->err = "arena exhausted (depth)"; return CSV_ENOMEM; }
    return CSV_OK;
}

// interval DBSCAN on device arrays in caller order
static int dbscan_iv_chain(csv_ctx *ctx, const DbscanIvWs &ws, const uint32_t *d_start, const uint32_t *d_end, uint64_t n, double eps,
                           int min_pts, int32_t *d_labels)
{
    if (n == 0) return CSV_OK;
    unsigned int *flag = ws.flag;
    void *tmp = ws.tmp;
    CSV_HIP(ctx, hipMemsetAsync(flag, 0, 4, ctx->stream));
    launch_check_sorted_u32(ctx->stream, d_start, n, flag);
    int rc = ensure_pinned(ctx, kPinScalars);
    if (rc) return rc;
    CSV_HIP(ctx, hipMemcpyAsync(ctx->pinned, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    CSV_HIP(ctx, wait_stream(ctx->stream));
    const bool unsorted = *(unsigned int *)ctx->pinned != 0;
    if (!unsorted) {
        TimerScope ts(ctx, CSV_K_DBSCAN);
        launch_dbscan_iv_sorted(ctx->stream, d_start, d_end, nullptr, n, n, eps, min_pts, nullptr, d_labels, tmp);
        return CSV_OK;
    }
    const SortWs &w = ws.w;
    uint32_t *s_s = ws.s_s, *e_s = ws.e_s;
    const uint32_t *perm;
    {
        TimerScope ts(ctx, CSV_K_SORT);
        launch_iota_keys_u32(ctx->stream, d_start, n, w.k0, w.v0);
        const int io = launch_radix_sort_u64(ctx->stream, w.k0, w.v0, w.k1, w.v1, n, 32, w.tmp, onesweep(ctx));
        perm = io ? w.v1 : w.v0;
        launch_gather_u32(ctx->stream, d_start, perm, n, s_s);
        launch_gather_u32(ctx->stream, d_end, perm, n, e_s);
    }
    TimerScope ts(ctx, CSV_K_DBSCAN);
    launch_dbscan_iv_sorted(ctx->stream, s_s, e_s, perm, n, n, eps, min_pts, nullptr, d_labels, tmp);
    return CSV_OK;
}

}  // namespace csv

using namespace csv;

// =============================================================================================
extern "C" {

int csvgpu_abi_version(void) { return CSVGPU_ABI_VERSION; }

const char *csvgpu_last_error(const csv_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

static csv_ctx *create_ctx(int device_ordinal, void *stream, int low_priority);
csv_ctx *csvgpu_create(int device_ordinal, void *stream) { return create_ctx(device_ordinal, stream, 0); }
csv_ctx *csvgpu_create_background(int device_ordinal) { return create_ctx(device_ordinal, nullptr, 1); }

static csv_ctx *create_ctx(int device_ordinal, void *stream, int low_priority)
{
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev <= 0) {
        (void)hipGetLastError();
        g_create_err = std::string("no usable HIP device: ") + (e != hipSuccess ? hipGetErrorString(e) : "device count 0");
        return nullptr;
    }
    if (device_ordinal < 0 || device_ordinal >= n_dev) { g_create_err = "device ordinal out of range"; return nullptr; }
    if (hipSetDevice(device_ordinal) != hipSuccess) { g_create_err = "hipSetDevice failed"; return nullptr; }
    csv_ctx *ctx = new (std::nothrow) csv_ctx();
    if (!ctx) { g_create_err = "out of host memory"; return nullptr; }
    ctx->device = device_ordinal;
    if (stream) { ctx->stream = (hipStream_t)stream; ctx->own_stream = false; }
    else {
        int least = 0, greatest = 0;
        if (low_priority) (void)hipDeviceGetStreamPriorityRange(&least, &greatest);
        const hipError_t se = low_priority ? hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, least) : hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
        if (se != hipSuccess) { g_create_err = "hipStreamCreate failed"; delete ctx; return nullptr; }
        ctx->own_stream = true;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_ordinal) == hipSuccess) ctx->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    return ctx;
}

static void split_state_free(csv_ctx *ctx);
void csvgpu_destroy(csv_ctx *ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    fold_timers(ctx);
    for (hipEvent_t e : ctx->event_pool) (void)hipEventDestroy(e);
    if (ctx->arena.base) (void)hipFree(ctx->arena.base);
    if (ctx->work.base) (void)hipFree(ctx->work.base);
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    if (ctx->job_pin) (void)hipHostFree(ctx->job_pin);
    for (auto &b : ctx->host_pool) (void)hipHostFree(b.first);
    for (auto &b : ctx->host_live) (void)hipHostFree(b.first);       // blocks the caller never returned
    if (ctx->side) (void)hipStreamDestroy(ctx->side);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    split_state_free(ctx);
    delete ctx;
}

int csvgpu_synchronize(csv_ctx *ctx)
{
    if (!ctx) return CSV_EINVAL;
    CSV_HIP(ctx, wait_stream(ctx->stream));
    return CSV_OK;
}

int csvgpu_set_tuning(csv_ctx *ctx, const csv_tuning *t)
{
    if (!ctx) return CSV_EINVAL;
    if (ctx->job_pin_busy || ctx->split_state) { ctx->err = "set_tuning: a job or a split order is open on this context"; return CSV_EINVAL; }
    const csv_tuning defaults = CSV_TUNING_DEFAULTS;
    if (!t) t = &defaults;
    if (t->scan_form < CSV_FORM_AUTO || t->scan_form > CSV_FORM_LANES) { ctx->err = "set_tuning: scan_form must be CSV_FORM_AUTO or one of the four forms"; return CSV_EINVAL; }
    if (t->split_tail < CSV_TAIL_AUTO || t->split_tail > CSV_TAIL_MAX) { ctx->err = "set_tuning: split_tail must be CSV_TAIL_AUTO or 0..CSV_TAIL_MAX"; return CSV_EINVAL; }
    for (int32_t flag : {t->sort_three_launch, t->dbscan_all_pairs, t->split_chain_only})
        if (flag != 0 && flag != 1) { ctx->err = "set_tuning: sort_three_launch, dbscan_all_pairs and split_chain_only must be 0 or 1"; return CSV_EINVAL; }
    ctx->tuning = *t;
    return CSV_OK;
}

int csvgpu_timing_enable(csv_ctx *ctx, int on) { if (!ctx) return CSV_EINVAL; ctx->timing = on < 0 ? 0 : (on > 3 ? 1 : on); return CSV_OK; }

int csvgpu_timing_reset(csv_ctx *ctx)
{
    if (!ctx) return CSV_EINVAL;
    CSV_HIP(ctx, wait_stream(ctx->stream));
    fold_timers(ctx);
    for (int i = 0; i < CSV_K_COUNT; i++) { ctx->t_ms[i] = 0; ctx->t_n[i] = 0; }
    ctx->timer_tick = 0;
    return CSV_OK;
}

int csvgpu_timing_get(csv_ctx *ctx, int kernel_id, double *total_ms, uint64_t *launches)
{
    if (!ctx || kernel_id < 0 || kernel_id >= CSV_K_COUNT) return CSV_EINVAL;
    CSV_HIP(ctx, wait_stream(ctx->stream));
    fold_timers(ctx);
    if (total_ms) *total_ms = ctx->t_ms[kernel_id];
    if (launches) *launches = ctx->t_n[kernel_id];
    return CSV_OK;
}

// ---------------------------------------------------------------------------------------------
int csvgpu_cigar_scan(csv_ctx *ctx, const csv_reads *reads, uint32_t depth_len, uint32_t min_oplen, uint8_t min_mapq,
                      csv_sig *out, uint64_t *n_out)
{
    int rc = check_reads(ctx, reads);
    if (rc) return rc;
    if (!n_out || (*n_out && !out)) { ctx->err = "cigar_scan: null output"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    const uint64_t cap = std::min<uint64_t>(*n_out, reads->n_cigar);
    ReadsWs rw;
    csv_sig *sig_raw = nullptr;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "cigar_scan", [&](Arena &a) {
            return carve_reads(a, reads->n_reads, reads->n_cigar, rw) && take(a, sig_raw, cap * sizeof(csv_sig) + 16);
        }))) return rc;
    DevReads dr;
    if ((rc = stage_reads(ctx, reads, rw, dr))) return rc;
    {
        TimerScope ts(ctx, CSV_K_CIGAR_SCAN);
        launch_cigar_scan(ctx->stream, ctx->n_cu, dr.d, depth_len, min_oplen, min_mapq, 1, sig_raw, cap, dr.ref_end, dr.q_start, dr.q_end, dr.ckpt, dr.cnt,
                          scan_extras(dr.cnt, depth_len, false, nullptr), nullptr, scan_form(ctx, reads->n_reads, reads->n_cigar));
    }
    ScanCounters h;
    if ((rc = read_counters(ctx, dr.cnt, h))) return rc;
    const uint64_t n = h.n_sig;
    *n_out = n;
    if (n > cap) { ctx->err = "cigar_scan: output capacity too small"; return CSV_ECAPACITY; }
    if (n == 0) return CSV_OK;
    SortWs w;
    csv_sig *sig_sorted = nullptr;
    if ((rc = arena_reserve_for(ctx, ctx->work, "sort", [&](Arena &a) { return take(a, sig_sorted, n * sizeof(csv_sig)) && sortws_carve(a, n, w); }))) return rc;
    order_signatures(ctx, sig_raw, n, depth_len, h.max_start, h.max_len, dr.cnt, false, w, sig_sorted, nullptr, nullptr);
    CSV_HIP(ctx, hipMemcpyAsync(out, sig_sorted, n * sizeof(csv_sig), hipMemcpyDeviceToHost, ctx->stream));
    CSV_HIP(ctx, wait_stream(ctx->stream));
    return CSV_OK;
}

int csvgpu_aln_intervals(csv_ctx *ctx, const csv_reads *reads, int32_t *ref_end, int32_t *q_start, int32_t *q_end)
{
    int rc = check_reads(ctx, reads);
    if (rc) return rc;
    if (reads->n_reads && (!ref_end || !q_start || !q_end)) { ctx->err = "aln_intervals: null output"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    ReadsWs rw;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "aln_intervals", [&](Arena &a) { return carve_reads(a, reads->n_reads, reads->n_cigar, rw); }))) return rc;
    DevReads dr;
    if ((rc = stage_reads(ctx, reads, rw, dr))) return rc;
    {
        TimerScope ts(ctx, CSV_K_CIGAR_SCAN);
        launch_cigar_scan(ctx->stream, ctx->n_cu, dr.d, 0, 0, 0, 0, nullptr, 0, dr.ref_end, dr.q_start, dr.q_end, dr.ckpt, dr.cnt, ScanExtras(), nullptr,
                          scan_form(ctx, reads->n_reads, reads->n_cigar));
    }
    const uint64_t n = reads->n_reads;
    if (n) {
        CSV_HIP(ctx, hipMemcpyAsync(ref_end, dr.ref_end, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        CSV_HIP(ctx, hipMemcpyAsync(q_start, dr.q_start, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        CSV_HIP(ctx, hipMemcpyAsync(q_end, dr.q_end, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    CSV_HIP(ctx, wait_stream(ctx->stream));
    return CSV_OK;
}

int csvgpu_depth(csv_ctx *ctx, const csv_reads *reads, uint32_t depth_len, uint32_t *depth, uint64_t *sum, uint32_t *nonzero)
{
    int rc = check_reads(ctx, reads);
    if (rc) return rc;
    (void)hipSetDevice(ctx->device);
    ReadsWs rw;
    uint32_t *d_depth = nullptr;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "depth", [&](Arena &a) {
            return carve_reads(a, reads->n_reads, reads->n_cigar, rw) && take(a, d_depth, (size_t)depth_len * 4 + 16);
        }))) return rc;
    DevReads dr;
    if ((rc = stage_reads(ctx, reads, rw, dr))) return rc;
    {
        TimerScope ts(ctx, CSV_K_CIGAR_SCAN);
        launch_cigar_scan(ctx->stream, ctx->n_cu, dr.d, depth_len, 0, 0, 0, nullptr, 0, dr.ref_end, dr.q_start, dr.q_end, dr.ckpt, dr.cnt, ScanExtras(), nullptr,
                          scan_form(ctx, reads->n_reads, reads->n_cigar));
    }
    ScanCounters h;
    if ((rc = read_counters(ctx, dr.cnt, h))) return rc;
    DepthWs dw;
    if ((rc = arena_reserve_for(ctx, ctx->work, "depth chain", [&](Arena &a) { return carve_depth(a, reads->n_reads, depth_len, dw); }))) return rc;
    if ((rc = depth_chain(ctx, dw, dr.d, dr.ref_end, dr.ckpt, h.unsorted != 0, depth_len, d_depth, dr.cnt, nullptr, 0, nullptr,
                          scan_form(ctx, reads->n_reads, reads->n_cigar)))) return rc;
    if (depth && depth_len) CSV_HIP(ctx, hipMemcpyAsync(depth, d_depth, (size_t)depth_len * 4, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = read_counters(ctx, dr.cnt, h))) return rc;
    if (sum) *sum = h.depth_sum;
    if (nonzero) *nonzero = h.depth_nonzero;
    return CSV_OK;
}

static int check_dbscan_args(csv_ctx *ctx, double eps, int32_t min_pts, bool interval)
{
    if (!ctx) return CSV_EINVAL;
    if (!(eps >= 0.0) || (interval && !(eps < 1.0))) { ctx->err = interval ? "dbscan: eps must be in [0,1)" : "dbscan1d: eps must be >= 0"; return CSV_EINVAL; }
    if (min_pts < 1) { ctx->err = "dbscan: min_pts must be >= 1"; return CSV_EINVAL; }
    return CSV_OK;
}

int csvgpu_dbscan_iv_dev(csv_ctx *ctx, const uint32_t *d_start, const uint32_t *d_end, uint64_t n, double eps,
                         int32_t min_pts, int32_t *d_labels)
{
    int rc = check_dbscan_args(ctx, eps, min_pts, true);
    if (rc) return rc;
    if (n && (!d_start || !d_end || !d_labels)) { ctx->err = "dbscan: null array"; return CSV_EINVAL; }
    if (n >= 0xffffffffull) { ctx->err = "dbscan: n too large"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    DbscanIvWs ws;
    if ((rc = arena_reserve_for(ctx, ctx->work, "dbscan", [&](Arena &a) { return carve_dbscan_iv(a, n, ws); }))) return rc;
    return dbscan_iv_chain(ctx, ws, d_start, d_end, n, eps, min_pts, d_labels);
}

int csvgpu_dbscan_iv(csv_ctx *ctx, const uint32_t *start, const uint32_t *end, uint64_t n, double eps, int32_t min_pts,
                     int32_t *labels)
{
    int rc = check_dbscan_args(ctx, eps, min_pts, true);
    if (rc) return rc;
    if (n == 0) return CSV_OK;
    if (!start || !end || !labels) { ctx->err = "dbscan: null array"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    uint32_t *ds = nullptr, *de = nullptr;
    int32_t *dl = nullptr;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "dbscan arrays", [&](Arena &a) { return take(a, ds, n * 4) && take(a, de, n * 4) && take(a, dl, n * 4); }))) return rc;
    CSV_HIP(ctx, hipMemcpyAsync(ds, start, n * 4, hipMemcpyHostToDevice, ctx->stream));
    CSV_HIP(ctx, hipMemcpyAsync(de, end, n * 4, hipMemcpyHostToDevice, ctx->stream));
    if ((rc = csvgpu_dbscan_iv_dev(ctx, ds, de, n, eps, min_pts, dl))) return rc;
    CSV_HIP(ctx, hipMemcpyAsync(labels, dl, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    CSV_HIP(ctx, wait_stream(ctx->stream));
    return CSV_OK;
}

int csvgpu_dbscan_iv_batch(csv_ctx *ctx, const uint32_t *start, const uint32_t *end, const uint64_t *seg_off, uint64_t n_seg, double eps,
                           int32_t min_pts, int32_t *labels)
{
    int rc = check_dbscan_args(ctx, eps, min_pts, true);
    if (rc) return rc;
    if (n_seg == 0) return CSV_OK;
    if (!seg_off) { ctx->err = "dbscan batch: null seg_off"; return CSV_EINVAL; }
    uint64_t max_len = 0;
    for (uint64_t s = 0; s < n_seg; s++) {
        if (seg_off[s + 1] < seg_off[s]) { ctx->err = "dbscan batch: seg_off not monotone"; return CSV_EINVAL; }
        max_len = std::max(max_len, seg_off[s + 1] - seg_off[s]);
    }
    const uint64_t n = seg_off[n_seg];
    if (n == 0) return CSV_OK;
    if (!start || !end || !labels) { ctx->err = "dbscan batch: null array"; return CSV_EINVAL; }
    if (n >= 0xffffffffull) { ctx->err = "dbscan batch: n too large"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    uint32_t *ds = nullptr, *de = nullptr;
    int32_t *dl = nullptr;
    uint64_t *doff = nullptr;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "dbscan batch arrays", [&](Arena &a) {
            return take(a, ds, n * 4) && take(a, de, n * 4) && take(a, dl, n * 4) && take(a, doff, (n_seg + 1) * 8);
        }))) return rc;
    hipStream_t st = ctx->stream;
    PinStage pin(ctx);
    const void *h_start, *h_end, *h_off;
    void *h_labels;
    if ((rc = pin_reserve_for(ctx, pin, [&](PinStage &p) {
            p.slot(kPinScalars);                             // the windowed path below reads its sortedness flag back through the block's first bytes
            h_start = p.in(start, n * 4); h_end = p.in(end, n * 4); h_off = p.in(seg_off, (n_seg + 1) * 8); h_labels = p.out(labels, n * 4);
        }))) return rc;
    CSV_HIP(ctx, hipMemcpyAsync(ds, h_start, n * 4, hipMemcpyHostToDevice, st));
    CSV_HIP(ctx, hipMemcpyAsync(de, h_end, n * 4, hipMemcpyHostToDevice, st));
    CSV_HIP(ctx, hipMemcpyAsync(doff, h_off, (n_seg + 1) * 8, hipMemcpyHostToDevice, st));
    {
        TimerScope ts(ctx, CSV_K_DBSCAN);
        launch_dbscan_iv_small_batched(st, ds, de, doff, n_seg, eps, min_pts, dl, ctx->tuning.dbscan_all_pairs != 0);
    }
    if (max_len > DBSCAN_IV_SMALL_MAX) {                     // the few sets that do not fit a workgroup's LDS: windowed path, one at a time
        CSV_HIP(ctx, wait_stream(st));                       // (that path waits for its sortedness flag: nothing of it overtakes the batch)
        for (uint64_t s = 0; s < n_seg; s++) {
            const uint64_t len = seg_off[s + 1] - seg_off[s];
            if (len <= DBSCAN_IV_SMALL_MAX) continue;
            if ((rc = csvgpu_dbscan_iv_dev(ctx, ds + seg_off[s], de + seg_off[s], len, eps, min_pts, dl + seg_off[s]))) return rc;
        }
    }
    CSV_HIP(ctx, hipMemcpyAsync(h_labels, dl, n * 4, hipMemcpyDeviceToHost, st));
    CSV_HIP(ctx, wait_stream(st));
    pin.finish();
    return CSV_OK;
}

int csvgpu_dbscan_1d_dev(csv_ctx *ctx, const int32_t *d_pts, const uint64_t *d_seg_off, uint64_t n_seg, uint64_t n_pts,
                         uint32_t max_seg_len, double eps, int32_t min_pts, int32_t *d_labels)
{
    int rc = check_dbscan_args(ctx, eps, min_pts, false);
    if (rc) return rc;
    if (n_seg == 0) return CSV_OK;
    if (!d_seg_off || (n_pts && (!d_pts || !d_labels))) { ctx->err = "dbscan1d: null array"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    const bool has_big = max_seg_len > DBSCAN1D_MAX_SEG;
    Dbscan1dWs ws;
    if ((rc = arena_reserve_for(ctx, ctx->work, "dbscan1d", [&](Arena &a) { return carve_dbscan1d(a, max_seg_len, ws); }))) return rc;
    unsigned int *flag = ws.flag;
    CSV_HIP(ctx, hipMemsetAsync(flag, 0, 4, ctx->stream));
    {
        TimerScope ts(ctx, CSV_K_DBSCAN1D);
        launch_dbscan_1d_batched(ctx->stream, d_pts, d_seg_off, n_seg, eps, min_pts, d_labels, flag);
    }
    if (!has_big) return CSV_OK;
    // segments longer than the LDS kernel's limit: generic sorted-window path, one segment at a time
    std::vector<uint64_t> off(n_seg + 1);
    CSV_HIP(ctx, hipMemcpyAsync(off.data(), d_seg_off, (n_seg + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    CSV_HIP(ctx, wait_stream(ctx->stream));
    const SortWs &w = ws.w;
    uint32_t *ks = ws.ks;
    void *tmp = ws.tmp;
    for (uint64_t s = 0; s < n_seg; s++) {
        const uint64_t n = off[s + 1] - off[s];
        if (n <= DBSCAN1D_MAX_SEG) continue;
        if (n > max_seg_len) { ctx->err = "dbscan1d: max_seg_len smaller than a segment"; return CSV_EINVAL; }
        TimerScope ts(ctx, CSV_K_DBSCAN1D);
        launch_iota_keys_i32(ctx->stream, d_pts + off[s], n, w.k0, w.v0);
        const int io = launch_radix_sort_u64(ctx->stream, w.k0, w.v0, w.k1, w.v1, n, 32, w.tmp, onesweep(ctx));
        const uint32_t *perm = io ? w.v1 : w.v0;
        launch_gather_u32(ctx->stream, (const uint32_t *)(d_pts + off[s]), perm, n, ks);   // points in sorted order
        launch_dbscan_1d_big(ctx->stream, (const int32_t *)ks, perm, n, eps, min_pts, d_labels + off[s], tmp);
    }
    return CSV_OK;
}

int csvgpu_dbscan_1d(csv_ctx *ctx, const int32_t *pts, const uint64_t *seg_off, uint64_t n_seg, double eps, int32_t min_pts,
                     int32_t *labels)
{
    int rc = check_dbscan_args(ctx, eps, min_pts, false);
    if (rc) return rc;
    if (n_seg == 0) return CSV_OK;
    if (!seg_off) { ctx->err = "dbscan1d: null seg_off"; return CSV_EINVAL; }
    const uint64_t n = seg_off[n_seg];
    uint64_t max_len = 0;
    for (uint64_t s = 0; s < n_seg; s++) {
        if (seg_off[s + 1] < seg_off[s]) { ctx->err = "dbscan1d: seg_off not monotone"; return CSV_EINVAL; }
        max_len = std::max(max_len, seg_off[s + 1] - seg_off[s]);
    }
    if (n == 0) return CSV_OK;
    if (!pts || !labels) { ctx->err = "dbscan1d: null array"; return CSV_EINVAL; }
    if (max_len >= 0xffffffffull) { ctx->err = "dbscan1d: segment too large"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    int32_t *dp = nullptr, *dl = nullptr;
    uint64_t *doff = nullptr;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "dbscan1d arrays", [&](Arena &a) { return take(a, dp, n * 4) && take(a, dl, n * 4) && take(a, doff, (n_seg + 1) * 8); }))) return rc;
    PinStage pin(ctx);
    const void *h_pts, *h_off;
    void *h_labels;
    if ((rc = pin_reserve_for(ctx, pin, [&](PinStage &p) { h_pts = p.in(pts, n * 4); h_off = p.in(seg_off, (n_seg + 1) * 8); h_labels = p.out(labels, n * 4); }))) return rc;
    CSV_HIP(ctx, hipMemcpyAsync(dp, h_pts, n * 4, hipMemcpyHostToDevice, ctx->stream));
    CSV_HIP(ctx, hipMemcpyAsync(doff, h_off, (n_seg + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (max_len > DBSCAN1D_MAX_SEG) CSV_HIP(ctx, wait_stream(ctx->stream));          // (the large-segment path reads the offsets back: nothing of it overtakes the staging)
    if ((rc = csvgpu_dbscan_1d_dev(ctx, dp, doff, n_seg, n, (uint32_t)max_len, eps, min_pts, dl))) return rc;      // (leaves the page-locked block alone)
    CSV_HIP(ctx, hipMemcpyAsync(h_labels, dl, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    CSV_HIP(ctx, wait_stream(ctx->stream));
    pin.finish();
    return CSV_OK;
}

int csvgpu_window_log2_dev(csv_ctx *ctx, const uint32_t *d_depth, uint32_t depth_len, const uint32_t *d_rs, const uint32_t *d_re,
                           const int32_t *d_ss, const uint64_t *d_win_off, uint64_t n_regions, uint64_t n_windows,
                           double mean_cov, double *d_log2, uint32_t *d_ws, uint32_t *d_we)
{
    if (!ctx) return CSV_EINVAL;
    if (n_regions == 0 || n_windows == 0) return CSV_OK;
    if (!d_depth || !d_rs || !d_re || !d_ss || !d_win_off || !d_log2 || !d_ws || !d_we) { ctx->err = "window_log2: null array"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    TimerScope ts(ctx, CSV_K_WINDOW);
    launch_window_log2(ctx->stream, d_depth, depth_len, d_rs, d_re, d_ss, d_win_off, n_regions, n_windows, mean_cov, d_log2, d_ws, d_we);
    return CSV_OK;
}

int csvgpu_window_log2(csv_ctx *ctx, const uint32_t *depth, uint32_t depth_len, const uint32_t *region_start,
                       const uint32_t *region_end, const int32_t *sample_size, const uint64_t *win_off, uint64_t n_regions,
                       double mean_cov, double *log2_cov, uint32_t *win_start, uint32_t *win_end)
{
    if (!ctx) return CSV_EINVAL;
    if (n_regions == 0) return CSV_OK;
    if (!depth || !region_start || !region_end || !sample_size || !win_off) { ctx->err = "window_log2: null array"; return CSV_EINVAL; }
    for (uint64_t r = 0; r < n_regions; r++) {
        if (sample_size[r] <= 0 || win_off[r + 1] - win_off[r] != (uint64_t)sample_size[r] || region_start[r] > region_end[r]) {
            ctx->err = "window_log2: bad region table"; return CSV_EINVAL;
        }
    }
    const uint64_t nw = win_off[n_regions];
    if (nw == 0) return CSV_OK;
    if (!log2_cov || !win_start || !win_end) { ctx->err = "window_log2: null output"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    uint32_t *dd = nullptr;
    WindowWs w;
    int rc = arena_reserve_for(ctx, ctx->arena, "window_log2", [&](Arena &a) { return take(a, dd, (size_t)depth_len * 4) && carve_window(a, n_regions, nw, w); });
    if (rc) return rc;
    uint32_t *drs = w.rs, *dre = w.re, *dws = w.ws, *dwe = w.we;
    int32_t *dss = w.ss;
    uint64_t *dwo = w.wo;
    double *dl2 = w.l2;
    hipStream_t s = ctx->stream;
    CSV_HIP(ctx, hipMemcpyAsync(dd, depth, (size_t)depth_len * 4, hipMemcpyHostToDevice, s));
    CSV_HIP(ctx, hipMemcpyAsync(drs, region_start, n_regions * 4, hipMemcpyHostToDevice, s));
    CSV_HIP(ctx, hipMemcpyAsync(dre, region_end, n_regions * 4, hipMemcpyHostToDevice, s));
    CSV_HIP(ctx, hipMemcpyAsync(dss, sample_size, n_regions * 4, hipMemcpyHostToDevice, s));
    CSV_HIP(ctx, hipMemcpyAsync(dwo, win_off, (n_regions + 1) * 8, hipMemcpyHostToDevice, s));
    if ((rc = csvgpu_window_log2_dev(ctx, dd, depth_len, drs, dre, dss, dwo, n_regions, nw, mean_cov, dl2, dws, dwe))) return rc;
    CSV_HIP(ctx, hipMemcpyAsync(log2_cov, dl2, nw * 8, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, hipMemcpyAsync(win_start, dws, nw * 4, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, hipMemcpyAsync(win_end, dwe, nw * 4, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, wait_stream(s));
    return CSV_OK;
}

int csvgpu_viterbi_dev(csv_ctx *ctx, const csv_hmm *hmm, const double *d_o1, const double *d_o2, const double *d_pfb,
                       const uint64_t *d_seq_off, uint64_t n_seq, uint64_t n_obs, int32_t *d_states, double *d_loglik)
{
    if (!ctx) return CSV_EINVAL;
    if (!hmm) { ctx->err = "viterbi: null hmm"; return CSV_EINVAL; }
    if (n_seq == 0) return CSV_OK;
    if (!d_seq_off || !d_loglik || (n_obs && (!d_o1 || !d_o2 || !d_pfb || !d_states))) { ctx->err = "viterbi: null array"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    void *tmp = nullptr;
    int rc = arena_reserve_for(ctx, ctx->work, "viterbi", [&](Arena &a) { return take(a, tmp, viterbi_tmp_bytes(n_obs, n_seq)); });
    if (rc) return rc;
    TimerScope ts(ctx, CSV_K_VITERBI);
    launch_viterbi(ctx->stream, *hmm, d_o1, d_o2, d_pfb, d_seq_off, n_seq, n_obs, d_states, d_loglik, tmp);
    return CSV_OK;
}

int csvgpu_viterbi(csv_ctx *ctx, const csv_hmm *hmm, const double *o1, const double *o2, const double *pfb,
                   const uint64_t *seq_off, uint64_t n_seq, int32_t *states, double *loglik)
{
    if (!ctx) return CSV_EINVAL;
    if (!hmm) { ctx->err = "viterbi: null hmm"; return CSV_EINVAL; }
    if (n_seq == 0) return CSV_OK;
    if (!seq_off || !loglik) { ctx->err = "viterbi: null array"; return CSV_EINVAL; }
    for (uint64_t s = 0; s < n_seq; s++) if (seq_off[s + 1] < seq_off[s]) { ctx->err = "viterbi: seq_off not monotone"; return CSV_EINVAL; }
    const uint64_t n = seq_off[n_seq];
    if (n && (!o1 || !o2 || !pfb || !states)) { ctx->err = "viterbi: null array"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    double *d1 = nullptr, *d2 = nullptr, *dp = nullptr, *dll = nullptr;
    uint64_t *doff = nullptr;
    int32_t *dst = nullptr;
    int rc = arena_reserve_for(ctx, ctx->arena, "viterbi arrays", [&](Arena &a) {
        return take(a, d1, n * 8 + 8) && take(a, d2, n * 8 + 8) && take(a, dp, n * 8 + 8) && take(a, doff, (n_seq + 1) * 8) && take(a, dst, n * 4 + 8) && take(a, dll, n_seq * 8);
    });
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    PinStage pin(ctx);
    const void *h1, *h2, *hp, *h_off;
    void *h_states, *h_ll;
    if ((rc = pin_reserve_for(ctx, pin, [&](PinStage &p) {
            h1 = p.in(o1, n * 8); h2 = p.in(o2, n * 8); hp = p.in(pfb, n * 8); h_off = p.in(seq_off, (n_seq + 1) * 8);
            h_states = p.out(states, n * 4); h_ll = p.out(loglik, n_seq * 8);
        }))) return rc;
    if (n) {
        CSV_HIP(ctx, hipMemcpyAsync(d1, h1, n * 8, hipMemcpyHostToDevice, s));
        CSV_HIP(ctx, hipMemcpyAsync(d2, h2, n * 8, hipMemcpyHostToDevice, s));
        CSV_HIP(ctx, hipMemcpyAsync(dp, hp, n * 8, hipMemcpyHostToDevice, s));
    }
    CSV_HIP(ctx, hipMemcpyAsync(doff, h_off, (n_seq + 1) * 8, hipMemcpyHostToDevice, s));
    if ((rc = csvgpu_viterbi_dev(ctx, hmm, d1, d2, dp, doff, n_seq, n, dst, dll))) return rc;
    if (n) CSV_HIP(ctx, hipMemcpyAsync(h_states, dst, n * 4, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, hipMemcpyAsync(h_ll, dll, n_seq * 8, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, wait_stream(s));
    pin.finish();
    return CSV_OK;
}

// ---------------------------------------------------------------------------------------------
// resident shards + the per-chromosome pipeline

static void shard_release(csv_shard *sh)
{
    if (!sh) return;
    if (sh->owned) {
        (void)hipFree((void *)sh->d.pos); (void)hipFree((void *)sh->d.flag); (void)hipFree((void *)sh->d.mapq);
        (void)hipFree((void *)sh->d.cigar_off); (void)hipFree((void *)sh->d.cigar);
    }
    (void)hipFree(sh->ref_end); (void)hipFree(sh->q_start); (void)hipFree(sh->q_end);
    (void)hipFree(sh->ckpt);
    (void)hipFree(sh->depth_items);
    (void)hipFree(sh->scan_split);
    (void)hipFree(sh->qhash);
    (void)hipFree(sh->depth); (void)hipFree(sh->sig_raw); (void)hipFree(sh->scratch); (void)hipFree(sh->counters);
    delete sh;
}

static csv_shard *shard_common(csv_ctx *ctx, csv_shard *sh)
{
    const uint64_t n = sh->d.n_reads;
    bool ok = true;
    ok &= hipMalloc((void **)&sh->ref_end, n * 4 + 16) == hipSuccess;
    ok &= hipMalloc((void **)&sh->q_start, n * 4 + 16) == hipSuccess;
    ok &= hipMalloc((void **)&sh->q_end, n * 4 + 16) == hipSuccess;
    ok &= hipMalloc((void **)&sh->depth, (size_t)sh->depth_len * 4 + 16) == hipSuccess;
    sh->counters_bytes = align_up(kCntBytes, 256) + depth_tiles_tmp_bytes(sh->depth_len);
    ok &= hipMalloc((void **)&sh->counters, sh->counters_bytes) == hipSuccess;
    sh->tile_range = (uint64_t *)((char *)sh->counters + align_up(kCntBytes, 256));
    ok &= hipMalloc((void **)&sh->ckpt, ckpt_bytes(sh->d.n_cigar)) == hipSuccess;
    ok &= hipMalloc(&sh->depth_items, depth_items_bytes(sh->depth_len) + 16) == hipSuccess;
    sh->form = scan_form(ctx, sh->d.n_reads, sh->d.n_cigar);
    ok &= hipMalloc((void **)&sh->scan_split, scan_split_bytes(ctx->n_cu, sh->d.n_reads, sh->form) + 16) == hipSuccess;
    sh->sig_cap = std::max<uint64_t>(1u << 18, n * 2);
    ok &= hipMalloc((void **)&sh->sig_raw, sh->sig_cap * sizeof(csv_sig)) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); ctx->err = "hipMalloc failed (shard)"; shard_release(sh); return nullptr; }
    // the scan's work split for this device's grid, once per shard (the offsets are on the device by now)
    launch_scan_split(ctx->stream, ctx->n_cu, sh->d, sh->scan_split, sh->form);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) { ctx->err = "scan split failed (shard)"; shard_release(sh); return nullptr; }
    return sh;
}

csv_shard *csvgpu_shard_upload(csv_ctx *ctx, const csv_reads *r, uint32_t depth_len)
{
    if (check_reads(ctx, r)) return nullptr;
    (void)hipSetDevice(ctx->device);
    csv_shard *sh = new (std::nothrow) csv_shard();
    if (!sh) { ctx->err = "out of host memory"; return nullptr; }
    sh->owned = true; sh->depth_len = depth_len; sh->d = *r; sh->d.tid = nullptr;
    sh->d.pos = nullptr; sh->d.flag = nullptr; sh->d.mapq = nullptr; sh->d.cigar_off = nullptr; sh->d.cigar = nullptr;
    const uint64_t n = r->n_reads, m = r->n_cigar;
    bool ok = true;
    ok &= hipMalloc((void **)&sh->d.pos, n * 4 + 16) == hipSuccess;
    ok &= hipMalloc((void **)&sh->d.flag, n * 2 + 16) == hipSuccess;
    ok &= hipMalloc((void **)&sh->d.mapq, n + 16) == hipSuccess;
    ok &= hipMalloc((void **)&sh->d.cigar_off, (n + 1) * 8) == hipSuccess;
    ok &= hipMalloc((void **)&sh->d.cigar, (m + CIGAR_PAD_WORDS) * 4) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); ctx->err = "hipMalloc failed (shard upload)"; shard_release(sh); return nullptr; }
    sh->cigar_pad = CIGAR_PAD_WORDS;
    hipStream_t s = ctx->stream;
    sh->unsorted = 0;                                    // known before the first scan: lets the pipeline queue the depth pass without waiting
    for (uint64_t i = 1; i < n; i++) if (r->pos[i] < r->pos[i - 1]) { sh->unsorted = 1; break; }
    bool cp = true;
    if (n) {
        cp &= hipMemcpyAsync((void *)sh->d.pos, r->pos, n * 4, hipMemcpyHostToDevice, s) == hipSuccess;
        cp &= hipMemcpyAsync((void *)sh->d.flag, r->flag, n * 2, hipMemcpyHostToDevice, s) == hipSuccess;
        cp &= hipMemcpyAsync((void *)sh->d.mapq, r->mapq, n, hipMemcpyHostToDevice, s) == hipSuccess;
    }
    cp &= hipMemcpyAsync((void *)sh->d.cigar_off, r->cigar_off, (n + 1) * 8, hipMemcpyHostToDevice, s) == hipSuccess;
    if (m) cp &= hipMemcpyAsync((void *)sh->d.cigar, r->cigar, m * 4, hipMemcpyHostToDevice, s) == hipSuccess;
    cp &= hipMemsetAsync((void *)(sh->d.cigar + m), 0, (size_t)CIGAR_PAD_WORDS * 4, s) == hipSuccess;
    cp &= hipStreamSynchronize(s) == hipSuccess;
    if (!cp) { ctx->err = "H2D copy failed (shard upload)"; shard_release(sh); return nullptr; }
    return shard_common(ctx, sh);
}

csv_shard *csvgpu_shard_wrap_dev(csv_ctx *ctx, const csv_reads *r, uint32_t depth_len)
{
    if (!ctx) return nullptr;
    (void)hipSetDevice(ctx->device);
    if (check_reads_dev(ctx, r)) return nullptr;
    csv_shard *sh = new (std::nothrow) csv_shard();
    if (!sh) { ctx->err = "out of host memory"; return nullptr; }
    sh->owned = false; sh->depth_len = depth_len; sh->d = *r;
    return shard_common(ctx, sh);
}

void csvgpu_shard_free(csv_ctx *ctx, csv_shard *sh)
{
    if (!ctx || !sh) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    shard_release(sh);
}

int csvgpu_aln_intervals_resident(csv_ctx *ctx, csv_shard *sh, int32_t *ref_end, int32_t *q_start, int32_t *q_end)
{
    if (!ctx || !sh) return CSV_EINVAL;
    const uint64_t n = sh->d.n_reads;
    if (n == 0) return CSV_OK;
    if (!ref_end || !q_start || !q_end) { ctx->err = "aln_intervals: null output"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    CSV_HIP(ctx, hipMemcpyAsync(ref_end, sh->ref_end, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    CSV_HIP(ctx, hipMemcpyAsync(q_start, sh->q_start, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    CSV_HIP(ctx, hipMemcpyAsync(q_end, sh->q_end, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    CSV_HIP(ctx, wait_stream(ctx->stream));
    return CSV_OK;
}

int csvgpu_window_log2_resident_many(csv_ctx *ctx, int n_shards, csv_shard *const *shards, const uint32_t *const *region_start,
                                     const uint32_t *const *region_end, const int32_t *const *sample_size, const uint64_t *const *win_off,
                                     const uint64_t *n_regions, const double *mean_cov, double *const *log2_cov, uint32_t *const *win_start,
                                     uint32_t *const *win_end)
{
    if (!ctx || n_shards < 0) return CSV_EINVAL;
    if (n_shards == 0) return CSV_OK;
    if (!shards || !region_start || !region_end || !sample_size || !win_off || !n_regions || !mean_cov || !log2_cov || !win_start || !win_end) {
        ctx->err = "window_log2_many: null table"; return CSV_EINVAL;
    }
    uint64_t R = 0, W = 0;
    for (int c = 0; c < n_shards; c++) {
        const uint64_t nr = n_regions[c];
        if (!nr) continue;
        if (!shards[c] || !region_start[c] || !region_end[c] || !sample_size[c] || !win_off[c]) { ctx->err = "window_log2_many: null array"; return CSV_EINVAL; }
        for (uint64_t r = 0; r < nr; r++)
            if (sample_size[c][r] <= 0 || win_off[c][r + 1] - win_off[c][r] != (uint64_t)sample_size[c][r] || region_start[c][r] > region_end[c][r] || win_off[c][0] != 0) {
                ctx->err = "window_log2_many: bad region table"; return CSV_EINVAL;
            }
        if (win_off[c][nr] && (!log2_cov[c] || !win_start[c] || !win_end[c])) { ctx->err = "window_log2_many: null output"; return CSV_EINVAL; }
        R += nr; W += win_off[c][nr];
    }
    if (W == 0) return CSV_OK;
    (void)hipSetDevice(ctx->device);
    // one page-locked block carries every shard's tables to the device and every shard's windows back
    const size_t in_bytes = align_up(R * 4, 8) * 3 + (R + (size_t)n_shards) * 8, out_bytes = W * 8 + 2 * align_up(W * 4, 8);
    char *h_in = nullptr, *h_out = nullptr, *d_in = nullptr, *d_out = nullptr;
    PinStage pin(ctx);
    int rc = pin_reserve_for(ctx, pin, [&](PinStage &p) { h_in = (char *)p.slot(in_bytes); h_out = (char *)p.slot(out_bytes); });
    if (rc) return rc;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "window_log2_many", [&](Arena &a) { return take(a, d_in, in_bytes) && take(a, d_out, out_bytes); }))) return rc;
    const size_t o_rs = 0, o_re = align_up(R * 4, 8), o_ss = 2 * align_up(R * 4, 8), o_wo = 3 * align_up(R * 4, 8);
    const size_t o_l2 = 0, o_ws = W * 8, o_we = W * 8 + align_up(W * 4, 8);
    uint64_t r0 = 0, w0 = 0;
    for (int c = 0; c < n_shards; c++) {
        const uint64_t nr = n_regions[c];
        if (!nr) continue;
        memcpy(h_in + o_rs + r0 * 4, region_start[c], nr * 4);
        memcpy(h_in + o_re + r0 * 4, region_end[c], nr * 4);
        memcpy(h_in + o_ss + r0 * 4, sample_size[c], nr * 4);
        memcpy(h_in + o_wo + (r0 + (uint64_t)c) * 8, win_off[c], (nr + 1) * 8);
        r0 += nr;
    }
    hipStream_t s = ctx->stream;
    CSV_HIP(ctx, hipMemcpyAsync(d_in, h_in, in_bytes, hipMemcpyHostToDevice, s));
    {
        TimerScope ts(ctx, CSV_K_WINDOW);
        r0 = 0;
        for (int c = 0; c < n_shards; c++) {
            const uint64_t nr = n_regions[c];
            if (!nr) continue;
            const uint64_t nw = win_off[c][nr];
            launch_window_log2(s, shards[c]->depth, shards[c]->depth_len, (const uint32_t *)(d_in + o_rs) + r0, (const uint32_t *)(d_in + o_re) + r0,
                               (const int32_t *)(d_in + o_ss) + r0, (const uint64_t *)(d_in + o_wo) + r0 + c, nr, nw, mean_cov[c],
                               (double *)(d_out + o_l2) + w0, (uint32_t *)(d_out + o_ws) + w0, (uint32_t *)(d_out + o_we) + w0);
            r0 += nr; w0 += nw;
        }
    }
    CSV_HIP(ctx, hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, wait_stream(s));
    w0 = 0;
    for (int c = 0; c < n_shards; c++) {
        const uint64_t nr = n_regions[c];
        if (!nr) continue;
        const uint64_t nw = win_off[c][nr];
        memcpy(log2_cov[c], h_out + o_l2 + w0 * 8, nw * 8);
        memcpy(win_start[c], h_out + o_ws + w0 * 4, nw * 4);
        memcpy(win_end[c], h_out + o_we + w0 * 4, nw * 4);
        w0 += nw;
    }
    return CSV_OK;
}

int csvgpu_aln_intervals_gather_batch(csv_ctx *ctx, int n_shards, csv_shard *const *shards, const uint32_t *rec, const uint64_t *rec_off,
                                      int32_t *ref_end, int32_t *q_start, int32_t *q_end)
{
    if (!ctx || n_shards < 0) return CSV_EINVAL;
    if (n_shards == 0) return CSV_OK;
    if (!shards || !rec_off) { ctx->err = "aln_intervals_gather: null array"; return CSV_EINVAL; }
    const uint64_t n = rec_off[n_shards];
    if (n == 0) return CSV_OK;
    if (!rec || !ref_end || !q_start || !q_end) { ctx->err = "aln_intervals_gather: null array"; return CSV_EINVAL; }
    for (int c = 0; c < n_shards; c++) {
        if (!shards[c] || rec_off[c + 1] < rec_off[c]) { ctx->err = "aln_intervals_gather: bad shard table"; return CSV_EINVAL; }
        for (uint64_t i = rec_off[c]; i < rec_off[c + 1]; i++) if (rec[i] >= shards[c]->d.n_reads) { ctx->err = "aln_intervals_gather: record index beyond the shard"; return CSV_EINVAL; }
    }
    (void)hipSetDevice(ctx->device);
    uint32_t *didx = nullptr, *dout = nullptr;
    int rc = arena_reserve_for(ctx, ctx->arena, "aln_intervals_gather", [&](Arena &a) { return take(a, didx, n * 4) && take(a, dout, 3 * n * 4); });
    if (rc) return rc;
    const uint32_t *h_idx = nullptr;
    uint32_t *h_out = nullptr;                                          // the index list goes out and the three arrays come back through one page-locked block
    PinStage pin(ctx);
    if ((rc = pin_reserve_for(ctx, pin, [&](PinStage &p) { h_idx = (const uint32_t *)p.in(rec, n * 4); h_out = (uint32_t *)p.slot(3 * n * 4); }))) return rc;
    hipStream_t s = ctx->stream;
    CSV_HIP(ctx, hipMemcpyAsync(didx, h_idx, n * 4, hipMemcpyHostToDevice, s));
    for (int c = 0; c < n_shards; c++) {
        const uint64_t o = rec_off[c], m = rec_off[c + 1] - o;
        if (!m) continue;
        const csv_shard *sh = shards[c];
        launch_gather3_u32(s, (const uint32_t *)sh->ref_end, (const uint32_t *)sh->q_start, (const uint32_t *)sh->q_end, didx + o, m, dout + o, dout + n + o, dout + 2 * n + o);
    }
    CSV_HIP(ctx, hipMemcpyAsync(h_out, dout, 3 * n * 4, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, wait_stream(s));
    memcpy(ref_end, h_out, n * 4); memcpy(q_start, h_out + n, n * 4); memcpy(q_end, h_out + 2 * n, n * 4);
    return CSV_OK;
}

int csvgpu_aln_intervals_gather_resident(csv_ctx *ctx, csv_shard *sh, const uint32_t *rec, uint64_t n, int32_t *ref_end, int32_t *q_start, int32_t *q_end)
{
    const uint64_t off[2] = {0, n};
    return csvgpu_aln_intervals_gather_batch(ctx, 1, &sh, rec, off, ref_end, q_start, q_end);
}

int csvgpu_shard_set_qname_hash(csv_ctx *ctx, csv_shard *sh, const uint64_t *qname_hash)
{
    if (!ctx || !sh) return CSV_EINVAL;
    const uint64_t n = sh->d.n_reads;
    if (n && !qname_hash) { ctx->err = "set_qname_hash: null array"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    if (!sh->qhash) {
        if (hipMalloc((void **)&sh->qhash, n * 8 + 16) != hipSuccess) { (void)hipGetLastError(); sh->qhash = nullptr; ctx->err = "hipMalloc failed (qname hashes)"; return CSV_ENOMEM; }
    }
    if (n) CSV_HIP(ctx, hipMemcpyAsync(sh->qhash, qname_hash, n * 8, hipMemcpyHostToDevice, ctx->stream));
    CSV_HIP(ctx, wait_stream(ctx->stream));
    return CSV_OK;
}

// the epochs of a libstdc++ hash table that grows by single insertions: node index at which each rehash happens, and the bucket
// count from there on — asked of the library's own policy object (what std::unordered_map itself consults)
static void split_order_epochs(uint64_t n_max, std::vector<uint64_t> &first_node, std::vector<uint64_t> &buckets)
{
    static std::mutex mu;
    static std::vector<uint64_t> c_first, c_bkt;
    static uint64_t covered = 0;                              // the plan is known for tables of up to `covered` nodes
    std::lock_guard<std::mutex> l(mu);
    if (n_max > covered) {
        c_first.clear(); c_bkt.clear();
        std::__detail::_Prime_rehash_policy pol;
        std::size_t nb = 1;
        const uint64_t want = std::max<uint64_t>(n_max, 1u << 20);
        for (uint64_t i = 0; i < want;) {
            const std::pair<bool, std::size_t> g = pol._M_need_rehash(nb, i, 1);
            if (g.first) { nb = g.second; c_first.push_back(i); c_bkt.push_back(nb); }
            // nothing can happen before the table is full again (max_load_factor 1): jump there
            i = (g.first || i + 1 >= nb) ? i + 1 : std::min<uint64_t>(want, (uint64_t)nb);
        }
        covered = want;
    }
    first_node = c_first; buckets = c_bkt;
}

}  // extern "C"

// What csvgpu_split_order_begin leaves for csvgpu_split_order_finish (one pending order per context; device pointers into ctx->arena / ctx->work).
struct csv_split_state : SplitNodesWs, SplitEpochsWs {
    int n_contigs = 0;
    SplitOrderTab tab;
    std::vector<uint64_t> N;
    uint64_t n_nodes = 0, n_max = 0, total_reads = 0;
    int D = 0;
    SplitTailHost th;
    size_t bm_words = 0;
    bool finished = false;
    bool self = false;                 // the supplementary hashes are taken from the same shards: the whole order was queued by _begin
    uint64_t self_bound = 0;           // survivors the page-locked block has room for (self)
    std::vector<csv_split_survivor> surv;
    std::vector<uint64_t> off;
};

static void split_state_free(csv_ctx *ctx) { if (ctx) { delete ctx->split_state; ctx->split_state = nullptr; } }

// nodes + every epoch that does not depend on the supplementary records: queued, not waited for (beyond the node counts)
static int split_order_tail(csv_ctx *ctx, csv_split_state *st, const uint64_t *d_supp, uint64_t n_supp, bool devn);

static int split_order_begin(csv_ctx *ctx, int n_contigs, csv_shard *const *shards, uint8_t min_mapq, int64_t n_supp_hint /* < 0: unknown */, bool self = false)
{
    if (!ctx) return CSV_EINVAL;
    delete ctx->split_state; ctx->split_state = nullptr;
    if (n_contigs < 0 || (uint32_t)n_contigs > SO_MAX_CONTIGS) { ctx->err = "split_order: at most 32 contigs per call"; return CSV_EINVAL; }
    if (n_contigs && !shards) { ctx->err = "split_order: null array"; return CSV_EINVAL; }
    std::unique_ptr<csv_split_state> st(new csv_split_state());
    st->n_contigs = n_contigs;
    st->off.assign((size_t)n_contigs + 1, 0);
    if (n_contigs == 0) { st->finished = true; ctx->split_state = st.release(); return CSV_OK; }
    (void)hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    SplitOrderTab &tab = st->tab;
    tab.A = (uint32_t)n_contigs;
    uint64_t total_reads = 0, n_blocks = 0;
    for (int c = 0; c < n_contigs; c++) {
        const csv_shard *sh = shards[c];
        if (!sh || (sh->d.n_reads && !sh->qhash)) { ctx->err = "split_order: a shard without query-name hashes (csvgpu_shard_set_qname_hash)"; return CSV_EINVAL; }
        tab.blk_off[c] = n_blocks;
        tab.n_reads[c] = sh->d.n_reads; tab.flag[c] = sh->d.flag; tab.mapq[c] = sh->d.mapq; tab.qhash[c] = sh->qhash;
        n_blocks += (sh->d.n_reads + 1023) / 1024;
        total_reads += sh->d.n_reads;
    }
    tab.blk_off[n_contigs] = n_blocks;
    st->total_reads = total_reads;
    if (total_reads == 0 || n_supp_hint == 0) { st->finished = true; ctx->split_state = st.release(); return CSV_OK; }
    if (total_reads >= 0xfffffff0ull) { ctx->err = "split_order: too many records in one call"; return CSV_EINVAL; }
    TimerScope ts(ctx, CSV_K_SPLIT_ORDER);

    // ---- nodes: the filter-passing primaries of every contig, file order ----
    // (the supplementary hashes arrive with _finish: at most one per record)
    int rc = arena_reserve_for(ctx, ctx->arena, "split order", [&](Arena &a) { return carve_split_nodes(a, n_blocks, total_reads, *st); });
    if (rc) return rc;
    unsigned int *d_nsupp = st->d_nsupp;
    uint32_t *blk = st->blk, *node_rec = st->node_rec, *list = st->list;
    void *es_tmp = st->es_tmp;
    uint64_t *node_hash = st->node_hash;
    CSV_HIP(ctx, hipMemsetAsync(blk + n_blocks, 0, 4, s));
    launch_so_count(s, tab, (uint32_t)n_blocks, min_mapq, blk);
    launch_exclusive_sum_u32(s, blk, n_blocks + 1, es_tmp);
    launch_so_scatter(s, tab, (uint32_t)n_blocks, min_mapq, blk, node_hash, node_rec);
    if ((rc = ensure_pinned(ctx, (n_blocks + 1) * 4 + 64 + 256))) return rc;
    CSV_HIP(ctx, hipMemcpyAsync(ctx->pinned, blk, (n_blocks + 1) * 4, hipMemcpyDeviceToHost, s));
    const size_t nsupp_at = align_up((n_blocks + 1) * 4, 64);
    if (self) {                                  // the supplementary records' hashes of the same shards (their count comes back with the node counts)
        CSV_HIP(ctx, hipMemsetAsync(d_nsupp, 0, 4, s));
        launch_so_supp(s, tab, (uint32_t)n_blocks, min_mapq, st->d_supp, d_nsupp);
        CSV_HIP(ctx, hipMemcpyAsync((char *)ctx->pinned + nsupp_at, d_nsupp, 4, hipMemcpyDeviceToHost, s));
    }
    CSV_HIP(ctx, wait_stream(s));
    const uint32_t *h_blk = (const uint32_t *)ctx->pinned;
    uint64_t n_supp_self = 0;
    if (self) {
        n_supp_self = *(const uint32_t *)((const char *)ctx->pinned + nsupp_at);
        n_supp_hint = (int64_t)n_supp_self;
        st->self = true;
        if (n_supp_self == 0) { st->finished = true; ctx->split_state = st.release(); return CSV_OK; }          // nothing survives
    }
    std::vector<uint64_t> &N = st->N;
    N.assign((size_t)n_contigs, 0);
    uint64_t n_nodes = h_blk[n_blocks], n_max = 0;
    for (int c = 0; c < n_contigs; c++) {
        tab.nbase[c] = h_blk[tab.blk_off[c]];
        N[(size_t)c] = (uint64_t)h_blk[tab.blk_off[c + 1]] - h_blk[tab.blk_off[c]];
        n_max = std::max(n_max, N[(size_t)c]);
    }
    tab.nbase[n_contigs] = (uint32_t)n_nodes;
    st->n_nodes = n_nodes; st->n_max = n_max;
    if (n_nodes == 0) { st->finished = true; ctx->split_state = st.release(); return CSV_OK; }

    // ---- the chain of epochs: a contig takes part in epoch k while it still has nodes inserted at or after the epoch's first node ----
    std::vector<uint64_t> first_node, buckets;
    split_order_epochs(n_max, first_node, buckets);
    // The last D epochs of every contig are ordered for the survivors (and the nodes their order depends on) only: splitorder.hip.
    // The sets double per level and the epochs halve, so D levels pay while 4^D <= nodes per supplementary record (about a hundred
    // in a long-read run: D = 3, also taken when the caller has not counted its supplementary records yet).
    int D = 0;
    {
        const uint64_t ratio = n_supp_hint > 0 ? n_nodes / (uint64_t)n_supp_hint : (n_nodes >= 4096 ? 64 : 1);
        while (D < (int)SO_TAIL_MAX && (ratio >> (2 * (D + 1))) >= 1) D++;
        if (ctx->tuning.split_tail != CSV_TAIL_AUTO) D = ctx->tuning.split_tail;
    }
    SplitTailHost &th = st->th;
    th.A = (uint32_t)n_contigs; th.wv = std::max(1, bits_of(n_nodes)); th.wa = std::max(1, bits_of((uint64_t)n_contigs - 1));
    if (n_nodes >= (1ull << 31) || th.wa + 2 * (th.wv + 1) > 64 || (self && n_nodes >= (1ull << 30))) D = 0;      // (self: the queued sorts count in 30 bits)
    th.D = (uint32_t)D;
    std::vector<int> K((size_t)n_contigs, -1);                       // a contig's last epoch
    for (int c = 0; c < n_contigs; c++) {
        for (size_t k = 0; k < first_node.size() && N[(size_t)c] > first_node[k]; k++) K[(size_t)c] = (int)k;
        th.nbase[c] = tab.nbase[c];
    }
    th.nbase[n_contigs] = (uint32_t)n_nodes;
    uint64_t tail_buckets = 0;
    for (int j = 0; j < D; j++) {
        uint64_t off = 0;
        for (int c = 0; c < n_contigs; c++) {
            const int e = K[(size_t)c] - j;
            th.B[j][c] = e >= 0 ? (uint32_t)buckets[(size_t)e] : 1u;
            th.F[j][c] = e >= 0 ? (uint32_t)first_node[(size_t)e] : 0u;
            th.boff[j][c] = (uint32_t)off;
            off += th.B[j][c];
        }
        if (off >= 0xffffffe0ull) { D = 0; th.D = 0; break; }
        for (int c = n_contigs; c <= (int)SO_MAX_CONTIGS; c++) th.boff[j][c] = (uint32_t)off;
        tail_buckets = std::max(tail_buckets, off);
    }
    st->D = D;
    auto in_chain = [&](int c, size_t k) { return N[(size_t)c] > first_node[k] && (int)k <= K[(size_t)c] - D; };
    uint64_t scratch = tail_buckets * 4;
    for (size_t k = 0; k < first_node.size(); k++) {
        uint64_t A = 0;
        for (int c = 0; c < n_contigs; c++) A += in_chain(c, k);
        scratch = std::max(scratch, A * buckets[k] * 4);
    }
    const size_t bm_words = st->bm_words = (size_t)((tail_buckets + 31) / 32 + 8);
    const uint64_t n_sort = std::max(n_nodes, n_supp_self);
    if ((rc = arena_reserve_for(ctx, ctx->work, "split order epochs", [&](Arena &a) { return carve_split_epochs(a, scratch, n_sort, n_nodes, D, bm_words, *st); }))) return rc;
    uint32_t *minT = st->minT;
    SortWs &w = st->w;
    CSV_HIP(ctx, hipMemsetAsync(st->d_count, 0, 256, s));

    // the first epochs (nodes and buckets in LDS) in one launch, one workgroup per contig
    size_t n_small = 0;
    {
        SplitSmallHost sm;
        while (n_small < first_node.size() && n_small < SO_SMALL_EPOCHS && buckets[n_small] <= SO_SMALL_B) n_small++;
        if (ctx->tuning.split_chain_only) n_small = 0;                          // (A/B and tests: every epoch through the chain's sorts)
        sm.A = (uint32_t)n_contigs; sm.n_epochs = (uint32_t)n_small;
        bool any = false;
        for (int c = 0; c <= n_contigs; c++) sm.nbase[c] = th.nbase[c];
        for (int c = 0; c < n_contigs; c++) {
            int kl = -1;
            for (size_t k = 0; k < n_small && in_chain(c, k); k++) kl = (int)k;
            sm.k_last[c] = kl; any |= kl >= 0;
        }
        for (size_t k = 0; k <= n_small && k < first_node.size(); k++) sm.first[k] = (uint32_t)std::min<uint64_t>(first_node[k], 0xffffffffu);
        if (n_small >= first_node.size()) sm.first[n_small] = 0xffffffffu;
        for (size_t k = 0; k < n_small; k++) sm.B[k] = (uint32_t)buckets[k];
        if (n_small && any) launch_so_small_epochs(s, sm, node_hash, list);
    }
    for (size_t k = n_small; k < first_node.size(); k++) {
        SplitOrderTab e;
        e.A = 0;
        uint64_t M = 0, m_max = 0;
        const uint64_t next_first = k + 1 < first_node.size() ? first_node[k + 1] : ~0ull;
        for (int c = 0; c < n_contigs; c++) {
            if (!in_chain(c, k)) continue;
            const uint64_t m = std::min(N[(size_t)c], next_first);                 // nodes present at the end of this epoch
            e.work_off[e.A] = M; e.nbase[e.A] = tab.nbase[c]; e.m_old[e.A] = (uint32_t)first_node[k];
            e.A++; M += m; m_max = std::max(m_max, m);
        }
        if (e.A == 0) break;
        e.work_off[e.A] = M;
        if (m_max <= 1) continue;                                                   // a single node: nothing to order
        const uint32_t B = (uint32_t)buckets[k];
        const int wbits = std::max(1, bits_of(m_max - 1));
        for (uint32_t a = 0; a < e.A; a++) e.rev_off[a] = M - e.work_off[a + 1];
        const int key_bits = std::max(1, bits_of(M - 1));
        CSV_HIP(ctx, hipMemsetAsync(minT, 0xff, (size_t)e.A * B * 4, s));
        launch_so_mint(s, e, M, B, node_hash, list, minT);
        launch_so_keys(s, e, M, B, wbits, node_hash, list, minT, w.k0, w.v0);
        const int io = launch_radix_sort_u64(s, w.k0, w.v0, w.k1, w.v1, M, key_bits, w.tmp, onesweep(ctx));
        launch_so_setlist(s, e, M, io ? w.v1 : w.v0, list);
    }
    if (D > 0) launch_st_inverse(s, th, (uint32_t)n_nodes, D - 1, list, st->prevrank);
    if (self) {
        // everything else too: the hashes sorted (64-bit keys, the values are not used), the survivors-only levels with the set sizes read on
        // the device, the survivors copied to the page-locked block — _finish only waits
        const int io = launch_radix_sort_u64(s, st->d_supp, w.v0, w.k1, w.v1, n_supp_self, 64, w.tmp, onesweep(ctx));
        if (io != 0) { ctx->err = "split_order: unexpected sort parity"; return CSV_EHIP; }
        if ((rc = split_order_tail(ctx, st.get(), st->d_supp, n_supp_self, true))) return rc;
        st->self_bound = std::min<uint64_t>(n_supp_self, n_nodes);
        if ((rc = ensure_pinned(ctx, 64 + st->self_bound * sizeof(csv_split_survivor) + 64))) return rc;
        CSV_HIP(ctx, hipMemcpyAsync(ctx->pinned, st->d_count, 8, hipMemcpyDeviceToHost, s));
        CSV_HIP(ctx, hipMemcpyAsync((char *)ctx->pinned + 64, st->d_out, st->self_bound * sizeof(csv_split_survivor), hipMemcpyDeviceToHost, s));
    }
    if (hipGetLastError() != hipSuccess) { ctx->err = "split_order: launch failed"; return CSV_EHIP; }
    ctx->split_state = st.release();
    return CSV_OK;
}

// the survivors in their final order: the last D epochs for them and the nodes their order depends on (or, D = 0, the chain's final
// positions). devn: the set sizes stay on the device (everything is queued, nothing waited for).
static int split_order_tail(csv_ctx *ctx, csv_split_state *st, const uint64_t *d_supp, uint64_t n_supp, bool devn)
{
    hipStream_t s = ctx->stream;
    const int D = st->D;
    const int n_contigs = st->n_contigs;
    SplitTailHost &th = st->th;
    SortWs &w = st->w;
    const uint64_t n_nodes = st->n_nodes, cap = n_nodes;
    if (D == 0) {
        // ---- survivors: nodes whose name hash is a supplementary record's; their final position orders them ----
        launch_so_survivors(s, st->tab, n_nodes, st->node_hash, st->node_rec, st->list, d_supp, n_supp, st->d_out, cap, st->d_count);
        return CSV_OK;
    }
    // ---- top-down: who takes part in the last D epochs (hashes only) ----
    unsigned int *d_setn = (unsigned int *)((char *)st->d_count + 64);
    uint32_t set_n[SO_TAIL_MAX + 1] = {0, 0, 0, 0};
    for (int j = 0; j < D; j++) CSV_HIP(ctx, hipMemsetAsync(st->bitmap[j], 0, st->bm_words * 4, s));
    CSV_HIP(ctx, hipMemsetAsync(st->filter, 0, st_filter_bytes(), s));
    launch_st_survivors(s, th, (uint32_t)n_nodes, st->node_hash, d_supp, n_supp, st->filter, st->is_surv, st->bitmap[0]);
    for (int j = 1; j <= D; j++)
        launch_st_member(s, th, (uint32_t)n_nodes, j, st->node_hash, st->bitmap[j - 1], j < D ? st->bitmap[j] : nullptr, st->set[j], d_setn + j);
    if (!devn) {
        CSV_HIP(ctx, hipMemcpyAsync(ctx->pinned, d_setn, 16, hipMemcpyDeviceToHost, s));
        CSV_HIP(ctx, wait_stream(s));
        for (int j = 1; j <= D; j++) set_n[j] = ((const uint32_t *)ctx->pinned)[j];
        // a t value is a list position or an insertion index (below the largest contig's node count) or a rank in a level's order (below the set's size)
        uint64_t t_max = st->n_max;
        for (int j = 1; j <= D; j++) t_max = std::max<uint64_t>(t_max, set_n[j]);
        th.wv = std::max(1, bits_of(t_max));
    } else {
        for (int j = 1; j <= D; j++) set_n[j] = (uint32_t)n_nodes;           // (bounds: the kernels read the sizes)
        th.wv = std::max(1, bits_of(n_nodes));
    }
    // ---- bottom-up: order S_D with the chain's positions, then each smaller set with the ranks of the order before ----
    const int key_bits = th.wa + 2 * (th.wv + 1);
    for (int j = D - 1; j >= 0; j--) {
        const uint32_t n = set_n[j + 1];
        const uint32_t *n_dev = devn ? d_setn + (j + 1) : nullptr;
        if (n == 0) continue;
        CSV_HIP(ctx, hipMemsetAsync(st->minT, 0xff, (size_t)th.boff[j][n_contigs] * 4, s));
        launch_st_mint(s, th, j, st->set[j + 1], n, n_dev, st->node_hash, st->prevrank, st->minT);
        launch_st_keys(s, th, j, st->set[j + 1], n, n_dev, st->node_hash, st->prevrank, st->minT, w.k0, w.v0);
        const int io = devn ? launch_radix_sort_u64_devn(s, w.k0, w.v0, w.k1, w.v1, n, n_dev, key_bits, w.tmp)
                            : launch_radix_sort_u64(s, w.k0, w.v0, w.k1, w.v1, n, key_bits, w.tmp, onesweep(ctx));
        if (io < 0) { ctx->err = "split_order: set too large for the queued sort"; return CSV_EINVAL; }
        const uint32_t *sorted = (devn || n > 1) ? (io ? w.v1 : w.v0) : w.v0;
        if (j > 0) launch_st_rank(s, sorted, n, n_dev, st->prevrank);
        else launch_st_emit(s, th, sorted, n, n_dev, st->is_surv, st->node_rec, st->d_out, cap, st->d_count);
    }
    return CSV_OK;
}

static int split_order_finish(csv_ctx *ctx, const uint64_t *supp_hash, uint64_t n_supp, uint32_t *out_rec, uint64_t capacity, uint64_t *out_off)
{
    if (!ctx) return CSV_EINVAL;
    csv_split_state *st = ctx->split_state;
    if (!st) { ctx->err = "split_order_finish without split_order_begin"; return CSV_EINVAL; }
    const int n_contigs = st->n_contigs;
    if (!out_off || (!st->self && n_supp && !supp_hash) || (capacity && !out_rec)) { ctx->err = "split_order: null array"; return CSV_EINVAL; }
    if (!st->self)
        for (uint64_t i = 1; i < n_supp; i++) if (supp_hash[i] <= supp_hash[i - 1]) { ctx->err = "split_order: supp_hash must be sorted and distinct"; return CSV_EINVAL; }
    for (int c = 0; c <= n_contigs; c++) out_off[c] = 0;
    (void)hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    if (!st->finished && !st->self) {
        if (n_supp == 0) {               // nothing survives
            CSV_HIP(ctx, wait_stream(s));
            st->finished = true;
        }
    }
    if (!st->finished) {
        TimerScope ts(ctx, CSV_K_SPLIT_ORDER);
        std::vector<csv_split_survivor> &surv = st->surv;
        int prc;
        if (st->self) {
            // everything was queued by _begin: the count and the survivors are in (or on their way to) the page-locked block
            CSV_HIP(ctx, wait_stream(s));
            const uint64_t n_surv = *(const unsigned long long *)ctx->pinned;
            if (n_surv > st->self_bound) { ctx->err = "split_order: more survivors than supplementary records"; return CSV_EHIP; }
            surv.resize(n_surv);
            if (n_surv) memcpy(surv.data(), (const char *)ctx->pinned + 64, n_surv * sizeof(csv_split_survivor));
        } else {
            const uint64_t n_nodes = st->n_nodes;
            // (room for one hash per record of these contigs was set aside by _begin; a run's other contigs can add more)
            struct TmpBuf { void *p = nullptr; ~TmpBuf() { if (p) (void)hipFree(p); } } big_supp;
            uint64_t *d_supp = st->d_supp;
            if (n_supp > st->total_reads) {
                if (hipMalloc(&big_supp.p, n_supp * 8) != hipSuccess) { (void)hipGetLastError(); big_supp.p = nullptr; ctx->err = "hipMalloc failed (supplementary hashes)"; return CSV_ENOMEM; }
                d_supp = (uint64_t *)big_supp.p;
            }
            // (through the context's page-locked block: a pageable copy is staged by the runtime under a lock the lanes' launches also take)
            prc = ensure_pinned(ctx, std::max<size_t>(n_supp * 8, 4096) + 64);
            if (prc) return prc;
            memcpy(ctx->pinned, supp_hash, n_supp * 8);
            CSV_HIP(ctx, hipMemcpyAsync(d_supp, ctx->pinned, n_supp * 8, hipMemcpyHostToDevice, s));
            CSV_HIP(ctx, wait_stream(s));                    // (the block is reused for the set sizes below)
            if ((prc = split_order_tail(ctx, st, d_supp, n_supp, false))) return prc;
            CSV_HIP(ctx, hipMemcpyAsync(ctx->pinned, st->d_count, 8, hipMemcpyDeviceToHost, s));
            CSV_HIP(ctx, wait_stream(s));
            const uint64_t n_surv = *(const unsigned long long *)ctx->pinned;
            if (n_surv > n_nodes) { ctx->err = "split_order: survivor count out of range"; return CSV_EHIP; }
            surv.resize(n_surv);
            if (n_surv) {
                if ((prc = ensure_pinned(ctx, n_surv * sizeof(csv_split_survivor) + 64))) return prc;
                CSV_HIP(ctx, hipMemcpyAsync(ctx->pinned, st->d_out, n_surv * sizeof(csv_split_survivor), hipMemcpyDeviceToHost, s));
                CSV_HIP(ctx, wait_stream(s));
                memcpy(surv.data(), ctx->pinned, n_surv * sizeof(csv_split_survivor));
            }
        }
        std::sort(surv.begin(), surv.end(), [](const csv_split_survivor &a, const csv_split_survivor &b) { return a.contig != b.contig ? a.contig < b.contig : a.pos < b.pos; });
        for (const csv_split_survivor &v : surv) st->off[v.contig + 1]++;
        for (int c = 0; c < n_contigs; c++) st->off[(size_t)c + 1] += st->off[(size_t)c];
        st->finished = true;
    }
    for (int c = 0; c <= n_contigs; c++) out_off[c] = st->off[(size_t)c];
    if (st->surv.size() > capacity) { ctx->err = "split_order: output capacity too small"; return CSV_ECAPACITY; }      // (the state stays: _finish again with more room)
    for (size_t i = 0; i < st->surv.size(); i++) out_rec[i] = st->surv[i].rec;
    delete st; ctx->split_state = nullptr;
    return CSV_OK;
}

extern "C" {

int csvgpu_split_order_begin(csv_ctx *ctx, int n_contigs, csv_shard *const *shards, uint8_t min_mapq)
{
    return split_order_begin(ctx, n_contigs, shards, min_mapq, -1);
}

int csvgpu_split_order_begin_self(csv_ctx *ctx, int n_contigs, csv_shard *const *shards, uint8_t min_mapq)
{
    return split_order_begin(ctx, n_contigs, shards, min_mapq, -1, true);
}

int csvgpu_split_order_finish(csv_ctx *ctx, const uint64_t *supp_hash, uint64_t n_supp, uint32_t *out_rec, uint64_t capacity, uint64_t *out_off)
{
    return split_order_finish(ctx, supp_hash, n_supp, out_rec, capacity, out_off);
}

int csvgpu_split_order(csv_ctx *ctx, int n_contigs, csv_shard *const *shards, uint8_t min_mapq, const uint64_t *supp_hash, uint64_t n_supp,
                       uint32_t *out_rec, uint64_t capacity, uint64_t *out_off)
{
    if (!ctx) return CSV_EINVAL;
    if (!out_off || (n_contigs > 0 && !shards) || (n_supp && !supp_hash) || (capacity && !out_rec)) { ctx->err = "split_order: null array"; return CSV_EINVAL; }
    if (n_contigs >= 0 && (uint32_t)n_contigs <= SO_MAX_CONTIGS) for (int c = 0; c <= n_contigs; c++) out_off[c] = 0;
    for (uint64_t i = 1; i < n_supp; i++) if (supp_hash[i] <= supp_hash[i - 1]) { ctx->err = "split_order: supp_hash must be sorted and distinct"; return CSV_EINVAL; }
    int rc = split_order_begin(ctx, n_contigs, shards, min_mapq, (int64_t)n_supp);
    if (rc) return rc;
    rc = split_order_finish(ctx, supp_hash, n_supp, out_rec, capacity, out_off);
    if (rc) { delete ctx->split_state; ctx->split_state = nullptr; }         // (one call: nothing is kept for a retry, the caller repeats it with the size from out_off)
    return rc;
}

}  // extern "C" (the chain below is templated; the entry points keep the C linkage of their declarations in csvgpu.h)

// The overlap groups that the order seeds (kernels/splitgroups.hip). One wait sizes the answer (members, groups, error word); the second is the
// answer's own copy. Everything in front of the first wait is queued without the host looking at the device.
// The chain in three steps, so that csvgpu_split_groups_fits can leave the groups where they lie: sg_queue reserves ctx->arena and the page-locked
// block (the chain's layout and stage, composed with the caller's: SgExtra below), stages the intervals and queues everything up to the copy of
// the three result words; sg_wait waits and reads them; the caller then reserves ctx->work for the member lists' sort (with whatever it
// needs beside it) and sg_fill_launch queues that sort.
constexpr uint32_t SG_ERR_DOMAIN = 2;             // in w.err: ORed in by an extra's kernel (the chain's own kernels OR in 1)
struct SgChain : SgWs {
    uint32_t n = 0;
    uint64_t n_seg = 0, max_len = 0;
    volatile uint64_t *h_res = nullptr;
    size_t pin_used = 0;                       // the page-locked block behind the chain's own staging: where the extra's stage runs
    uint64_t total = 0, n_groups = 0;
    const uint32_t *d_members = nullptr;       // after sg_fill
    const uint32_t *sort_flag = nullptr;       // the fill sort's gave-up word (device), or null
};

// host arrays on their way to carved device slices through the page-locked block
struct Upload { const void *dst, *src; size_t bytes; const void *pin; };
struct Uploads {                               // (the longest list: the eleven tables and four offset arrays of csvgpu_split_fits)
    Upload v[16];
    size_t n = 0;
    void add(const void *dst, const void *src, size_t bytes) { v[n++] = Upload{dst, src, bytes, nullptr}; }
    Upload *begin() { return v; }
    Upload *end() { return v + n; }
    const Upload *begin() const { return v; }
    const Upload *end() const { return v + n; }
};
static void stage_uploads(PinStage &p, Uploads &u) { for (Upload &x : u) x.pin = p.in(x.src, x.bytes); }
static int queue_uploads(csv_ctx *ctx, const Uploads &u, const char *what)
{
    for (const Upload &x : u) {
        if (!x.bytes) continue;
        const hipError_t e = hipMemcpyAsync((void *)x.dst, x.pin, x.bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) { ctx->err = std::string(what) + hipGetErrorString(e); return CSV_EHIP; }
    }
    return CSV_OK;
}

// What a fused entry point adds to the chain's two reservations: carve() takes its slices of ctx->arena behind the chain's (carved() follows the
// real pass: the upload list is built there, from the final pointers), stage() its slots of the page-locked block behind the chain's (planned by sg_queue; run for real by the extra's own queue(), or by the caller at c.pin_used once
// sg_queue has returned). on_device: start / end are not the caller's but written on the device, into c.d_start / c.d_end, by what queue()
// queues; the chain then skips its upload — and the caller's host range check. The chain's zeroed block (w.err with it) is cleared in front
// of queue(): what it queues may OR SG_ERR_DOMAIN into *c.w.err, which sg_wait reports as CSV_EINVAL.
struct SgNoExtra {
    static constexpr bool on_device = false;
    bool carve(Arena &) { return true; }
    void carved() {}
    void stage(PinStage &) {}
    int queue(SgChain &, PinStage &) { return CSV_OK; }
};

template <class Extra>
static int sg_queue(csv_ctx *ctx, const int32_t *start, const int32_t *end, const uint64_t *seg_off, uint64_t n_seg, uint32_t n, uint64_t max_len,
                    SgChain &c, Extra &x)
{
    (void)hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    int rc;
    c.n = n; c.n_seg = n_seg; c.max_len = max_len;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "split_groups", [&](Arena &a) { return carve_split_groups(a, n, n_seg, c) && x.carve(a); }))) return rc;
    x.carved();
    SplitGroupsWs &w = c.w;
    SortWs &sw = c.sw;
    int32_t *d_start = c.d_start, *d_end = c.d_end;
    uint64_t *d_seg = c.d_seg;
    void *es_tmp = c.es_tmp;
    constexpr bool on_device = Extra::on_device;

    const void *h_start = nullptr, *h_end = nullptr, *h_seg = nullptr;
    auto own = [&](PinStage &p) {
        if (!on_device) { h_start = p.in(start, (size_t)n * 4); h_end = p.in(end, (size_t)n * 4); }
        h_seg = p.in(seg_off, (n_seg + 1) * 8);
        c.h_res = (volatile uint64_t *)p.slot(256);
    };
    PinStage plan, pin(ctx);
    own(plan); x.stage(plan);
    if ((rc = ensure_pinned(ctx, plan.used))) return rc;
    own(pin);
    c.pin_used = pin.used;
    if (!on_device) {
        CSV_HIP(ctx, hipMemcpyAsync(d_start, h_start, (size_t)n * 4, hipMemcpyHostToDevice, s));
        CSV_HIP(ctx, hipMemcpyAsync(d_end, h_end, (size_t)n * 4, hipMemcpyHostToDevice, s));
    }
    CSV_HIP(ctx, hipMemcpyAsync(d_seg, h_seg, (n_seg + 1) * 8, hipMemcpyHostToDevice, s));
    if (on_device) {
        CSV_HIP(ctx, hipMemsetAsync(c.zero, 0, c.zero_bytes, s));
        if ((rc = x.queue(c, pin))) return rc;
    }
    const int key_bits = 32 + bits_of(n_seg - 1);
    const bool one_launch = onesweep(ctx);
    {
        TimerScope ts(ctx, CSV_K_SPLIT_GROUPS);
        if (!on_device) CSV_HIP(ctx, hipMemsetAsync(c.zero, 0, c.zero_bytes, s));
        launch_sg_keys(s, d_start, d_seg, n_seg, n, sw.k0, sw.v0);
        const int io = launch_radix_sort_u64(s, sw.k0, sw.v0, sw.k1, sw.v1, n, key_bits, sw.tmp, one_launch);
        launch_sg_links(s, w, io ? sw.k1 : sw.k0, io ? sw.v1 : sw.v0, d_start, d_end, d_seg, n);
        launch_exclusive_sum_u32(s, w.hist, (uint64_t)n + 1, es_tmp);
        launch_sg_seeds(s, w, n);
        launch_exclusive_sum_u32(s, w.cnt, (uint64_t)n + 1, es_tmp);
        launch_exclusive_sum_u32(s, w.keep, (uint64_t)n + 1, es_tmp);
        launch_sg_offsets(s, w, d_seg, n_seg, n, radix_sort_gave_up(sw.tmp, n, key_bits, one_launch));
        CSV_HIP(ctx, hipMemcpyAsync((void *)c.h_res, w.res, 24, hipMemcpyDeviceToHost, s));
    }
    return CSV_OK;
}

static int sg_wait(csv_ctx *ctx, SgChain &c)
{
    CSV_HIP(ctx, wait_stream(ctx->stream));
    c.total = c.h_res[0]; c.n_groups = c.h_res[1];
    if (c.h_res[2] & SG_ERR_DOMAIN) { ctx->err = "split_resident_fits: a coordinate of the shards is negative or end < start"; return CSV_EINVAL; }
    if (c.h_res[2]) { ctx->err = "split_groups: a bounded device loop gave up (radix look-back or seeding rounds)"; return CSV_EHIP; }
    if (c.n_groups > c.n || c.total < 2 * c.n_groups) { ctx->err = "split_groups: counts out of range"; return CSV_EHIP; }
    return CSV_OK;
}

// ---- the members: (group ‖ pre) keys, one stable sort for every group of the call ---------------------------------------------------------
static void sg_fill_launch(csv_ctx *ctx, SgChain &c, SortWs &fw)
{
    const int pre_bits = std::max(1, bits_of(c.max_len - 1)), fill_bits = pre_bits + bits_of(c.n_groups - 1);
    const bool one_launch = onesweep(ctx);
    launch_sg_fill(ctx->stream, c.w, (uint32_t)c.n_groups, pre_bits, fw.k0, fw.v0);
    const int io = launch_radix_sort_u64(ctx->stream, fw.k0, fw.v0, fw.k1, fw.v1, c.total, fill_bits, fw.tmp, one_launch);
    c.d_members = io ? fw.v1 : fw.v0;
    c.sort_flag = radix_sort_gave_up(fw.tmp, c.total, fill_bits, one_launch);
}

int csvgpu_split_groups(csv_ctx *ctx, const int32_t *start, const int32_t *end, const uint64_t *seg_off, uint64_t n_seg, uint64_t *seg_group_off,
                        uint64_t *group_off, uint32_t *members, uint64_t *n_members)
{
    if (!ctx) return CSV_EINVAL;
    if (!seg_off || !seg_group_off || !group_off || !n_members) { ctx->err = "split_groups: null array"; return CSV_EINVAL; }
    if (ctx->split_state) { ctx->err = "split_groups: a split order is pending on this context"; return CSV_EINVAL; }
    if (n_seg >= 0xffffffffull) { ctx->err = "split_groups: too many segments"; return CSV_EINVAL; }
    uint64_t max_len = 0;
    for (uint64_t c = 0; c < n_seg; c++) {
        if (seg_off[c + 1] < seg_off[c]) { ctx->err = "split_groups: seg_off not ascending"; return CSV_EINVAL; }
        max_len = std::max(max_len, seg_off[c + 1] - seg_off[c]);
    }
    const uint64_t n64 = seg_off[n_seg] - seg_off[0];
    if (seg_off[0] != 0) { ctx->err = "split_groups: seg_off[0] must be 0"; return CSV_EINVAL; }
    if (n64 >= 0xffffffffull) { ctx->err = "split_groups: more than 2^32 - 1 members"; return CSV_EINVAL; }
    const uint64_t capacity = *n_members;
    if (n64 && (!start || !end)) { ctx->err = "split_groups: null array"; return CSV_EINVAL; }
    if (capacity && !members) { ctx->err = "split_groups: null members with a capacity"; return CSV_EINVAL; }
    for (uint64_t i = 0; i < n64; i++) if (end[i] < start[i]) { ctx->err = "split_groups: end < start"; return CSV_EINVAL; }
    const uint32_t n = (uint32_t)n64;
    *n_members = 0;
    if (n == 0 || max_len < 2) {                             // no segment can hold a group of two
        for (uint64_t c = 0; c <= n_seg; c++) seg_group_off[c] = 0;
        group_off[0] = 0;
        return CSV_OK;
    }
    int rc;
    SgChain ch;
    SgNoExtra none;
    if ((rc = sg_queue(ctx, start, end, seg_off, n_seg, n, max_len, ch, none))) return rc;
    if ((rc = sg_wait(ctx, ch))) return rc;
    hipStream_t s = ctx->stream;
    const uint64_t total = ch.total, n_groups = ch.n_groups;
    *n_members = total;
    if (total > capacity) { ctx->err = "split_groups: members capacity too small"; return CSV_ECAPACITY; }
    if (total >= 0xffffffffull) { ctx->err = "split_groups: more than 2^32 - 1 entries in the answer"; *n_members = 0; return CSV_EINVAL; }
    if (n_groups == 0) {
        for (uint64_t c = 0; c <= n_seg; c++) seg_group_off[c] = 0;
        group_off[0] = 0;
        return CSV_OK;
    }
    SortWs fw;
    if ((rc = arena_reserve_for(ctx, ctx->work, "split_groups fill", [&](Arena &a) { return sortws_carve(a, total, fw); }))) return rc;
    constexpr size_t kPinnedOutMax = (size_t)64 << 20;       // larger answers are copied straight into the caller's array
    const bool members_pinned = total * 4 <= kPinnedOutMax;
    PinStage out(ctx);
    uint32_t *h_sort_err = nullptr;
    void *h_sgo = nullptr, *h_go = nullptr, *h_mem = nullptr;
    if ((rc = pin_reserve_for(ctx, out, [&](PinStage &p) {
            h_sort_err = (uint32_t *)p.slot(256);
            h_sgo = p.out(seg_group_off, (n_seg + 1) * 8); h_go = p.out(group_off, (n_groups + 1) * 8);
            if (members_pinned) h_mem = p.out(members, total * 4);
        }))) return rc;
    *h_sort_err = 0;
    {
        TimerScope ts(ctx, CSV_K_SPLIT_GROUPS);
        sg_fill_launch(ctx, ch, fw);
        if (ch.sort_flag) CSV_HIP(ctx, hipMemcpyAsync(h_sort_err, ch.sort_flag, 4, hipMemcpyDeviceToHost, s));
        CSV_HIP(ctx, hipMemcpyAsync(h_sgo, ch.w.seg_group_off, (n_seg + 1) * 8, hipMemcpyDeviceToHost, s));
        CSV_HIP(ctx, hipMemcpyAsync(h_go, ch.w.group_off, (n_groups + 1) * 8, hipMemcpyDeviceToHost, s));
        if (members_pinned) CSV_HIP(ctx, hipMemcpyAsync(h_mem, ch.d_members, total * 4, hipMemcpyDeviceToHost, s));
        else CSV_HIP(ctx, hipMemcpyAsync(members, ch.d_members, total * 4, hipMemcpyDeviceToHost, s));
    }
    CSV_HIP(ctx, wait_stream(s));
    if (*h_sort_err) { ctx->err = "split_groups: a radix pass's look-back gave up"; *n_members = 0; return CSV_EHIP; }
    out.finish();
    return CSV_OK;
}

// ---- the groups' evidence (kernels/splitfits.hip) ------------------------------------------------------------------------------------------
// Everything the two entry points share: argument checks, the tables' way to the device, the launch with its one readback, and the sets too
// large for LDS (materialised one by one, labelled by the large-segment path of csvgpu_dbscan_1d, reduced out of global memory).
static int sf_check(csv_ctx *ctx, const csv_split_tables *t, const uint64_t *seg_off, uint64_t n_seg, double eps, int32_t min_pts, uint64_t &max_len)
{
    int rc = check_dbscan_args(ctx, eps, min_pts, false);
    if (rc) return rc;
    if (!t || !seg_off) { ctx->err = "split_fits: null array"; return CSV_EINVAL; }
    if (ctx->split_state) { ctx->err = "split_fits: a split order is pending on this context"; return CSV_EINVAL; }
    if (n_seg >= 0xffffffffull) { ctx->err = "split_fits: too many segments"; return CSV_EINVAL; }
    if (seg_off[0] != 0) { ctx->err = "split_fits: seg_off[0] must be 0"; return CSV_EINVAL; }
    max_len = 0;
    for (uint64_t c = 0; c < n_seg; c++) {
        if (seg_off[c + 1] < seg_off[c]) { ctx->err = "split_fits: seg_off not ascending"; return CSV_EINVAL; }
        max_len = std::max(max_len, seg_off[c + 1] - seg_off[c]);
    }
    const uint64_t nm = t->n_members, ns = t->n_supp;
    if (seg_off[n_seg] != nm) { ctx->err = "split_fits: seg_off does not end at the tables' member count"; return CSV_EINVAL; }
    if (nm >= 0xffffffffull || ns >= 0xffffffffull) { ctx->err = "split_fits: more than 2^32 - 1 members or supplementary records"; return CSV_EINVAL; }
    if (!t->supp_off || (nm && (!t->start || !t->end || !t->q_start || !t->q_end || !t->reverse)) ||
        (ns && (!t->supp_start || !t->supp_end || !t->supp_q_start || !t->supp_q_end || !t->supp_flags))) { ctx->err = "split_fits: null array in the tables"; return CSV_EINVAL; }
    if (t->supp_off[0] != 0 || t->supp_off[nm] != ns) { ctx->err = "split_fits: supp_off must run from 0 to n_supp"; return CSV_EINVAL; }
    for (uint64_t m = 0; m < nm; m++) {
        if (t->supp_off[m + 1] < t->supp_off[m]) { ctx->err = "split_fits: supp_off not ascending"; return CSV_EINVAL; }
        if (t->start[m] < 0 || t->q_start[m] < 0 || t->q_end[m] < 0 || t->end[m] < t->start[m]) { ctx->err = "split_fits: a member's coordinate is negative or end < start"; return CSV_EINVAL; }
    }
    for (uint64_t z = 0; z < ns; z++) {
        if (t->supp_flags[z] & 2u) continue;                 // another tid: only the flags are read
        if (t->supp_start[z] < 0 || t->supp_q_start[z] < 0 || t->supp_q_end[z] < 0 || t->supp_end[z] < t->supp_start[z]) {
            ctx->err = "split_fits: a supplementary record's coordinate is negative or end < start"; return CSV_EINVAL;
        }
    }
    return CSV_OK;
}

// the tables' way to their carved slices (carve_sf_tables with the same with_start_end)
static void sf_uploads(const csv_split_tables *t, const SplitFitsIn &in, bool with_start_end, Uploads &u)
{
    const uint64_t nm = t->n_members, ns = t->n_supp;
    if (with_start_end) { u.add(in.start, t->start, nm * 4); u.add(in.end, t->end, nm * 4); }
    u.add(in.q_start, t->q_start, nm * 4); u.add(in.q_end, t->q_end, nm * 4); u.add(in.reverse, t->reverse, nm);
    u.add(in.supp_off, t->supp_off, (nm + 1) * 8);
    u.add(in.supp_start, t->supp_start, ns * 4); u.add(in.supp_end, t->supp_end, ns * 4);
    u.add(in.supp_q_start, t->supp_q_start, ns * 4); u.add(in.supp_q_end, t->supp_q_end, ns * 4);
    u.add(in.supp_flags, t->supp_flags, ns);
}

struct SfRun : SfRunWs {                       // (carve_sf_run(n_groups, B) in the arena the run works in)
    SplitFitsIn in;
    uint64_t B = 0;                            // no set has more points
    volatile uint64_t *h_res = nullptr;        // sets and points beyond the LDS kernel
    void *h_out = nullptr;                     // the records' slot of the page-locked block
};
// the run's part of a stage: the two counters and the records
static void sf_stage(PinStage &p, SfRun &r, csv_split_fit *out)
{
    r.h_res = (volatile uint64_t *)p.slot(256);
    r.h_out = p.out(out, (size_t)r.in.n_groups * sizeof(csv_split_fit));
}

// the launch and the copies of the records and the two counters into the page-locked block; the caller adds its own copies and waits
static int sf_queue(csv_ctx *ctx, SfRun &r, double eps, int32_t min_pts)
{
    const uint64_t G = r.in.n_groups;
    hipStream_t s = ctx->stream;
    TimerScope ts(ctx, CSV_K_SPLIT_FITS);
    CSV_HIP(ctx, hipMemsetAsync(r.d_big_n, 0, G * 6 * 4, s));
    CSV_HIP(ctx, hipMemsetAsync(r.d_res, 0, 16, s));
    launch_sf_fits(s, r.in, eps, min_pts, r.d_out, r.d_big_n, r.d_res);
    CSV_HIP(ctx, hipMemcpyAsync((void *)r.h_res, r.d_res, 16, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, hipMemcpyAsync(r.h_out, r.d_out, G * sizeof(csv_split_fit), hipMemcpyDeviceToHost, s));
    return CSV_OK;
}

// after the wait, when r.h_res[0] sets were too large for LDS (the page-locked block is free again: its outputs have been taken)
static int sf_big(csv_ctx *ctx, SfRun &r, double eps, int32_t min_pts, csv_split_fit *out)
{
    const uint64_t n_big = r.h_res[0], G = r.in.n_groups, B = r.B;
    hipStream_t s = ctx->stream;
    int rc;
    std::vector<uint32_t> big_n(G * 6);
    CSV_HIP(ctx, hipMemcpyAsync(big_n.data(), r.d_big_n, G * 6 * 4, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, wait_stream(s));
    if (B <= DBSCAN1D_MAX_SEG) { ctx->err = "split_fits: a set larger than its bound"; return CSV_EHIP; }
    int32_t *pts = r.pts, *ks = r.ks, *labels = r.labels;      // (carved with the run: B > DBSCAN1D_MAX_SEG)
    uint32_t *sizes = r.sizes;
    void *tmp = r.tmp;
    const SortWs &w = r.w;
    PinStage pin(ctx);
    uint32_t *h_flags = nullptr;
    void *h_out = nullptr;
    if ((rc = pin_reserve_for(ctx, pin, [&](PinStage &p) { h_flags = (uint32_t *)p.slot(n_big * 4); h_out = p.out(out, G * sizeof(csv_split_fit)); }))) return rc;
    memset(h_flags, 0, n_big * 4);
    const bool one_launch = onesweep(ctx);
    {
        TimerScope ts(ctx, CSV_K_SPLIT_FITS);
        uint64_t k = 0;
        for (uint64_t item = 0; item < G * 6; item++) {
            const uint32_t n = big_n[item];
            if (!n) continue;
            if (n > B || n <= DBSCAN1D_MAX_SEG || k >= n_big) { ctx->err = "split_fits: large-set counts out of range"; return CSV_EHIP; }
            launch_sf_big_points(s, r.in, (uint32_t)item, pts);
            launch_iota_keys_i32(s, pts, n, w.k0, w.v0);
            const int io = launch_radix_sort_u64(s, w.k0, w.v0, w.k1, w.v1, n, 32, w.tmp, one_launch);
            const uint32_t *perm = io ? w.v1 : w.v0;
            if (const uint32_t *flag = radix_sort_gave_up(w.tmp, n, 32, one_launch)) CSV_HIP(ctx, hipMemcpyAsync(h_flags + k, flag, 4, hipMemcpyDeviceToHost, s));
            launch_gather_u32(s, (const uint32_t *)pts, perm, n, (uint32_t *)ks);
            launch_dbscan_1d_big(s, ks, perm, n, eps, min_pts, labels, tmp);
            CSV_HIP(ctx, hipMemsetAsync(sizes, 0, (size_t)n * 4, s));
            launch_sf_big_reduce(s, ks, perm, labels, n, sizes, r.d_out + item / 6, (int)(item % 6));
            k++;
        }
        CSV_HIP(ctx, hipMemcpyAsync(h_out, r.d_out, G * sizeof(csv_split_fit), hipMemcpyDeviceToHost, s));
    }
    CSV_HIP(ctx, wait_stream(s));
    for (uint64_t k = 0; k < n_big; k++) if (h_flags[k]) { ctx->err = "split_fits: a radix pass's look-back gave up"; return CSV_EHIP; }
    pin.finish();
    return CSV_OK;
}

// what the fused calls share behind the chain's queue (r.in's tables set): the one sizing readback, the member lists' sort, the fits' launch and
// its records, the sets too large for LDS
static int sgf_finish(csv_ctx *ctx, SgChain &ch, SfRun &r, uint64_t n_seg, uint64_t max_len, uint64_t ns, double eps, int32_t min_pts,
                      uint64_t *seg_group_off, csv_split_fit *out, uint64_t *n_groups)
{
    int rc;
    hipStream_t s = ctx->stream;
    if ((rc = sg_wait(ctx, ch))) return rc;
    const uint64_t G = ch.n_groups, total = ch.total;
    if (total >= 0xffffffffull) { ctx->err = "split_fits: more than 2^32 - 1 entries in the groups"; return CSV_EINVAL; }
    if (G == 0) {
        for (uint64_t c = 0; c <= n_seg; c++) seg_group_off[c] = 0;
        return CSV_OK;
    }
    r.B = std::max(std::min(total, max_len), ns);
    SortWs fw;
    if ((rc = arena_reserve_for(ctx, ctx->work, "split_fits work", [&](Arena &a) { return sortws_carve(a, total, fw) && carve_sf_run(a, G, r.B, r); }))) return rc;
    r.in.n_groups = (uint32_t)G;
    PinStage pin(ctx);
    uint32_t *h_sort_err = nullptr;
    void *h_sgo = nullptr;
    if ((rc = pin_reserve_for(ctx, pin, [&](PinStage &p) {
            h_sort_err = (uint32_t *)p.slot(256);
            h_sgo = p.out(seg_group_off, (n_seg + 1) * 8);
            sf_stage(p, r, out);
        }))) return rc;
    *h_sort_err = 0;
    {
        TimerScope ts(ctx, CSV_K_SPLIT_GROUPS);
        sg_fill_launch(ctx, ch, fw);
        if (ch.sort_flag) CSV_HIP(ctx, hipMemcpyAsync(h_sort_err, ch.sort_flag, 4, hipMemcpyDeviceToHost, s));
        CSV_HIP(ctx, hipMemcpyAsync(h_sgo, ch.w.seg_group_off, (n_seg + 1) * 8, hipMemcpyDeviceToHost, s));
    }
    r.in.seg_off = ch.d_seg; r.in.seg_group_off = ch.w.seg_group_off; r.in.group_off = ch.w.group_off; r.in.members = ch.d_members;
    r.in.n_seg = n_seg;
    if ((rc = sf_queue(ctx, r, eps, min_pts))) return rc;
    CSV_HIP(ctx, wait_stream(s));
    if (*h_sort_err) { ctx->err = "split_fits: a radix pass's look-back gave up"; return CSV_EHIP; }
    pin.finish();
    *n_groups = G;
    if (r.h_res[0] == 0) return CSV_OK;
    return sf_big(ctx, r, eps, min_pts, out);
}

int csvgpu_split_fits(csv_ctx *ctx, const csv_split_tables *t, const uint64_t *seg_off, uint64_t n_seg, const uint64_t *seg_group_off,
                      const uint64_t *group_off, const uint32_t *members, double eps, int32_t min_pts, csv_split_fit *out)
{
    if (!ctx) return CSV_EINVAL;
    uint64_t max_len = 0;
    int rc = sf_check(ctx, t, seg_off, n_seg, eps, min_pts, max_len);
    if (rc) return rc;
    if (!seg_group_off || !group_off) { ctx->err = "split_fits: null array"; return CSV_EINVAL; }
    if (seg_group_off[0] != 0 || group_off[0] != 0) { ctx->err = "split_fits: group offsets must start at 0"; return CSV_EINVAL; }
    for (uint64_t c = 0; c < n_seg; c++) if (seg_group_off[c + 1] < seg_group_off[c]) { ctx->err = "split_fits: seg_group_off not ascending"; return CSV_EINVAL; }
    const uint64_t G = seg_group_off[n_seg];
    if (G > t->n_members) { ctx->err = "split_fits: more groups than members"; return CSV_EINVAL; }
    uint64_t max_group = 0;
    for (uint64_t g = 0; g < G; g++) {
        if (group_off[g + 1] < group_off[g]) { ctx->err = "split_fits: group_off not ascending"; return CSV_EINVAL; }
        max_group = std::max(max_group, group_off[g + 1] - group_off[g]);
    }
    if (G == 0) return CSV_OK;
    const uint64_t total = group_off[G];
    if (total >= 0xffffffffull) { ctx->err = "split_fits: more than 2^32 - 1 entries in the groups"; return CSV_EINVAL; }
    if (!out || (total && !members)) { ctx->err = "split_fits: null array"; return CSV_EINVAL; }
    {   // members: inside their segment, and distinct within a group (a group is a set of reads; the large-set bound below counts on it)
        std::vector<uint64_t> seen(max_len, 0);              // by member of the current segment: the last group (+ 1) that held it
        for (uint64_t c = 0; c < n_seg; c++) {
            const uint64_t len = seg_off[c + 1] - seg_off[c];
            for (uint64_t g = seg_group_off[c]; g < seg_group_off[c + 1]; g++)
                for (uint64_t q = group_off[g]; q < group_off[g + 1]; q++) {
                    if (members[q] >= len) { ctx->err = "split_fits: a member index outside its segment"; return CSV_EINVAL; }
                    if (seen[members[q]] == g + 1) { ctx->err = "split_fits: a member twice in one group"; return CSV_EINVAL; }
                    seen[members[q]] = g + 1;
                }
        }
    }
    (void)hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    const uint64_t nm = t->n_members, ns = t->n_supp;
    SfRun r;
    r.B = std::max(max_group, ns);
    uint64_t *d_seg = nullptr, *d_sgo = nullptr, *d_go = nullptr;
    uint32_t *d_mem = nullptr;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "split_fits", [&](Arena &a) {
            return carve_sf_tables(a, nm, ns, true, r.in) && take(a, d_seg, (n_seg + 1) * 8) && take(a, d_sgo, (n_seg + 1) * 8) && take(a, d_go, (G + 1) * 8) &&
                   take(a, d_mem, total * 4) && carve_sf_run(a, G, r.B, r);
        }))) return rc;
    r.in.seg_off = d_seg; r.in.seg_group_off = d_sgo; r.in.group_off = d_go; r.in.members = d_mem;
    r.in.n_seg = n_seg; r.in.n_groups = (uint32_t)G;
    Uploads up;
    sf_uploads(t, r.in, true, up);
    up.add(d_seg, seg_off, (n_seg + 1) * 8); up.add(d_sgo, seg_group_off, (n_seg + 1) * 8);
    up.add(d_go, group_off, (G + 1) * 8); up.add(d_mem, members, total * 4);
    PinStage pin(ctx);
    if ((rc = pin_reserve_for(ctx, pin, [&](PinStage &p) { stage_uploads(p, up); sf_stage(p, r, out); }))) return rc;
    if ((rc = queue_uploads(ctx, up, "split_fits: copying the tables: "))) return rc;
    if ((rc = sf_queue(ctx, r, eps, min_pts))) return rc;
    CSV_HIP(ctx, wait_stream(s));
    pin.finish();
    if (r.h_res[0] == 0) return CSV_OK;
    return sf_big(ctx, r, eps, min_pts, out);
}

namespace {
// the caller's tables beside the chain (SgExtra of csvgpu_split_groups_fits); start / end are the chain's copies
struct SfTablesExtra {
    static constexpr bool on_device = false;
    const csv_split_tables *t; SplitFitsIn &in; Uploads up;
    bool carve(Arena &a) { return carve_sf_tables(a, t->n_members, t->n_supp, false, in); }
    void carved() { sf_uploads(t, in, false, up); }
    void stage(PinStage &p) { stage_uploads(p, up); }
    int queue(SgChain &, PinStage &) { return CSV_OK; }
};
}  // namespace

int csvgpu_split_groups_fits(csv_ctx *ctx, const csv_split_tables *t, const uint64_t *seg_off, uint64_t n_seg, double eps, int32_t min_pts,
                             uint64_t *seg_group_off, csv_split_fit *out, uint64_t *n_groups)
{
    if (!ctx) return CSV_EINVAL;
    uint64_t max_len = 0;
    int rc = sf_check(ctx, t, seg_off, n_seg, eps, min_pts, max_len);
    if (rc) return rc;
    if (!seg_group_off || !n_groups) { ctx->err = "split_fits: null array"; return CSV_EINVAL; }
    const uint64_t nm = t->n_members, ns = t->n_supp;
    if (nm && !out) { ctx->err = "split_fits: null array"; return CSV_EINVAL; }
    *n_groups = 0;
    if (nm == 0 || max_len < 2) {                            // no segment can hold a group of two
        for (uint64_t c = 0; c <= n_seg; c++) seg_group_off[c] = 0;
        return CSV_OK;
    }
    hipStream_t s = ctx->stream;
    SgChain ch;
    SfRun r;
    SfTablesExtra tables{t, r.in, {}};
    if ((rc = sg_queue(ctx, t->start, t->end, seg_off, n_seg, (uint32_t)nm, max_len, ch, tables))) return rc;
    r.in.start = ch.d_start; r.in.end = ch.d_end;
    {   // the tables travel while the chain runs
        PinStage pin(ctx, ch.pin_used);
        tables.stage(pin);
        if ((rc = queue_uploads(ctx, tables.up, "split_fits: copying the tables: "))) { (void)wait_stream(s); return rc; }
    }
    return sgf_finish(ctx, ch, r, n_seg, max_len, ns, eps, min_pts, seg_group_off, out, n_groups);
}

// ---- the tables from the resident shards (kernels/splittables.hip) ------------------------------------------------------------------------
// What the two entry points share: the checks of the references (everything the kernel indexes with is bounded here), their way to the device
// and the launch.
static int sr_check(csv_ctx *ctx, uint64_t n_seg, csv_shard *const *shards, const csv_split_refs *f, const uint64_t *seg_off, uint64_t &max_len)
{
    if (!f || !seg_off || (n_seg && !shards)) { ctx->err = "split_tables_resident: null array"; return CSV_EINVAL; }
    if (ctx->split_state) { ctx->err = "split_tables_resident: a split order is pending on this context"; return CSV_EINVAL; }
    if (n_seg >= 0xffffffffull) { ctx->err = "split_tables_resident: too many segments"; return CSV_EINVAL; }
    const uint64_t nm = f->n_members, ns = f->n_supp;
    if (nm >= 0xffffffffull || ns >= 0xffffffffull) { ctx->err = "split_tables_resident: 2^32 - 1 or more members or supplementary entries"; return CSV_EINVAL; }
    if (!f->supp_off || (nm && !f->member_rec) || (ns && (!f->supp_rec || !f->supp_where))) { ctx->err = "split_tables_resident: null array in the references"; return CSV_EINVAL; }
    if (seg_off[0] != 0) { ctx->err = "split_tables_resident: seg_off[0] must be 0"; return CSV_EINVAL; }
    max_len = 0;
    for (uint64_t c = 0; c < n_seg; c++) {
        if (seg_off[c + 1] < seg_off[c]) { ctx->err = "split_tables_resident: seg_off not ascending"; return CSV_EINVAL; }
        max_len = std::max(max_len, seg_off[c + 1] - seg_off[c]);
    }
    if (seg_off[n_seg] != nm) { ctx->err = "split_tables_resident: seg_off does not end at the references' member count"; return CSV_EINVAL; }
    if (f->supp_off[0] != 0 || f->supp_off[nm] != ns) { ctx->err = "split_tables_resident: supp_off must run from 0 to n_supp"; return CSV_EINVAL; }
    for (uint64_t m = 0; m < nm; m++) if (f->supp_off[m + 1] < f->supp_off[m]) { ctx->err = "split_tables_resident: supp_off not ascending"; return CSV_EINVAL; }
    for (uint64_t c = 0; c < n_seg; c++) {
        const csv_shard *sh = shards[c];
        if (!sh || (sh->d.n_reads && (!sh->d.pos || !sh->d.flag || !sh->ref_end || !sh->q_start || !sh->q_end))) { ctx->err = "split_tables_resident: null shard"; return CSV_EINVAL; }
        const uint64_t n_reads = sh->d.n_reads;
        for (uint64_t m = seg_off[c]; m < seg_off[c + 1]; m++) {
            if (f->member_rec[m] >= n_reads) { ctx->err = "split_tables_resident: a member's record index beyond its shard"; return CSV_EINVAL; }
            for (uint64_t z = f->supp_off[m]; z < f->supp_off[m + 1]; z++) {
                const uint8_t w = f->supp_where[z];
                if (w != 0 && w != 2 && w != 3) { ctx->err = "split_tables_resident: supp_where must be 0, 2 or 3"; return CSV_EINVAL; }
                if (w == 0 && f->supp_rec[z] >= n_reads) { ctx->err = "split_tables_resident: a supplementary record index beyond its shard"; return CSV_EINVAL; }
            }
        }
    }
    return CSV_OK;
}

// the references and the shard table on their way to carve_sr_refs' slices, and the launch behind them. d_seg: seg_off on the device.
// in.supp_off is what the fits read afterwards.
struct SrRefs {
    std::vector<SplitTabSeg> tab;
    Uploads up;
    SplitTablesIn in;
    void uploads(uint64_t n_seg, csv_shard *const *shards, const csv_split_refs *f)       // after the carve
    {
        const uint64_t nm = f->n_members, ns = f->n_supp;
        tab.resize(n_seg);
        for (uint64_t c = 0; c < n_seg; c++) { const csv_shard *sh = shards[c]; tab[c] = SplitTabSeg{sh->d.pos, sh->d.flag, sh->ref_end, sh->q_start, sh->q_end}; }
        up.add(in.seg, tab.data(), n_seg * sizeof(SplitTabSeg)); up.add(in.member_rec, f->member_rec, nm * 4); up.add(in.supp_off, f->supp_off, (nm + 1) * 8);
        up.add(in.supp_rec, f->supp_rec, ns * 4); up.add(in.supp_where, f->supp_where, ns);
        in.n_seg = n_seg; in.n_members = (uint32_t)nm; in.n_supp = (uint32_t)ns;
    }
    int launch(csv_ctx *ctx, const uint64_t *d_seg, const SplitTablesOut &out)
    {
        const int rc = queue_uploads(ctx, up, "split_tables_resident: copying the references: ");
        if (rc) return rc;
        in.seg_off = d_seg;
        TimerScope ts(ctx, CSV_K_MISC);
        launch_st_tables(ctx->stream, in, out);
        return CSV_OK;
    }
};

int csvgpu_split_tables_resident(csv_ctx *ctx, uint64_t n_seg, csv_shard *const *shards, const csv_split_refs *f, const uint64_t *seg_off, csv_split_tables *t)
{
    if (!ctx) return CSV_EINVAL;
    uint64_t max_len = 0;
    int rc = sr_check(ctx, n_seg, shards, f, seg_off, max_len);
    if (rc) return rc;
    if (!t) { ctx->err = "split_tables_resident: null array"; return CSV_EINVAL; }
    const uint64_t nm = f->n_members, ns = f->n_supp;
    if (!t->supp_off || (nm && (!t->start || !t->end || !t->q_start || !t->q_end || !t->reverse)) ||
        (ns && (!t->supp_start || !t->supp_end || !t->supp_q_start || !t->supp_q_end || !t->supp_flags))) { ctx->err = "split_tables_resident: null array in the tables"; return CSV_EINVAL; }
    if (nm == 0) {
        t->n_members = t->n_supp = 0;
        ((uint64_t *)t->supp_off)[0] = 0;
        return CSV_OK;
    }
    (void)hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    SplitTablesOut o;
    SrRefs refs;
    uint64_t *d_seg = nullptr;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "split_tables_resident", [&](Arena &a) {
            return take(a, o.start, nm * 4) && take(a, o.end, nm * 4) && take(a, d_seg, (n_seg + 1) * 8) && take(a, o.err, 256) && sr_carve(a, nm, ns, o) &&
                   carve_sr_refs(a, n_seg, nm, ns, refs.in);
        }))) return rc;
    o.err_bit = 1;
    refs.uploads(n_seg, shards, f);
    struct Down { void *dst; const void *src; size_t bytes; void *pin; };
    Down down[] = {{(void *)t->start, o.start, nm * 4, nullptr}, {(void *)t->end, o.end, nm * 4, nullptr}, {(void *)t->q_start, o.q_start, nm * 4, nullptr},
                   {(void *)t->q_end, o.q_end, nm * 4, nullptr}, {(void *)t->reverse, o.reverse, nm, nullptr},
                   {(void *)t->supp_start, o.supp_start, ns * 4, nullptr}, {(void *)t->supp_end, o.supp_end, ns * 4, nullptr},
                   {(void *)t->supp_q_start, o.supp_q_start, ns * 4, nullptr}, {(void *)t->supp_q_end, o.supp_q_end, ns * 4, nullptr},
                   {(void *)t->supp_flags, o.supp_flags, ns, nullptr}};
    PinStage pin(ctx);
    const void *h_seg = nullptr;
    volatile uint32_t *h_err = nullptr;
    if ((rc = pin_reserve_for(ctx, pin, [&](PinStage &p) {
            h_seg = p.in(seg_off, (n_seg + 1) * 8);
            stage_uploads(p, refs.up);
            h_err = (volatile uint32_t *)p.slot(256);
            for (Down &d : down) d.pin = p.out(d.dst, d.bytes);
        }))) return rc;
    CSV_HIP(ctx, hipMemsetAsync(o.err, 0, 4, s));
    CSV_HIP(ctx, hipMemcpyAsync(d_seg, h_seg, (n_seg + 1) * 8, hipMemcpyHostToDevice, s));
    if ((rc = refs.launch(ctx, d_seg, o))) { (void)wait_stream(s); return rc; }
    CSV_HIP(ctx, hipMemcpyAsync((void *)h_err, o.err, 4, hipMemcpyDeviceToHost, s));
    for (const Down &d : down) if (d.bytes) CSV_HIP(ctx, hipMemcpyAsync(d.pin, d.src, d.bytes, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, wait_stream(s));
    if (*h_err) { ctx->err = "split_tables_resident: a coordinate of the shards is negative or end < start"; return CSV_EINVAL; }
    pin.finish();
    memcpy((void *)t->supp_off, f->supp_off, (nm + 1) * 8);
    t->n_members = nm; t->n_supp = ns;
    return CSV_OK;
}

namespace {
// the tables built on the device in front of the chain (SgExtra of csvgpu_split_resident_fits)
struct SrFill {
    static constexpr bool on_device = true;
    csv_ctx *ctx; uint64_t n_seg; csv_shard *const *shards; const csv_split_refs *f;
    SplitFitsIn *fits_in;
    SplitTablesOut o;
    SrRefs refs;
    bool carve(Arena &a) { return sr_carve(a, f->n_members, f->n_supp, o) && carve_sr_refs(a, n_seg, f->n_members, f->n_supp, refs.in); }
    void carved() { refs.uploads(n_seg, shards, f); }
    void stage(PinStage &p) { stage_uploads(p, refs.up); }
    int queue(SgChain &c, PinStage &pin)
    {
        o.start = c.d_start; o.end = c.d_end;
        o.err = c.w.err; o.err_bit = SG_ERR_DOMAIN;
        stage(pin);
        const int rc = refs.launch(ctx, c.d_seg, o);
        if (rc) return rc;
        SplitFitsIn &r = *fits_in;
        r.start = o.start; r.end = o.end; r.q_start = o.q_start; r.q_end = o.q_end; r.reverse = o.reverse; r.supp_off = refs.in.supp_off;
        r.supp_start = o.supp_start; r.supp_end = o.supp_end; r.supp_q_start = o.supp_q_start; r.supp_q_end = o.supp_q_end; r.supp_flags = o.supp_flags;
        return CSV_OK;
    }
};
}  // namespace

int csvgpu_split_resident_fits(csv_ctx *ctx, uint64_t n_seg, csv_shard *const *shards, const csv_split_refs *f, const uint64_t *seg_off, double eps,
                               int32_t min_pts, uint64_t *seg_group_off, csv_split_fit *out, uint64_t *n_groups)
{
    if (!ctx) return CSV_EINVAL;
    int rc = check_dbscan_args(ctx, eps, min_pts, false);
    if (rc) return rc;
    uint64_t max_len = 0;
    if ((rc = sr_check(ctx, n_seg, shards, f, seg_off, max_len))) return rc;
    if (!seg_group_off || !n_groups) { ctx->err = "split_resident_fits: null array"; return CSV_EINVAL; }
    const uint64_t nm = f->n_members, ns = f->n_supp;
    if (nm && !out) { ctx->err = "split_resident_fits: null array"; return CSV_EINVAL; }
    *n_groups = 0;
    if (nm == 0 || max_len < 2) {                            // no segment can hold a group of two
        for (uint64_t c = 0; c <= n_seg; c++) seg_group_off[c] = 0;
        return CSV_OK;
    }
    SgChain ch;
    SfRun r;
    SrFill fill;
    fill.ctx = ctx; fill.n_seg = n_seg; fill.shards = shards; fill.f = f; fill.fits_in = &r.in;
    if ((rc = sg_queue(ctx, nullptr, nullptr, seg_off, n_seg, (uint32_t)nm, max_len, ch, fill))) { (void)wait_stream(ctx->stream); return rc; }
    return sgf_finish(ctx, ch, r, n_seg, max_len, ns, eps, min_pts, seg_group_off, out, n_groups);
}

// ---- the copy-number observations (kernels/cnobs.hip) --------------------------------------------------------------------------------------
namespace {
// What the two entry points share: the checks, the tables' way up, windows -> order -> offsets -> fill, and the count's readback.
struct CnCall {
    uint64_t R = 0, W = 0, S = 0, bound = 0, cap = 0, total = 0;
    CnWs w;
    PinStage pin;
    void *h_off = nullptr, *h_pos = nullptr, *h_baf = nullptr, *h_pfb = nullptr, *h_l2 = nullptr, *h_snp = nullptr, *h_states = nullptr, *h_ll = nullptr;
};

// the epochs a region of up to CN_MAX_WINDOWS nodes can reach, from the library's own policy; false if a bucket count does not fit its form
bool cn_epochs(CnEpochs &ep)
{
    std::vector<uint64_t> first, bkt;
    split_order_epochs(CN_MAX_WINDOWS, first, bkt);
    ep = CnEpochs();
    for (size_t k = 0; k < first.size() && first[k] < CN_MAX_WINDOWS; k++) {
        if (ep.n == CN_MAX_EPOCHS || bkt[k] > (first[k] < CN_SMALL_MAX ? CN_SMALL_MAX : CN_MAX_WINDOWS)) return false;
        ep.first[ep.n] = (uint32_t)first[k]; ep.B[ep.n] = (uint32_t)bkt[k]; ep.n++;
    }
    ep.first[ep.n] = 0xffffffffu;
    return ep.n > 0 && ep.first[0] == 0;
}

int cn_run(csv_ctx *ctx, const char *what, const csv_cn_regions *in, bool decode, bool want_baf, bool want_pfb, bool want_l2, bool want_snp,
           const uint64_t *n_obs, CnCall &c)
{
    auto bad = [&](const char *msg) { ctx->err = std::string(what) + ": " + msg; return (int)CSV_EINVAL; };
    if (!in || !n_obs) return bad("null argument");
    if (ctx->split_state) return bad("a split order is pending on this context");
    if (in->n_shards < 0) return bad("negative shard count");
    if (in->n_shards && (!in->shards || !in->mean_cov)) return bad("null array");
    if (!in->reg_off || in->reg_off[0] != 0) return bad("reg_off missing or not starting at 0");
    for (int s = 0; s < in->n_shards; s++) {
        if (in->reg_off[s + 1] < in->reg_off[s]) return bad("reg_off not ascending");
        if (in->reg_off[s + 1] > in->reg_off[s] && !in->shards[s]) return bad("null shard");
    }
    const uint64_t R = in->n_shards ? in->reg_off[in->n_shards] : 0;
    c.R = R; c.cap = *n_obs;
    if (R == 0) return CSV_OK;
    if (R >= 0xffffffffull) return bad("2^32 - 1 or more regions");
    if (!in->region_start || !in->region_end || !in->sample_size || !in->snp_off) return bad("null array");
    if (in->snp_off[0] != 0) return bad("snp_off must start at 0");
    uint64_t W = 0;
    for (uint64_t r = 0; r < R; r++) {
        if (in->snp_off[r + 1] < in->snp_off[r]) return bad("snp_off not ascending");
        if (in->sample_size[r] <= 0) return bad("sample_size <= 0");
        if (in->region_start[r] > in->region_end[r]) return bad("region start > end");
        if (in->region_end[r] >= 0x7fffffffu) return bad("a window coordinate could reach 2^31");
        const uint64_t ss = std::max<uint64_t>(in->snp_off[r + 1] - in->snp_off[r], (uint64_t)in->sample_size[r]);
        if (ss > CN_MAX_WINDOWS) return bad("more than 5087 windows in a region");
        W += ss;
    }
    const uint64_t S = in->snp_off[R];
    if (S && (!in->snp_pos || !in->snp_baf || !in->snp_pfb)) return bad("null array");
    for (uint64_t r = 0; r < R; r++)
        for (uint64_t k = in->snp_off[r] + 1; k < in->snp_off[r + 1]; k++)
            if (in->snp_pos[k] < in->snp_pos[k - 1]) return bad("SNP positions decrease inside a region");
    if (W + 3 * S >= 0xffffffffull) return bad("2^32 - 1 or more windows, records or observations");
    c.W = W; c.S = S; c.bound = W + 3 * S;
    CnEpochs ep;
    if (!cn_epochs(ep)) { ctx->err = std::string(what) + ": this C++ library's hash table does not grow as the kernels assume"; return CSV_EHIP; }

    (void)hipSetDevice(ctx->device);
    const uint64_t n_sh = (uint64_t)in->n_shards;
    int rc;
    if ((rc = arena_reserve_for(ctx, ctx->arena, what, [&](Arena &a) { return carve_cn_obs(a, R, W, n_sh, S, decode, c.w); }))) return rc;
    const CnInLayout L(R, n_sh, S);
    const uint64_t room = std::min(c.cap, c.bound);          // what can come back
    char *h_in = nullptr;
    uint64_t *h_total = nullptr;
    c.pin = PinStage(ctx);
    if ((rc = pin_reserve_for(ctx, c.pin, [&](PinStage &p) {
            h_total = (uint64_t *)p.slot(256); h_in = (char *)p.slot(L.bytes);
            c.h_off = p.slot((R + 1) * 8); c.h_pos = p.slot(room * 4);
            if (want_baf) c.h_baf = p.slot(room * 8);
            if (want_pfb) c.h_pfb = p.slot(room * 8);
            if (want_l2) c.h_l2 = p.slot(room * 8);
            if (want_snp) c.h_snp = p.slot(room);
            if (decode) { c.h_states = p.slot(room * 4); c.h_ll = p.slot(R * 8); }
        }))) return rc;
    // the tables: per-shard window offsets for the window kernel (each shard's start at 0), flat ones for the order kernels
    memcpy(h_in + L.rs, in->region_start, R * 4);
    memcpy(h_in + L.re, in->region_end, R * 4);
    int32_t *h_ss = (int32_t *)(h_in + L.ss);
    uint64_t *h_wo = (uint64_t *)(h_in + L.wo);
    uint32_t *h_wbase = (uint32_t *)(h_in + L.wbase), *h_soff = (uint32_t *)(h_in + L.soff), *h_small = (uint32_t *)(h_in + L.small), *h_big = (uint32_t *)(h_in + L.big);
    uint64_t wflat = 0;
    uint32_t n_small = 0, n_big = 0;
    for (uint64_t s = 0; s < n_sh; s++) {
        uint64_t wrel = 0;
        for (uint64_t r = in->reg_off[s]; r < in->reg_off[s + 1]; r++) {
            const uint64_t ss = std::max<uint64_t>(in->snp_off[r + 1] - in->snp_off[r], (uint64_t)in->sample_size[r]);
            h_ss[r] = (int32_t)ss; h_wo[r + s] = wrel; h_wbase[r] = (uint32_t)wflat; h_soff[r] = (uint32_t)in->snp_off[r];
            if (ss <= CN_SMALL_MAX) h_small[n_small++] = (uint32_t)r; else h_big[n_big++] = (uint32_t)r;
            wrel += ss; wflat += ss;
        }
        h_wo[in->reg_off[s + 1] + s] = wrel;
    }
    h_wbase[R] = (uint32_t)W; h_soff[R] = (uint32_t)S;
    if (S) { memcpy(h_in + L.spos, in->snp_pos, S * 4); memcpy(h_in + L.sbaf, in->snp_baf, S * 8); memcpy(h_in + L.spfb, in->snp_pfb, S * 8); }

    hipStream_t st = ctx->stream;
    char *d_in = c.w.in;
    CSV_HIP(ctx, hipMemcpyAsync(d_in, h_in, L.bytes, hipMemcpyHostToDevice, st));
    CSV_HIP(ctx, hipMemsetAsync(c.w.sl.tot, 0, (R + 1) * 4, st));
    {
        TimerScope ts(ctx, CSV_K_WINDOW);
        for (uint64_t s = 0; s < n_sh; s++) {
            const uint64_t r0 = in->reg_off[s], nr = in->reg_off[s + 1] - r0;
            if (!nr) continue;
            const uint64_t w0 = h_wbase[r0], nw = h_wo[r0 + nr + s];
            launch_window_log2(st, in->shards[s]->depth, in->shards[s]->depth_len, (const uint32_t *)(d_in + L.rs) + r0, (const uint32_t *)(d_in + L.re) + r0,
                               (const int32_t *)(d_in + L.ss) + r0, (const uint64_t *)(d_in + L.wo) + r0 + s, nr, nw, in->mean_cov[s], c.w.l2 + w0, c.w.ws + w0, c.w.we + w0);
        }
        launch_cn_order(st, c.w.ws, c.w.we, (const uint32_t *)(d_in + L.wbase), (const uint32_t *)(d_in + L.soff), (const uint32_t *)(d_in + L.spos),
                        (const uint32_t *)(d_in + L.small), n_small, (const uint32_t *)(d_in + L.big), n_big, ep, c.w.sl);
        launch_exclusive_sum_u32(st, c.w.sl.tot, R + 1, c.w.es_tmp);
        launch_cn_fill(st, c.w.sl, (uint32_t)W, (uint32_t)R, c.w.sl.tot, c.w.ws, c.w.we, c.w.l2, (const uint32_t *)(d_in + L.spos), (const double *)(d_in + L.sbaf),
                       (const double *)(d_in + L.spfb), c.w.o);
    }
    CSV_HIP(ctx, hipMemcpyAsync(h_total, c.w.o.obs_off + R, 8, hipMemcpyDeviceToHost, st));
    CSV_HIP(ctx, wait_stream(st));
    c.total = *h_total;
    if (c.total > c.bound) { ctx->err = std::string(what) + ": more observations than the bound"; return CSV_EHIP; }
    return CSV_OK;
}

// the answer's arrays to the page-locked block (queued; the caller waits and finishes)
int cn_download(csv_ctx *ctx, CnCall &c, uint64_t *obs_off, uint32_t *pos, double *baf, double *pfb, double *log2_cov, uint8_t *is_snp)
{
    hipStream_t st = ctx->stream;
    const uint64_t n = c.total;
    struct Down { void *dst, *pin; const void *src; size_t bytes; };
    const Down down[] = {{obs_off, c.h_off, c.w.o.obs_off, (c.R + 1) * 8}, {pos, c.h_pos, c.w.o.pos, n * 4}, {baf, c.h_baf, c.w.o.baf, n * 8},
                         {pfb, c.h_pfb, c.w.o.pfb, n * 8}, {log2_cov, c.h_l2, c.w.o.log2_cov, n * 8}, {is_snp, c.h_snp, c.w.o.is_snp, n}};
    for (const Down &d : down) {
        if (!d.dst || !d.pin) continue;
        CSV_HIP(ctx, hipMemcpyAsync(d.pin, d.src, d.bytes, hipMemcpyDeviceToHost, st));
        c.pin.outs.push_back(PinStage::Out{d.dst, d.pin, d.bytes});
    }
    return CSV_OK;
}
}  // namespace

int csvgpu_cn_observations_resident_many(csv_ctx *ctx, const csv_cn_regions *in, uint64_t *obs_off, uint32_t *pos, double *baf, double *pfb,
                                         double *log2_cov, uint8_t *is_snp, uint64_t *n_obs)
{
    if (!ctx) return CSV_EINVAL;
    const char *what = "cn_observations";
    if (!obs_off) { ctx->err = std::string(what) + ": null array"; return CSV_EINVAL; }
    if (n_obs && *n_obs && (!pos || !baf || !pfb || !log2_cov || !is_snp)) { ctx->err = std::string(what) + ": null array with a capacity"; return CSV_EINVAL; }
    CnCall c;
    int rc = cn_run(ctx, what, in, false, true, true, true, true, n_obs, c);
    if (rc) return rc;
    *n_obs = c.total;
    if (c.R == 0) { obs_off[0] = 0; return CSV_OK; }
    if (c.total > c.cap) { ctx->err = std::string(what) + ": capacity too small"; return CSV_ECAPACITY; }
    if ((rc = cn_download(ctx, c, obs_off, pos, baf, pfb, log2_cov, is_snp))) return rc;
    CSV_HIP(ctx, wait_stream(ctx->stream));
    c.pin.finish();
    return CSV_OK;
}

int csvgpu_cn_decode_resident_many(csv_ctx *ctx, const csv_cn_regions *in, const csv_hmm *hmm, uint64_t *obs_off, uint32_t *pos, int32_t *states,
                                   double *loglik, double *baf, double *pfb, double *log2_cov, uint8_t *is_snp, uint64_t *n_obs)
{
    if (!ctx) return CSV_EINVAL;
    const char *what = "cn_decode";
    if (!hmm) { ctx->err = std::string(what) + ": null hmm"; return CSV_EINVAL; }
    if (!obs_off || !loglik) { ctx->err = std::string(what) + ": null array"; return CSV_EINVAL; }
    if (n_obs && *n_obs && (!pos || !states)) { ctx->err = std::string(what) + ": null array with a capacity"; return CSV_EINVAL; }
    CnCall c;
    int rc = cn_run(ctx, what, in, true, baf != nullptr, pfb != nullptr, log2_cov != nullptr, is_snp != nullptr, n_obs, c);
    if (rc) return rc;
    *n_obs = c.total;
    if (c.R == 0) { obs_off[0] = 0; return CSV_OK; }
    if (c.total > c.cap) { ctx->err = std::string(what) + ": capacity too small"; return CSV_ECAPACITY; }
    if ((rc = csvgpu_viterbi_dev(ctx, hmm, c.w.o.log2_cov, c.w.o.baf, c.w.o.pfb, c.w.o.obs_off, c.R, c.total, c.w.states, c.w.loglik))) return rc;
    if ((rc = cn_download(ctx, c, obs_off, pos, baf, pfb, log2_cov, is_snp))) return rc;
    hipStream_t st = ctx->stream;
    CSV_HIP(ctx, hipMemcpyAsync(c.h_states, c.w.states, c.total * 4, hipMemcpyDeviceToHost, st));
    CSV_HIP(ctx, hipMemcpyAsync(c.h_ll, c.w.loglik, c.R * 8, hipMemcpyDeviceToHost, st));
    c.pin.outs.push_back(PinStage::Out{states, c.h_states, c.total * 4});
    c.pin.outs.push_back(PinStage::Out{loglik, c.h_ll, c.R * 8});
    CSV_HIP(ctx, wait_stream(st));
    c.pin.finish();
    return CSV_OK;
}

extern "C" {

int csvgpu_window_log2_resident(csv_ctx *ctx, csv_shard *sh, const uint32_t *region_start, const uint32_t *region_end,
                                const int32_t *sample_size, const uint64_t *win_off, uint64_t n_regions, double mean_cov,
                                double *log2_cov, uint32_t *win_start, uint32_t *win_end)
{
    if (!ctx || !sh) return CSV_EINVAL;
    if (n_regions == 0) return CSV_OK;
    if (!region_start || !region_end || !sample_size || !win_off) { ctx->err = "window_log2: null array"; return CSV_EINVAL; }
    for (uint64_t r = 0; r < n_regions; r++) {
        if (sample_size[r] <= 0 || win_off[r + 1] - win_off[r] != (uint64_t)sample_size[r] || region_start[r] > region_end[r]) {
            ctx->err = "window_log2: bad region table"; return CSV_EINVAL;
        }
    }
    const uint64_t nw = win_off[n_regions];
    if (nw == 0) return CSV_OK;
    if (!log2_cov || !win_start || !win_end) { ctx->err = "window_log2: null output"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    WindowWs w;
    int rc = arena_reserve_for(ctx, ctx->arena, "window_log2", [&](Arena &a) { return carve_window(a, n_regions, nw, w); });
    if (rc) return rc;
    uint32_t *drs = w.rs, *dre = w.re, *dws = w.ws, *dwe = w.we;
    int32_t *dss = w.ss;
    uint64_t *dwo = w.wo;
    double *dl2 = w.l2;
    hipStream_t s = ctx->stream;
    CSV_HIP(ctx, hipMemcpyAsync(drs, region_start, n_regions * 4, hipMemcpyHostToDevice, s));
    CSV_HIP(ctx, hipMemcpyAsync(dre, region_end, n_regions * 4, hipMemcpyHostToDevice, s));
    CSV_HIP(ctx, hipMemcpyAsync(dss, sample_size, n_regions * 4, hipMemcpyHostToDevice, s));
    CSV_HIP(ctx, hipMemcpyAsync(dwo, win_off, (n_regions + 1) * 8, hipMemcpyHostToDevice, s));
    if ((rc = csvgpu_window_log2_dev(ctx, sh->depth, sh->depth_len, drs, dre, dss, dwo, n_regions, nw, mean_cov, dl2, dws, dwe))) return rc;
    CSV_HIP(ctx, hipMemcpyAsync(log2_cov, dl2, nw * 8, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, hipMemcpyAsync(win_start, dws, nw * 4, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, hipMemcpyAsync(win_end, dwe, nw * 4, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, wait_stream(s));
    return CSV_OK;
}

int csvgpu_depth_lookup_resident(csv_ctx *ctx, csv_shard *sh, const uint32_t *pos, uint64_t n, int32_t *depth_out)
{
    if (!ctx || !sh) return CSV_EINVAL;
    if (n == 0) return CSV_OK;
    if (!pos || !depth_out) { ctx->err = "depth_lookup: null array"; return CSV_EINVAL; }
    if (!sh->depth) { ctx->err = "depth_lookup: shard has no depth map (run csvgpu_chr_pipeline_dev first)"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    uint32_t *dpos = nullptr;
    int32_t *dout = nullptr;
    int rc = arena_reserve_for(ctx, ctx->arena, "depth_lookup", [&](Arena &a) { return take(a, dpos, n * 4) && take(a, dout, n * 4); });
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    CSV_HIP(ctx, hipMemcpyAsync(dpos, pos, n * 4, hipMemcpyHostToDevice, s));
    csv::launch_depth_lookup(s, sh->depth, sh->depth_len, dpos, n, dout);
    CSV_HIP(ctx, hipMemcpyAsync(depth_out, dout, n * 4, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, wait_stream(s));
    return CSV_OK;
}

int csvgpu_chr_fetch(csv_ctx *ctx, csv_shard *sh, const csv_chr_result *res, csv_sig *host_sig, int32_t *host_labels)
{
    if (!ctx || !sh || !res) return CSV_EINVAL;
    if (res->n_sig == 0) return CSV_OK;
    if (!host_sig || !host_labels) { ctx->err = "chr_fetch: null output"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    CSV_HIP(ctx, hipMemcpyAsync(host_sig, res->sig_del, res->n_sig * sizeof(csv_sig), hipMemcpyDeviceToHost, ctx->stream));
    CSV_HIP(ctx, hipMemcpyAsync(host_labels, res->label_del, res->n_sig * sizeof(int32_t), hipMemcpyDeviceToHost, ctx->stream));
    CSV_HIP(ctx, wait_stream(ctx->stream));
    return CSV_OK;
}

int csvgpu_download(csv_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes)
{
    if (!ctx || (bytes && (!host_dst || !dev_src))) return CSV_EINVAL;
    if (!bytes) return CSV_OK;
    (void)hipSetDevice(ctx->device);
    CSV_HIP(ctx, hipMemcpyAsync(host_dst, dev_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    CSV_HIP(ctx, wait_stream(ctx->stream));
    return CSV_OK;
}

csv_gate *csvgpu_gate_create(void) { return new (std::nothrow) csv_gate(); }

// Creates the gate's stream now instead of at the first job. The runtime deals its hardware queues (four by default) to streams in
// creation order, and a stream that waits for an event holds up every other stream of its hardware queue: a gate opened BEFORE the lanes'
// contexts are created shares its queue with none of the first lanes' streams.
int csvgpu_gate_open(csv_gate *gate, int device_ordinal)
{
    if (!gate) return CSV_EINVAL;
    if (gate->stream) return gate->device == device_ordinal ? CSV_OK : CSV_EINVAL;
    if (hipSetDevice(device_ordinal) != hipSuccess) { (void)hipGetLastError(); return CSV_ENODEV; }
    if (hipStreamCreateWithFlags(&gate->stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); gate->stream = nullptr; return CSV_EHIP; }
    gate->device = device_ordinal;
    return CSV_OK;
}

void csvgpu_gate_destroy(csv_gate *gate)
{
    if (!gate) return;
    if (gate->stream) { (void)hipSetDevice(gate->device); (void)hipStreamSynchronize(gate->stream); (void)hipStreamDestroy(gate->stream); }
    delete gate;
}

int csvgpu_set_gate(csv_ctx *ctx, csv_gate *gate)
{
    if (!ctx) return CSV_EINVAL;
    ctx->gate = gate;
    return CSV_OK;
}

void *csvgpu_host_alloc(csv_ctx *ctx, size_t bytes)
{
    if (!ctx || !bytes) return nullptr;
    for (size_t i = 0; i < ctx->host_pool.size(); i++) {
        if (ctx->host_pool[i].second >= bytes && ctx->host_pool[i].second <= 2 * bytes + 4096) {
            ctx->host_live.push_back(ctx->host_pool[i]);
            ctx->host_pool.erase(ctx->host_pool.begin() + (std::ptrdiff_t)i);
            return ctx->host_live.back().first;
        }
    }
    (void)hipSetDevice(ctx->device);
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); ctx->err = "hipHostMalloc failed"; return nullptr; }
    ctx->host_live.emplace_back(p, bytes);
    return p;
}

void csvgpu_host_free(csv_ctx *ctx, void *p)
{
    if (!ctx || !p) return;
    for (size_t i = 0; i < ctx->host_live.size(); i++) {
        if (ctx->host_live[i].first != p) continue;
        ctx->host_pool.push_back(ctx->host_live[i]);
        ctx->host_live.erase(ctx->host_live.begin() + (std::ptrdiff_t)i);
        while (ctx->host_pool.size() > 8) {                // bounded: drop the oldest
            (void)hipHostFree(ctx->host_pool.front().first);
            ctx->host_pool.erase(ctx->host_pool.begin());
        }
        return;
    }
}

// ---- one chromosome as a job in three steps, so that the caller can queue the scan + depth pass of the next chromosome before it
// waits for this one's results (the device then never idles across the host's turn-around) ----
struct csv_job {
    csv_shard *sh = nullptr;
    uint32_t min_oplen = 50; uint8_t min_mapq = 20; double min_pts_pct = 0.1;
    hipEvent_t ev_zero = nullptr, ev_scan = nullptr, ev_depth = nullptr, ev_mid = nullptr, ev_done = nullptr, t0 = nullptr;
    bool on_gate = false;                // the pair runs on a gate's stream: this context's stream meets it only in job_cluster (ev_depth)
    char *pin = nullptr;                 // 512 B page-locked: [0,256) counters behind the scan, [256,512) counters at the end
    bool depth_queued = false, clustered = false, copied = false;
    uint64_t n = 0, n_del = 0, capacity = 0;
    csv_sig *sig_sorted = nullptr;
    int32_t *labels = nullptr;
};

// CSV_MAX_JOBS rotating 512-byte page-locked slots per context; a slot belongs to its job from begin to end / abort, so a caller
// that holds more than CSV_MAX_JOBS jobs open on one context is refused instead of aliasing another job's counters.
static char *job_pin_slot(csv_ctx *ctx)
{
    constexpr size_t kSlots = CSV_MAX_JOBS, kSlot = 512;
    if (!ctx->job_pin && hipHostMalloc((void **)&ctx->job_pin, kSlots * kSlot, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    for (size_t k = 0; k < kSlots; k++) {
        const size_t i = (ctx->job_pin_next + k) % kSlots;
        if (ctx->job_pin_busy & (1u << i)) continue;
        ctx->job_pin_busy |= 1u << i;
        ctx->job_pin_next = i + 1;
        return ctx->job_pin + i * kSlot;
    }
    return nullptr;
}
static void job_pin_release(csv_ctx *ctx, char *p)
{
    if (!p || !ctx->job_pin) return;
    ctx->job_pin_busy &= ~(1u << (size_t)((p - ctx->job_pin) / 512));
}

// scan (+ counters on their way to the host + depth pass, when the shard's sortedness is known). For a coordinate-sorted shard the
// device sees scan -> depth tiles back to back: the scan leaves the bucket counts and the tiles' candidate ranges behind, the
// counters travel beside the depth pass, and everything small (offsets, scatter, ranking, clustering) is queued behind it.
// With a gate, the scan + depth pairs of all attached contexts go onto the gate's one stream — back to back in queue order, no
// hand-over between queues — while each context's own (higher-priority) stream runs its small kernels beside the other lane's pair.
static int job_queue_front(csv_ctx *ctx, csv_job *job)
{
    csv_shard *sh = job->sh;
    hipStream_t s = ctx->stream;
    ScanCounters *cnt = (ScanCounters *)sh->counters;
    int rc;
    const bool sorted = sh->unsorted == 0;
    if (!job->ev_scan) job->ev_scan = get_event(ctx);          // (handed to the timers by an earlier pass of this job)
    if (!job->ev_depth) job->ev_depth = get_event(ctx);
    if (!job->ev_scan || !job->ev_depth) { ctx->err = "job: cannot allocate events"; return CSV_ENOMEM; }
    CSV_HIP(ctx, hipMemsetAsync(cnt, 0, sorted ? sh->counters_bytes : kCntBytes, s));
    csv_gate *gate = sorted ? ctx->gate : nullptr;
    hipStream_t big = s;
    std::unique_lock<std::mutex> turn;
    if (gate) {
        turn = std::unique_lock<std::mutex>(gate->mu);
        // (stream priorities — this stream low, the contexts' own high — measured 2 % slower: a small kernel waits for a whole
        // workgroup slot of the resident big kernel either way)
        if (!gate->stream) {
            if (hipStreamCreateWithFlags(&gate->stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); gate->stream = nullptr; }
            gate->device = ctx->device;
        }
        if (gate->stream && gate->device == ctx->device) {
            big = gate->stream;
            CSV_HIP(ctx, hipEventRecord(job->ev_zero, s));                 // the pair starts behind this context's memset (and whatever it was queued behind)
            CSV_HIP(ctx, hipStreamWaitEvent(big, job->ev_zero, 0));
        }
    }
    // On the gate's stream every recorded event is a barrier packet between the big kernels of ALL lanes (~5 us each): the pair is
    // timed with the two events the job records there anyway plus one in front (scan = ev_scan - t0, depth = ev_depth - ev_scan).
    // (at level 2 only every fourth pair: the extra event in front of the scan is a barrier packet on the stream all lanes share, 2.5 % of
    // the throughput when every pair has one; the averages are over the timed pairs)
    if (job->t0) { ctx->event_pool.push_back(job->t0); job->t0 = nullptr; }          // (a re-run after the signature buffer grew)
    const bool pair_timers = big != s && ctx->timing != 0 && (ctx->timing == 1 || ctx->timing == 3 || (ctx->timer_tick++ & 3u) == 0);
    hipEvent_t t0 = nullptr;
    if (pair_timers) {
        t0 = get_event(ctx);
        if (t0) CSV_HIP(ctx, hipEventRecord(t0, big));
        launch_cigar_scan(big, ctx->n_cu, sh->d, sh->depth_len, job->min_oplen, job->min_mapq, 1, sh->sig_raw, sh->sig_cap, sh->ref_end,
                          sh->q_start, sh->q_end, sh->ckpt, cnt, scan_extras(cnt, sh->depth_len, true, sh->tile_range), sh->owned ? sh->scan_split : nullptr, sh->form, sh->cigar_pad);
    } else if (big != s) {                  // on the gate's stream, not a timed pair: no events of its own
        launch_cigar_scan(big, ctx->n_cu, sh->d, sh->depth_len, job->min_oplen, job->min_mapq, 1, sh->sig_raw, sh->sig_cap, sh->ref_end,
                          sh->q_start, sh->q_end, sh->ckpt, cnt, scan_extras(cnt, sh->depth_len, true, sh->tile_range), sh->owned ? sh->scan_split : nullptr, sh->form, sh->cigar_pad);
    } else {
        TimerScope ts(ctx, CSV_K_CIGAR_SCAN, big);
        launch_cigar_scan(big, ctx->n_cu, sh->d, sh->depth_len, job->min_oplen, job->min_mapq, 1, sh->sig_raw, sh->sig_cap, sh->ref_end,
                          sh->q_start, sh->q_end, sh->ckpt, cnt, scan_extras(cnt, sh->depth_len, true, sorted ? sh->tile_range : nullptr), sh->owned ? sh->scan_split : nullptr, sh->form, sh->cigar_pad);
    }
    job->depth_queued = false;
    if (sh->unsorted >= 0) {
        // The depth pass does not depend on the signature count, so it is queued BEFORE the host waits for the counters: the
        // device works through it while the host wakes up, sizes the ordering and clustering launches and queues them.
        job->on_gate = big != s;
        if (job->on_gate) {
            // On a gate nothing of this job touches the context's own stream until job_cluster: a caller that queues several jobs ahead must
            // not find one job's clustering kernels behind a wait for a LATER job's scan. The counters leave from the gate's stream itself,
            // between the two big kernels (256 bytes to page-locked memory), ev_scan tells the host they have landed, and job_cluster makes
            // the context's stream wait for ev_depth before min_pts. (A relay through a side stream per context was tried: three more
            // streams whose only work is to wait share the four hardware queues with everything else and stalled the caller's context.)
            CSV_HIP(ctx, hipMemcpyAsync(job->pin, cnt, sizeof(ScanCounters), hipMemcpyDeviceToHost, big));
            CSV_HIP(ctx, hipEventRecord(job->ev_scan, big));
            launch_depth_tiles(big, sh->d, nullptr, sh->ref_end, sh->ckpt, sh->depth_len, sh->depth, cnt, sh->tile_range, sh->cigar_pad, sh->depth_items, sh->form);
            CSV_HIP(ctx, hipEventRecord(job->ev_depth, big));
            turn.unlock();
            job->t0 = pair_timers ? t0 : nullptr;            // (handed to the timers with ev_scan / ev_depth when the job ends)
        } else {
            // The counters leave on a side stream beside the depth pass.
            if (!ctx->side) CSV_HIP(ctx, hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
            hipStream_t cs = ctx->side;
            CSV_HIP(ctx, hipEventRecord(job->ev_scan, big));
            CSV_HIP(ctx, hipStreamWaitEvent(cs, job->ev_scan, 0));
            CSV_HIP(ctx, hipMemcpyAsync(job->pin, cnt, sizeof(ScanCounters), hipMemcpyDeviceToHost, cs));
            CSV_HIP(ctx, hipEventRecord(job->ev_mid, cs));
            DepthWs dw;
            if ((rc = depth_work(ctx, sh, &dw))) return rc;
            if ((rc = depth_chain(ctx, dw, sh->d, sh->ref_end, sh->ckpt, sh->unsorted != 0, sh->depth_len, sh->depth, cnt,
                                  sorted ? sh->tile_range : nullptr, sh->cigar_pad, sh->depth_items, sh->form))) return rc;
            launch_min_pts(s, cnt, job->min_pts_pct);
        }
        job->depth_queued = true;
    }
    return CSV_OK;
}

static void job_free(csv_ctx *ctx, csv_job *job)
{
    if (!job) return;
    job_pin_release(ctx, job->pin);
    if (job->t0 && job->ev_scan && job->ev_depth && job->on_gate && ctx->gate && ctx->gate->stream) {
        // a timed pair on the gate's stream: scan = ev_scan - t0 (the 256-byte counters copy included), depth = ev_depth - ev_scan; the
        // timers own the three events from here (folded when the times are read)
        Timer a; a.id = CSV_K_CIGAR_SCAN; a.a = job->t0; a.b = job->ev_scan; a.s = ctx->gate->stream;
        Timer b; b.id = CSV_K_DEPTH; b.a = job->ev_scan; b.b = job->ev_depth; b.s = ctx->gate->stream; b.own_a = false;
        ctx->timers.push_back(a); ctx->timers.push_back(b);
        job->t0 = nullptr; job->ev_scan = nullptr; job->ev_depth = nullptr;
    }
    if (job->t0) ctx->event_pool.push_back(job->t0);
    if (job->ev_zero) ctx->event_pool.push_back(job->ev_zero);
    if (job->ev_scan) ctx->event_pool.push_back(job->ev_scan);
    if (job->ev_depth) ctx->event_pool.push_back(job->ev_depth);
    if (job->ev_mid) ctx->event_pool.push_back(job->ev_mid);
    if (job->ev_done) ctx->event_pool.push_back(job->ev_done);
    delete job;
}

csv_job *csvgpu_chr_job_begin(csv_ctx *ctx, csv_shard *sh, uint32_t min_oplen, uint8_t min_mapq, double min_pts_pct)
{
    if (!ctx || !sh) return nullptr;
    (void)hipSetDevice(ctx->device);
    csv_job *job = new (std::nothrow) csv_job();
    if (!job) { ctx->err = "out of host memory"; return nullptr; }
    job->sh = sh; job->min_oplen = min_oplen; job->min_mapq = min_mapq; job->min_pts_pct = min_pts_pct;
    job->ev_zero = get_event(ctx); job->ev_scan = get_event(ctx); job->ev_depth = get_event(ctx); job->ev_mid = get_event(ctx); job->ev_done = get_event(ctx);
    job->pin = job_pin_slot(ctx);
    if (!job->pin && ctx->job_pin) { ctx->err = "job: more than CSV_MAX_JOBS jobs open on this context"; job_free(ctx, job); return nullptr; }
    if (!job->pin || !job->ev_zero || !job->ev_scan || !job->ev_depth || !job->ev_mid || !job->ev_done) { ctx->err = "job: cannot allocate events / page-locked memory"; job_free(ctx, job); return nullptr; }
    if (depth_work(ctx, sh, nullptr) || job_queue_front(ctx, job)) { job_free(ctx, job); return nullptr; }
    return job;
}

int csvgpu_chr_job_cluster(csv_ctx *ctx, csv_job *job, double eps, csv_sig *host_sig, int32_t *host_labels, uint64_t capacity)
{
    if (!ctx || !job || job->clustered) return CSV_EINVAL;
    if (!(eps >= 0.0) || !(eps < 1.0)) { ctx->err = "pipeline: eps must be in [0,1)"; return CSV_EINVAL; }
    if (capacity && (!host_sig || !host_labels)) { ctx->err = "pipeline: null output"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    csv_shard *sh = job->sh;
    hipStream_t s = ctx->stream;
    ScanCounters *cnt = (ScanCounters *)sh->counters;
    ScanCounters h;
    int rc;
    for (int attempt = 0;; attempt++) {
        if (job->depth_queued) {
            CSV_HIP(ctx, wait_event(job->on_gate ? job->ev_scan : job->ev_mid));
            memcpy(&h, job->pin, sizeof(ScanCounters));
        } else {
            if ((rc = read_counters(ctx, cnt, h))) return rc;             // first scan of wrapped arrays: wait, then decide
            sh->unsorted = h.unsorted != 0;
        }
        if (h.n_sig <= sh->sig_cap) break;
        if (attempt) { ctx->err = "pipeline: signature buffer overflow twice"; return CSV_ENOMEM; }
        CSV_HIP(ctx, wait_stream(s));                            // the queued depth pass reads what the re-run scan rewrites
        // the larger buffer first: if it cannot be had, the shard keeps its old buffer AND its old capacity (a later job on this
        // shard must never see a capacity without a buffer behind it — the scan's `g < sig_cap` guard would write through null)
        const uint64_t new_cap = h.n_sig + h.n_sig / 8 + 1024;
        csv_sig *bigger = nullptr;
        if (csv_test_fail_alloc() || hipMalloc((void **)&bigger, new_cap * sizeof(csv_sig)) != hipSuccess) {
            (void)hipGetLastError();
            ctx->err = "hipMalloc failed (signature buffer)";
            return CSV_ENOMEM;
        }
        (void)hipFree(sh->sig_raw);
        sh->sig_raw = bigger; sh->sig_cap = new_cap;
        if ((rc = job_queue_front(ctx, job))) return rc;
    }
    const uint64_t n = h.n_sig, n_del = h.n_del;
    const uint32_t max_bucket = h.max_len;

    // shard scratch: sorted signatures, SoA start/end, labels, sort + dbscan workspace (grow-only)
    JobScratch js;
    const size_t need = arena_plan_bytes([&](Arena &a) { return carve_job_scratch(a, n, js); });
    if (need > sh->scratch_cap) {
        if (sh->scratch) CSV_HIP(ctx, hipFree(sh->scratch));
        sh->scratch = nullptr; sh->scratch_cap = 0;
        CSV_HIP(ctx, hipMalloc((void **)&sh->scratch, need + need / 4));
        sh->scratch_cap = need + need / 4;
    }
    Arena sa; sa.base = sh->scratch; sa.cap = sh->scratch_cap; sa.used = 0;
    if (!carve_job_scratch(sa, n, js)) { ctx->err = "shard scratch exhausted"; return CSV_ENOMEM; }
    csv_sig *sig_sorted = js.sig_sorted;
    uint32_t *st = js.st, *en = js.en;
    int32_t *labels = js.labels;
    SortWs &w = js.w;
    void *db_tmp = js.db_tmp;

    // depth map + mean coverage + min_pts (device scalar), unless already queued behind the scan
    if (!job->depth_queued) {
        DepthWs dw;
        if ((rc = depth_work(ctx, sh, &dw))) return rc;
        if ((rc = depth_chain(ctx, dw, sh->d, sh->ref_end, sh->ckpt, sh->unsorted != 0, sh->depth_len, sh->depth, cnt, nullptr, sh->cigar_pad, sh->depth_items, sh->form))) return rc;
        launch_min_pts(s, cnt, job->min_pts_pct);
    }

    // ordering: DEL calls then INS calls, each in chr_sv_calls order
    order_signatures(ctx, sh->sig_raw, n, sh->depth_len, h.max_start, max_bucket, cnt, true, w, sig_sorted, st, en);

    // min_pts (and with it the clustering) reads what the depth pass leaves; the ordering above did not have to wait for it
    if (job->depth_queued && job->on_gate) {
        CSV_HIP(ctx, hipStreamWaitEvent(s, job->ev_depth, 0));
        launch_min_pts(s, cnt, job->min_pts_pct);
    }
    // per-type interval DBSCAN (mergeSVs walks DEL ... INS, sv_object.cpp:62-68)
    {
        TimerScope ts(ctx, CSV_K_DBSCAN);
        // DEL calls [0, n_del) and INS calls [n_del, n) are clustered side by side in the same five launches
        if (n) launch_dbscan_iv_sorted(s, st, en, nullptr, n, n_del, eps, 0, &cnt->min_pts, labels, db_tmp);
    }
    job->copied = capacity && n && n <= capacity;
    if (job->copied) {                                                   // results ride behind the last kernel, one wait for everything
        CSV_HIP(ctx, hipMemcpyAsync(host_sig, sig_sorted, n * sizeof(csv_sig), hipMemcpyDeviceToHost, s));
        CSV_HIP(ctx, hipMemcpyAsync(host_labels, labels, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    CSV_HIP(ctx, hipMemcpyAsync(job->pin + 256, cnt, sizeof(ScanCounters), hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, hipEventRecord(job->ev_done, s));
    job->n = n; job->n_del = n_del; job->capacity = capacity; job->sig_sorted = sig_sorted; job->labels = labels;
    job->clustered = true;
    return CSV_OK;
}

int csvgpu_chr_job_end(csv_ctx *ctx, csv_job *job, csv_chr_result *res)
{
    if (!ctx || !job) return CSV_EINVAL;
    (void)hipSetDevice(ctx->device);
    int rc = CSV_OK;
    if (!job->clustered) { ctx->err = "job_end before job_cluster"; rc = CSV_EINVAL; }
    else if (wait_event(job->ev_done) != hipSuccess) { (void)hipGetLastError(); ctx->err = "job: device error"; rc = CSV_EHIP; }
    else if (res) {
        ScanCounters h;
        memcpy(&h, job->pin + 256, sizeof(ScanCounters));
        csv_shard *sh = job->sh;
        res->n_sig = job->n; res->n_del = job->n_del; res->n_ins = job->n - job->n_del;
        res->depth_sum = h.depth_sum; res->depth_nonzero = h.depth_nonzero; res->min_pts = h.min_pts; res->mean_cov = h.mean_cov;
        res->sig_del = job->sig_sorted; res->sig_ins = job->sig_sorted + job->n_del;
        res->label_del = job->labels; res->label_ins = job->labels + job->n_del;
        res->depth = sh->depth; res->ref_end = sh->ref_end; res->q_start = sh->q_start; res->q_end = sh->q_end;
        if (job->capacity && job->n > job->capacity) { ctx->err = "pipeline_fetch: host buffers too small"; rc = CSV_ECAPACITY; }
    }
    job_free(ctx, job);
    return rc;
}

int csvgpu_chr_job_abort(csv_ctx *ctx, csv_job *job)
{
    if (!ctx || !job) return CSV_EINVAL;
    (void)hipSetDevice(ctx->device);
    // whatever the job queued reads the shard's buffers: let it drain before the caller reuses or frees them
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->gate && ctx->gate->stream) (void)hipStreamSynchronize(ctx->gate->stream);
    if (ctx->side) (void)hipStreamSynchronize(ctx->side);
    job_free(ctx, job);                                  // ctx->err keeps the failure that led here
    return CSV_OK;
}

#ifdef CSV_TEST_HOOKS
// Test hook (error-path tests): the next n device allocations guarded by csv_test_fail_alloc() fail.
void csvgpu_test_fail_next_alloc(int n) { csv::g_fail_alloc.store(n); }

// Test hooks (tests/test_gpu_sort_primitives.py): the device primitives of sort.hip and launch_prefix_max, called unchanged on staged
// host arrays. The whole arena is filled with a sentinel byte before the inputs go in — the workspace starts as the garbage a chain
// leaves in it — and every buffer a primitive may write has CSVGPU_TEST_GUARD spare elements behind it that must keep the sentinel.
static constexpr int kHookFill = 0xA5;
static int hook_region_clean(csv_ctx *ctx, const void *dev, size_t bytes, bool &clean)
{
    std::vector<unsigned char> h(bytes);
    if (bytes) CSV_HIP(ctx, hipMemcpyAsync(h.data(), dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    CSV_HIP(ctx, wait_stream(ctx->stream));
    for (unsigned char b : h) if (b != kHookFill) { clean = false; break; }
    return CSV_OK;
}

// room slots per ping-pong buffer (+ the guard), a workspace of radix_sort_tmp_bytes(room) exactly (+ a guard); n pairs staged
static int hook_sort_stage(csv_ctx *ctx, const uint64_t *keys, const uint32_t *vals, uint64_t n, uint64_t room, SortWs &w, void *&tmp_guard, uint32_t *&d_n)
{
    const uint64_t m = room + CSVGPU_TEST_GUARD;
    Arena &a = ctx->arena;
    const int rc = arena_reserve_for(ctx, a, "test hook", [&](Arena &p) {
        return sortws_carve(p, m, w) &&
               take(p, w.tmp, radix_sort_tmp_bytes(room)) &&      // (not the one carved for m slots: the size a chain gives a sort of `room` keys)
               take(p, tmp_guard, CSVGPU_TEST_GUARD) && take(p, d_n, 256);
    });
    if (rc) return rc;
    CSV_HIP(ctx, hipMemsetAsync(a.base, kHookFill, a.used, ctx->stream));
    if (n) {
        CSV_HIP(ctx, hipMemcpyAsync(w.k0, keys, n * 8, hipMemcpyHostToDevice, ctx->stream));
        CSV_HIP(ctx, hipMemcpyAsync(w.v0, vals, n * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    return CSV_OK;
}

// result pair, flag word and the state of slots [n, room + guard) of all four buffers and of the workspace's guard
static int hook_sort_collect(csv_ctx *ctx, const SortWs &w, const void *tmp_guard, int io, uint64_t n, uint64_t room, const uint32_t *flag,
                             uint64_t *keys_out, uint32_t *vals_out, uint32_t *gave_up, int32_t *tail_ok)
{
    CSV_HIP(ctx, hipGetLastError());
    *gave_up = 0;
    if (n) {
        CSV_HIP(ctx, hipMemcpyAsync(keys_out, io ? w.k1 : w.k0, n * 8, hipMemcpyDeviceToHost, ctx->stream));
        CSV_HIP(ctx, hipMemcpyAsync(vals_out, io ? w.v1 : w.v0, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (flag) CSV_HIP(ctx, hipMemcpyAsync(gave_up, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    const uint64_t tail = room + CSVGPU_TEST_GUARD - n;
    bool clean = true;
    int rc;
    if ((rc = hook_region_clean(ctx, w.k0 + n, tail * 8, clean)) || (rc = hook_region_clean(ctx, w.k1 + n, tail * 8, clean)) ||
        (rc = hook_region_clean(ctx, w.v0 + n, tail * 4, clean)) || (rc = hook_region_clean(ctx, w.v1 + n, tail * 4, clean)) ||
        (rc = hook_region_clean(ctx, tmp_guard, CSVGPU_TEST_GUARD, clean))) return rc;
    *tail_ok = clean ? 1 : 0;
    return CSV_OK;
}

int csvgpu_test_radix_sort(csv_ctx *ctx, const uint64_t *keys, const uint32_t *vals, uint64_t n, int32_t key_bits, int32_t onesweep,
                           uint64_t *keys_out, uint32_t *vals_out, uint32_t *gave_up, int32_t *tail_ok)
{
    if (!ctx) return CSV_EINVAL;
    if (!gave_up || !tail_ok || (n && (!keys || !vals || !keys_out || !vals_out))) { ctx->err = "test_radix_sort: null array"; return CSV_EINVAL; }
    if (n >= (1ull << 30) || key_bits < 1 || key_bits > 64) { ctx->err = "test_radix_sort: n or key_bits out of range"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    SortWs w; void *tmp_guard; uint32_t *d_n;
    int rc = hook_sort_stage(ctx, keys, vals, n, n, w, tmp_guard, d_n);
    if (rc) return rc;
    const int io = launch_radix_sort_u64(ctx->stream, w.k0, w.v0, w.k1, w.v1, n, key_bits, w.tmp, onesweep != 0);
    return hook_sort_collect(ctx, w, tmp_guard, io, n, n, radix_sort_gave_up(w.tmp, n, key_bits, onesweep != 0), keys_out, vals_out, gave_up, tail_ok);
}

int csvgpu_test_radix_sort_devn(csv_ctx *ctx, const uint64_t *keys, const uint32_t *vals, uint64_t n, uint64_t n_bound, int32_t key_bits,
                                uint64_t *keys_out, uint32_t *vals_out, uint32_t *gave_up, int32_t *tail_ok)
{
    if (!ctx) return CSV_EINVAL;
    if (!gave_up || !tail_ok || (n && (!keys || !vals || !keys_out || !vals_out))) { ctx->err = "test_radix_sort_devn: null array"; return CSV_EINVAL; }
    if (n > n_bound || key_bits < 1 || key_bits > 64) { ctx->err = "test_radix_sort_devn: n above n_bound, or key_bits out of range"; return CSV_EINVAL; }
    if (n_bound >= (1ull << 30)) {
        // Buffers of that many slots are not staged: the launcher is asked with none, and has to refuse before it touches one.
        if (launch_radix_sort_u64_devn(ctx->stream, nullptr, nullptr, nullptr, nullptr, n_bound, nullptr, key_bits, nullptr) < 0) {
            ctx->err = "test_radix_sort_devn: n_bound refused by the launcher"; return CSV_EINVAL;
        }
        ctx->err = "test_radix_sort_devn: the launcher took an n_bound of 2^30 or more"; return CSV_EHIP;
    }
    (void)hipSetDevice(ctx->device);
    SortWs w; void *tmp_guard; uint32_t *d_n;
    int rc = hook_sort_stage(ctx, keys, vals, n, n_bound, w, tmp_guard, d_n);
    if (rc) return rc;
    const uint32_t n32 = (uint32_t)n;
    CSV_HIP(ctx, hipMemcpyAsync(d_n, &n32, 4, hipMemcpyHostToDevice, ctx->stream));
    const int io = launch_radix_sort_u64_devn(ctx->stream, w.k0, w.v0, w.k1, w.v1, n_bound, d_n, key_bits, w.tmp);
    if (io < 0) { ctx->err = "test_radix_sort_devn: n_bound refused by the launcher"; return CSV_EINVAL; }
    return hook_sort_collect(ctx, w, tmp_guard, io, n, n_bound, radix_sort_gave_up(w.tmp, n_bound, key_bits, true), keys_out, vals_out, gave_up, tail_ok);
}

int csvgpu_test_exclusive_sum(csv_ctx *ctx, uint32_t *data, uint64_t n)
{
    if (!ctx) return CSV_EINVAL;
    if (n && !data) { ctx->err = "test_exclusive_sum: null array"; return CSV_EINVAL; }
    if (n >= (1ull << 32)) { ctx->err = "test_exclusive_sum: n out of range"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    Arena &a = ctx->arena;
    uint32_t *d = nullptr;
    void *tmp = nullptr, *tmp_guard = nullptr;
    int rc = arena_reserve_for(ctx, a, "test hook", [&](Arena &p) {
        return take(p, d, (n + CSVGPU_TEST_GUARD) * 4) && take(p, tmp, exclusive_sum_tmp_bytes(n)) && take(p, tmp_guard, CSVGPU_TEST_GUARD);
    });
    if (rc) return rc;
    CSV_HIP(ctx, hipMemsetAsync(a.base, kHookFill, a.used, ctx->stream));
    if (n) CSV_HIP(ctx, hipMemcpyAsync(d, data, n * 4, hipMemcpyHostToDevice, ctx->stream));
    launch_exclusive_sum_u32(ctx->stream, d, n, tmp);
    CSV_HIP(ctx, hipGetLastError());
    if (n) CSV_HIP(ctx, hipMemcpyAsync(data, d, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    bool clean = true;
    if ((rc = hook_region_clean(ctx, d + n, (size_t)CSVGPU_TEST_GUARD * 4, clean)) || (rc = hook_region_clean(ctx, tmp_guard, CSVGPU_TEST_GUARD, clean))) return rc;
    if (!clean) { ctx->err = "test_exclusive_sum: wrote past n"; return CSV_EHIP; }
    return CSV_OK;
}

int csvgpu_test_prefix_max(csv_ctx *ctx, const int32_t *in, uint64_t n, int32_t *out)
{
    if (!ctx) return CSV_EINVAL;
    if (n && (!in || !out)) { ctx->err = "test_prefix_max: null array"; return CSV_EINVAL; }
    if (n >= (1ull << 32)) { ctx->err = "test_prefix_max: n out of range"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    Arena &a = ctx->arena;
    int32_t *di = nullptr, *dout = nullptr;
    void *tmp = nullptr, *tmp_guard = nullptr;
    int rc = arena_reserve_for(ctx, a, "test hook", [&](Arena &p) {
        return take(p, di, n * 4) && take(p, dout, (n + CSVGPU_TEST_GUARD) * 4) && take(p, tmp, prefix_max_tmp_bytes(n)) && take(p, tmp_guard, CSVGPU_TEST_GUARD);
    });
    if (rc) return rc;
    CSV_HIP(ctx, hipMemsetAsync(a.base, kHookFill, a.used, ctx->stream));
    if (n) CSV_HIP(ctx, hipMemcpyAsync(di, in, n * 4, hipMemcpyHostToDevice, ctx->stream));
    launch_prefix_max(ctx->stream, di, dout, n, tmp);
    CSV_HIP(ctx, hipGetLastError());
    if (n) CSV_HIP(ctx, hipMemcpyAsync(out, dout, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    bool clean = true;
    if ((rc = hook_region_clean(ctx, dout + n, (size_t)CSVGPU_TEST_GUARD * 4, clean)) || (rc = hook_region_clean(ctx, tmp_guard, CSVGPU_TEST_GUARD, clean))) return rc;
    if (!clean) { ctx->err = "test_prefix_max: wrote past n"; return CSV_EHIP; }
    return CSV_OK;
}
#endif

static int chr_pipeline(csv_ctx *ctx, csv_shard *sh, uint32_t min_oplen, uint8_t min_mapq, double eps, double min_pts_pct, csv_chr_result *res,
                        csv_sig *host_sig, int32_t *host_labels, uint64_t capacity)
{
    if (!ctx || !sh || !res) return CSV_EINVAL;
    if (!(eps >= 0.0) || !(eps < 1.0)) { ctx->err = "pipeline: eps must be in [0,1)"; return CSV_EINVAL; }
    csv_job *job = csvgpu_chr_job_begin(ctx, sh, min_oplen, min_mapq, min_pts_pct);
    if (!job) return ctx->err.find("hipMalloc") != std::string::npos ? CSV_ENOMEM : CSV_EHIP;
    const int rc = csvgpu_chr_job_cluster(ctx, job, eps, host_sig, host_labels, capacity);
    if (rc) { csvgpu_chr_job_abort(ctx, job); return rc; }
    return csvgpu_chr_job_end(ctx, job, res);
}

int csvgpu_chr_pipeline_dev(csv_ctx *ctx, csv_shard *sh, uint32_t min_oplen, uint8_t min_mapq, double eps, double min_pts_pct,
                            csv_chr_result *res)
{
    return chr_pipeline(ctx, sh, min_oplen, min_mapq, eps, min_pts_pct, res, nullptr, nullptr, 0);
}

int csvgpu_chr_pipeline_fetch(csv_ctx *ctx, csv_shard *sh, uint32_t min_oplen, uint8_t min_mapq, double eps, double min_pts_pct,
                              csv_chr_result *res, csv_sig *host_sig, int32_t *host_labels, uint64_t capacity)
{
    if (capacity && (!host_sig || !host_labels)) { if (ctx) ctx->err = "pipeline_fetch: null output"; return CSV_EINVAL; }
    return chr_pipeline(ctx, sh, min_oplen, min_mapq, eps, min_pts_pct, res, host_sig, host_labels, capacity);
}

}  // extern "C"
