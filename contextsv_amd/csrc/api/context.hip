// context.hip — the context of the C-ABI in include/csvgpu.h: create / destroy, tuning, the arenas, the page-locked block and the builders'
// growing arrays (DevBuf), the timers and their event pool, the gate, the caller's page-locked blocks. No CPU fallback lives in the glue:
// every result is produced by the kernels under kernels/.
#include <new>

#include "glue.hpp"

namespace csv {

static std::string g_create_err;

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

int ensure_pinned(csv_ctx *ctx, size_t bytes)
{
    if (bytes <= ctx->pinned_cap) return CSV_OK;
    if (ctx->pinned) CSV_HIP(ctx, hipHostFree(ctx->pinned));
    ctx->pinned = nullptr; ctx->pinned_cap = 0;
    CSV_HIP(ctx, hipHostMalloc(&ctx->pinned, bytes, hipHostMallocDefault));
    ctx->pinned_cap = bytes;
    return CSV_OK;
}

int devbuf_ensure(csv_ctx *ctx, DevBuf &b, uint64_t used, uint64_t need, const char *what)
{
    if (need <= b.cap) return CSV_OK;
    const uint64_t cap = std::max(need, b.cap + b.cap / 2);
    char *p = nullptr;
    if (test_fail_alloc() || hipMalloc((void **)&p, cap) != hipSuccess) { (void)hipGetLastError(); ctx->err = std::string("hipMalloc failed (") + what + " growth)"; return CSV_ENOMEM; }
    // (a new shard builder's offset arrays count their first entry as used before they exist: nothing to copy from then)
    hipError_t e = used && b.p ? hipMemcpyAsync(p, b.p, std::min(used, b.cap), hipMemcpyDeviceToDevice, ctx->stream) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { (void)hipFree(p); ctx->err = std::string(what) + " growth: " + hipGetErrorString(e); return CSV_EHIP; }
    (void)hipFree(b.p);
    b.p = p; b.cap = cap;
    return CSV_OK;
}

hipEvent_t get_event(csv_ctx *ctx)
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

}  // namespace csv

using namespace csv;

int csvgpu_abi_version(void) { return CSVGPU_ABI_VERSION; }

const char *csvgpu_last_error(const csv_ctx *ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

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

csv_ctx *csvgpu_create(int device_ordinal, void *stream) { return create_ctx(device_ordinal, stream, 0); }
csv_ctx *csvgpu_create_background(int device_ordinal) { return create_ctx(device_ordinal, nullptr, 1); }

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

int csvgpu_set_cigar_packing(csv_ctx *ctx, int on)
{
    if (!ctx) return CSV_EINVAL;
    if (ctx->job_pin_busy || ctx->split_state) { ctx->err = "set_cigar_packing: a job or a split order is open on this context"; return CSV_EINVAL; }
    if (on != 0 && on != 1) { ctx->err = "set_cigar_packing: on must be 0 or 1"; return CSV_EINVAL; }
    ctx->cigar_packing = on;
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

void *csvgpu_dev_alloc(csv_ctx *ctx, size_t bytes)
{
    if (!ctx) return nullptr;
    (void)hipSetDevice(ctx->device);
    void *p = nullptr;
    if (test_fail_alloc() || hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) { (void)hipGetLastError(); ctx->err = "hipMalloc failed (csvgpu_dev_alloc)"; return nullptr; }
    return p;
}

void csvgpu_dev_free(csv_ctx *ctx, void *dev_ptr)
{
    if (!ctx || !dev_ptr) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(dev_ptr);
}

int csvgpu_upload(csv_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes)
{
    if (!ctx || (bytes && (!dev_dst || !host_src))) return CSV_EINVAL;
    if (!bytes) return CSV_OK;
    (void)hipSetDevice(ctx->device);
    Transfer t(ctx);
    int rc = t.open("csvgpu_upload");
    if (rc || (rc = t.up(dev_dst, host_src, bytes))) return rc;
    return t.wait();
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
