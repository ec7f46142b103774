// testhooks.hip — what libcsvgpu_testhooks.so has and libcsvgpu.so has not: the CSV_TEST_HOOKS block of include/csvgpu.h (the Makefile defines
// the macro for this file alone, so that the block's declarations are visible) and the counting csv::test_fail_alloc(). Never shipped.
#include <atomic>

#include "glue.hpp"

namespace csv {

static std::atomic<int> g_fail_alloc{0};
bool test_fail_alloc()
{
    int n = g_fail_alloc.load();
    while (n > 0) if (g_fail_alloc.compare_exchange_weak(n, n - 1)) return true;
    return false;
}

}  // namespace csv

using namespace csv;

// Test hook (error-path tests): the next n device allocations guarded by csv::test_fail_alloc() fail.
void csvgpu_test_fail_next_alloc(int n) { g_fail_alloc.store(n); }

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
