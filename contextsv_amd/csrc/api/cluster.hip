// cluster.hip — interval DBSCAN and 1-D DBSCAN: the windowed chain on device arrays and the five entry points.
#include "glue.hpp"

namespace csv {

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
    uint32_t *s_s = ws.s_s, *e_s = ws.e_s;
    const uint32_t *perm;
    {
        TimerScope ts(ctx, CSV_K_SORT);
        perm = sorted_perm(ctx, d_start, n, ws.w);
        launch_gather_u32(ctx->stream, d_start, perm, n, s_s);
        launch_gather_u32(ctx->stream, d_end, perm, n, e_s);
    }
    TimerScope ts(ctx, CSV_K_DBSCAN);
    launch_dbscan_iv_sorted(ctx->stream, s_s, e_s, perm, n, n, eps, min_pts, nullptr, d_labels, tmp);
    return CSV_OK;
}

int check_dbscan_args(csv_ctx *ctx, double eps, int32_t min_pts, bool interval)
{
    if (!ctx) return CSV_EINVAL;
    if (!(eps >= 0.0) || (interval && !(eps < 1.0))) { ctx->err = interval ? "dbscan: eps must be in [0,1)" : "dbscan1d: eps must be >= 0"; return CSV_EINVAL; }
    if (min_pts < 1) { ctx->err = "dbscan: min_pts must be >= 1"; return CSV_EINVAL; }
    return CSV_OK;
}

}  // namespace csv

using namespace csv;

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
    if ((rc = check_seg_off(ctx, "dbscan batch: seg_off not monotone", seg_off, n_seg, max_len))) return rc;
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
    uint32_t *ks = ws.ks;
    void *tmp = ws.tmp;
    for (uint64_t s = 0; s < n_seg; s++) {
        const uint64_t n = off[s + 1] - off[s];
        if (n <= DBSCAN1D_MAX_SEG) continue;
        if (n > max_seg_len) { ctx->err = "dbscan1d: max_seg_len smaller than a segment"; return CSV_EINVAL; }
        TimerScope ts(ctx, CSV_K_DBSCAN1D);
        const uint32_t *perm = sorted_perm(ctx, d_pts + off[s], n, ws.w);
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
    if ((rc = check_seg_off(ctx, "dbscan1d: seg_off not monotone", seg_off, n_seg, max_len))) return rc;
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
