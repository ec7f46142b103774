// reads.hip — a shard's reads on the device: the checks of the host arrays, their staging, and the chains behind the scan (the signatures'
// order, the depth pass) that the host-pointer entry points here and the per-chromosome job share.
#include "glue.hpp"

namespace csv {

static constexpr uint64_t kMaxReadWords = 0x7ffff000ull;       // exclusive bound on one read's CIGAR words
static inline uint32_t *bucket_off(ScanCounters *cnt) { return (uint32_t *)((char *)cnt + 256); }
static inline uint32_t *bucket_cur(ScanCounters *cnt) { return bucket_off(cnt) + BK_N; }

// copy a host shard into its carved slices (carve_reads); o: the view of them (32-bit words, no pad behind them, the form of this call)
static int stage_reads(csv_ctx *ctx, const csv_reads *r, const ReadsWs &w, ReadsView &o)
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
    o = ReadsView{*r, CigarPack(), 0, scan_form(ctx, n, m), w.ref_end, w.q_start, w.q_end, w.ckpt, w.cnt};
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
int check_reads(csv_ctx *ctx, const csv_reads *r)
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
int check_reads_dev(csv_ctx *ctx, const csv_reads *r)
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

// The scan form of a shard created, or a host-pointer call made, on this context: the forced one (csv_tuning), behind scan_form_for's guard.
int scan_form(const csv_ctx *ctx, uint64_t n_reads, uint64_t n_cigar)
{
    const int by_rule = scan_form_for(n_reads, n_cigar);
    return (ctx->tuning.scan_form == CSV_FORM_AUTO || n_cigar >= 0xffffffffull) ? by_rule : ctx->tuning.scan_form;
}

int read_counters(csv_ctx *ctx, const ScanCounters *d_cnt, ScanCounters &h)
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
ScanExtras scan_extras(ScanCounters *cnt, uint32_t depth_len, bool with_type, uint64_t *tile_range)
{
    ScanExtras x;
    const KeyLayout k = key_layout(depth_len, false, with_type);
    x.bucket_hist = bucket_off(cnt); x.type_pos = k.type_pos; x.bucket_shift = k.bucket_shift;
    x.tile_range = tile_range; x.n_tiles = tile_range ? depth_n_tiles(depth_len) : 0;
    return x;
}

void order_signatures(csv_ctx *ctx, const csv_sig *sig_raw, uint64_t n, uint32_t depth_len, uint32_t overflow, uint32_t max_bucket,
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

// depth chain on device arrays. pmax / ord / range scratch is `ws` (carve_depth); a.tile_range != nullptr: the scan already produced the
// tiles' candidate ranges (coordinate-sorted shard) and only the tile kernel remains.
int depth_chain(csv_ctx *ctx, const DepthWs &ws, const ReadsView &v, bool unsorted, DepthArgs a)
{
    const csv_reads &d = v.d;
    const uint64_t n = d.n_reads;
    TimerScope ts(ctx, CSV_K_DEPTH);
    a.ord = nullptr;
    if (n == 0 || a.depth_len == 0) {
        if (a.depth && a.depth_len) CSV_HIP(ctx, hipMemsetAsync(a.depth, 0, (size_t)a.depth_len * 4, ctx->stream));
        return CSV_OK;
    }
    if (a.tile_range && !unsorted) {
        launch_depth_tiles(ctx->stream, v, a);
        return CSV_OK;
    }
    int32_t *pmax = ws.pmax;
    void *ptmp = ws.ptmp;
    uint64_t *ttmp = ws.ttmp;
    const int32_t *pos_s = d.pos;
    const int32_t *end_s = v.ref_end;
    if (unsorted) {
        // shard not coordinate-sorted: sort the read indices by pos on device and feed the tile search through `ord`
        uint32_t *pos_g = ws.pos_g, *end_g = ws.end_g;
        const uint32_t *perm = sorted_perm(ctx, d.pos, n, ws.w);
        launch_gather_u32(ctx->stream, (const uint32_t *)d.pos, perm, n, pos_g);
        launch_gather_u32(ctx->stream, (const uint32_t *)v.ref_end, perm, n, end_g);
        a.ord = perm; pos_s = (const int32_t *)pos_g; end_s = (const int32_t *)end_g;
    }
    launch_prefix_max(ctx->stream, end_s, pmax, n, ptmp);
    launch_depth_ranges(ctx->stream, pos_s, pmax, n, a.depth_len, ttmp);
    a.tile_range = ttmp;
    launch_depth_tiles(ctx->stream, v, a);
    return CSV_OK;
}

}  // namespace csv

using namespace csv;

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
    ReadsView dr;
    if ((rc = stage_reads(ctx, reads, rw, dr))) return rc;
    {
        TimerScope ts(ctx, CSV_K_CIGAR_SCAN);
        launch_cigar_scan(ctx->stream, ctx->n_cu, dr, ScanArgs{depth_len, min_oplen, min_mapq, 1, sig_raw, cap, scan_extras(dr.cnt, depth_len, false, nullptr), nullptr});
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
    ReadsView dr;
    if ((rc = stage_reads(ctx, reads, rw, dr))) return rc;
    {
        TimerScope ts(ctx, CSV_K_CIGAR_SCAN);
        launch_cigar_scan(ctx->stream, ctx->n_cu, dr, ScanArgs{0, 0, 0, 0, nullptr, 0, ScanExtras(), nullptr});
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
    ReadsView dr;
    if ((rc = stage_reads(ctx, reads, rw, dr))) return rc;
    {
        TimerScope ts(ctx, CSV_K_CIGAR_SCAN);
        launch_cigar_scan(ctx->stream, ctx->n_cu, dr, ScanArgs{depth_len, 0, 0, 0, nullptr, 0, ScanExtras(), nullptr});
    }
    ScanCounters h;
    if ((rc = read_counters(ctx, dr.cnt, h))) return rc;
    DepthWs dw;
    if ((rc = arena_reserve_for(ctx, ctx->work, "depth chain", [&](Arena &a) { return carve_depth(a, reads->n_reads, depth_len, dw); }))) return rc;
    if ((rc = depth_chain(ctx, dw, dr, h.unsorted != 0, DepthArgs{depth_len, d_depth, nullptr, nullptr, nullptr}))) return rc;
    if (depth && depth_len) CSV_HIP(ctx, hipMemcpyAsync(depth, d_depth, (size_t)depth_len * 4, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = read_counters(ctx, dr.cnt, h))) return rc;
    if (sum) *sum = h.depth_sum;
    if (nonzero) *nonzero = h.depth_nonzero;
    return CSV_OK;
}
