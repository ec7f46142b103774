// shard.hip — resident shards: upload / wrap / free, and what is read out of one.
#include <new>

#include "glue.hpp"
#include "../cigar_pack_core.hpp"

namespace csv {

namespace cpk = cigar_pack_core;

void shard_release(csv_shard *sh)
{
    if (!sh) return;
    if (sh->owned) {
        (void)hipFree((void *)sh->d.pos); (void)hipFree((void *)sh->d.flag); (void)hipFree((void *)sh->d.mapq);
        (void)hipFree((void *)sh->d.cigar_off); (void)hipFree((void *)sh->d.cigar);
    }
    (void)hipFree(sh->ref_end); (void)hipFree(sh->q_start); (void)hipFree(sh->q_end);
    (void)hipFree(sh->cig_half); (void)hipFree(sh->esc_piece); (void)hipFree(sh->esc_tab);
    (void)hipFree(sh->ckpt);
    (void)hipFree(sh->sel_scratch);
    (void)hipFree(sh->depth_items);
    (void)hipFree(sh->scan_split);
    (void)hipFree(sh->qhash);
    (void)hipFree(sh->seq_off); (void)hipFree(sh->seq); (void)hipFree(sh->name_off); (void)hipFree(sh->name);
    (void)hipFree(sh->depth); (void)hipFree(sh->sig_raw); (void)hipFree(sh->scratch); (void)hipFree(sh->counters);
    delete sh;
}

csv_shard *shard_common(csv_ctx *ctx, csv_shard *sh)
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

// The 16-bit form of a freshly uploaded wave-form shard (cigar_pack_core.hpp), made on the device from the 32-bit words: escapes counted per
// 512-op piece, the exclusive sum, one read-back that sizes the table, the halfwords and the table written, the 32-bit array freed. A shard
// with more escapes than 1 / 64 of its ops, or one whose halfword array cannot be had, stays at 32 bits. CSV_OK either way; CSV_EHIP on a
// failed launch or copy.
static int shard_pack_cigar(csv_ctx *ctx, csv_shard *sh)
{
    const uint64_t m = sh->d.n_cigar, np = cpk::n_pieces(m);
    if (m == 0 || np + 1 >= 0xffffffffull) return CSV_OK;         // (the per-piece index counts in 32 bits: at most m / 64 escapes, m below 2^40)
    hipStream_t s = ctx->stream;
    int rc = ensure_pinned(ctx, kPinScalars);
    if (rc) return rc;
    uint32_t *piece = nullptr;
    void *es_tmp = nullptr;
    uint16_t *half = nullptr;
    uint64_t *tab = nullptr;
    auto drop = [&]() { (void)hipFree(piece); (void)hipFree(es_tmp); (void)hipFree(half); (void)hipFree(tab); (void)hipGetLastError(); };
    if (hipMalloc((void **)&piece, (np + 1) * 4) != hipSuccess || hipMalloc(&es_tmp, exclusive_sum_tmp_bytes(np + 1) + 16) != hipSuccess) { drop(); return CSV_OK; }
    launch_cigar_esc_count(s, sh->d.cigar, m, piece);
    launch_exclusive_sum_u32(s, piece, np + 1, es_tmp);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->pinned, piece + np, 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { drop(); ctx->err = std::string("shard upload: counting the escapes failed: ") + hipGetErrorString(e); return CSV_EHIP; }
    const uint64_t n_esc = *(const uint32_t *)ctx->pinned;
    if (!cpk::packs(m, n_esc)) { drop(); return CSV_OK; }
    // INVARIANT the two big kernels rely on: the halfword array is allocated (and, behind op m, zeroed) up to the end of its last 512-op piece
    // plus CIGAR_PAD_WORDS halfwords. Every 1 KiB LDS-DMA piece of the scan starts at a multiple of 512 ops below m, so it ends at or in front of
    // the last piece's end; every lane load of the depth walk starts below m rounded up to 4 ops and is at most 16 bytes long, so it ends in
    // front of the pad's end. The table has one entry to spare behind its last.
    const uint64_t n_half = np * cpk::PIECE_OPS + CIGAR_PAD_WORDS;
    if (hipMalloc((void **)&half, n_half * 2) != hipSuccess || hipMalloc((void **)&tab, (n_esc + 1) * 8) != hipSuccess) { drop(); return CSV_OK; }
    e = hipMemsetAsync(half + np * cpk::PIECE_OPS, 0, (size_t)CIGAR_PAD_WORDS * 2, s);
    if (e == hipSuccess) e = hipMemsetAsync(tab + n_esc, 0, 8, s);
    if (e == hipSuccess) { launch_cigar_pack(s, sh->d.cigar, m, piece, half, tab); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { drop(); ctx->err = std::string("shard upload: packing the CIGAR array failed: ") + hipGetErrorString(e); return CSV_EHIP; }
    (void)hipFree(es_tmp);
    (void)hipFree((void *)sh->d.cigar);
    sh->d.cigar = nullptr;
    sh->cig_half = half; sh->esc_piece = piece; sh->esc_tab = tab; sh->n_esc = n_esc;
    return CSV_OK;
}

}  // namespace csv

using namespace csv;

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
    if (ctx->cigar_packing && scan_form(ctx, n, m) == SCAN_FORM_WAVE && shard_pack_cigar(ctx, sh)) { shard_release(sh); return nullptr; }
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

uint64_t csvgpu_shard_cigar_bytes(const csv_shard *sh)
{
    if (!sh) return 0;
    if (!sh->cig_half) return 4 * (sh->d.n_cigar + (uint64_t)sh->cigar_pad);
    const uint64_t np = cpk::n_pieces(sh->d.n_cigar);
    return 2 * (np * cpk::PIECE_OPS + (uint64_t)sh->cigar_pad) + 4 * (np + 1) + 8 * (sh->n_esc + 1);
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
