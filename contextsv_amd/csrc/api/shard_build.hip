// shard_build.hip — a resident shard built on the device from BAM batches: the builder (arrays that grow, batches appended behind the
// tail by csvgpu_bam_unpack_dev or from the host parser's arrays), its hand-over to a csv_shard of the kind csvgpu_shard_upload makes, what
// is read back out of such a shard, and the ALT strings cut from its packed sequences (kernels/shardbuild.hip). Replaces the BamShard's host
// arrays and their csvgpu_shard_upload (host/bam_io.cpp readContig, host/sv_caller.cpp run), and the base loop of SVCaller::toSVCall.
#include <new>

#include "glue.hpp"

using namespace csv;

namespace {

constexpr uint64_t kSlack = 16;                      // bytes kept behind every array's last element, as csvgpu_shard_upload allocates them

}  // namespace

struct csv_shard_builder {
    uint32_t want = 0;
    int device = 0;
    DevBuf pos, flag, mapq, cigar_off, cigar, seq_off, seq, name_off, name, name_hash;
    csv_shard_sizes n{0, 0, 0, 0};
    uint32_t *unsorted = nullptr;                    // device word: some appended pos[i] < pos[i - 1]
};

namespace {

bool wants(const csv_shard_builder *b, uint32_t what) { return (b->want & what) != 0; }

// (the growth of glue.hpp, with the builder's name in its texts)
int ensure(csv_ctx *ctx, DevBuf &b, uint64_t used, uint64_t need) { return devbuf_ensure(ctx, b, used, need, "shard builder"); }

// room for `add` more behind the builder's totals in every array it keeps
int ensure_all(csv_ctx *ctx, csv_shard_builder *b, const csv_shard_sizes &add)
{
    const csv_shard_sizes &n = b->n;
    const uint64_t r = n.n_reads + add.n_reads;
    int rc;
    if ((rc = ensure(ctx, b->pos, n.n_reads * 4, r * 4 + kSlack)) || (rc = ensure(ctx, b->flag, n.n_reads * 2, r * 2 + kSlack)) ||
        (rc = ensure(ctx, b->mapq, n.n_reads, r + kSlack)) || (rc = ensure(ctx, b->cigar_off, (n.n_reads + 1) * 8, (r + 1) * 8 + kSlack)) ||
        (rc = ensure(ctx, b->cigar, n.n_cigar * 4, (n.n_cigar + add.n_cigar + CIGAR_PAD_WORDS) * 4))) return rc;
    if (wants(b, CSV_SB_SEQ) && ((rc = ensure(ctx, b->seq_off, (n.n_reads + 1) * 8, (r + 1) * 8 + kSlack)) ||
                                 (rc = ensure(ctx, b->seq, n.n_seq, n.n_seq + add.n_seq + kSlack)))) return rc;
    if (wants(b, CSV_SB_NAMES) && ((rc = ensure(ctx, b->name_off, (n.n_reads + 1) * 8, (r + 1) * 8 + kSlack)) ||
                                   (rc = ensure(ctx, b->name, n.n_name, n.n_name + add.n_name + kSlack)))) return rc;
    if (wants(b, CSV_SB_NAME_HASH) && (rc = ensure(ctx, b->name_hash, n.n_reads * 8, r * 8 + kSlack))) return rc;
    return CSV_OK;
}

void builder_release(csv_shard_builder *b)
{
    if (!b) return;
    for (DevBuf *x : {&b->pos, &b->flag, &b->mapq, &b->cigar_off, &b->cigar, &b->seq_off, &b->seq, &b->name_off, &b->name, &b->name_hash}) (void)hipFree(x->p);
    (void)hipFree(b->unsorted);
    delete b;
}

// the arrays of one csvgpu_bam_unpack_dev call that writes behind the builder's tail, with the given capacities
csv_bam_out tail_out(const csv_shard_builder *b, const csv_shard_sizes &cap)
{
    const csv_shard_sizes &n = b->n;
    csv_bam_out o{};
    o.pos = (int32_t *)b->pos.p + n.n_reads; o.flag = (uint16_t *)b->flag.p + n.n_reads; o.mapq = (uint8_t *)b->mapq.p + n.n_reads;
    o.cigar_off = (uint64_t *)b->cigar_off.p + n.n_reads; o.cigar = (uint32_t *)b->cigar.p + n.n_cigar;
    if (wants(b, CSV_SB_SEQ)) { o.seq_off = (uint64_t *)b->seq_off.p + n.n_reads; o.seq = (uint8_t *)b->seq.p + n.n_seq; }
    if (wants(b, CSV_SB_NAMES)) { o.name_off = (uint64_t *)b->name_off.p + n.n_reads; o.name = (uint8_t *)b->name.p + n.n_name; }
    if (wants(b, CSV_SB_NAME_HASH)) o.name_hash = (uint64_t *)b->name_hash.p + n.n_reads;
    o.cap_records = cap.n_reads; o.cap_cigar = cap.n_cigar; o.cap_seq = cap.n_seq; o.cap_name = cap.n_name;
    return o;
}

// the sortedness of the records [first, first + n) into the builder's word, queued behind whatever wrote them: the caller waits
int note_order(csv_ctx *ctx, csv_shard_builder *b, uint64_t first, uint64_t n)
{
    launch_sb_unsorted(ctx->stream, (const int32_t *)b->pos.p, first, n, b->unsorted);
    CSV_HIP(ctx, hipGetLastError());
    return CSV_OK;
}

int bad(csv_ctx *ctx, const char *msg) { ctx->err = msg; return CSV_EINVAL; }

}  // namespace

csv_shard_builder *csvgpu_shard_builder_create(csv_ctx *ctx, uint32_t want, const csv_shard_sizes *reserve)
{
    if (!ctx) return nullptr;
    if (want & ~(uint32_t)(CSV_SB_SEQ | CSV_SB_NAMES | CSV_SB_NAME_HASH)) { ctx->err = "shard_builder_create: unknown bit in want"; return nullptr; }
    (void)hipSetDevice(ctx->device);
    csv_shard_builder *b = new (std::nothrow) csv_shard_builder();
    if (!b) { ctx->err = "out of host memory"; return nullptr; }
    b->want = want; b->device = ctx->device;
    // the sortedness word, room for the reserve, and the offsets of an empty shard: one entry, 0 (an append writes its own first entry over
    // the tail's last: the same value)
    auto queue = [&]() -> int {
        CSV_HIP(ctx, hipMalloc((void **)&b->unsorted, 256));
        CSV_HIP(ctx, hipMemsetAsync(b->unsorted, 0, 4, ctx->stream));
        const int rc = ensure_all(ctx, b, reserve ? *reserve : csv_shard_sizes{0, 0, 0, 0});
        if (rc) return rc;
        for (DevBuf *x : {&b->cigar_off, &b->seq_off, &b->name_off}) if (x->p) CSV_HIP(ctx, hipMemsetAsync(x->p, 0, 8, ctx->stream));
        CSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return CSV_OK;
    };
    if (queue() != CSV_OK) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(ctx->stream);
        builder_release(b);
        return nullptr;
    }
    return b;
}

void csvgpu_shard_builder_destroy(csv_ctx *ctx, csv_shard_builder *b)
{
    if (!ctx || !b) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    builder_release(b);
}

int csvgpu_shard_builder_sizes(csv_ctx *ctx, const csv_shard_builder *b, csv_shard_sizes *out)
{
    if (!ctx || !b || !out) return CSV_EINVAL;
    *out = b->n;
    return CSV_OK;
}

int csvgpu_shard_builder_append_bam(csv_ctx *ctx, csv_shard_builder *b, const uint8_t *d_bytes, uint64_t len, const uint32_t *anchors, uint32_t n_anchors,
                                    int32_t tid, int64_t end, csv_bam_counts *counts)
{
    if (!ctx || !b || !counts) return CSV_EINVAL;
    if (b->device != ctx->device) return bad(ctx, "shard_builder_append_bam: the builder lives on another device");
    (void)hipSetDevice(ctx->device);
    // the sizing call: no room offered, the exact counts back (CSV_OK when nothing is kept: there is nothing to write then)
    csv_bam_out o = tail_out(b, csv_shard_sizes{0, 0, 0, 0});
    int rc = csvgpu_bam_unpack_dev(ctx, d_bytes, len, anchors, n_anchors, tid, end, b->n.n_cigar, b->n.n_seq, b->n.n_name, &o, counts);
    if (rc != CSV_ECAPACITY) return rc;                                   // CSV_OK (nothing kept), 1 (declined) or an error: nothing appended
    const csv_shard_sizes add{counts->n_kept, counts->n_cigar, counts->n_seq, counts->n_name};
    if (b->n.n_reads + add.n_reads >= 0xffffffffull) return bad(ctx, "shard_builder_append_bam: more than 2^32-2 reads in one shard");
    if ((rc = ensure_all(ctx, b, add))) return rc;
    o = tail_out(b, add);
    rc = csvgpu_bam_unpack_dev(ctx, d_bytes, len, anchors, n_anchors, tid, end, b->n.n_cigar, b->n.n_seq, b->n.n_name, &o, counts);
    if (rc == CSV_ECAPACITY || rc == 1) { ctx->err = "shard_builder_append_bam: the second pass disagrees with the sizing pass"; return CSV_EHIP; }
    if (rc) return rc;
    if ((rc = note_order(ctx, b, b->n.n_reads, add.n_reads))) return rc;
    CSV_HIP(ctx, wait_stream(ctx->stream));
    b->n.n_reads += add.n_reads; b->n.n_cigar += add.n_cigar; b->n.n_seq += add.n_seq; b->n.n_name += add.n_name;
    return CSV_OK;
}

int csvgpu_shard_builder_append_host(csv_ctx *ctx, csv_shard_builder *b, const csv_reads *r, const uint64_t *seq_off, const uint8_t *seq,
                                     const uint64_t *name_off, const uint8_t *name, const uint64_t *name_hash)
{
    if (!ctx || !b) return CSV_EINVAL;
    if (b->device != ctx->device) return bad(ctx, "shard_builder_append_host: the builder lives on another device");
    int rc = check_reads(ctx, r);
    if (rc) return rc;
    const uint64_t k = r->n_reads;
    if (k == 0) return CSV_OK;
    if ((wants(b, CSV_SB_SEQ) && !seq_off) || (wants(b, CSV_SB_NAMES) && !name_off) || (wants(b, CSV_SB_NAME_HASH) && !name_hash))
        return bad(ctx, "shard_builder_append_host: a wanted array is null");
    csv_shard_sizes add{k, r->cigar_off[k] - r->cigar_off[0], 0, 0};
    auto span = [&](const uint64_t *off, const uint8_t *data, uint64_t &n) {
        for (uint64_t i = 0; i < k; i++) if (off[i + 1] < off[i]) return false;
        n = off[k] - off[0];
        return n == 0 || data != nullptr;
    };
    if (wants(b, CSV_SB_SEQ) && !span(seq_off, seq, add.n_seq)) return bad(ctx, "shard_builder_append_host: seq_off not monotone, or seq null");
    if (wants(b, CSV_SB_NAMES) && !span(name_off, name, add.n_name)) return bad(ctx, "shard_builder_append_host: name_off not monotone, or name null");
    if (b->n.n_reads + k >= 0xffffffffull) return bad(ctx, "shard_builder_append_host: more than 2^32-2 reads in one shard");
    (void)hipSetDevice(ctx->device);
    if ((rc = ensure_all(ctx, b, add))) return rc;
    Transfer t(ctx);
    if ((rc = t.open("shard_builder_append_host"))) return rc;
    const csv_bam_out o = tail_out(b, add);
    hipStream_t s = ctx->stream;
    // an offset array goes up as it is and is rebased where it lies: + the builder's total, - the batch's own first offset
    auto offsets = [&](uint64_t *d_off, const uint64_t *h_off, uint64_t total) {
        const int rc2 = t.up(d_off, h_off, (k + 1) * 8);
        if (rc2 == CSV_OK) launch_sb_add(s, d_off, k + 1, total - h_off[0]);
        return rc2;
    };
    if ((rc = t.up(o.pos, r->pos, k * 4)) || (rc = t.up(o.flag, r->flag, k * 2)) || (rc = t.up(o.mapq, r->mapq, k)) || (rc = offsets(o.cigar_off, r->cigar_off, b->n.n_cigar)) ||
        (rc = t.up(o.cigar, r->cigar ? r->cigar + r->cigar_off[0] : nullptr, add.n_cigar * 4))) return rc;
    if (wants(b, CSV_SB_SEQ) && ((rc = offsets(o.seq_off, seq_off, b->n.n_seq)) || (rc = t.up(o.seq, seq ? seq + seq_off[0] : nullptr, add.n_seq)))) return rc;
    if (wants(b, CSV_SB_NAMES) && ((rc = offsets(o.name_off, name_off, b->n.n_name)) || (rc = t.up(o.name, name ? name + name_off[0] : nullptr, add.n_name)))) return rc;
    if (wants(b, CSV_SB_NAME_HASH) && (rc = t.up(o.name_hash, name_hash, k * 8))) return rc;
    if ((rc = note_order(ctx, b, b->n.n_reads, k)) || (rc = t.wait())) return rc;
    b->n.n_reads += k; b->n.n_cigar += add.n_cigar; b->n.n_seq += add.n_seq; b->n.n_name += add.n_name;
    return CSV_OK;
}

csv_shard *csvgpu_shard_builder_finish(csv_ctx *ctx, csv_shard_builder *b, uint32_t depth_len)
{
    if (!ctx || !b) return nullptr;
    (void)hipSetDevice(ctx->device);
    if (b->device != ctx->device) { ctx->err = "shard_builder_finish: the builder lives on another device"; builder_release(b); return nullptr; }
    csv_shard *sh = new (std::nothrow) csv_shard();
    int rc = ensure_pinned(ctx, kPinScalars);
    if (!sh || rc) { if (!sh) ctx->err = "out of host memory"; delete sh; (void)hipStreamSynchronize(ctx->stream); builder_release(b); return nullptr; }
    hipStream_t s = ctx->stream;
    bool ok = hipMemcpyAsync(ctx->pinned, b->unsorted, 4, hipMemcpyDeviceToHost, s) == hipSuccess;
    ok &= hipMemsetAsync((uint32_t *)b->cigar.p + b->n.n_cigar, 0, (size_t)CIGAR_PAD_WORDS * 4, s) == hipSuccess;
    ok &= hipStreamSynchronize(s) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); ctx->err = "shard_builder_finish: reading the builder's state failed"; delete sh; builder_release(b); return nullptr; }
    // the arrays change hands: from here on shard_release frees them
    sh->owned = true; sh->depth_len = depth_len; sh->cigar_pad = CIGAR_PAD_WORDS;
    sh->unsorted = *(const uint32_t *)ctx->pinned ? 1 : 0;
    sh->d.n_reads = b->n.n_reads; sh->d.n_cigar = b->n.n_cigar; sh->d.tid = nullptr;
    sh->d.pos = (const int32_t *)b->pos.p; sh->d.flag = (const uint16_t *)b->flag.p; sh->d.mapq = (const uint8_t *)b->mapq.p;
    sh->d.cigar_off = (const uint64_t *)b->cigar_off.p; sh->d.cigar = (const uint32_t *)b->cigar.p;
    sh->seq_off = (uint64_t *)b->seq_off.p; sh->seq = (uint8_t *)b->seq.p; sh->n_seq = b->n.n_seq;
    sh->name_off = (uint64_t *)b->name_off.p; sh->name = (uint8_t *)b->name.p; sh->n_name = b->n.n_name;
    sh->qhash = (uint64_t *)b->name_hash.p;
    (void)hipFree(b->unsorted);
    delete b;
    return shard_common(ctx, sh);
}

int csvgpu_shard_sizes(csv_ctx *ctx, const csv_shard *sh, csv_shard_sizes *out)
{
    if (!ctx || !sh || !out) return CSV_EINVAL;
    *out = csv_shard_sizes{sh->d.n_reads, sh->d.n_cigar, sh->seq ? sh->n_seq : 0, sh->n_name};
    return CSV_OK;
}

// (the fetches: an array the caller passes null for is skipped)
int csvgpu_shard_fetch_reads(csv_ctx *ctx, csv_shard *sh, int32_t *pos, uint16_t *flag, uint8_t *mapq, uint64_t *cigar_off, uint32_t *cigar)
{
    if (!ctx || !sh) return CSV_EINVAL;
    (void)hipSetDevice(ctx->device);
    Transfer t(ctx);
    int rc = t.open("shard_fetch_reads");
    if (rc) return rc;
    const uint64_t n = sh->d.n_reads;
    if ((rc = t.down(pos, sh->d.pos, n * 4)) || (rc = t.down(flag, sh->d.flag, n * 2)) || (rc = t.down(mapq, sh->d.mapq, n)) ||
        (rc = t.down(cigar_off, sh->d.cigar_off, (n + 1) * 8))) return rc;
    const CigarPack pack = shard_view(sh).pack;
    if (!pack.half) { if ((rc = t.down(cigar, sh->d.cigar, sh->d.n_cigar * 4))) return rc; }
    else if (cigar) {
        // a packed shard (shard.hip) gives the caller's 32-bit words back: unpacked on the device one piece of the transfer at a time
        uint32_t *stage = nullptr;
        if ((rc = arena_reserve_for(ctx, ctx->arena, "shard_fetch_reads", [&](Arena &a) { return take(a, stage, kPiece); }))) return rc;
        const uint64_t per = kPiece / 4;
        for (uint64_t o = 0; o < sh->d.n_cigar; o += per) {
            const uint64_t k = std::min(per, sh->d.n_cigar - o);
            launch_cigar_unpack(ctx->stream, pack, o, k, stage);
            CSV_HIP(ctx, hipGetLastError());
            if ((rc = t.down(cigar + o, stage, k * 4))) return rc;
        }
    }
    return t.wait();
}

int csvgpu_shard_fetch_names(csv_ctx *ctx, csv_shard *sh, uint64_t *name_off, uint8_t *name, uint64_t *name_hash)
{
    if (!ctx || !sh) return CSV_EINVAL;
    if ((name_off || name) && !sh->name_off) return bad(ctx, "shard_fetch_names: the shard holds no names");
    if (name_hash && !sh->qhash) return bad(ctx, "shard_fetch_names: the shard holds no name hashes");
    (void)hipSetDevice(ctx->device);
    Transfer t(ctx);
    int rc = t.open("shard_fetch_names");
    if (rc) return rc;
    const uint64_t n = sh->d.n_reads;
    if ((rc = t.down(name_off, sh->name_off, (n + 1) * 8)) || (rc = t.down(name, sh->name, sh->n_name)) || (rc = t.down(name_hash, sh->qhash, n * 8))) return rc;
    return t.wait();
}

int csvgpu_shard_drop_sequences(csv_ctx *ctx, csv_shard *sh)
{
    if (!ctx || !sh) return CSV_EINVAL;
    (void)hipSetDevice(ctx->device);
    CSV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    (void)hipFree(sh->seq_off); (void)hipFree(sh->seq);
    sh->seq_off = nullptr; sh->seq = nullptr; sh->n_seq = 0;
    return CSV_OK;
}

int csvgpu_alt_bases_resident(csv_ctx *ctx, csv_shard *sh, const uint32_t *read, const uint32_t *qpos, const uint64_t *out_off, uint64_t n, char *out)
{
    if (!ctx || !sh) return CSV_EINVAL;
    if (!sh->seq_off) return bad(ctx, "alt_bases: the shard holds no sequences (built without them, or dropped)");
    if (n == 0) return CSV_OK;
    if (!read || !qpos || !out_off) return bad(ctx, "alt_bases: null array");
    for (uint64_t i = 0; i < n; i++) {
        if (read[i] >= sh->d.n_reads) return bad(ctx, "alt_bases: record index beyond the shard");
        if (out_off[i + 1] < out_off[i]) return bad(ctx, "alt_bases: out_off decreases");
    }
    const uint64_t first = out_off[0], total = out_off[n] - first;
    if (total == 0) return CSV_OK;
    if (!out) return bad(ctx, "alt_bases: null output");
    (void)hipSetDevice(ctx->device);
    uint32_t *d_read = nullptr, *d_qpos = nullptr;
    uint64_t *d_off = nullptr;
    uint8_t *d_out = nullptr;
    int rc = arena_reserve_for(ctx, ctx->arena, "alt_bases", [&](Arena &a) { return take(a, d_read, n * 4) && take(a, d_qpos, n * 4) && take(a, d_off, (n + 1) * 8) && take(a, d_out, total); });
    if (rc) return rc;
    const void *h_read = nullptr, *h_qpos = nullptr;
    uint64_t *h_off = nullptr;
    void *h_out = nullptr;
    PinStage pin(ctx);
    if ((rc = pin_reserve_for(ctx, pin, [&](PinStage &p) {
            h_read = p.in(read, n * 4); h_qpos = p.in(qpos, n * 4); h_off = (uint64_t *)p.slot((n + 1) * 8); h_out = p.out(out + first, total);
        }))) return rc;
    for (uint64_t i = 0; i <= n; i++) h_off[i] = out_off[i] - first;           // (the device's output starts at the first item's character)
    hipStream_t s = ctx->stream;
    CSV_HIP(ctx, hipMemcpyAsync(d_read, h_read, n * 4, hipMemcpyHostToDevice, s));
    CSV_HIP(ctx, hipMemcpyAsync(d_qpos, h_qpos, n * 4, hipMemcpyHostToDevice, s));
    CSV_HIP(ctx, hipMemcpyAsync(d_off, h_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
    {
        TimerScope ts(ctx, CSV_K_MISC);
        launch_alt_bases(s, sh->seq_off, sh->seq, d_read, d_qpos, d_off, n, d_out);
    }
    CSV_HIP(ctx, hipGetLastError());
    CSV_HIP(ctx, hipMemcpyAsync(h_out, d_out, total, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, wait_stream(s));
    pin.finish();
    return CSV_OK;
}
