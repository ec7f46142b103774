// fasta.hip — the reference genome loaded and queried on the device: the builder (one base array that grows, FASTA text appended in pieces
// cut anywhere), its hand-over to a csv_genome, the genome's description and the cuts of it (kernels/fasta.hip). The rules are
// fasta_core.hpp; the text and the header lines' events travel through a Transfer, the array grows as a DevBuf, and the line ends are counted
// by vcf.hip's count_lines (all glue.hpp). Replaces the line loop of ReferenceGenome::setFilepath and the substr of ::query (host/fasta_query.cpp), and the
// ambiguity masking of the VCF writer's REF lookups (host/vcf_writer.cpp).
#include <new>

#include "../fasta_core.hpp"
#include "glue.hpp"

using namespace csv;
using fastacore::Assembler;
using fastacore::LINE_HEADER;

namespace {

constexpr uint64_t kSlack = 16;                      // bytes kept behind the array's last base

}  // namespace

struct csv_genome_builder {
    int device = 0;
    DevBuf seq;                                      // the kept residue bytes, in file order
    uint64_t n_kept = 0;
    uint64_t n_text = 0, n_lines = 0;                // what was appended: bytes, line ends
    Assembler a;                                     // the records so far, and what crosses the cut between two appends
};

namespace {

int bad(csv_ctx *ctx, const char *msg) { ctx->err = msg; return CSV_EINVAL; }

void builder_release(csv_genome_builder *b)
{
    if (!b) return;
    (void)hipFree(b->seq.p);
    delete b;
}

// n_slots == 0: what the count of the line ends needs; the per-line slices behind it keep the first ones where they are
bool carve_fasta(Arena &a, uint64_t n_tiles, uint64_t n_slots, uint64_t len, FastaWs &w)
{
    char *vhead = nullptr, *head = nullptr;
    const bool ok = take(a, vhead, 256) && take(a, head, 256) && take(a, w.vcf.tile_cnt, (n_tiles + 1) * 4) && take(a, w.vcf.es_tmp, exclusive_sum_tmp_bytes(n_tiles + 1));
    w.vcf.head = (VcfHead *)vhead;
    w.head = (FastaHead *)head;
    if (!ok || n_slots == 0) return ok;
    return take(a, w.vcf.line_start, n_slots * 4) && take(a, w.kept, (n_slots + 1) * 4) && take(a, w.hdr, (n_slots + 1) * 4) && take(a, w.nlen, (n_slots + 1) * 4) &&
           take(a, w.blank, n_slots) && take(a, w.es_tmp, exclusive_sum_tmp_bytes(n_slots + 1)) && take(a, w.ev.kept, n_slots * 4) &&
           take(a, w.ev.name_off, n_slots * 4) && take(a, w.ev.name_len, n_slots * 4) && take(a, w.ev.blank, n_slots) && take(a, w.ev.names, len);
}

// One piece of the text, on the device. The builder changes only once everything has come back: a failure leaves it as it was (bytes
// written behind its tail are not part of it). Everything queued has come back on CSV_OK.
int run_append(csv_ctx *ctx, Transfer &t, csv_genome_builder *b, const uint8_t *d_text, uint32_t len)
{
    hipStream_t s = ctx->stream;
    int rc;
    if ((rc = devbuf_ensure(ctx, b->seq, b->n_kept, b->n_kept + len + kSlack, "genome builder"))) return rc;
    const uint32_t n_tiles = vcf_tiles(d_text, len);
    FastaWs w;
    uint32_t n_slots = 0;
    if ((rc = count_lines(ctx, t, "genome_append", "genome_append: 2^32 lines or more in one call", d_text, len, w.vcf,
                          [&](Arena &a, uint64_t slots) { return carve_fasta(a, n_tiles, slots, len, w); },
                          [&]() -> int {                 // the line ends counted (the timer around the launch alone)
                              TimerScope ts(ctx, CSV_K_MISC);
                              launch_vcf_count(s, d_text, len, w.vcf);
                              return CSV_OK;
                          }, n_slots))) return rc;
    const FastaCarry carry{(uint8_t)b->a.mid_line, b->a.kind};
    {
        TimerScope ts(ctx, CSV_K_MISC);
        launch_vcf_starts(s, d_text, len, w.vcf);
        launch_fasta_lines(s, d_text, len, n_slots, carry, w);
        launch_fasta_compact(s, d_text, len, w, (uint8_t *)b->seq.p + b->n_kept);
    }
    FastaHead h;
    if ((rc = t.peek(&h, w.head, sizeof(FastaHead)))) return rc;
    if (h.n_kept > len || h.n_hdr > n_slots || h.n_name > len || h.tail_len > len) { ctx->err = "genome_append: the counts leave the text"; return CSV_EHIP; }
    const uint32_t nh = h.n_hdr;
    std::vector<uint32_t> kept(nh), name_off(nh), name_len(nh);
    std::vector<uint8_t> blank(nh), names(h.n_name);
    if ((rc = t.down(kept.data(), w.ev.kept, (size_t)nh * 4)) || (rc = t.down(name_off.data(), w.ev.name_off, (size_t)nh * 4)) ||
        (rc = t.down(name_len.data(), w.ev.name_len, (size_t)nh * 4)) || (rc = t.down(blank.data(), w.ev.blank, nh)) || (rc = t.down(names.data(), w.ev.names, h.n_name))) return rc;
    for (uint32_t i = 0; i < nh; i++)
        if ((uint64_t)name_off[i] + name_len[i] > h.n_name || kept[i] > h.n_kept) { ctx->err = "genome_append: a header line's event leaves the text"; return CSV_EHIP; }
    // the header lines, in file order, to the records (fasta_core.hpp: the same function the CPU check feeds)
    fastacore::PieceEvents e;
    e.n_hdr = nh; e.kept = kept.data(); e.name_off = name_off.data(); e.name_len = name_len.data(); e.blank = blank.data(); e.names = names.data();
    e.tail_len = h.tail_len; e.tail_kind = (uint8_t)h.tail_kind;
    fastacore::apply_piece(b->a, b->n_kept, e);
    b->n_kept += h.n_kept;
    b->n_text += len;
    b->n_lines += n_slots - 1;                           // the line ends
    return CSV_OK;
}

int check_append(csv_ctx *ctx, csv_genome_builder *b, const uint8_t *text, uint64_t len)
{
    if (!ctx || !b) return CSV_EINVAL;
    if (b->device != ctx->device) return bad(ctx, "genome_builder_append: the builder lives on another device");
    if (len >= (1ull << 32)) return bad(ctx, "genome_builder_append: a text of 2^32 bytes or more in one call");
    if (len && !text) return bad(ctx, "genome_builder_append: null pointer");
    return CSV_OK;
}

}  // namespace

csv_genome_builder *csvgpu_genome_builder_create(csv_ctx *ctx, uint64_t reserve_bytes)
{
    if (!ctx) return nullptr;
    (void)hipSetDevice(ctx->device);
    csv_genome_builder *b = new (std::nothrow) csv_genome_builder();
    if (!b) { ctx->err = "out of host memory"; return nullptr; }
    b->device = ctx->device;
    if (devbuf_ensure(ctx, b->seq, 0, reserve_bytes + kSlack, "genome builder") != CSV_OK) { builder_release(b); return nullptr; }
    return b;
}

void csvgpu_genome_builder_destroy(csv_ctx *ctx, csv_genome_builder *b)
{
    if (!ctx || !b) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    builder_release(b);
}

int csvgpu_genome_builder_append_dev(csv_ctx *ctx, csv_genome_builder *b, const uint8_t *d_text, uint64_t len)
{
    int rc = check_append(ctx, b, d_text, len);
    if (rc || len == 0) return rc;
    (void)hipSetDevice(ctx->device);
    Transfer t(ctx);
    if ((rc = t.open("genome_builder_append"))) return rc;
    return run_append(ctx, t, b, d_text, (uint32_t)len);
}

int csvgpu_genome_builder_append(csv_ctx *ctx, csv_genome_builder *b, const uint8_t *text, uint64_t len)
{
    int rc = check_append(ctx, b, text, len);
    if (rc || len == 0) return rc;
    (void)hipSetDevice(ctx->device);
    uint8_t *d_text = nullptr;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "genome_append", [&](Arena &a) { return take(a, d_text, len + 16); }))) return rc;
    Transfer t(ctx);
    if ((rc = t.open("genome_builder_append"))) return rc;
    if ((rc = t.up(d_text, text, len))) return rc;
    return run_append(ctx, t, b, d_text, (uint32_t)len);
}

csv_genome *csvgpu_genome_builder_finish(csv_ctx *ctx, csv_genome_builder *b)
{
    if (!ctx || !b) return nullptr;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (b->device != ctx->device) { ctx->err = "genome_builder_finish: the builder lives on another device"; builder_release(b); return nullptr; }
    csv_genome *g = new (std::nothrow) csv_genome();
    if (!g) { ctx->err = "out of host memory"; builder_release(b); return nullptr; }
    const uint64_t total = b->a.finish(b->n_kept);
    if (b->a.too_long() >= 0) {
        ctx->err = "genome_builder_finish: contig '" + b->a.rec[(size_t)b->a.too_long()].name + "' has 2^32 bytes or more";
        delete g; builder_release(b);
        return nullptr;
    }
    g->device = b->device; g->total = total; g->n_text = b->n_text; g->n_lines = b->n_lines;
    for (const fastacore::Record &r : b->a.rec) {
        g->rec.push_back(csv_genome_rec{r.start, (uint32_t)(r.end - r.start), g->names.size(), (uint32_t)r.name.size()});
        g->names += r.name;
    }
    g->seq = b->seq.p;                                   // the array changes hands
    b->seq.p = nullptr;
    builder_release(b);
    return g;
}

void csvgpu_genome_free(csv_ctx *ctx, csv_genome *g)
{
    if (!ctx || !g) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(g->seq);
    delete g;
}

int csvgpu_genome_describe(csv_ctx *ctx, const csv_genome *g, uint64_t cap_records, uint64_t cap_name_bytes, uint64_t *name_off, char *names, uint32_t *length,
                           csv_genome_counts *counts)
{
    if (!ctx || !g || !counts) return CSV_EINVAL;
    const uint64_t n = g->rec.size(), nb = g->names.size();
    *counts = csv_genome_counts{n, nb, g->total, g->n_text, g->n_lines};
    if (n > cap_records || nb > cap_name_bytes) { ctx->err = "genome_describe: output capacity too small"; return CSV_ECAPACITY; }   // (the sizing call ends here)
    if (n && (!length || !name_off || !names)) return bad(ctx, "genome_describe: null pointer");
    for (uint64_t i = 0; i < n; i++) { name_off[i] = g->rec[i].name_off; length[i] = g->rec[i].len; }
    if (name_off) name_off[n] = nb;
    if (nb) memcpy(names, g->names.data(), nb);
    return CSV_OK;
}

int csvgpu_genome_fetch(csv_ctx *ctx, const csv_genome *g, const uint32_t *record, const uint32_t *pos_start, const uint32_t *pos_end, const uint64_t *out_off,
                        uint64_t n, int mask, char *out)
{
    if (!ctx || !g) return CSV_EINVAL;
    if (g->device != ctx->device) return bad(ctx, "genome_fetch: the genome lives on another device");
    if (n == 0) return CSV_OK;
    if (!record || !pos_start || !pos_end || !out_off) return bad(ctx, "genome_fetch: null array");
    std::vector<uint64_t> src(n);
    for (uint64_t i = 0; i < n; i++) {
        if (record[i] >= g->rec.size()) return bad(ctx, "genome_fetch: record index beyond the genome");
        if (out_off[i + 1] < out_off[i]) return bad(ctx, "genome_fetch: out_off decreases");
        const csv_genome_rec &r = g->rec[record[i]];
        uint32_t first = 0;
        const uint32_t len = fastacore::cut_len(r.len, pos_start[i], pos_end[i], first);
        if (out_off[i + 1] - out_off[i] != len) return bad(ctx, "genome_fetch: an item's room is not its cut's length");
        src[i] = len ? r.start + first : 0;
    }
    const uint64_t first = out_off[0], total = out_off[n] - first;
    if (total == 0) return CSV_OK;
    if (!out) return bad(ctx, "genome_fetch: null output");
    (void)hipSetDevice(ctx->device);
    uint64_t *d_src = nullptr, *d_off = nullptr;
    uint8_t *d_out = nullptr;
    int rc = arena_reserve_for(ctx, ctx->arena, "genome_fetch", [&](Arena &a) { return take(a, d_src, n * 8) && take(a, d_off, (n + 1) * 8) && take(a, d_out, total); });
    if (rc) return rc;
    const void *h_src = nullptr;
    uint64_t *h_off = nullptr;
    void *h_out = nullptr;
    PinStage pin(ctx);
    if ((rc = pin_reserve_for(ctx, pin, [&](PinStage &p) { h_src = p.in(src.data(), n * 8); h_off = (uint64_t *)p.slot((n + 1) * 8); h_out = p.out(out + first, total); }))) return rc;
    for (uint64_t i = 0; i <= n; i++) h_off[i] = out_off[i] - first;            // (the device's output starts at the first item's byte)
    hipStream_t s = ctx->stream;
    CSV_HIP(ctx, hipMemcpyAsync(d_src, h_src, n * 8, hipMemcpyHostToDevice, s));
    CSV_HIP(ctx, hipMemcpyAsync(d_off, h_off, (n + 1) * 8, hipMemcpyHostToDevice, s));
    {
        TimerScope ts(ctx, CSV_K_MISC);
        launch_fasta_cut(s, (const uint8_t *)g->seq, d_src, d_off, n, total, mask != 0, d_out);
    }
    CSV_HIP(ctx, hipGetLastError());
    CSV_HIP(ctx, hipMemcpyAsync(h_out, d_out, total, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, wait_stream(s));
    pin.finish();
    return CSV_OK;
}
