// snp_build.hip — resident SNP columns built on the device from VCF text batches (kernels/snpbuild.hip; the rules in snp_build_core.hpp):
// the builder's arrays that grow, the append that reuses the parse of vcf.hip with its outputs staged on the device, the one sort of
// finish, and what is made from a contig's columns (the fetch, the population parse, the table). Replaces the `keep` lambda and the merge
// loop of SNPFile::load and `sorted` in SNPFile::table (host/snp_io.cpp).
#include <memory>
#include <new>
#include <type_traits>

#include "glue.hpp"
#include "../snp_build_core.hpp"

using namespace csv;

struct csv_snp_builder {
    int device = 0;
    DevBuf pos, baf, run, key;                       // [n] uint32 / the double's bits / snpbuild run word / order key
    DevBuf scratch;                                  // one append's run flags, their sum's workspace and the run table
    uint64_t n = 0, n_runs = 0;
    uint64_t max_key = 0; uint32_t max_host_id = 0;  // over all records / over the host-appended ones
};

struct csv_snp_columns {
    int device = 0;
    char *block = nullptr;
    const uint32_t *pos = nullptr; const uint64_t *baf = nullptr;    // [n] ordered by (contig id, order key)
    uint64_t n = 0;
    struct Contig { uint32_t id; uint64_t first, count; bool ascending; };
    std::vector<Contig> contigs;                     // those that hold a record, by ascending id
};

namespace {

int bad(csv_ctx *ctx, const char *who, const char *msg) { ctx->err = std::string(who) + ": " + msg; return CSV_EINVAL; }

void builder_release(csv_snp_builder *b)
{
    for (DevBuf *d : {&b->pos, &b->baf, &b->run, &b->key, &b->scratch}) (void)hipFree(d->p);
    delete b;
}

// room for `add` more records behind the tail in every array
int ensure_records(csv_ctx *ctx, csv_snp_builder *b, uint64_t add)
{
    const uint64_t n = b->n, want = n + add;
    int rc;
    if ((rc = devbuf_ensure(ctx, b->pos, n * 4, want * 4, "snp builder")) || (rc = devbuf_ensure(ctx, b->baf, n * 8, want * 8, "snp builder")) ||
        (rc = devbuf_ensure(ctx, b->run, n * 4, want * 4, "snp builder")) || (rc = devbuf_ensure(ctx, b->key, n * 8, want * 8, "snp builder"))) return rc;
    return CSV_OK;
}

struct AppendWs { uint32_t *flags = nullptr; void *es_tmp = nullptr; uint32_t *run_first = nullptr, *run_line_off = nullptr, *run_chrom_len = nullptr; };
// one append's scratch over a block of its own (the arenas hold the text and the parse's workspace); base == nullptr plans
size_t carve_append(char *base, uint64_t k, AppendWs &w)
{
    size_t used = 0;
    auto piece = [&](auto *&p, size_t bytes) { p = (std::remove_reference_t<decltype(p)>)(base ? base + used : nullptr); used += align_up(bytes, 256); };
    piece(w.flags, (k + 1) * 4); piece(w.es_tmp, exclusive_sum_tmp_bytes(k + 1));
    piece(w.run_first, k * 4); piece(w.run_line_off, k * 4); piece(w.run_chrom_len, k * 4);
    return used;
}

int append_text(csv_ctx *ctx, csv_snp_builder *b, bool dev, const uint8_t *text, uint64_t len, uint64_t text_base, int dp_int, int ad_int, const csv_snp_runs *out,
                csv_snp_append_counts *counts)
{
    if (!ctx) return CSV_EINVAL;
    const char *who = "snp_builder_append";
    if (!b || !out || !counts) return bad(ctx, who, "null pointer");
    if (len >= (1ull << 32)) return bad(ctx, who, "a text of 2^32 bytes or more");
    if (text_base > snpbuild::KEY_LIMIT || len > snpbuild::KEY_LIMIT - text_base) return bad(ctx, who, "text_base + len above 2^48");
    if (len && !text) return bad(ctx, who, "null pointer");
    if ((out->cap_runs && (!out->run_first || !out->run_line_off || !out->run_chrom_len)) || (out->cap_defer && !out->defer_off)) return bad(ctx, who, "null pointer");
    if (b->device != ctx->device) return bad(ctx, who, "a builder of another device");
    *counts = csv_snp_append_counts{};
    counts->first_run = b->n_runs;
    if (len == 0) return CSV_OK;
    (void)hipSetDevice(ctx->device);
    int rc;
    const uint8_t *d_text = text;
    Transfer t(ctx);
    if (!dev) {
        VcfTextWs tw;
        if ((rc = arena_reserve_for(ctx, ctx->arena, who, [&](Arena &a) { return carve_vcf_text(a, len, 0, tw); }))) return rc;
        if ((rc = t.open(who)) || (rc = t.up(tw.text, text, len))) return rc;
        d_text = tw.text;
    } else if ((rc = t.open(who))) return rc;
    VcfWs w;
    csv_vcf_counts vc{};
    rc = vcf_snp_stage(ctx, t, d_text, (uint32_t)len, dp_int, ad_int, vc, w);
    if (rc == 1) { counts->status = vc.status; return 1; }
    if (rc) return rc;
    const uint64_t K = vc.n_kept, D = vc.n_deferred;
    counts->n_lines = vc.n_lines; counts->n_kept = K; counts->n_deferred = D;
    hipStream_t s = ctx->stream;
    AppendWs aw;
    uint32_t R = 0;
    if (K) {
        if ((rc = devbuf_ensure(ctx, b->scratch, 0, carve_append(nullptr, K, aw), "snp builder"))) return rc;
        carve_append(b->scratch.p, K, aw);
        {
            TimerScope ts(ctx, CSV_K_MISC);
            launch_snp_run_flags(s, d_text, w.out.line_off, w.out.chrom_len, (uint32_t)K, aw.flags, aw.es_tmp);
        }
        CSV_HIP(ctx, hipGetLastError());
        if ((rc = t.peek(&R, aw.flags + K, 4))) return rc;
        if (R == 0 || R > K) { ctx->err = "snp_builder_append: the run count leaves the records"; return CSV_EHIP; }
    }
    counts->n_runs = R;
    if (R > out->cap_runs || D > out->cap_defer) { ctx->err = "snp_builder_append: output capacity too small"; return CSV_ECAPACITY; }
    if (b->n_runs + R >= snpbuild::HOST_TAG) return bad(ctx, who, "2^31 runs or more");
    if (K) {
        if ((rc = ensure_records(ctx, b, K))) return rc;
        SnpAppendArgs a{};
        a.n = (uint32_t)K; a.ridx = aw.flags;
        a.line_off = w.out.line_off; a.chrom_len = w.out.chrom_len; a.rec_pos = w.out.pos; a.rec_baf = (const uint64_t *)w.out.value;
        a.tail = b->n; a.text_base = text_base; a.run_base = (uint32_t)b->n_runs;
        a.pos = (uint32_t *)b->pos.p; a.baf = (uint64_t *)b->baf.p; a.run = (uint32_t *)b->run.p; a.key = (uint64_t *)b->key.p;
        a.run_first = aw.run_first; a.run_line_off = aw.run_line_off; a.run_chrom_len = aw.run_chrom_len;
        {
            TimerScope ts(ctx, CSV_K_MISC);
            launch_snp_append(s, a);
        }
        CSV_HIP(ctx, hipGetLastError());
        if ((rc = t.down(out->run_first, aw.run_first, (size_t)R * 4)) || (rc = t.down(out->run_line_off, aw.run_line_off, (size_t)R * 4)) ||
            (rc = t.down(out->run_chrom_len, aw.run_chrom_len, (size_t)R * 4))) return rc;
    }
    if ((rc = t.down(out->defer_off, w.out.defer_off, (size_t)D * 4)) || (rc = t.wait())) return rc;
    // (only now: a failure above leaves the tail where it was, and whatever was written behind it is written again)
    b->n += K; b->n_runs += R;
    b->max_key = std::max(b->max_key, text_base + len - 1);
    return CSV_OK;
}

const csv_snp_columns::Contig *contig_of(const csv_snp_columns *cols, uint32_t id)
{
    auto it = std::lower_bound(cols->contigs.begin(), cols->contigs.end(), id, [](const csv_snp_columns::Contig &c, uint32_t v) { return c.id < v; });
    return it != cols->contigs.end() && it->id == id ? &*it : nullptr;
}

int af_parse(csv_ctx *ctx, bool dev, const csv_snp_columns *cols, uint32_t contig_id, const uint8_t *text, uint64_t len, const char *contig, uint32_t contig_len,
             const char *needle, uint32_t needle_len, const csv_vcf_out *out, csv_vcf_counts *counts)
{
    if (!ctx) return CSV_EINVAL;
    const char *who = "snp_columns_af_parse";
    if (!cols) return bad(ctx, who, "null pointer");
    if (cols->device != ctx->device) return bad(ctx, who, "columns of another device");
    const csv_snp_columns::Contig *c = contig_of(cols, contig_id);
    if (!c) return bad(ctx, who, "a contig that holds no record");
    if (!c->ascending) return bad(ctx, who, "a contig that is not ascending");
    return vcf_af_parse_sorted_dev(ctx, dev, text, len, contig, contig_len, needle, needle_len, cols->pos + c->first, c->count, out, counts);
}

}  // namespace

csv_snp_builder *csvgpu_snp_builder_create(csv_ctx *ctx, uint64_t reserve_records)
{
    if (!ctx) return nullptr;
    if (reserve_records >= 0xffffffffull) { ctx->err = "snp_builder_create: 2^32 - 1 records or more"; return nullptr; }
    if (hipSetDevice(ctx->device) != hipSuccess) { (void)hipGetLastError(); ctx->err = "snp_builder_create: no device"; return nullptr; }
    csv_snp_builder *b = new (std::nothrow) csv_snp_builder();
    if (!b) { ctx->err = "snp_builder_create: no memory"; return nullptr; }
    b->device = ctx->device;
    if (reserve_records && ensure_records(ctx, b, reserve_records) != CSV_OK) { builder_release(b); return nullptr; }
    return b;
}

int csvgpu_snp_builder_append(csv_ctx *ctx, csv_snp_builder *b, const uint8_t *text, uint64_t len, uint64_t text_base, int dp_int, int ad_int,
                              const csv_snp_runs *out, csv_snp_append_counts *counts)
{
    return append_text(ctx, b, false, text, len, text_base, dp_int, ad_int, out, counts);
}

int csvgpu_snp_builder_append_dev(csv_ctx *ctx, csv_snp_builder *b, const uint8_t *d_text, uint64_t len, uint64_t text_base, int dp_int, int ad_int,
                                  const csv_snp_runs *out, csv_snp_append_counts *counts)
{
    return append_text(ctx, b, true, d_text, len, text_base, dp_int, ad_int, out, counts);
}

int csvgpu_snp_builder_append_host(csv_ctx *ctx, csv_snp_builder *b, uint64_t n, const uint32_t *contig_id, const uint64_t *order_key, const uint32_t *pos,
                                   const double *baf)
{
    if (!ctx) return CSV_EINVAL;
    const char *who = "snp_builder_append_host";
    if (!b) return bad(ctx, who, "null pointer");
    if (n && (!contig_id || !order_key || !pos || !baf)) return bad(ctx, who, "null array with a count");
    if (b->device != ctx->device) return bad(ctx, who, "a builder of another device");
    if (n >= 0xffffffffull) return bad(ctx, who, "2^32 - 1 records or more");
    uint64_t max_key = b->max_key;
    uint32_t max_id = b->max_host_id;
    std::vector<uint32_t> run(n);
    for (uint64_t i = 0; i < n; i++) {
        if (contig_id[i] >= snpbuild::ID_LIMIT) return bad(ctx, who, "a contig id at or above 2^16");
        if (order_key[i] >= snpbuild::KEY_LIMIT) return bad(ctx, who, "an order key at or above 2^48");
        run[i] = snpbuild::HOST_TAG | contig_id[i];
        max_key = std::max(max_key, order_key[i]); max_id = std::max(max_id, contig_id[i]);
    }
    if (n == 0) return CSV_OK;
    (void)hipSetDevice(ctx->device);
    int rc;
    if ((rc = ensure_records(ctx, b, n))) return rc;
    Transfer t(ctx);
    if ((rc = t.open(who))) return rc;
    if ((rc = t.up(b->pos.p + b->n * 4, pos, n * 4)) || (rc = t.up(b->baf.p + b->n * 8, baf, n * 8)) || (rc = t.up(b->run.p + b->n * 4, run.data(), n * 4)) ||
        (rc = t.up(b->key.p + b->n * 8, order_key, n * 8)) || (rc = t.wait())) return rc;
    b->n += n; b->max_key = max_key; b->max_host_id = max_id;
    return CSV_OK;
}

void csvgpu_snp_builder_destroy(csv_ctx *ctx, csv_snp_builder *b)
{
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    builder_release(b);
}

csv_snp_columns *csvgpu_snp_builder_finish(csv_ctx *ctx, csv_snp_builder *b, const uint32_t *run_contig, uint64_t n_runs)
{
    if (!b) { if (ctx) ctx->err = "snp_builder_finish: null pointer"; return nullptr; }
    (void)hipSetDevice(b->device);
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    struct Release { csv_snp_builder *b; ~Release() { builder_release(b); } } consumed{b};
    if (!ctx) return nullptr;
    const char *who = "snp_builder_finish";
    auto fail = [&](const std::string &msg) { ctx->err = std::string(who) + ": " + msg; return (csv_snp_columns *)nullptr; };
    if (b->device != ctx->device) return fail("a builder of another device");
    if (n_runs != b->n_runs) return fail("n_runs is not the builder's run count");
    if (n_runs && !run_contig) return fail("null array with a count");
    uint32_t max_id = b->max_host_id;
    for (uint64_t r = 0; r < n_runs; r++) {
        if (run_contig[r] >= snpbuild::ID_LIMIT) return fail("a contig id at or above 2^16");
        max_id = std::max(max_id, run_contig[r]);
    }
    const uint64_t n = b->n;
    if (n >= 0xffffffffull) return fail("2^32 - 1 records or more");
    std::unique_ptr<csv_snp_columns> cols(new (std::nothrow) csv_snp_columns());
    if (!cols) return fail("no memory");
    cols->device = ctx->device;
    if (n == 0) return cols.release();
    const uint64_t C = (uint64_t)max_id + 1;
    const int shift = snpbuild::bits_for(b->max_key), key_bits = std::max(1, shift + snpbuild::bits_for(max_id));
    struct { uint32_t *run_contig, *first, *end, *desc, *dup; SortWs sw; } w{};
    if (arena_reserve_for(ctx, ctx->arena, who, [&](Arena &a) {
            return take(a, w.run_contig, n_runs * 4) && take(a, w.first, C * 4) && take(a, w.end, C * 4) && take(a, w.desc, C * 4) && take(a, w.dup, 256) &&
                   sortws_carve(a, n, w.sw);
        })) return nullptr;
    const size_t o_baf = align_up(n * 4, 256), bytes = o_baf + align_up(n * 8, 256);
    char *blk = nullptr;
    if (test_fail_alloc() || hipMalloc((void **)&blk, bytes) != hipSuccess) { (void)hipGetLastError(); return fail("hipMalloc failed"); }
    hipStream_t s = ctx->stream;
    auto release = [&](const std::string &msg) { (void)hipStreamSynchronize(s); (void)hipFree(blk); return msg.empty() ? (csv_snp_columns *)nullptr : fail(msg); };
    Transfer t(ctx);
    if (t.open(who)) { (void)hipFree(blk); return nullptr; }
    // (first | end | desc | dup are carved back to back)
    if (hipMemsetAsync(w.first, 0, (size_t)((char *)w.dup - (char *)w.first) + 256, s) != hipSuccess) return release("memset failed");
    if (n_runs && t.up(w.run_contig, run_contig, n_runs * 4)) return release("");
    uint32_t *d_pos = (uint32_t *)blk; uint64_t *d_baf = (uint64_t *)(blk + o_baf);
    const uint32_t *gave_up = nullptr;
    {
        TimerScope ts(ctx, CSV_K_MISC);
        launch_snp_keys(s, (const uint32_t *)b->run.p, (const uint64_t *)b->key.p, w.run_contig, (uint32_t)n, shift, w.sw.k0, w.sw.v0);
        const int io = launch_radix_sort_u64(s, w.sw.k0, w.sw.v0, w.sw.k1, w.sw.v1, n, key_bits, w.sw.tmp, onesweep(ctx));
        gave_up = radix_sort_gave_up(w.sw.tmp, n, key_bits, onesweep(ctx));
        launch_snp_columns(s, io ? w.sw.k1 : w.sw.k0, io ? w.sw.v1 : w.sw.v0, (const uint32_t *)b->pos.p, (const uint64_t *)b->baf.p, (uint32_t)n, shift, d_pos, d_baf,
                           w.first, w.end, w.desc, w.dup);
    }
    if (hipGetLastError() != hipSuccess) return release("a kernel launch failed");
    uint32_t gave = 0, dup = 0;
    if (gave_up && n > 1 && t.peek(&gave, gave_up, 4)) return release("");
    std::vector<uint32_t> first(C), end(C), desc(C);
    if (t.down(first.data(), w.first, C * 4) || t.down(end.data(), w.end, C * 4) || t.down(desc.data(), w.desc, C * 4) || t.peek(&dup, w.dup, 4)) return release("");
    if (gave) { release(""); ctx->err = "snp_builder_finish: a radix pass gave up"; return nullptr; }
    if (dup) return release("two records of a contig share an order key");
    uint64_t total = 0;
    for (uint64_t id = 0; id < C; id++) {
        if (end[id] == 0) continue;                                           // (a contig that holds a record ends behind slot 0)
        if (end[id] <= first[id] || end[id] > n) return release("the contigs' slots leave the records");
        cols->contigs.push_back({(uint32_t)id, first[id], (uint64_t)end[id] - first[id], desc[id] == 0});
        total += end[id] - first[id];
    }
    if (total != n) return release("the contigs' counts are not the records");
    cols->block = blk; cols->pos = d_pos; cols->baf = d_baf; cols->n = n;
    return cols.release();
}

int csvgpu_snp_columns_describe(const csv_snp_columns *cols, uint64_t cap, uint32_t *contig_id, uint64_t *count, uint8_t *ascending, uint64_t *n_contigs)
{
    if (!cols || !n_contigs) return CSV_EINVAL;
    *n_contigs = cols->contigs.size();
    if (cap < cols->contigs.size()) return CSV_ECAPACITY;
    for (size_t i = 0; i < cols->contigs.size(); i++) {
        if (contig_id) contig_id[i] = cols->contigs[i].id;
        if (count) count[i] = cols->contigs[i].count;
        if (ascending) ascending[i] = cols->contigs[i].ascending;
    }
    return CSV_OK;
}

int csvgpu_snp_columns_fetch(csv_ctx *ctx, const csv_snp_columns *cols, uint32_t contig_id, uint32_t *pos, double *baf)
{
    if (!ctx) return CSV_EINVAL;
    const char *who = "snp_columns_fetch";
    if (!cols) return bad(ctx, who, "null pointer");
    if (cols->device != ctx->device) return bad(ctx, who, "columns of another device");
    const csv_snp_columns::Contig *c = contig_of(cols, contig_id);
    if (!c) return bad(ctx, who, "a contig that holds no record");
    (void)hipSetDevice(ctx->device);
    Transfer t(ctx);
    int rc;
    if ((rc = t.open(who)) || (rc = t.down(pos, cols->pos + c->first, c->count * 4)) || (rc = t.down(baf, cols->baf + c->first, c->count * 8))) return rc;
    return t.wait();
}

int csvgpu_snp_columns_af_parse(csv_ctx *ctx, const csv_snp_columns *cols, uint32_t contig_id, const uint8_t *text, uint64_t len, const char *contig,
                                uint32_t contig_len, const char *needle, uint32_t needle_len, const csv_vcf_out *out, csv_vcf_counts *counts)
{
    return af_parse(ctx, false, cols, contig_id, text, len, contig, contig_len, needle, needle_len, out, counts);
}

int csvgpu_snp_columns_af_parse_dev(csv_ctx *ctx, const csv_snp_columns *cols, uint32_t contig_id, const uint8_t *d_text, uint64_t len, const char *contig,
                                    uint32_t contig_len, const char *needle, uint32_t needle_len, const csv_vcf_out *d_out, csv_vcf_counts *counts)
{
    return af_parse(ctx, true, cols, contig_id, d_text, len, contig, contig_len, needle, needle_len, d_out, counts);
}

csv_snp_table *csvgpu_snp_columns_table(csv_ctx *ctx, const csv_snp_columns *cols, uint32_t contig_id, const uint32_t *af_pos, const double *af, uint64_t n_af)
{
    if (!ctx) return nullptr;
    auto fail = [&](const char *msg) { ctx->err = std::string("snp_columns_table: ") + msg; return (csv_snp_table *)nullptr; };
    if (!cols) return fail("null pointer");
    if (cols->device != ctx->device) return fail("columns of another device");
    const csv_snp_columns::Contig *c = contig_of(cols, contig_id);
    if (!c) return fail("a contig that holds no record");
    if (!c->ascending) return fail("positions are not ascending");
    return snp_table_hits_mixed(ctx, "snp_columns_table", cols->pos + c->first, (const double *)(cols->baf + c->first), af_pos, af, c->count, n_af);
}

void csvgpu_snp_columns_free(csv_ctx *ctx, csv_snp_columns *cols)
{
    if (!cols) return;
    (void)hipSetDevice(cols->device);
    if (ctx) (void)hipStreamSynchronize(ctx->stream);
    (void)hipFree(cols->block);
    delete cols;
}
