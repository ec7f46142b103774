// vcf.hip — VCF text lines parsed on the device (kernels/vcfparse.hip): the checks of the arguments, the two read-backs (the text's line
// ends, which size the per-line workspace; the counts, held against the caller's capacities before anything is written), and for the
// host-pointer form the pieced copies through the page-locked block (a Transfer, glue.hpp). The count of the line ends (count_lines) also
// serves fasta.hip. Replaces, with the kernels, what the host reader does per line in SNPFile::load and SNPFile::table (host/snp_io.cpp:
// snp_record_of_line, af_record_of_line).
#include "glue.hpp"

using namespace csv;

namespace {

int bad(csv_ctx *ctx, const char *msg) { ctx->err = std::string("vcf_parse: ") + msg; return CSV_EINVAL; }

struct Call {                                             // one call's arguments, host side
    bool af = false, io = false;
    int dp_int = 0, ad_int = 0;
    const char *contig = nullptr, *needle = nullptr; uint32_t contig_len = 0, needle_len = 0;
    const uint32_t *sorted_pos = nullptr; uint64_t n = 0;   // io: host array, else device
    bool sorted_dev = false;                              // io with sorted_pos on the device all the same (a contig's resident column)
};

int check_args(csv_ctx *ctx, const uint8_t *text, uint64_t len, const Call &c, const csv_vcf_out *out, csv_vcf_counts *counts)
{
    if (!out || !counts) return bad(ctx, "null pointer");
    if (len >= (1ull << 32)) return bad(ctx, "a text of 2^32 bytes or more");
    if (len && !text) return bad(ctx, "null pointer");
    if ((out->cap && (!out->line_off || !out->pos || !out->value || (!c.af && !out->chrom_len))) || (out->cap_defer && !out->defer_off)) return bad(ctx, "null pointer");
    if (c.af) {
        if (!c.needle || (c.contig_len && !c.contig) || (c.n && !c.sorted_pos)) return bad(ctx, "null pointer");
        if (c.needle_len == 0 || c.needle_len > 64) return bad(ctx, "needle_len 0 or above 64");
        for (uint32_t i = 0; i < c.needle_len; i++)
            if (c.needle[i] == '\t' || c.needle[i] == '\n' || c.needle[i] == '\r') return bad(ctx, "a needle with a tab or a line end in it");
        if (c.n >= (1ull << 32)) return bad(ctx, "2^32 positions or more");
        if (c.io && !c.sorted_dev) for (uint64_t i = 1; i < c.n; i++) if (c.sorted_pos[i] < c.sorted_pos[i - 1]) return bad(ctx, "sorted_pos not ascending");
    }
    return CSV_OK;
}

}  // namespace

namespace csv {

int count_lines(csv_ctx *ctx, Transfer &t, const char *what, const char *too_many, const uint8_t *d_text, uint32_t len, const VcfWs &w,
                const std::function<bool(Arena &, uint64_t)> &carve, const std::function<int()> &first_pass, uint32_t &n_slots)
{
    const uint32_t n_tiles = vcf_tiles(d_text, len);
    int rc;
    if ((rc = arena_reserve_for(ctx, ctx->work, what, [&](Arena &a) { return carve(a, 0); }))) return rc;
    if ((rc = first_pass())) return rc;
    uint32_t n_ends = 0;
    if ((rc = t.peek(&n_ends, w.tile_cnt + n_tiles, 4))) return rc;
    if (n_ends > len) { ctx->err = std::string(what) + ": the line ends' count leaves the text"; return CSV_EHIP; }
    if (n_ends == UINT32_MAX) { ctx->err = too_many; return CSV_EINVAL; }
    n_slots = n_ends + 1;
    // The per-line arrays behind the first carve's slices, which keep their contents unless the arena had to grow: a grown arena is a new
    // allocation (possibly at the old address, so the pointer says nothing; the capacity rises with every growth) and they are made again.
    const size_t cap_before = ctx->work.cap;
    if ((rc = arena_reserve_for(ctx, ctx->work, what, [&](Arena &a) { return carve(a, n_slots); }))) return rc;
    return ctx->work.cap != cap_before ? first_pass() : (int)CSV_OK;
}

}  // namespace csv

namespace {

// What the entry points share. d_text / d_sorted: on the device; d_out: the caller's device arrays, or null for the workspace's staged ones
// (io). Returns CSV_OK (the last kernel queued, not waited for) / 1 (declined) / CSV_E*. w: the carved workspace.
int run_parse(csv_ctx *ctx, Transfer &t, const uint8_t *d_text, uint32_t len, const Call &c, const uint32_t *d_sorted, const VcfOut *d_out, const csv_vcf_out &caps,
              csv_vcf_counts &cnt, VcfWs &w)
{
    hipStream_t s = ctx->stream;
    const uint32_t n_tiles = vcf_tiles(d_text, len);
    const uint64_t n_strings = c.af ? (uint64_t)c.contig_len + c.needle_len : 0;
    std::vector<uint8_t> strings(n_strings);
    if (c.af) { if (c.contig_len) memcpy(strings.data(), c.contig, c.contig_len); memcpy(strings.data() + c.contig_len, c.needle, c.needle_len); }
    int rc;
    uint32_t n_slots = 0;
    if ((rc = count_lines(ctx, t, "vcf_parse", "vcf_parse: 2^32 lines or more", d_text, len, w,
                          [&](Arena &a, uint64_t slots) { return carve_vcf(a, n_tiles, n_strings, slots, c.io, c.af, caps.cap, caps.cap_defer, w); },
                          [&]() -> int {                 // the strings up, the line ends counted (the timer around the launch alone)
                              const int rc2 = n_strings ? t.up(w.strings, strings.data(), n_strings) : (int)CSV_OK;
                              if (rc2) return rc2;
                              TimerScope ts(ctx, CSV_K_MISC);
                              launch_vcf_count(s, d_text, len, w);
                              return CSV_OK;
                          }, n_slots))) return rc;
    VcfParseArgs a{};
    a.af = c.af; a.dp_int = c.dp_int != 0; a.ad_int = c.ad_int != 0;
    a.contig = w.strings; a.needle = w.strings + c.contig_len; a.contig_len = c.contig_len; a.needle_len = c.needle_len;
    a.sorted_pos = d_sorted; a.n_sorted = c.n;
    {
        TimerScope ts(ctx, CSV_K_MISC);
        launch_vcf_starts(s, d_text, len, w);
        launch_vcf_parse(s, d_text, len, n_slots, a, 0, w);
    }
    VcfHead h;
    if ((rc = t.peek(&h, w.head, sizeof(VcfHead)))) return rc;
    cnt = csv_vcf_counts{};
    if (h.hash_off < (unsigned long long)h.stop_off) { cnt.status = (h.hash_off << 8) | CSV_VCF_HEADER_LINE; return 1; }
    if (h.n_kept > n_slots || h.n_defer > n_slots || h.n_lines > n_slots) { ctx->err = "vcf_parse: the counts leave the text"; return CSV_EHIP; }
    cnt.n_lines = h.n_lines; cnt.n_kept = h.n_kept; cnt.n_deferred = h.n_defer;
    cnt.stop_off = h.stop_off == 0xffffffffu ? UINT64_MAX : h.stop_off;
    if (cnt.n_kept > caps.cap || cnt.n_deferred > caps.cap_defer) { ctx->err = "vcf_parse: output capacity too small"; return CSV_ECAPACITY; }
    {
        TimerScope ts(ctx, CSV_K_MISC);
        launch_vcf_emit(s, n_slots, c.af, w, d_out ? *d_out : w.out);
    }
    CSV_HIP(ctx, hipGetLastError());
    return CSV_OK;
}

int parse_dev(csv_ctx *ctx, const uint8_t *d_text, uint64_t len, const Call &c, const csv_vcf_out *d_out, csv_vcf_counts *counts)
{
    if (!ctx) return CSV_EINVAL;
    int rc = check_args(ctx, d_text, len, c, d_out, counts);
    if (rc) return rc;
    *counts = csv_vcf_counts{};
    counts->stop_off = UINT64_MAX;
    if (len == 0) return CSV_OK;
    (void)hipSetDevice(ctx->device);
    Transfer t(ctx);
    if ((rc = t.open("vcf_parse"))) return rc;
    VcfWs w;
    const VcfOut o{d_out->line_off, d_out->chrom_len, d_out->pos, d_out->value, d_out->defer_off};
    rc = run_parse(ctx, t, d_text, (uint32_t)len, c, c.sorted_pos, &o, *d_out, *counts, w);
    return rc == CSV_OK ? t.wait() : rc;                                  // (the caller's device arrays are complete on return)
}

int parse_host(csv_ctx *ctx, const uint8_t *text, uint64_t len, const Call &c, const csv_vcf_out *out, csv_vcf_counts *counts)
{
    if (!ctx) return CSV_EINVAL;
    int rc = check_args(ctx, text, len, c, out, counts);
    if (rc) return rc;
    *counts = csv_vcf_counts{};
    counts->stop_off = UINT64_MAX;
    if (len == 0) return CSV_OK;
    (void)hipSetDevice(ctx->device);
    VcfTextWs tw;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "vcf_parse", [&](Arena &a) { return carve_vcf_text(a, len, c.sorted_dev ? 0 : c.n, tw); }))) return rc;
    Transfer t(ctx);
    if ((rc = t.open("vcf_parse"))) return rc;
    if ((rc = t.up(tw.text, text, len))) return rc;
    if (c.n && !c.sorted_dev && (rc = t.up(tw.sorted_pos, c.sorted_pos, c.n * 4))) return rc;
    VcfWs w;
    if ((rc = run_parse(ctx, t, tw.text, (uint32_t)len, c, c.sorted_dev ? c.sorted_pos : tw.sorted_pos, nullptr, *out, *counts, w))) return rc;
    const uint64_t k = counts->n_kept, d = counts->n_deferred;
    if ((rc = t.down(out->line_off, w.out.line_off, k * 4)) || (rc = t.down(out->pos, w.out.pos, k * 4)) || (rc = t.down(out->value, w.out.value, k * 8)) ||
        (rc = t.down(out->defer_off, w.out.defer_off, d * 4))) return rc;
    if (!c.af && (rc = t.down(out->chrom_len, w.out.chrom_len, k * 4))) return rc;
    return t.wait();
}

Call snp_call(int dp_int, int ad_int, bool io) { Call c; c.io = io; c.dp_int = dp_int; c.ad_int = ad_int; return c; }
Call af_call(const char *contig, uint32_t contig_len, const char *needle, uint32_t needle_len, const uint32_t *sorted_pos, uint64_t n, bool io)
{
    Call c;
    c.af = true; c.io = io; c.contig = contig; c.contig_len = contig_len; c.needle = needle; c.needle_len = needle_len; c.sorted_pos = sorted_pos; c.n = n;
    return c;
}

}  // namespace

int csvgpu_vcf_snp_parse(csv_ctx *ctx, const uint8_t *text, uint64_t len, int dp_int, int ad_int, const csv_vcf_out *out, csv_vcf_counts *counts)
{
    return parse_host(ctx, text, len, snp_call(dp_int, ad_int, true), out, counts);
}

int csvgpu_vcf_snp_parse_dev(csv_ctx *ctx, const uint8_t *d_text, uint64_t len, int dp_int, int ad_int, const csv_vcf_out *d_out, csv_vcf_counts *counts)
{
    return parse_dev(ctx, d_text, len, snp_call(dp_int, ad_int, false), d_out, counts);
}

int csvgpu_vcf_af_parse(csv_ctx *ctx, const uint8_t *text, uint64_t len, const char *contig, uint32_t contig_len, const char *needle, uint32_t needle_len,
                        const uint32_t *sorted_pos, uint64_t n, const csv_vcf_out *out, csv_vcf_counts *counts)
{
    return parse_host(ctx, text, len, af_call(contig, contig_len, needle, needle_len, sorted_pos, n, true), out, counts);
}

int csvgpu_vcf_af_parse_dev(csv_ctx *ctx, const uint8_t *d_text, uint64_t len, const char *contig, uint32_t contig_len, const char *needle, uint32_t needle_len,
                            const uint32_t *d_sorted_pos, uint64_t n, const csv_vcf_out *d_out, csv_vcf_counts *counts)
{
    return parse_dev(ctx, d_text, len, af_call(contig, contig_len, needle, needle_len, d_sorted_pos, n, false), d_out, counts);
}

namespace csv {

int vcf_snp_stage(csv_ctx *ctx, Transfer &t, const uint8_t *d_text, uint32_t len, int dp_int, int ad_int, csv_vcf_counts &cnt, VcfWs &w)
{
    csv_vcf_out caps{};
    caps.cap = caps.cap_defer = UINT64_MAX;                 // (the staged arrays hold a record per line at the most)
    return run_parse(ctx, t, d_text, len, snp_call(dp_int, ad_int, true), nullptr, nullptr, caps, cnt, w);
}

int vcf_af_parse_sorted_dev(csv_ctx *ctx, bool dev_text, const uint8_t *text, uint64_t len, const char *contig, uint32_t contig_len, const char *needle,
                            uint32_t needle_len, const uint32_t *d_sorted_pos, uint64_t n, const csv_vcf_out *out, csv_vcf_counts *counts)
{
    Call c = af_call(contig, contig_len, needle, needle_len, d_sorted_pos, n, !dev_text);
    c.sorted_dev = true;
    return dev_text ? parse_dev(ctx, text, len, c, out, counts) : parse_host(ctx, text, len, c, out, counts);
}

}  // namespace csv
