// vcf_format.hip — the VCF writer's record lines on the device (csvgpu_vcf_format / _dev): the batch's tables staged in the context's arena,
// the sizing pass, ONE readback of the head (the text's bytes, the counts, the first refused call), the write pass, and the text's way down.
// The rules are vcf_format_core.hpp, the kernels kernels/vcfformat.hip. Replaces the record loop of writeVCF (host/vcf_writer.cpp; the
// reference's SVCaller::saveToVCF, sv_caller.cpp:1067-1330, with ::getReadDepth, :1332-1344); the header stays the host's.
#include "../vcf_format_core.hpp"
#include "glue.hpp"

using namespace csv;

static_assert(sizeof(csv_vcf_call) == sizeof(vcffmt::Call) && offsetof(csv_vcf_call, start) == offsetof(vcffmt::Call, start) && offsetof(csv_vcf_call, end) == offsetof(vcffmt::Call, end) &&
              offsetof(csv_vcf_call, sv_type) == offsetof(vcffmt::Call, sv_type) && offsetof(csv_vcf_call, cluster_size) == offsetof(vcffmt::Call, cluster_size) &&
              offsetof(csv_vcf_call, hmm_likelihood) == offsetof(vcffmt::Call, hmm_likelihood) && offsetof(csv_vcf_call, id) == offsetof(vcffmt::Call, id) &&
              offsetof(csv_vcf_call, aln_flags) == offsetof(vcffmt::Call, aln_flags) && offsetof(csv_vcf_call, genotype) == offsetof(vcffmt::Call, genotype) &&
              offsetof(csv_vcf_call, cn_state) == offsetof(vcffmt::Call, cn_state) && offsetof(csv_vcf_call, aln_offset) == offsetof(vcffmt::Call, aln_offset),
              "csv_vcf_call is the core's Call");

namespace {

int bad(csv_ctx *ctx, const char *msg) { ctx->err = msg; return CSV_EINVAL; }

int vcf_format_run(csv_ctx *ctx, const csv_genome *g, const csv_vcf_contig *contigs, uint32_t n_contigs, const uint64_t *call_off, const csv_vcf_call *calls,
                   const uint64_t *alt_off, const char *alts, const char *method, uint32_t method_len, uint64_t cap, char *text, bool dev_text, uint8_t *line_status,
                   csv_vcf_format_counts *counts)
{
    if (!ctx) return CSV_EINVAL;
    if (!g || !counts) return bad(ctx, "vcf_format: null argument");
    if (g->device != ctx->device) return bad(ctx, "vcf_format: the genome lives on another device");
    if (n_contigs && (!contigs || !call_off)) return bad(ctx, "vcf_format: null array");
    if (method_len > vcffmt::kMethodMax || (method_len && !method)) return bad(ctx, "vcf_format: a method string of more than 64 bytes, or none");
    if (cap && !text) return bad(ctx, "vcf_format: null output");
    if (n_contigs && call_off[0] != 0) return bad(ctx, "vcf_format: call_off must start at 0");
    for (uint32_t t = 0; t < n_contigs; t++)
        if (call_off[t + 1] < call_off[t]) return bad(ctx, "vcf_format: call_off decreases");
    const uint64_t n = n_contigs ? call_off[n_contigs] : 0;
    if (n >= 0xffffffffull) return bad(ctx, "vcf_format: 2^32 - 1 calls or more");
    if (n && (!calls || !alt_off)) return bad(ctx, "vcf_format: null array");
    for (uint64_t i = 0; i < n; i++)
        if (alt_off[i + 1] < alt_off[i]) return bad(ctx, "vcf_format: alt_off decreases");
    const uint64_t alt_base = n ? alt_off[0] : 0, n_alt = n ? alt_off[n] - alt_base : 0;
    if (n_alt && !alts) return bad(ctx, "vcf_format: null array");
    const vcffmt::Call *core_calls = (const vcffmt::Call *)calls;

    // the contigs as the kernels see them; an upper bound of the text from the cuts' lengths (the gap rows and the depth change no length
    // by more than the short fields' bound)
    std::vector<VfContig> tab((size_t)n_contigs + 1);
    std::string names;
    std::vector<uint32_t> gs, ge;
    uint64_t bound = 0;
    for (uint32_t t = 0; t < n_contigs; t++) {
        const csv_vcf_contig &c = contigs[t];
        if ((c.name_len && !c.name) || (c.n_gaps && (!c.gap_start || !c.gap_end))) return bad(ctx, "vcf_format: null array in a contig");
        if (c.genome_record < -1 || c.genome_record >= (int64_t)g->rec.size()) return bad(ctx, "vcf_format: record index beyond the genome");
        VfContig &v = tab[t];
        v.call_first = call_off[t];
        v.name_off = names.size(); v.name_len = c.name_len;
        names.append(c.name ? c.name : "", c.name_len);
        v.gap_first = gs.size(); v.n_gaps = c.n_gaps;
        gs.insert(gs.end(), c.gap_start, c.gap_start + c.n_gaps);
        ge.insert(ge.end(), c.gap_end, c.gap_end + c.n_gaps);
        v.contig_len = c.genome_record < 0 ? -1 : (int64_t)g->rec[(size_t)c.genome_record].len;
        v.rec_start = c.genome_record < 0 ? 0 : g->rec[(size_t)c.genome_record].start;
        v.depth = c.shard ? c.shard->depth : nullptr;
        if (v.depth) {                                    // a shard carries no device of its own: its depth map says where it lies
            hipPointerAttribute_t at;
            if (hipPointerGetAttributes(&at, v.depth) != hipSuccess) { (void)hipGetLastError(); return bad(ctx, "vcf_format: a shard's depth map is no device memory"); }
            if (at.device != ctx->device) return bad(ctx, "vcf_format: a shard lives on another device");
        }
        v.depth_len = c.shard ? c.shard->depth_len : 0;
        v.pad = 0;
        for (uint64_t i = call_off[t]; i < call_off[t + 1]; i++) {
            if (!vcffmt::asks_depth(core_calls[i])) continue;
            if (!v.depth) return bad(ctx, "vcf_format: a contig with a call to write has no shard, or its shard no depth map (run csvgpu_chr_pipeline_dev first)");
            const uint64_t alen = alt_off[i + 1] - alt_off[i];
            const vcffmt::Line L = vcffmt::decide(core_calls[i], v.contig_len, nullptr, nullptr, 0, (const uint8_t *)alts + alt_off[i], alen);
            if (!L.why) bound += (uint64_t)c.name_len + L.ref_len + alen + method_len + vcffmt::kShortMax;
        }
    }
    tab[n_contigs] = VfContig{};
    tab[n_contigs].call_first = n;
    memset(counts, 0, sizeof(*counts));
    if (n == 0) return CSV_OK;

    (void)hipSetDevice(ctx->device);
    const uint64_t room = dev_text ? 0 : std::min(bound, cap);       // (a text above `cap` is never written)
    VfArgs a{};
    VfContig *d_tab = nullptr;
    uint8_t *d_names = nullptr, *d_alts = nullptr, *d_method = nullptr, *d_text = nullptr, *d_calls = nullptr;
    uint32_t *d_gs = nullptr, *d_ge = nullptr;
    uint64_t *d_alt_off = nullptr;
    char *d_head = nullptr;
    // (the one reservation of the call; the test hook stands in front of it, so a failure inside arena_reserve itself — the arena's block
    // freed, the larger one refused — is not what the hook exercises: that path is the arena's, shared with every entry point)
    if (test_fail_alloc()) { ctx->err = "hipMalloc failed (vcf format)"; return CSV_ENOMEM; }
    int rc = arena_reserve_for(ctx, ctx->arena, "vcf_format", [&](Arena &ar) {
        return take(ar, d_tab, tab.size() * sizeof(VfContig)) && take(ar, d_names, names.size() + 16) && take(ar, d_gs, gs.size() * 4 + 16) && take(ar, d_ge, ge.size() * 4 + 16) &&
               take(ar, d_calls, n * sizeof(csv_vcf_call)) && take(ar, d_alt_off, (n + 1) * 8) && take(ar, d_alts, n_alt + 16) && take(ar, d_method, (size_t)method_len + 16) &&
               take(ar, a.len, (n + 1) * 4) && take(ar, a.depth, n * 4) && take(ar, a.status, n) && take(ar, d_head, 256) && take(ar, a.es_tmp, exclusive_sum_tmp_bytes(n + 1)) &&
               take(ar, d_text, room + 16);
    });
    if (rc) return rc;
    std::vector<uint64_t> rel((size_t)n + 1);
    for (uint64_t i = 0; i <= n; i++) rel[i] = alt_off[i] - alt_base;
    VfHead h{};
    h.first_refused = ~0ull;
    Transfer t(ctx);
    if ((rc = t.open("vcf_format"))) return rc;
    if ((rc = t.up(d_tab, tab.data(), tab.size() * sizeof(VfContig))) || (rc = t.up(d_names, names.data(), names.size())) || (rc = t.up(d_gs, gs.data(), gs.size() * 4)) ||
        (rc = t.up(d_ge, ge.data(), ge.size() * 4)) || (rc = t.up(d_calls, calls, n * sizeof(csv_vcf_call))) || (rc = t.up(d_alt_off, rel.data(), (n + 1) * 8)) ||
        (rc = t.up(d_alts, alts ? alts + alt_base : nullptr, n_alt)) || (rc = t.up(d_method, method, method_len)) || (rc = t.up(d_head, &h, sizeof(h)))) return rc;
    a.contig = d_tab; a.n_contigs = n_contigs; a.calls = d_calls; a.n_calls = n; a.alt_off = d_alt_off; a.alts = d_alts; a.names = d_names; a.method = d_method;
    a.method_len = method_len; a.gap_start = d_gs; a.gap_end = d_ge; a.seq = (const uint8_t *)g->seq; a.head = (VfHead *)d_head;
    hipStream_t s = ctx->stream;
    {
        TimerScope ts(ctx, CSV_K_MISC);
        launch_vcf_format_size(s, a);
    }
    CSV_HIP(ctx, hipGetLastError());
    if ((rc = t.peek(&h, d_head, sizeof(h)))) return rc;                     // the one readback that decides everything
    if (h.first_refused != ~0ull) { counts->declined_why = (uint32_t)(h.first_refused & 0xff); return 1; }
    if (h.text_bytes >= (1ull << 32)) { counts->declined_why = vcffmt::WHY_TEXT_BYTES; return 1; }
    counts->text_bytes = h.text_bytes; counts->n_lines = h.n_lines; counts->total = h.total; counts->unclassified = h.unclassified; counts->gap_filtered = h.gap_filtered;
    if (h.n_lines > n || h.text_bytes > bound) { ctx->err = "vcf_format: the counts leave the batch"; return CSV_EHIP; }
    if (h.text_bytes > cap) { ctx->err = "vcf_format: output capacity too small"; return CSV_ECAPACITY; }
    if (line_status && (rc = t.down(line_status, a.status, n))) return rc;
    if (h.text_bytes == 0) return CSV_OK;
    {
        TimerScope ts(ctx, CSV_K_MISC);
        launch_vcf_format_write(s, a, h.text_bytes, dev_text ? (uint8_t *)text : d_text);
    }
    CSV_HIP(ctx, hipGetLastError());
    return dev_text ? t.wait() : t.down(text, d_text, h.text_bytes);
}

}  // namespace

int csvgpu_vcf_format(csv_ctx *ctx, const csv_genome *g, const csv_vcf_contig *contigs, uint32_t n_contigs, const uint64_t *call_off, const csv_vcf_call *calls,
                      const uint64_t *alt_off, const char *alts, const char *method, uint32_t method_len, uint64_t cap, char *text, uint8_t *line_status,
                      csv_vcf_format_counts *counts)
{
    return vcf_format_run(ctx, g, contigs, n_contigs, call_off, calls, alt_off, alts, method, method_len, cap, text, false, line_status, counts);
}

int csvgpu_vcf_format_dev(csv_ctx *ctx, const csv_genome *g, const csv_vcf_contig *contigs, uint32_t n_contigs, const uint64_t *call_off, const csv_vcf_call *calls,
                          const uint64_t *alt_off, const char *alts, const char *method, uint32_t method_len, uint64_t cap, char *d_text, uint8_t *line_status,
                          csv_vcf_format_counts *counts)
{
    return vcf_format_run(ctx, g, contigs, n_contigs, call_off, calls, alt_off, alts, method, method_len, cap, d_text, true, line_status, counts);
}
