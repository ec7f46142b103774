// copynumber.hip — windows of log2 coverage, Viterbi decoding, and the copy-number observations built on the device.
#include "glue.hpp"

using namespace csv;

int csvgpu_window_log2_dev(csv_ctx *ctx, const uint32_t *d_depth, uint32_t depth_len, const uint32_t *d_rs, const uint32_t *d_re,
                           const int32_t *d_ss, const uint64_t *d_win_off, uint64_t n_regions, uint64_t n_windows,
                           double mean_cov, double *d_log2, uint32_t *d_ws, uint32_t *d_we)
{
    if (!ctx) return CSV_EINVAL;
    if (n_regions == 0 || n_windows == 0) return CSV_OK;
    if (!d_depth || !d_rs || !d_re || !d_ss || !d_win_off || !d_log2 || !d_ws || !d_we) { ctx->err = "window_log2: null array"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    TimerScope ts(ctx, CSV_K_WINDOW);
    launch_window_log2(ctx->stream, d_depth, depth_len, d_rs, d_re, d_ss, d_win_off, n_regions, n_windows, mean_cov, d_log2, d_ws, d_we);
    return CSV_OK;
}

static bool region_table_ok(const uint32_t *region_start, const uint32_t *region_end, const int32_t *sample_size, const uint64_t *win_off, uint64_t n_regions)
{
    for (uint64_t r = 0; r < n_regions; r++)
        if (sample_size[r] <= 0 || win_off[r + 1] - win_off[r] != (uint64_t)sample_size[r] || region_start[r] > region_end[r]) return false;
    return true;
}

// Host region tables in, host windows out. The depth map is the caller's (`depth`: staged here, in front of the tables) or a resident shard's
// (`depth` null, d_depth).
static int window_log2_tables(csv_ctx *ctx, const uint32_t *depth, const uint32_t *d_depth, uint32_t depth_len, const uint32_t *region_start,
                              const uint32_t *region_end, const int32_t *sample_size, const uint64_t *win_off, uint64_t n_regions,
                              double mean_cov, double *log2_cov, uint32_t *win_start, uint32_t *win_end)
{
    if (n_regions == 0) return CSV_OK;
    if (!region_start || !region_end || !sample_size || !win_off) { ctx->err = "window_log2: null array"; return CSV_EINVAL; }
    if (!region_table_ok(region_start, region_end, sample_size, win_off, n_regions)) { ctx->err = "window_log2: bad region table"; return CSV_EINVAL; }
    const uint64_t nw = win_off[n_regions];
    if (nw == 0) return CSV_OK;
    if (!log2_cov || !win_start || !win_end) { ctx->err = "window_log2: null output"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    uint32_t *dd = nullptr;
    WindowWs w;
    int rc = arena_reserve_for(ctx, ctx->arena, "window_log2", [&](Arena &a) { return (!depth || take(a, dd, (size_t)depth_len * 4)) && carve_window(a, n_regions, nw, w); });
    if (rc) return rc;
    uint32_t *drs = w.rs, *dre = w.re, *dws = w.ws, *dwe = w.we;
    int32_t *dss = w.ss;
    uint64_t *dwo = w.wo;
    double *dl2 = w.l2;
    hipStream_t s = ctx->stream;
    if (depth) {
        CSV_HIP(ctx, hipMemcpyAsync(dd, depth, (size_t)depth_len * 4, hipMemcpyHostToDevice, s));
        d_depth = dd;
    }
    CSV_HIP(ctx, hipMemcpyAsync(drs, region_start, n_regions * 4, hipMemcpyHostToDevice, s));
    CSV_HIP(ctx, hipMemcpyAsync(dre, region_end, n_regions * 4, hipMemcpyHostToDevice, s));
    CSV_HIP(ctx, hipMemcpyAsync(dss, sample_size, n_regions * 4, hipMemcpyHostToDevice, s));
    CSV_HIP(ctx, hipMemcpyAsync(dwo, win_off, (n_regions + 1) * 8, hipMemcpyHostToDevice, s));
    if ((rc = csvgpu_window_log2_dev(ctx, d_depth, depth_len, drs, dre, dss, dwo, n_regions, nw, mean_cov, dl2, dws, dwe))) return rc;
    CSV_HIP(ctx, hipMemcpyAsync(log2_cov, dl2, nw * 8, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, hipMemcpyAsync(win_start, dws, nw * 4, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, hipMemcpyAsync(win_end, dwe, nw * 4, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, wait_stream(s));
    return CSV_OK;
}

int csvgpu_window_log2(csv_ctx *ctx, const uint32_t *depth, uint32_t depth_len, const uint32_t *region_start,
                       const uint32_t *region_end, const int32_t *sample_size, const uint64_t *win_off, uint64_t n_regions,
                       double mean_cov, double *log2_cov, uint32_t *win_start, uint32_t *win_end)
{
    if (!ctx) return CSV_EINVAL;
    if (n_regions && !depth) { ctx->err = "window_log2: null array"; return CSV_EINVAL; }
    return window_log2_tables(ctx, depth, nullptr, depth_len, region_start, region_end, sample_size, win_off, n_regions, mean_cov, log2_cov, win_start, win_end);
}

int csvgpu_window_log2_resident(csv_ctx *ctx, csv_shard *sh, const uint32_t *region_start, const uint32_t *region_end,
                                const int32_t *sample_size, const uint64_t *win_off, uint64_t n_regions, double mean_cov,
                                double *log2_cov, uint32_t *win_start, uint32_t *win_end)
{
    if (!ctx || !sh) return CSV_EINVAL;
    return window_log2_tables(ctx, nullptr, sh->depth, sh->depth_len, region_start, region_end, sample_size, win_off, n_regions, mean_cov, log2_cov, win_start, win_end);
}

int csvgpu_viterbi_dev(csv_ctx *ctx, const csv_hmm *hmm, const double *d_o1, const double *d_o2, const double *d_pfb,
                       const uint64_t *d_seq_off, uint64_t n_seq, uint64_t n_obs, int32_t *d_states, double *d_loglik)
{
    if (!ctx) return CSV_EINVAL;
    if (!hmm) { ctx->err = "viterbi: null hmm"; return CSV_EINVAL; }
    if (n_seq == 0) return CSV_OK;
    if (!d_seq_off || !d_loglik || (n_obs && (!d_o1 || !d_o2 || !d_pfb || !d_states))) { ctx->err = "viterbi: null array"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    void *tmp = nullptr;
    int rc = arena_reserve_for(ctx, ctx->work, "viterbi", [&](Arena &a) { return take(a, tmp, viterbi_tmp_bytes(n_obs, n_seq)); });
    if (rc) return rc;
    TimerScope ts(ctx, CSV_K_VITERBI);
    launch_viterbi(ctx->stream, *hmm, d_o1, d_o2, d_pfb, d_seq_off, n_seq, n_obs, d_states, d_loglik, tmp);
    return CSV_OK;
}

int csvgpu_viterbi(csv_ctx *ctx, const csv_hmm *hmm, const double *o1, const double *o2, const double *pfb,
                   const uint64_t *seq_off, uint64_t n_seq, int32_t *states, double *loglik)
{
    if (!ctx) return CSV_EINVAL;
    if (!hmm) { ctx->err = "viterbi: null hmm"; return CSV_EINVAL; }
    if (n_seq == 0) return CSV_OK;
    if (!seq_off || !loglik) { ctx->err = "viterbi: null array"; return CSV_EINVAL; }
    for (uint64_t s = 0; s < n_seq; s++) if (seq_off[s + 1] < seq_off[s]) { ctx->err = "viterbi: seq_off not monotone"; return CSV_EINVAL; }
    const uint64_t n = seq_off[n_seq];
    if (n && (!o1 || !o2 || !pfb || !states)) { ctx->err = "viterbi: null array"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    double *d1 = nullptr, *d2 = nullptr, *dp = nullptr, *dll = nullptr;
    uint64_t *doff = nullptr;
    int32_t *dst = nullptr;
    int rc = arena_reserve_for(ctx, ctx->arena, "viterbi arrays", [&](Arena &a) {
        return take(a, d1, n * 8 + 8) && take(a, d2, n * 8 + 8) && take(a, dp, n * 8 + 8) && take(a, doff, (n_seq + 1) * 8) && take(a, dst, n * 4 + 8) && take(a, dll, n_seq * 8);
    });
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    PinStage pin(ctx);
    const void *h1, *h2, *hp, *h_off;
    void *h_states, *h_ll;
    if ((rc = pin_reserve_for(ctx, pin, [&](PinStage &p) {
            h1 = p.in(o1, n * 8); h2 = p.in(o2, n * 8); hp = p.in(pfb, n * 8); h_off = p.in(seq_off, (n_seq + 1) * 8);
            h_states = p.out(states, n * 4); h_ll = p.out(loglik, n_seq * 8);
        }))) return rc;
    if (n) {
        CSV_HIP(ctx, hipMemcpyAsync(d1, h1, n * 8, hipMemcpyHostToDevice, s));
        CSV_HIP(ctx, hipMemcpyAsync(d2, h2, n * 8, hipMemcpyHostToDevice, s));
        CSV_HIP(ctx, hipMemcpyAsync(dp, hp, n * 8, hipMemcpyHostToDevice, s));
    }
    CSV_HIP(ctx, hipMemcpyAsync(doff, h_off, (n_seq + 1) * 8, hipMemcpyHostToDevice, s));
    if ((rc = csvgpu_viterbi_dev(ctx, hmm, d1, d2, dp, doff, n_seq, n, dst, dll))) return rc;
    if (n) CSV_HIP(ctx, hipMemcpyAsync(h_states, dst, n * 4, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, hipMemcpyAsync(h_ll, dll, n_seq * 8, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, wait_stream(s));
    pin.finish();
    return CSV_OK;
}

int csvgpu_window_log2_resident_many(csv_ctx *ctx, int n_shards, csv_shard *const *shards, const uint32_t *const *region_start,
                                     const uint32_t *const *region_end, const int32_t *const *sample_size, const uint64_t *const *win_off,
                                     const uint64_t *n_regions, const double *mean_cov, double *const *log2_cov, uint32_t *const *win_start,
                                     uint32_t *const *win_end)
{
    if (!ctx || n_shards < 0) return CSV_EINVAL;
    if (n_shards == 0) return CSV_OK;
    if (!shards || !region_start || !region_end || !sample_size || !win_off || !n_regions || !mean_cov || !log2_cov || !win_start || !win_end) {
        ctx->err = "window_log2_many: null table"; return CSV_EINVAL;
    }
    uint64_t R = 0, W = 0;
    for (int c = 0; c < n_shards; c++) {
        const uint64_t nr = n_regions[c];
        if (!nr) continue;
        if (!shards[c] || !region_start[c] || !region_end[c] || !sample_size[c] || !win_off[c]) { ctx->err = "window_log2_many: null array"; return CSV_EINVAL; }
        if (win_off[c][0] != 0 || !region_table_ok(region_start[c], region_end[c], sample_size[c], win_off[c], nr)) { ctx->err = "window_log2_many: bad region table"; return CSV_EINVAL; }
        if (win_off[c][nr] && (!log2_cov[c] || !win_start[c] || !win_end[c])) { ctx->err = "window_log2_many: null output"; return CSV_EINVAL; }
        R += nr; W += win_off[c][nr];
    }
    if (W == 0) return CSV_OK;
    (void)hipSetDevice(ctx->device);
    // one page-locked block carries every shard's tables to the device and every shard's windows back
    const size_t in_bytes = align_up(R * 4, 8) * 3 + (R + (size_t)n_shards) * 8, out_bytes = W * 8 + 2 * align_up(W * 4, 8);
    char *h_in = nullptr, *h_out = nullptr, *d_in = nullptr, *d_out = nullptr;
    PinStage pin(ctx);
    int rc = pin_reserve_for(ctx, pin, [&](PinStage &p) { h_in = (char *)p.slot(in_bytes); h_out = (char *)p.slot(out_bytes); });
    if (rc) return rc;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "window_log2_many", [&](Arena &a) { return take(a, d_in, in_bytes) && take(a, d_out, out_bytes); }))) return rc;
    const size_t o_rs = 0, o_re = align_up(R * 4, 8), o_ss = 2 * align_up(R * 4, 8), o_wo = 3 * align_up(R * 4, 8);
    const size_t o_l2 = 0, o_ws = W * 8, o_we = W * 8 + align_up(W * 4, 8);
    uint64_t r0 = 0, w0 = 0;
    for (int c = 0; c < n_shards; c++) {
        const uint64_t nr = n_regions[c];
        if (!nr) continue;
        memcpy(h_in + o_rs + r0 * 4, region_start[c], nr * 4);
        memcpy(h_in + o_re + r0 * 4, region_end[c], nr * 4);
        memcpy(h_in + o_ss + r0 * 4, sample_size[c], nr * 4);
        memcpy(h_in + o_wo + (r0 + (uint64_t)c) * 8, win_off[c], (nr + 1) * 8);
        r0 += nr;
    }
    hipStream_t s = ctx->stream;
    CSV_HIP(ctx, hipMemcpyAsync(d_in, h_in, in_bytes, hipMemcpyHostToDevice, s));
    {
        TimerScope ts(ctx, CSV_K_WINDOW);
        r0 = 0;
        for (int c = 0; c < n_shards; c++) {
            const uint64_t nr = n_regions[c];
            if (!nr) continue;
            const uint64_t nw = win_off[c][nr];
            launch_window_log2(s, shards[c]->depth, shards[c]->depth_len, (const uint32_t *)(d_in + o_rs) + r0, (const uint32_t *)(d_in + o_re) + r0,
                               (const int32_t *)(d_in + o_ss) + r0, (const uint64_t *)(d_in + o_wo) + r0 + c, nr, nw, mean_cov[c],
                               (double *)(d_out + o_l2) + w0, (uint32_t *)(d_out + o_ws) + w0, (uint32_t *)(d_out + o_we) + w0);
            r0 += nr; w0 += nw;
        }
    }
    CSV_HIP(ctx, hipMemcpyAsync(h_out, d_out, out_bytes, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, wait_stream(s));
    w0 = 0;
    for (int c = 0; c < n_shards; c++) {
        const uint64_t nr = n_regions[c];
        if (!nr) continue;
        const uint64_t nw = win_off[c][nr];
        memcpy(log2_cov[c], h_out + o_l2 + w0 * 8, nw * 8);
        memcpy(win_start[c], h_out + o_ws + w0 * 4, nw * 4);
        memcpy(win_end[c], h_out + o_we + w0 * 4, nw * 4);
        w0 += nw;
    }
    return CSV_OK;
}

// ---- the copy-number observations (kernels/cnobs.hip) --------------------------------------------------------------------------------------
namespace {
// What the two entry points share: the checks, the tables' way up, windows -> order -> offsets -> fill, and the count's readback.
struct CnCall {
    uint64_t R = 0, W = 0, S = 0, bound = 0, cap = 0, total = 0;
    CnWs w;
    PinStage pin;
    void *h_off = nullptr, *h_pos = nullptr, *h_baf = nullptr, *h_pfb = nullptr, *h_l2 = nullptr, *h_snp = nullptr, *h_states = nullptr, *h_ll = nullptr;
};

// the epochs a region of up to CN_MAX_WINDOWS nodes can reach, from the library's own policy; false if a bucket count does not fit its form
bool cn_epochs(CnEpochs &ep)
{
    std::vector<uint64_t> first, bkt;
    split_order_epochs(CN_MAX_WINDOWS, first, bkt);
    ep = CnEpochs();
    for (size_t k = 0; k < first.size() && first[k] < CN_MAX_WINDOWS; k++) {
        if (ep.n == CN_MAX_EPOCHS || bkt[k] > (first[k] < CN_SMALL_MAX ? CN_SMALL_MAX : CN_MAX_WINDOWS)) return false;
        ep.first[ep.n] = (uint32_t)first[k]; ep.B[ep.n] = (uint32_t)bkt[k]; ep.n++;
    }
    ep.first[ep.n] = 0xffffffffu;
    return ep.n > 0 && ep.first[0] == 0;
}

int cn_run(csv_ctx *ctx, const char *what, const csv_cn_regions *in, bool decode, bool want_baf, bool want_pfb, bool want_l2, bool want_snp,
           const uint64_t *n_obs, CnCall &c)
{
    auto bad = [&](const char *msg) { ctx->err = std::string(what) + ": " + msg; return (int)CSV_EINVAL; };
    if (!in || !n_obs) return bad("null argument");
    if (ctx->split_state) return bad("a split order is pending on this context");
    if (in->n_shards < 0) return bad("negative shard count");
    if (in->n_shards && (!in->shards || !in->mean_cov)) return bad("null array");
    if (!in->reg_off || in->reg_off[0] != 0) return bad("reg_off missing or not starting at 0");
    for (int s = 0; s < in->n_shards; s++) {
        if (in->reg_off[s + 1] < in->reg_off[s]) return bad("reg_off not ascending");
        if (in->reg_off[s + 1] > in->reg_off[s] && !in->shards[s]) return bad("null shard");
    }
    const uint64_t R = in->n_shards ? in->reg_off[in->n_shards] : 0;
    c.R = R; c.cap = *n_obs;
    if (R == 0) return CSV_OK;
    if (R >= 0xffffffffull) return bad("2^32 - 1 or more regions");
    if (!in->region_start || !in->region_end || !in->sample_size || !in->snp_off) return bad("null array");
    if (in->snp_off[0] != 0) return bad("snp_off must start at 0");
    uint64_t W = 0;
    for (uint64_t r = 0; r < R; r++) {
        if (in->snp_off[r + 1] < in->snp_off[r]) return bad("snp_off not ascending");
        if (in->sample_size[r] <= 0) return bad("sample_size <= 0");
        if (in->region_start[r] > in->region_end[r]) return bad("region start > end");
        if (in->region_end[r] >= 0x7fffffffu) return bad("a window coordinate could reach 2^31");
        const uint64_t ss = std::max<uint64_t>(in->snp_off[r + 1] - in->snp_off[r], (uint64_t)in->sample_size[r]);
        if (ss > CN_MAX_WINDOWS) return bad("more than 5087 windows in a region");
        W += ss;
    }
    const uint64_t S = in->snp_off[R];
    if (S && (!in->snp_pos || !in->snp_baf || !in->snp_pfb)) return bad("null array");
    for (uint64_t r = 0; r < R; r++)
        for (uint64_t k = in->snp_off[r] + 1; k < in->snp_off[r + 1]; k++)
            if (in->snp_pos[k] < in->snp_pos[k - 1]) return bad("SNP positions decrease inside a region");
    if (W + 3 * S >= 0xffffffffull) return bad("2^32 - 1 or more windows, records or observations");
    c.W = W; c.S = S; c.bound = W + 3 * S;
    CnEpochs ep;
    if (!cn_epochs(ep)) { ctx->err = std::string(what) + ": this C++ library's hash table does not grow as the kernels assume"; return CSV_EHIP; }

    (void)hipSetDevice(ctx->device);
    const uint64_t n_sh = (uint64_t)in->n_shards;
    int rc;
    if ((rc = arena_reserve_for(ctx, ctx->arena, what, [&](Arena &a) { return carve_cn_obs(a, R, W, n_sh, S, decode, c.w); }))) return rc;
    const CnInLayout L(R, n_sh, S);
    const uint64_t room = std::min(c.cap, c.bound);          // what can come back
    char *h_in = nullptr;
    uint64_t *h_total = nullptr;
    c.pin = PinStage(ctx);
    if ((rc = pin_reserve_for(ctx, c.pin, [&](PinStage &p) {
            h_total = (uint64_t *)p.slot(256); h_in = (char *)p.slot(L.bytes);
            c.h_off = p.slot((R + 1) * 8); c.h_pos = p.slot(room * 4);
            if (want_baf) c.h_baf = p.slot(room * 8);
            if (want_pfb) c.h_pfb = p.slot(room * 8);
            if (want_l2) c.h_l2 = p.slot(room * 8);
            if (want_snp) c.h_snp = p.slot(room);
            if (decode) { c.h_states = p.slot(room * 4); c.h_ll = p.slot(R * 8); }
        }))) return rc;
    // the tables: per-shard window offsets for the window kernel (each shard's start at 0), flat ones for the order kernels
    memcpy(h_in + L.rs, in->region_start, R * 4);
    memcpy(h_in + L.re, in->region_end, R * 4);
    int32_t *h_ss = (int32_t *)(h_in + L.ss);
    uint64_t *h_wo = (uint64_t *)(h_in + L.wo);
    uint32_t *h_wbase = (uint32_t *)(h_in + L.wbase), *h_soff = (uint32_t *)(h_in + L.soff), *h_small = (uint32_t *)(h_in + L.small), *h_big = (uint32_t *)(h_in + L.big);
    uint64_t wflat = 0;
    uint32_t n_small = 0, n_big = 0;
    for (uint64_t s = 0; s < n_sh; s++) {
        uint64_t wrel = 0;
        for (uint64_t r = in->reg_off[s]; r < in->reg_off[s + 1]; r++) {
            const uint64_t ss = std::max<uint64_t>(in->snp_off[r + 1] - in->snp_off[r], (uint64_t)in->sample_size[r]);
            h_ss[r] = (int32_t)ss; h_wo[r + s] = wrel; h_wbase[r] = (uint32_t)wflat; h_soff[r] = (uint32_t)in->snp_off[r];
            if (ss <= CN_SMALL_MAX) h_small[n_small++] = (uint32_t)r; else h_big[n_big++] = (uint32_t)r;
            wrel += ss; wflat += ss;
        }
        h_wo[in->reg_off[s + 1] + s] = wrel;
    }
    h_wbase[R] = (uint32_t)W; h_soff[R] = (uint32_t)S;
    if (S) { memcpy(h_in + L.spos, in->snp_pos, S * 4); memcpy(h_in + L.sbaf, in->snp_baf, S * 8); memcpy(h_in + L.spfb, in->snp_pfb, S * 8); }

    hipStream_t st = ctx->stream;
    char *d_in = c.w.in;
    CSV_HIP(ctx, hipMemcpyAsync(d_in, h_in, L.bytes, hipMemcpyHostToDevice, st));
    CSV_HIP(ctx, hipMemsetAsync(c.w.sl.tot, 0, (R + 1) * 4, st));
    {
        TimerScope ts(ctx, CSV_K_WINDOW);
        for (uint64_t s = 0; s < n_sh; s++) {
            const uint64_t r0 = in->reg_off[s], nr = in->reg_off[s + 1] - r0;
            if (!nr) continue;
            const uint64_t w0 = h_wbase[r0], nw = h_wo[r0 + nr + s];
            launch_window_log2(st, in->shards[s]->depth, in->shards[s]->depth_len, (const uint32_t *)(d_in + L.rs) + r0, (const uint32_t *)(d_in + L.re) + r0,
                               (const int32_t *)(d_in + L.ss) + r0, (const uint64_t *)(d_in + L.wo) + r0 + s, nr, nw, in->mean_cov[s], c.w.l2 + w0, c.w.ws + w0, c.w.we + w0);
        }
        launch_cn_order(st, c.w.ws, c.w.we, (const uint32_t *)(d_in + L.wbase), (const uint32_t *)(d_in + L.soff), (const uint32_t *)(d_in + L.spos),
                        (const uint32_t *)(d_in + L.small), n_small, (const uint32_t *)(d_in + L.big), n_big, ep, c.w.sl);
        launch_exclusive_sum_u32(st, c.w.sl.tot, R + 1, c.w.es_tmp);
        launch_cn_fill(st, c.w.sl, (uint32_t)W, (uint32_t)R, c.w.sl.tot, c.w.ws, c.w.we, c.w.l2, (const uint32_t *)(d_in + L.spos), (const double *)(d_in + L.sbaf),
                       (const double *)(d_in + L.spfb), c.w.o);
    }
    CSV_HIP(ctx, hipMemcpyAsync(h_total, c.w.o.obs_off + R, 8, hipMemcpyDeviceToHost, st));
    CSV_HIP(ctx, wait_stream(st));
    c.total = *h_total;
    if (c.total > c.bound) { ctx->err = std::string(what) + ": more observations than the bound"; return CSV_EHIP; }
    return CSV_OK;
}

// cn_run fed by resident SNP tables (kernels/snptable.hip): the record ranges, the window counts, the offset tables, the lists and the compact
// records are made on the device; one readback of the plan's head sizes the rest. CSV_OK / 1 (declined, the reason in ctx->err) / CSV_E*.
int cn_tables_run(csv_ctx *ctx, const char *what, const csv_cn_table_regions *in, bool decode, bool want_baf, bool want_pfb, bool want_l2, bool want_snp,
                  uint64_t *n_obs, CnCall &c)
{
    auto bad = [&](const char *msg) { ctx->err = std::string(what) + ": " + msg; return (int)CSV_EINVAL; };
    if (!in || !n_obs) return bad("null argument");
    if (ctx->split_state) return bad("a split order is pending on this context");
    if (in->n_shards < 0) return bad("negative shard count");
    if (in->n_shards && (!in->shards || !in->mean_cov || !in->tables)) return bad("null array");
    if (!in->reg_off || in->reg_off[0] != 0) return bad("reg_off missing or not starting at 0");
    for (int s = 0; s < in->n_shards; s++) {
        if (in->reg_off[s + 1] < in->reg_off[s]) return bad("reg_off not ascending");
        if (in->reg_off[s + 1] > in->reg_off[s] && !in->shards[s]) return bad("null shard");
        if (in->tables[s] && in->tables[s]->device != ctx->device) return bad("a table of another device");
    }
    const uint64_t R = in->n_shards ? in->reg_off[in->n_shards] : 0;
    c.R = R; c.cap = *n_obs;
    if (R == 0) return CSV_OK;
    if (R >= 0xffffffffull) return bad("2^32 - 1 or more regions");
    if (!in->region_start || !in->region_end || !in->sample_size) return bad("null array");
    for (uint64_t r = 0; r < R; r++) {
        if (in->sample_size[r] <= 0) return bad("sample_size <= 0");
        if (in->region_start[r] > in->region_end[r]) return bad("region start > end");
        if (in->region_end[r] >= 0x7fffffffu) return bad("a window coordinate could reach 2^31");
        if ((uint32_t)in->sample_size[r] > CN_MAX_WINDOWS) return bad("more than 5087 windows in a region");
    }
    CnEpochs ep;
    if (!cn_epochs(ep)) { ctx->err = std::string(what) + ": this C++ library's hash table does not grow as the kernels assume"; return CSV_EHIP; }

    (void)hipSetDevice(ctx->device);
    const uint64_t n_sh = (uint64_t)in->n_shards;
    const CnUpLayout L(R, n_sh);
    const size_t head_bytes = CN_PLAN_HEAD_BYTES + (n_sh + 1) * 4;
    CnTabWs w;
    int rc;
    if ((rc = arena_reserve_for(ctx, ctx->arena, what, [&](Arena &a) { return carve_cn_tables(a, R, n_sh, 0, 0, decode, w); }))) return rc;
    hipStream_t st = ctx->stream;
    // what goes up: the regions, each region's shard, the tables as the kernels see them, the shards' first regions
    auto fill_up = [&](char *h_up) {
        memcpy(h_up + L.rs, in->region_start, R * 4);
        memcpy(h_up + L.re, in->region_end, R * 4);
        memcpy(h_up + L.ssf, in->sample_size, R * 4);
        uint32_t *rsh = (uint32_t *)(h_up + L.rsh), *roff = (uint32_t *)(h_up + L.roff);
        SnpTabDev *tabs = (SnpTabDev *)(h_up + L.tabs);
        for (uint64_t s = 0; s < n_sh; s++) {
            for (uint64_t r = in->reg_off[s]; r < in->reg_off[s + 1]; r++) rsh[r] = (uint32_t)s;
            tabs[s] = snp_table_dev(in->tables[s]); roff[s] = (uint32_t)in->reg_off[s];
        }
        roff[n_sh] = (uint32_t)R;
    };
    auto queue_plan = [&](const char *h_up) -> int {
        CSV_HIP(ctx, hipMemcpyAsync(w.up, h_up, L.bytes, hipMemcpyHostToDevice, st));
        TimerScope ts(ctx, CSV_K_WINDOW);
        launch_cn_plan(st, w.p, (uint32_t)R, (uint32_t)n_sh);
        return CSV_OK;
    };
    std::vector<char> head(head_bytes);
    {
        PinStage pin(ctx);
        char *h_up = nullptr, *h_head = nullptr;
        if ((rc = pin_reserve_for(ctx, pin, [&](PinStage &p) { h_head = (char *)p.slot(head_bytes); h_up = (char *)p.slot(L.bytes); }))) return rc;
        fill_up(h_up);
        if ((rc = queue_plan(h_up))) return rc;
        CSV_HIP(ctx, hipMemcpyAsync(h_head, w.p.head, head_bytes, hipMemcpyDeviceToHost, st));
        CSV_HIP(ctx, wait_stream(st));
        memcpy(head.data(), h_head, head_bytes);
    }
    const CnPlanHead h = *(const CnPlanHead *)head.data();
    const uint32_t *shard_w0 = (const uint32_t *)(head.data() + CN_PLAN_HEAD_BYTES);
    if (h.flags & CN_PLAN_OVER_WINDOWS) { ctx->err = std::string(what) + ": declined: a region's SNP records call for more than 5087 windows"; return 1; }
    if (h.W + 3 * h.S >= 0xffffffffull) { ctx->err = std::string(what) + ": declined: 2^32 - 1 or more windows, records or observations"; return 1; }
    const uint64_t W = h.W, S = h.S;
    if ((uint64_t)h.n_small + h.n_big != R || shard_w0[n_sh] != W || shard_w0[0] != 0) { ctx->err = std::string(what) + ": the plan's totals disagree"; return CSV_EHIP; }
    c.W = W; c.S = S; c.bound = W + 3 * S;
    if (c.cap < c.bound) { *n_obs = c.bound; ctx->err = std::string(what) + ": capacity too small"; return CSV_ECAPACITY; }

    // (a grown arena is a new allocation, possibly at the old address: the pointer says nothing, the capacity rises with every growth)
    const size_t cap_before = ctx->arena.cap;
    if ((rc = arena_reserve_for(ctx, ctx->arena, what, [&](Arena &a) { return carve_cn_tables(a, R, n_sh, W, S, decode, w); }))) return rc;
    const uint64_t room = c.bound;                            // what can come back
    char *h_up = nullptr;
    uint64_t *h_total = nullptr;
    c.pin = PinStage(ctx);
    if ((rc = pin_reserve_for(ctx, c.pin, [&](PinStage &p) {
            h_total = (uint64_t *)p.slot(256); h_up = (char *)p.slot(L.bytes);
            c.h_off = p.slot((R + 1) * 8); c.h_pos = p.slot(room * 4);
            if (want_baf) c.h_baf = p.slot(room * 8);
            if (want_pfb) c.h_pfb = p.slot(room * 8);
            if (want_l2) c.h_l2 = p.slot(room * 8);
            if (want_snp) c.h_snp = p.slot(room);
            if (decode) { c.h_states = p.slot(room * 4); c.h_ll = p.slot(R * 8); }
        }))) return rc;
    if (ctx->arena.cap != cap_before) {                       // the arena grew: the plan again, into the new one
        fill_up(h_up);
        if ((rc = queue_plan(h_up))) return rc;
    }
    c.w.o = w.o; c.w.states = w.states; c.w.loglik = w.loglik;
    CSV_HIP(ctx, hipMemsetAsync(w.sl.tot, 0, (R + 1) * 4, st));
    {
        TimerScope ts(ctx, CSV_K_WINDOW);
        for (uint64_t s = 0; s < n_sh; s++) {
            const uint64_t r0 = in->reg_off[s], nr = in->reg_off[s + 1] - r0;
            if (!nr) continue;
            const uint64_t w0 = shard_w0[s], nw = shard_w0[s + 1] - shard_w0[s];
            launch_window_log2(st, in->shards[s]->depth, in->shards[s]->depth_len, w.p.rs + r0, w.p.re + r0, w.p.ss + r0, w.p.wo + r0 + s, nr, nw, in->mean_cov[s],
                               w.l2 + w0, w.ws + w0, w.we + w0);
        }
        launch_snp_gather(st, w.p, (uint32_t)R, (uint32_t)S, w.spos, w.sbaf, w.spfb);
        launch_cn_order(st, w.ws, w.we, w.p.wbase, w.p.soff, w.spos, w.p.small, h.n_small, w.p.big, h.n_big, ep, w.sl);
        launch_exclusive_sum_u32(st, w.sl.tot, R + 1, w.p.es_tmp);
        launch_cn_fill(st, w.sl, (uint32_t)W, (uint32_t)R, w.sl.tot, w.ws, w.we, w.l2, w.spos, (const double *)w.sbaf, (const double *)w.spfb, w.o);
    }
    CSV_HIP(ctx, hipMemcpyAsync(h_total, w.o.obs_off + R, 8, hipMemcpyDeviceToHost, st));
    CSV_HIP(ctx, wait_stream(st));
    c.total = *h_total;
    if (c.total > c.bound) { ctx->err = std::string(what) + ": more observations than the bound"; return CSV_EHIP; }
    return CSV_OK;
}

// the answer's arrays to the page-locked block (queued; the caller waits and finishes)
int cn_download(csv_ctx *ctx, CnCall &c, uint64_t *obs_off, uint32_t *pos, double *baf, double *pfb, double *log2_cov, uint8_t *is_snp)
{
    hipStream_t st = ctx->stream;
    const uint64_t n = c.total;
    struct Down { void *dst, *pin; const void *src; size_t bytes; };
    const Down down[] = {{obs_off, c.h_off, c.w.o.obs_off, (c.R + 1) * 8}, {pos, c.h_pos, c.w.o.pos, n * 4}, {baf, c.h_baf, c.w.o.baf, n * 8},
                         {pfb, c.h_pfb, c.w.o.pfb, n * 8}, {log2_cov, c.h_l2, c.w.o.log2_cov, n * 8}, {is_snp, c.h_snp, c.w.o.is_snp, n}};
    for (const Down &d : down) {
        if (!d.dst || !d.pin) continue;
        CSV_HIP(ctx, hipMemcpyAsync(d.pin, d.src, d.bytes, hipMemcpyDeviceToHost, st));
        c.pin.outs.push_back(PinStage::Out{d.dst, d.pin, d.bytes});
    }
    return CSV_OK;
}
}  // namespace

int csvgpu_cn_observations_resident_many(csv_ctx *ctx, const csv_cn_regions *in, uint64_t *obs_off, uint32_t *pos, double *baf, double *pfb,
                                         double *log2_cov, uint8_t *is_snp, uint64_t *n_obs)
{
    if (!ctx) return CSV_EINVAL;
    const char *what = "cn_observations";
    if (!obs_off) { ctx->err = std::string(what) + ": null array"; return CSV_EINVAL; }
    if (n_obs && *n_obs && (!pos || !baf || !pfb || !log2_cov || !is_snp)) { ctx->err = std::string(what) + ": null array with a capacity"; return CSV_EINVAL; }
    CnCall c;
    int rc = cn_run(ctx, what, in, false, true, true, true, true, n_obs, c);
    if (rc) return rc;
    *n_obs = c.total;
    if (c.R == 0) { obs_off[0] = 0; return CSV_OK; }
    if (c.total > c.cap) { ctx->err = std::string(what) + ": capacity too small"; return CSV_ECAPACITY; }
    if ((rc = cn_download(ctx, c, obs_off, pos, baf, pfb, log2_cov, is_snp))) return rc;
    CSV_HIP(ctx, wait_stream(ctx->stream));
    c.pin.finish();
    return CSV_OK;
}

int csvgpu_cn_observations_tables_many(csv_ctx *ctx, const csv_cn_table_regions *in, uint64_t *obs_off, uint32_t *pos, double *baf, double *pfb,
                                       double *log2_cov, uint8_t *is_snp, uint64_t *n_obs)
{
    if (!ctx) return CSV_EINVAL;
    const char *what = "cn_observations_tables";
    if (!obs_off) { ctx->err = std::string(what) + ": null array"; return CSV_EINVAL; }
    if (n_obs && *n_obs && (!pos || !baf || !pfb || !log2_cov || !is_snp)) { ctx->err = std::string(what) + ": null array with a capacity"; return CSV_EINVAL; }
    CnCall c;
    int rc = cn_tables_run(ctx, what, in, false, true, true, true, true, n_obs, c);
    if (rc) return rc;
    *n_obs = c.total;
    if (c.R == 0) { obs_off[0] = 0; return CSV_OK; }
    if ((rc = cn_download(ctx, c, obs_off, pos, baf, pfb, log2_cov, is_snp))) return rc;
    CSV_HIP(ctx, wait_stream(ctx->stream));
    c.pin.finish();
    return CSV_OK;
}

int csvgpu_cn_decode_tables_many(csv_ctx *ctx, const csv_cn_table_regions *in, const csv_hmm *hmm, uint64_t *obs_off, uint32_t *pos, int32_t *states,
                                 double *loglik, double *baf, double *pfb, double *log2_cov, uint8_t *is_snp, uint64_t *n_obs)
{
    if (!ctx) return CSV_EINVAL;
    const char *what = "cn_decode_tables";
    if (!hmm) { ctx->err = std::string(what) + ": null hmm"; return CSV_EINVAL; }
    if (!obs_off || !loglik) { ctx->err = std::string(what) + ": null array"; return CSV_EINVAL; }
    if (n_obs && *n_obs && (!pos || !states)) { ctx->err = std::string(what) + ": null array with a capacity"; return CSV_EINVAL; }
    CnCall c;
    int rc = cn_tables_run(ctx, what, in, true, baf != nullptr, pfb != nullptr, log2_cov != nullptr, is_snp != nullptr, n_obs, c);
    if (rc) return rc;
    *n_obs = c.total;
    if (c.R == 0) { obs_off[0] = 0; return CSV_OK; }
    if ((rc = csvgpu_viterbi_dev(ctx, hmm, c.w.o.log2_cov, c.w.o.baf, c.w.o.pfb, c.w.o.obs_off, c.R, c.total, c.w.states, c.w.loglik))) return rc;
    if ((rc = cn_download(ctx, c, obs_off, pos, baf, pfb, log2_cov, is_snp))) return rc;
    hipStream_t st = ctx->stream;
    CSV_HIP(ctx, hipMemcpyAsync(c.h_states, c.w.states, c.total * 4, hipMemcpyDeviceToHost, st));
    CSV_HIP(ctx, hipMemcpyAsync(c.h_ll, c.w.loglik, c.R * 8, hipMemcpyDeviceToHost, st));
    c.pin.outs.push_back(PinStage::Out{states, c.h_states, c.total * 4});
    c.pin.outs.push_back(PinStage::Out{loglik, c.h_ll, c.R * 8});
    CSV_HIP(ctx, wait_stream(st));
    c.pin.finish();
    return CSV_OK;
}

int csvgpu_cn_decode_resident_many(csv_ctx *ctx, const csv_cn_regions *in, const csv_hmm *hmm, uint64_t *obs_off, uint32_t *pos, int32_t *states,
                                   double *loglik, double *baf, double *pfb, double *log2_cov, uint8_t *is_snp, uint64_t *n_obs)
{
    if (!ctx) return CSV_EINVAL;
    const char *what = "cn_decode";
    if (!hmm) { ctx->err = std::string(what) + ": null hmm"; return CSV_EINVAL; }
    if (!obs_off || !loglik) { ctx->err = std::string(what) + ": null array"; return CSV_EINVAL; }
    if (n_obs && *n_obs && (!pos || !states)) { ctx->err = std::string(what) + ": null array with a capacity"; return CSV_EINVAL; }
    CnCall c;
    int rc = cn_run(ctx, what, in, true, baf != nullptr, pfb != nullptr, log2_cov != nullptr, is_snp != nullptr, n_obs, c);
    if (rc) return rc;
    *n_obs = c.total;
    if (c.R == 0) { obs_off[0] = 0; return CSV_OK; }
    if (c.total > c.cap) { ctx->err = std::string(what) + ": capacity too small"; return CSV_ECAPACITY; }
    if ((rc = csvgpu_viterbi_dev(ctx, hmm, c.w.o.log2_cov, c.w.o.baf, c.w.o.pfb, c.w.o.obs_off, c.R, c.total, c.w.states, c.w.loglik))) return rc;
    if ((rc = cn_download(ctx, c, obs_off, pos, baf, pfb, log2_cov, is_snp))) return rc;
    hipStream_t st = ctx->stream;
    CSV_HIP(ctx, hipMemcpyAsync(c.h_states, c.w.states, c.total * 4, hipMemcpyDeviceToHost, st));
    CSV_HIP(ctx, hipMemcpyAsync(c.h_ll, c.w.loglik, c.R * 8, hipMemcpyDeviceToHost, st));
    c.pin.outs.push_back(PinStage::Out{states, c.h_states, c.total * 4});
    c.pin.outs.push_back(PinStage::Out{loglik, c.h_ll, c.R * 8});
    CSV_HIP(ctx, wait_stream(st));
    c.pin.finish();
    return CSV_OK;
}
