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

// One window launch per shard that has regions. Shard s's regions are [r0, r0 + nr) of the device tables rs / re / ss, its window offsets (from
// 0) are at wo + r0 + s, and its windows are [w0, w0 + nw) of l2 / ws / we.
struct ShardSpan { uint64_t r0, nr, w0, nw; };
static void launch_windows_per_shard(hipStream_t st, int n_shards, csv_shard *const *shards, const double *mean_cov, const ShardSpan *spans, const uint32_t *rs,
                                     const uint32_t *re, const int32_t *ss, const uint64_t *wo, double *l2, uint32_t *ws, uint32_t *we)
{
    for (int s = 0; s < n_shards; s++) {
        const ShardSpan &p = spans[s];
        if (!p.nr) continue;
        launch_window_log2(st, shards[s]->depth, shards[s]->depth_len, rs + p.r0, re + p.r0, ss + p.r0, wo + p.r0 + s, p.nr, p.nw, mean_cov[s], l2 + p.w0, ws + p.w0, we + p.w0);
    }
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
    std::vector<ShardSpan> spans(n_shards);
    uint64_t r0 = 0, w0 = 0;
    for (int c = 0; c < n_shards; c++) {
        const uint64_t nr = n_regions[c];
        if (!nr) continue;
        memcpy(h_in + o_rs + r0 * 4, region_start[c], nr * 4);
        memcpy(h_in + o_re + r0 * 4, region_end[c], nr * 4);
        memcpy(h_in + o_ss + r0 * 4, sample_size[c], nr * 4);
        memcpy(h_in + o_wo + (r0 + (uint64_t)c) * 8, win_off[c], (nr + 1) * 8);
        spans[c] = ShardSpan{r0, nr, w0, win_off[c][nr]};
        r0 += nr; w0 += win_off[c][nr];
    }
    hipStream_t s = ctx->stream;
    CSV_HIP(ctx, hipMemcpyAsync(d_in, h_in, in_bytes, hipMemcpyHostToDevice, s));
    {
        TimerScope ts(ctx, CSV_K_WINDOW);
        launch_windows_per_shard(s, n_shards, shards, mean_cov, spans.data(), (const uint32_t *)(d_in + o_rs), (const uint32_t *)(d_in + o_re), (const int32_t *)(d_in + o_ss),
                                 (const uint64_t *)(d_in + o_wo), (double *)(d_out + o_l2), (uint32_t *)(d_out + o_ws), (uint32_t *)(d_out + o_we));
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
// the caller's arrays (states / loglik: the decode calls'; baf / pfb / log2_cov / is_snp each optional there)
struct CnOut { uint64_t *obs_off; uint32_t *pos; int32_t *states; double *loglik, *baf, *pfb, *log2_cov; uint8_t *is_snp; };

// What the four entry points hold: the counts, the workspace's back half, the page-locked slots of what comes back.
struct CnCall {
    const char *what;                                         // the entry point, as the messages name it
    const csv_hmm *hmm;                                       // the decode calls'
    bool decode;
    CnOut out;
    uint64_t R = 0, W = 0, S = 0, bound = 0, cap = 0, total = 0;
    CnBack b;
    PinStage pin{};
    void *h_off = nullptr, *h_pos = nullptr, *h_baf = nullptr, *h_pfb = nullptr, *h_l2 = nullptr, *h_snp = nullptr, *h_states = nullptr, *h_ll = nullptr;
};

// what both routes' `in` say of the shards and their regions; own_*: the route's own per-shard / per-region arrays are there
struct CnRegions {
    int32_t n_shards; csv_shard *const *shards; const double *mean_cov; const uint64_t *reg_off;
    const uint32_t *region_start, *region_end; const int32_t *sample_size;
    bool own_shard_arrays, own_region_arrays;
};

// the tables and the compact SNP records on the device, as either route leaves them for the tail
struct CnDev {
    const uint32_t *rs, *re; const int32_t *ss; const uint64_t *wo;            // per shard (launch_window_log2): wo starts at 0 in every shard
    const uint32_t *wbase, *soff, *small, *big; uint32_t n_small, n_big;        // flat (launch_cn_order)
    uint32_t *spos; uint64_t *sbaf, *spfb;                                      // values as their bits
    void *es_tmp;
    const CnPlan *gather;                                                       // the table route: the records are gathered from the tables first
};

// the epochs a region of up to CN_MAX_WINDOWS nodes can reach, from the library's own policy; CSV_EHIP if a bucket count does not fit its form
int cn_epochs(csv_ctx *ctx, const char *what, CnEpochs &ep)
{
    std::vector<uint64_t> first, bkt;
    split_order_epochs(CN_MAX_WINDOWS, first, bkt);
    ep = CnEpochs();
    bool ok = true;
    for (size_t k = 0; k < first.size() && first[k] < CN_MAX_WINDOWS; k++) {
        if (ep.n == CN_MAX_EPOCHS || bkt[k] > (first[k] < CN_SMALL_MAX ? CN_SMALL_MAX : CN_MAX_WINDOWS)) { ok = false; break; }
        ep.first[ep.n] = (uint32_t)first[k]; ep.B[ep.n] = (uint32_t)bkt[k]; ep.n++;
    }
    ep.first[ep.n] = 0xffffffffu;
    if (ok && ep.n > 0 && ep.first[0] == 0) return CSV_OK;
    ctx->err = std::string(what) + ": this C++ library's hash table does not grow as the kernels assume";
    return CSV_EHIP;
}

// Everything the host can see of the shards and the regions. own_shard(s) and own_region(r, windows) are the route's own checks of a shard and
// of a region (a message, or null); the latter says how many windows the region has as far as the host knows. R == 0 on CSV_OK: nothing to do.
template <class Shard, class Region>
int cn_check_regions(csv_ctx *ctx, const char *what, const CnRegions &v, Shard own_shard, Region own_region, uint64_t &R, uint64_t &W)
{
    auto bad = [&](const char *msg) { ctx->err = std::string(what) + ": " + msg; return (int)CSV_EINVAL; };
    R = W = 0;
    if (ctx->split_state) return bad("a split order is pending on this context");
    if (v.n_shards < 0) return bad("negative shard count");
    if (v.n_shards && (!v.shards || !v.mean_cov || !v.own_shard_arrays)) return bad("null array");
    if (!v.reg_off || v.reg_off[0] != 0) return bad("reg_off missing or not starting at 0");
    for (int s = 0; s < v.n_shards; s++) {
        if (v.reg_off[s + 1] < v.reg_off[s]) return bad("reg_off not ascending");
        if (v.reg_off[s + 1] > v.reg_off[s] && !v.shards[s]) return bad("null shard");
        if (const char *msg = own_shard(s)) return bad(msg);
    }
    R = v.n_shards ? v.reg_off[v.n_shards] : 0;
    if (R == 0) return CSV_OK;
    if (R >= 0xffffffffull) return bad("2^32 - 1 or more regions");
    if (!v.region_start || !v.region_end || !v.sample_size || !v.own_region_arrays) return bad("null array");
    for (uint64_t r = 0; r < R; r++) {
        uint64_t windows = 0;
        if (const char *msg = own_region(r, windows)) return bad(msg);
        if (v.sample_size[r] <= 0) return bad("sample_size <= 0");
        if (v.region_start[r] > v.region_end[r]) return bad("region start > end");
        if (v.region_end[r] >= 0x7fffffffu) return bad("a window coordinate could reach 2^31");
        if (windows > CN_MAX_WINDOWS) return bad("more than 5087 windows in a region");
        W += windows;
    }
    return CSV_OK;
}

// the entry points' own checks of what the caller gave: the arrays for the answer, the regions (have_in), the capacity
int cn_check_call(csv_ctx *ctx, CnCall &c, bool have_in, const uint64_t *n_obs)
{
    auto bad = [&](const char *msg) { ctx->err = std::string(c.what) + ": " + msg; return (int)CSV_EINVAL; };
    const CnOut &o = c.out;
    if (c.decode && !c.hmm) return bad("null hmm");
    if (!o.obs_off || (c.decode && !o.loglik)) return bad("null array");
    if (n_obs && *n_obs && (!o.pos || (c.decode ? !o.states : !o.baf || !o.pfb || !o.log2_cov || !o.is_snp))) return bad("null array with a capacity");
    if (!have_in || !n_obs) return bad("null argument");
    c.cap = *n_obs;
    return CSV_OK;
}

// the page-locked slots of what comes back: `room` observations at the most, an optional array only where the caller gave one
void cn_pin_outputs(PinStage &p, CnCall &c, uint64_t room)
{
    c.h_off = p.slot((c.R + 1) * 8); c.h_pos = p.slot(room * 4);
    if (c.out.baf) c.h_baf = p.slot(room * 8);
    if (c.out.pfb) c.h_pfb = p.slot(room * 8);
    if (c.out.log2_cov) c.h_l2 = p.slot(room * 8);
    if (c.out.is_snp) c.h_snp = p.slot(room);
    if (c.decode) { c.h_states = p.slot(room * 4); c.h_ll = p.slot(c.R * 8); }
}

// memset -> windows -> (the table route's records) -> order -> offsets -> fill, and the count's readback through h_total
int cn_tail(csv_ctx *ctx, const char *what, const CnRegions &v, const std::vector<ShardSpan> &spans, const CnDev &d, const CnEpochs &ep, uint64_t *h_total, CnCall &c)
{
    hipStream_t st = ctx->stream;
    const CnBack &b = c.b;
    CSV_HIP(ctx, hipMemsetAsync(b.sl.tot, 0, (c.R + 1) * 4, st));
    {
        TimerScope ts(ctx, CSV_K_WINDOW);
        launch_windows_per_shard(st, v.n_shards, v.shards, v.mean_cov, spans.data(), d.rs, d.re, d.ss, d.wo, b.l2, b.ws, b.we);
        if (d.gather) launch_snp_gather(st, *d.gather, (uint32_t)c.R, (uint32_t)c.S, d.spos, d.sbaf, d.spfb);
        launch_cn_order(st, b.ws, b.we, d.wbase, d.soff, d.spos, d.small, d.n_small, d.big, d.n_big, ep, b.sl);
        launch_exclusive_sum_u32(st, b.sl.tot, c.R + 1, d.es_tmp);
        launch_cn_fill(st, b.sl, (uint32_t)c.W, (uint32_t)c.R, b.sl.tot, b.ws, b.we, b.l2, d.spos, (const double *)d.sbaf, (const double *)d.spfb, b.o);
    }
    CSV_HIP(ctx, hipMemcpyAsync(h_total, b.o.obs_off + c.R, 8, hipMemcpyDeviceToHost, st));
    CSV_HIP(ctx, wait_stream(st));
    c.total = *h_total;
    if (c.total > c.bound) { ctx->err = std::string(what) + ": more observations than the bound"; return CSV_EHIP; }
    return CSV_OK;
}

// The SNP records come from the host: the region tables are made here and go up in one copy.
int cn_run(csv_ctx *ctx, const csv_cn_regions *in, const uint64_t *n_obs, CnCall &c)
{
    const char *what = c.what;
    auto bad = [&](const char *msg) { ctx->err = std::string(what) + ": " + msg; return (int)CSV_EINVAL; };
    int rc = cn_check_call(ctx, c, in != nullptr, n_obs);
    if (rc) return rc;
    const CnRegions v{in->n_shards, in->shards, in->mean_cov, in->reg_off, in->region_start, in->region_end, in->sample_size, true, in->snp_off != nullptr};
    rc = cn_check_regions(ctx, what, v, [](int) { return (const char *)nullptr; }, [&](uint64_t r, uint64_t &windows) -> const char * {
        if (r == 0 && in->snp_off[0] != 0) return "snp_off must start at 0";
        if (in->snp_off[r + 1] < in->snp_off[r]) return "snp_off not ascending";
        windows = std::max<uint64_t>(in->snp_off[r + 1] - in->snp_off[r], (uint64_t)in->sample_size[r]);
        return nullptr;
    }, c.R, c.W);
    if (rc || c.R == 0) return rc;
    const uint64_t R = c.R, W = c.W, S = in->snp_off[R];
    if (S && (!in->snp_pos || !in->snp_baf || !in->snp_pfb)) return bad("null array");
    for (uint64_t r = 0; r < R; r++)
        for (uint64_t k = in->snp_off[r] + 1; k < in->snp_off[r + 1]; k++)
            if (in->snp_pos[k] < in->snp_pos[k - 1]) return bad("SNP positions decrease inside a region");
    if (W + 3 * S >= 0xffffffffull) return bad("2^32 - 1 or more windows, records or observations");
    c.S = S; c.bound = W + 3 * S;
    CnEpochs ep;
    if ((rc = cn_epochs(ctx, what, ep))) return rc;

    (void)hipSetDevice(ctx->device);
    const uint64_t n_sh = (uint64_t)in->n_shards;
    CnWs w;
    if ((rc = arena_reserve_for(ctx, ctx->arena, what, [&](Arena &a) { return carve_cn_obs(a, R, W, n_sh, S, c.decode, w); }))) return rc;
    c.b = w.b;
    const CnInLayout L(R, n_sh, S);
    char *h_in = nullptr;
    uint64_t *h_total = nullptr;
    c.pin = PinStage(ctx);
    if ((rc = pin_reserve_for(ctx, c.pin, [&](PinStage &p) {
            h_total = (uint64_t *)p.slot(256); h_in = (char *)p.slot(L.bytes);
            cn_pin_outputs(p, c, std::min(c.cap, c.bound));
        }))) return rc;
    // the tables: per-shard window offsets for the window kernel (each shard's start at 0), flat ones for the order kernels
    memcpy(h_in + L.rs, in->region_start, R * 4);
    memcpy(h_in + L.re, in->region_end, R * 4);
    int32_t *h_ss = (int32_t *)(h_in + L.ss);
    uint64_t *h_wo = (uint64_t *)(h_in + L.wo);
    uint32_t *h_wbase = (uint32_t *)(h_in + L.wbase), *h_soff = (uint32_t *)(h_in + L.soff), *h_small = (uint32_t *)(h_in + L.small), *h_big = (uint32_t *)(h_in + L.big);
    std::vector<ShardSpan> spans(n_sh);
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
        spans[s] = ShardSpan{in->reg_off[s], in->reg_off[s + 1] - in->reg_off[s], wflat - wrel, wrel};
    }
    h_wbase[R] = (uint32_t)W; h_soff[R] = (uint32_t)S;
    if (S) { memcpy(h_in + L.spos, in->snp_pos, S * 4); memcpy(h_in + L.sbaf, in->snp_baf, S * 8); memcpy(h_in + L.spfb, in->snp_pfb, S * 8); }

    char *d_in = w.in;
    CSV_HIP(ctx, hipMemcpyAsync(d_in, h_in, L.bytes, hipMemcpyHostToDevice, ctx->stream));
    const CnDev d{(const uint32_t *)(d_in + L.rs), (const uint32_t *)(d_in + L.re), (const int32_t *)(d_in + L.ss), (const uint64_t *)(d_in + L.wo),
                  (const uint32_t *)(d_in + L.wbase), (const uint32_t *)(d_in + L.soff), (const uint32_t *)(d_in + L.small), (const uint32_t *)(d_in + L.big), n_small, n_big,
                  (uint32_t *)(d_in + L.spos), (uint64_t *)(d_in + L.sbaf), (uint64_t *)(d_in + L.spfb), w.es_tmp, nullptr};
    return cn_tail(ctx, what, v, spans, d, ep, h_total, c);
}

// cn_run fed by resident SNP tables (kernels/snptable.hip): the record ranges, the window counts, the offset tables, the lists and the compact
// records are made on the device; one readback of the plan's head sizes the rest. CSV_OK / 1 (declined, the reason in ctx->err) / CSV_E*.
int cn_tables_run(csv_ctx *ctx, const csv_cn_table_regions *in, uint64_t *n_obs, CnCall &c)
{
    const char *what = c.what;
    int rc = cn_check_call(ctx, c, in != nullptr, n_obs);
    if (rc) return rc;
    const CnRegions v{in->n_shards, in->shards, in->mean_cov, in->reg_off, in->region_start, in->region_end, in->sample_size, in->tables != nullptr, true};
    rc = cn_check_regions(ctx, what, v, [&](int s) { return in->tables[s] && in->tables[s]->device != ctx->device ? "a table of another device" : nullptr; },
                          [&](uint64_t r, uint64_t &windows) -> const char * { windows = (uint32_t)in->sample_size[r]; return nullptr; }, c.R, c.W);      // (c.W: the floors' sum until the plan has counted)
    if (rc || c.R == 0) return rc;
    const uint64_t R = c.R;
    CnEpochs ep;
    if ((rc = cn_epochs(ctx, what, ep))) return rc;

    (void)hipSetDevice(ctx->device);
    const uint64_t n_sh = (uint64_t)in->n_shards;
    const CnUpLayout L(R, n_sh);
    const size_t head_bytes = CN_PLAN_HEAD_BYTES + (n_sh + 1) * 4;
    CnTabWs w;
    if ((rc = arena_reserve_for(ctx, ctx->arena, what, [&](Arena &a) { return carve_cn_tables(a, R, n_sh, 0, 0, c.decode, w); }))) return rc;
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
    if ((rc = arena_reserve_for(ctx, ctx->arena, what, [&](Arena &a) { return carve_cn_tables(a, R, n_sh, W, S, c.decode, w); }))) return rc;
    c.b = w.b;
    char *h_up = nullptr;
    uint64_t *h_total = nullptr;
    c.pin = PinStage(ctx);
    if ((rc = pin_reserve_for(ctx, c.pin, [&](PinStage &p) {
            h_total = (uint64_t *)p.slot(256); h_up = (char *)p.slot(L.bytes);
            cn_pin_outputs(p, c, c.bound);
        }))) return rc;
    if (ctx->arena.cap != cap_before) {                       // the arena grew: the plan again, into the new one
        fill_up(h_up);
        if ((rc = queue_plan(h_up))) return rc;
    }
    std::vector<ShardSpan> spans(n_sh);
    for (uint64_t s = 0; s < n_sh; s++) spans[s] = ShardSpan{in->reg_off[s], in->reg_off[s + 1] - in->reg_off[s], shard_w0[s], (uint64_t)shard_w0[s + 1] - shard_w0[s]};
    const CnDev d{w.p.rs, w.p.re, w.p.ss, w.p.wo, w.p.wbase, w.p.soff, w.p.small, w.p.big, h.n_small, h.n_big, w.spos, w.sbaf, w.spfb, w.p.es_tmp, &w.p};
    return cn_tail(ctx, what, v, spans, d, ep, h_total, c);
}

// after either run: the count, the capacity, the decoding where it is asked for, and the answer through the page-locked block to the caller's
// arrays: each one the caller gave and that has a slot
int cn_finish(csv_ctx *ctx, CnCall &c, uint64_t *n_obs)
{
    *n_obs = c.total;
    if (c.R == 0) { c.out.obs_off[0] = 0; return CSV_OK; }
    // (the table route has turned a capacity below the bound away before it ran)
    if (c.total > c.cap) { ctx->err = std::string(c.what) + ": capacity too small"; return CSV_ECAPACITY; }
    const CnObs &o = c.b.o;
    const uint64_t n = c.total;
    int rc;
    if (c.decode && (rc = csvgpu_viterbi_dev(ctx, c.hmm, o.log2_cov, o.baf, o.pfb, o.obs_off, c.R, n, c.b.states, c.b.loglik))) return rc;
    struct Down { void *dst, *pin; const void *src; size_t bytes; };
    const Down down[] = {{c.out.obs_off, c.h_off, o.obs_off, (c.R + 1) * 8}, {c.out.pos, c.h_pos, o.pos, n * 4}, {c.out.baf, c.h_baf, o.baf, n * 8},
                         {c.out.pfb, c.h_pfb, o.pfb, n * 8}, {c.out.log2_cov, c.h_l2, o.log2_cov, n * 8}, {c.out.is_snp, c.h_snp, o.is_snp, n},
                         {c.out.states, c.h_states, c.b.states, n * 4}, {c.out.loglik, c.h_ll, c.b.loglik, c.R * 8}};
    for (const Down &d : down) {
        if (!d.dst || !d.pin) continue;
        CSV_HIP(ctx, hipMemcpyAsync(d.pin, d.src, d.bytes, hipMemcpyDeviceToHost, ctx->stream));
        c.pin.outs.push_back(PinStage::Out{d.dst, d.pin, d.bytes});
    }
    CSV_HIP(ctx, wait_stream(ctx->stream));
    c.pin.finish();
    return CSV_OK;
}
}  // namespace

int csvgpu_cn_observations_resident_many(csv_ctx *ctx, const csv_cn_regions *in, uint64_t *obs_off, uint32_t *pos, double *baf, double *pfb,
                                         double *log2_cov, uint8_t *is_snp, uint64_t *n_obs)
{
    if (!ctx) return CSV_EINVAL;
    CnCall c{"cn_observations", nullptr, false, {obs_off, pos, nullptr, nullptr, baf, pfb, log2_cov, is_snp}};
    const int rc = cn_run(ctx, in, n_obs, c);
    return rc ? rc : cn_finish(ctx, c, n_obs);
}

int csvgpu_cn_observations_tables_many(csv_ctx *ctx, const csv_cn_table_regions *in, uint64_t *obs_off, uint32_t *pos, double *baf, double *pfb,
                                       double *log2_cov, uint8_t *is_snp, uint64_t *n_obs)
{
    if (!ctx) return CSV_EINVAL;
    CnCall c{"cn_observations_tables", nullptr, false, {obs_off, pos, nullptr, nullptr, baf, pfb, log2_cov, is_snp}};
    const int rc = cn_tables_run(ctx, in, n_obs, c);
    return rc ? rc : cn_finish(ctx, c, n_obs);
}

int csvgpu_cn_decode_tables_many(csv_ctx *ctx, const csv_cn_table_regions *in, const csv_hmm *hmm, uint64_t *obs_off, uint32_t *pos, int32_t *states,
                                 double *loglik, double *baf, double *pfb, double *log2_cov, uint8_t *is_snp, uint64_t *n_obs)
{
    if (!ctx) return CSV_EINVAL;
    CnCall c{"cn_decode_tables", hmm, true, {obs_off, pos, states, loglik, baf, pfb, log2_cov, is_snp}};
    const int rc = cn_tables_run(ctx, in, n_obs, c);
    return rc ? rc : cn_finish(ctx, c, n_obs);
}

int csvgpu_cn_decode_resident_many(csv_ctx *ctx, const csv_cn_regions *in, const csv_hmm *hmm, uint64_t *obs_off, uint32_t *pos, int32_t *states,
                                   double *loglik, double *baf, double *pfb, double *log2_cov, uint8_t *is_snp, uint64_t *n_obs)
{
    if (!ctx) return CSV_EINVAL;
    CnCall c{"cn_decode", hmm, true, {obs_off, pos, states, loglik, baf, pfb, log2_cov, is_snp}};
    const int rc = cn_run(ctx, in, n_obs, c);
    return rc ? rc : cn_finish(ctx, c, n_obs);
}
