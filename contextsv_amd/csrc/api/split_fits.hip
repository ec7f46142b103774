// split_fits.hip — the split reads' overlap groups, their evidence, and the tables both are computed from.
#include "glue.hpp"

using namespace csv;

// The overlap groups that the order seeds (kernels/splitgroups.hip). One wait sizes the answer (members, groups, error word); the second is the
// answer's own copy. Everything in front of the first wait is queued without the host looking at the device.
// The chain in three steps, so that csvgpu_split_groups_fits can leave the groups where they lie: sg_queue reserves ctx->arena and the page-locked
// block (the chain's layout and stage, composed with the caller's: SgExtra below), stages the intervals and queues everything up to the copy of
// the three result words; sg_wait waits and reads them; the caller then reserves ctx->work for the member lists' sort (with whatever it
// needs beside it) and sg_fill_launch queues that sort.
constexpr uint32_t SG_ERR_DOMAIN = 2;             // in w.err: ORed in by an extra's kernel (the chain's own kernels OR in 1)
struct SgChain : SgWs {
    uint32_t n = 0;
    uint64_t n_seg = 0, max_len = 0;
    volatile uint64_t *h_res = nullptr;
    size_t pin_used = 0;                       // the page-locked block behind the chain's own staging: where the extra's stage runs
    uint64_t total = 0, n_groups = 0;
    const uint32_t *d_members = nullptr;       // after sg_fill
    const uint32_t *sort_flag = nullptr;       // the fill sort's gave-up word (device), or null
};


// host arrays on their way to carved device slices through the page-locked block
struct Upload { const void *dst, *src; size_t bytes; const void *pin; };
struct Uploads {                               // (the longest list: the eleven tables and four offset arrays of csvgpu_split_fits)
    Upload v[16];
    size_t n = 0;
    void add(const void *dst, const void *src, size_t bytes) { v[n++] = Upload{dst, src, bytes, nullptr}; }
    Upload *begin() { return v; }
    Upload *end() { return v + n; }
    const Upload *begin() const { return v; }
    const Upload *end() const { return v + n; }
};
static void stage_uploads(PinStage &p, Uploads &u) { for (Upload &x : u) x.pin = p.in(x.src, x.bytes); }
static int queue_uploads(csv_ctx *ctx, const Uploads &u, const char *what)
{
    for (const Upload &x : u) {
        if (!x.bytes) continue;
        const hipError_t e = hipMemcpyAsync((void *)x.dst, x.pin, x.bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) { ctx->err = std::string(what) + hipGetErrorString(e); return CSV_EHIP; }
    }
    return CSV_OK;
}

// What a fused entry point adds to the chain's two reservations: carve() takes its slices of ctx->arena behind the chain's (carved() follows the
// real pass: the upload list is built there, from the final pointers), stage() its slots of the page-locked block behind the chain's (planned by sg_queue; run for real by the extra's own queue(), or by the caller at c.pin_used once
// sg_queue has returned). on_device: start / end are not the caller's but written on the device, into c.d_start / c.d_end, by what queue()
// queues; the chain then skips its upload — and the caller's host range check. The chain's zeroed block (w.err with it) is cleared in front
// of queue(): what it queues may OR SG_ERR_DOMAIN into *c.w.err, which sg_wait reports as CSV_EINVAL.
struct SgNoExtra {
    static constexpr bool on_device = false;
    bool carve(Arena &) { return true; }
    void carved() {}
    void stage(PinStage &) {}
    int queue(SgChain &, PinStage &) { return CSV_OK; }
};

template <class Extra>
static int sg_queue(csv_ctx *ctx, const int32_t *start, const int32_t *end, const uint64_t *seg_off, uint64_t n_seg, uint32_t n, uint64_t max_len,
                    SgChain &c, Extra &x)
{
    (void)hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    int rc;
    c.n = n; c.n_seg = n_seg; c.max_len = max_len;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "split_groups", [&](Arena &a) { return carve_split_groups(a, n, n_seg, c) && x.carve(a); }))) return rc;
    x.carved();
    SplitGroupsWs &w = c.w;
    SortWs &sw = c.sw;
    int32_t *d_start = c.d_start, *d_end = c.d_end;
    uint64_t *d_seg = c.d_seg;
    void *es_tmp = c.es_tmp;
    constexpr bool on_device = Extra::on_device;

    const void *h_start = nullptr, *h_end = nullptr, *h_seg = nullptr;
    auto own = [&](PinStage &p) {
        if (!on_device) { h_start = p.in(start, (size_t)n * 4); h_end = p.in(end, (size_t)n * 4); }
        h_seg = p.in(seg_off, (n_seg + 1) * 8);
        c.h_res = (volatile uint64_t *)p.slot(256);
    };
    PinStage plan, pin(ctx);
    own(plan); x.stage(plan);
    if ((rc = ensure_pinned(ctx, plan.used))) return rc;
    own(pin);
    c.pin_used = pin.used;
    if (!on_device) {
        CSV_HIP(ctx, hipMemcpyAsync(d_start, h_start, (size_t)n * 4, hipMemcpyHostToDevice, s));
        CSV_HIP(ctx, hipMemcpyAsync(d_end, h_end, (size_t)n * 4, hipMemcpyHostToDevice, s));
    }
    CSV_HIP(ctx, hipMemcpyAsync(d_seg, h_seg, (n_seg + 1) * 8, hipMemcpyHostToDevice, s));
    if (on_device) {
        CSV_HIP(ctx, hipMemsetAsync(c.zero, 0, c.zero_bytes, s));
        if ((rc = x.queue(c, pin))) return rc;
    }
    const int key_bits = 32 + bits_of(n_seg - 1);
    const bool one_launch = onesweep(ctx);
    {
        TimerScope ts(ctx, CSV_K_SPLIT_GROUPS);
        if (!on_device) CSV_HIP(ctx, hipMemsetAsync(c.zero, 0, c.zero_bytes, s));
        launch_sg_keys(s, d_start, d_seg, n_seg, n, sw.k0, sw.v0);
        const int io = launch_radix_sort_u64(s, sw.k0, sw.v0, sw.k1, sw.v1, n, key_bits, sw.tmp, one_launch);
        launch_sg_links(s, w, io ? sw.k1 : sw.k0, io ? sw.v1 : sw.v0, d_start, d_end, d_seg, n);
        launch_exclusive_sum_u32(s, w.hist, (uint64_t)n + 1, es_tmp);
        launch_sg_seeds(s, w, n);
        launch_exclusive_sum_u32(s, w.cnt, (uint64_t)n + 1, es_tmp);
        launch_exclusive_sum_u32(s, w.keep, (uint64_t)n + 1, es_tmp);
        launch_sg_offsets(s, w, d_seg, n_seg, n, radix_sort_gave_up(sw.tmp, n, key_bits, one_launch));
        CSV_HIP(ctx, hipMemcpyAsync((void *)c.h_res, w.res, 24, hipMemcpyDeviceToHost, s));
    }
    return CSV_OK;
}

static int sg_wait(csv_ctx *ctx, SgChain &c)
{
    CSV_HIP(ctx, wait_stream(ctx->stream));
    c.total = c.h_res[0]; c.n_groups = c.h_res[1];
    if (c.h_res[2] & SG_ERR_DOMAIN) { ctx->err = "split_resident_fits: a coordinate of the shards is negative or end < start"; return CSV_EINVAL; }
    if (c.h_res[2]) { ctx->err = "split_groups: a bounded device loop gave up (radix look-back or seeding rounds)"; return CSV_EHIP; }
    if (c.n_groups > c.n || c.total < 2 * c.n_groups) { ctx->err = "split_groups: counts out of range"; return CSV_EHIP; }
    return CSV_OK;
}

// ---- the members: (group ‖ pre) keys, one stable sort for every group of the call ---------------------------------------------------------
static void sg_fill_launch(csv_ctx *ctx, SgChain &c, SortWs &fw)
{
    const int pre_bits = std::max(1, bits_of(c.max_len - 1)), fill_bits = pre_bits + bits_of(c.n_groups - 1);
    const bool one_launch = onesweep(ctx);
    launch_sg_fill(ctx->stream, c.w, (uint32_t)c.n_groups, pre_bits, fw.k0, fw.v0);
    const int io = launch_radix_sort_u64(ctx->stream, fw.k0, fw.v0, fw.k1, fw.v1, c.total, fill_bits, fw.tmp, one_launch);
    c.d_members = io ? fw.v1 : fw.v0;
    c.sort_flag = radix_sort_gave_up(fw.tmp, c.total, fill_bits, one_launch);
}

int csvgpu_split_groups(csv_ctx *ctx, const int32_t *start, const int32_t *end, const uint64_t *seg_off, uint64_t n_seg, uint64_t *seg_group_off,
                        uint64_t *group_off, uint32_t *members, uint64_t *n_members)
{
    if (!ctx) return CSV_EINVAL;
    if (!seg_off || !seg_group_off || !group_off || !n_members) { ctx->err = "split_groups: null array"; return CSV_EINVAL; }
    if (ctx->split_state) { ctx->err = "split_groups: a split order is pending on this context"; return CSV_EINVAL; }
    if (n_seg >= 0xffffffffull) { ctx->err = "split_groups: too many segments"; return CSV_EINVAL; }
    uint64_t max_len = 0;
    int rc = check_seg_off(ctx, "split_groups: seg_off not ascending", seg_off, n_seg, max_len);
    if (rc) return rc;
    const uint64_t n64 = seg_off[n_seg] - seg_off[0];
    if (seg_off[0] != 0) { ctx->err = "split_groups: seg_off[0] must be 0"; return CSV_EINVAL; }
    if (n64 >= 0xffffffffull) { ctx->err = "split_groups: more than 2^32 - 1 members"; return CSV_EINVAL; }
    const uint64_t capacity = *n_members;
    if (n64 && (!start || !end)) { ctx->err = "split_groups: null array"; return CSV_EINVAL; }
    if (capacity && !members) { ctx->err = "split_groups: null members with a capacity"; return CSV_EINVAL; }
    for (uint64_t i = 0; i < n64; i++) if (end[i] < start[i]) { ctx->err = "split_groups: end < start"; return CSV_EINVAL; }
    const uint32_t n = (uint32_t)n64;
    *n_members = 0;
    if (n == 0 || max_len < 2) {                             // no segment can hold a group of two
        for (uint64_t c = 0; c <= n_seg; c++) seg_group_off[c] = 0;
        group_off[0] = 0;
        return CSV_OK;
    }
    SgChain ch;
    SgNoExtra none;
    if ((rc = sg_queue(ctx, start, end, seg_off, n_seg, n, max_len, ch, none))) return rc;
    if ((rc = sg_wait(ctx, ch))) return rc;
    hipStream_t s = ctx->stream;
    const uint64_t total = ch.total, n_groups = ch.n_groups;
    *n_members = total;
    if (total > capacity) { ctx->err = "split_groups: members capacity too small"; return CSV_ECAPACITY; }
    if (total >= 0xffffffffull) { ctx->err = "split_groups: more than 2^32 - 1 entries in the answer"; *n_members = 0; return CSV_EINVAL; }
    if (n_groups == 0) {
        for (uint64_t c = 0; c <= n_seg; c++) seg_group_off[c] = 0;
        group_off[0] = 0;
        return CSV_OK;
    }
    SortWs fw;
    if ((rc = arena_reserve_for(ctx, ctx->work, "split_groups fill", [&](Arena &a) { return sortws_carve(a, total, fw); }))) return rc;
    constexpr size_t kPinnedOutMax = (size_t)64 << 20;       // larger answers are copied straight into the caller's array
    const bool members_pinned = total * 4 <= kPinnedOutMax;
    PinStage out(ctx);
    uint32_t *h_sort_err = nullptr;
    void *h_sgo = nullptr, *h_go = nullptr, *h_mem = nullptr;
    if ((rc = pin_reserve_for(ctx, out, [&](PinStage &p) {
            h_sort_err = (uint32_t *)p.slot(256);
            h_sgo = p.out(seg_group_off, (n_seg + 1) * 8); h_go = p.out(group_off, (n_groups + 1) * 8);
            if (members_pinned) h_mem = p.out(members, total * 4);
        }))) return rc;
    *h_sort_err = 0;
    {
        TimerScope ts(ctx, CSV_K_SPLIT_GROUPS);
        sg_fill_launch(ctx, ch, fw);
        if (ch.sort_flag) CSV_HIP(ctx, hipMemcpyAsync(h_sort_err, ch.sort_flag, 4, hipMemcpyDeviceToHost, s));
        CSV_HIP(ctx, hipMemcpyAsync(h_sgo, ch.w.seg_group_off, (n_seg + 1) * 8, hipMemcpyDeviceToHost, s));
        CSV_HIP(ctx, hipMemcpyAsync(h_go, ch.w.group_off, (n_groups + 1) * 8, hipMemcpyDeviceToHost, s));
        if (members_pinned) CSV_HIP(ctx, hipMemcpyAsync(h_mem, ch.d_members, total * 4, hipMemcpyDeviceToHost, s));
        else CSV_HIP(ctx, hipMemcpyAsync(members, ch.d_members, total * 4, hipMemcpyDeviceToHost, s));
    }
    CSV_HIP(ctx, wait_stream(s));
    if (*h_sort_err) { ctx->err = "split_groups: a radix pass's look-back gave up"; *n_members = 0; return CSV_EHIP; }
    out.finish();
    return CSV_OK;
}

// ---- the groups' evidence (kernels/splitfits.hip) ------------------------------------------------------------------------------------------
// Everything the two entry points share: argument checks, the tables' way to the device, the launch with its one readback, and the sets too
// large for LDS (materialised one by one, labelled by the large-segment path of csvgpu_dbscan_1d, reduced out of global memory).
static int sf_check(csv_ctx *ctx, const csv_split_tables *t, const uint64_t *seg_off, uint64_t n_seg, double eps, int32_t min_pts, uint64_t &max_len)
{
    int rc = check_dbscan_args(ctx, eps, min_pts, false);
    if (rc) return rc;
    if (!t || !seg_off) { ctx->err = "split_fits: null array"; return CSV_EINVAL; }
    if (ctx->split_state) { ctx->err = "split_fits: a split order is pending on this context"; return CSV_EINVAL; }
    if (n_seg >= 0xffffffffull) { ctx->err = "split_fits: too many segments"; return CSV_EINVAL; }
    if (seg_off[0] != 0) { ctx->err = "split_fits: seg_off[0] must be 0"; return CSV_EINVAL; }
    if ((rc = check_seg_off(ctx, "split_fits: seg_off not ascending", seg_off, n_seg, max_len))) return rc;
    const uint64_t nm = t->n_members, ns = t->n_supp;
    if (seg_off[n_seg] != nm) { ctx->err = "split_fits: seg_off does not end at the tables' member count"; return CSV_EINVAL; }
    if (nm >= 0xffffffffull || ns >= 0xffffffffull) { ctx->err = "split_fits: more than 2^32 - 1 members or supplementary records"; return CSV_EINVAL; }
    if (!t->supp_off || (nm && (!t->start || !t->end || !t->q_start || !t->q_end || !t->reverse)) ||
        (ns && (!t->supp_start || !t->supp_end || !t->supp_q_start || !t->supp_q_end || !t->supp_flags))) { ctx->err = "split_fits: null array in the tables"; return CSV_EINVAL; }
    if (t->supp_off[0] != 0 || t->supp_off[nm] != ns) { ctx->err = "split_fits: supp_off must run from 0 to n_supp"; return CSV_EINVAL; }
    for (uint64_t m = 0; m < nm; m++) {
        if (t->supp_off[m + 1] < t->supp_off[m]) { ctx->err = "split_fits: supp_off not ascending"; return CSV_EINVAL; }
        if (t->start[m] < 0 || t->q_start[m] < 0 || t->q_end[m] < 0 || t->end[m] < t->start[m]) { ctx->err = "split_fits: a member's coordinate is negative or end < start"; return CSV_EINVAL; }
    }
    for (uint64_t z = 0; z < ns; z++) {
        if (t->supp_flags[z] & 2u) continue;                 // another tid: only the flags are read
        if (t->supp_start[z] < 0 || t->supp_q_start[z] < 0 || t->supp_q_end[z] < 0 || t->supp_end[z] < t->supp_start[z]) {
            ctx->err = "split_fits: a supplementary record's coordinate is negative or end < start"; return CSV_EINVAL;
        }
    }
    return CSV_OK;
}

// the tables' way to their carved slices (carve_sf_tables with the same with_start_end)
static void sf_uploads(const csv_split_tables *t, const SplitFitsIn &in, bool with_start_end, Uploads &u)
{
    const uint64_t nm = t->n_members, ns = t->n_supp;
    if (with_start_end) { u.add(in.start, t->start, nm * 4); u.add(in.end, t->end, nm * 4); }
    u.add(in.q_start, t->q_start, nm * 4); u.add(in.q_end, t->q_end, nm * 4); u.add(in.reverse, t->reverse, nm);
    u.add(in.supp_off, t->supp_off, (nm + 1) * 8);
    u.add(in.supp_start, t->supp_start, ns * 4); u.add(in.supp_end, t->supp_end, ns * 4);
    u.add(in.supp_q_start, t->supp_q_start, ns * 4); u.add(in.supp_q_end, t->supp_q_end, ns * 4);
    u.add(in.supp_flags, t->supp_flags, ns);
}

struct SfRun : SfRunWs {                       // (carve_sf_run(n_groups, B) in the arena the run works in)
    SplitFitsIn in;
    uint64_t B = 0;                            // no set has more points
    volatile uint64_t *h_res = nullptr;        // sets and points beyond the LDS kernel
    void *h_out = nullptr;                     // the records' slot of the page-locked block
};
// the run's part of a stage: the two counters and the records
static void sf_stage(PinStage &p, SfRun &r, csv_split_fit *out)
{
    r.h_res = (volatile uint64_t *)p.slot(256);
    r.h_out = p.out(out, (size_t)r.in.n_groups * sizeof(csv_split_fit));
}

// the launch and the copies of the records and the two counters into the page-locked block; the caller adds its own copies and waits
static int sf_queue(csv_ctx *ctx, SfRun &r, double eps, int32_t min_pts)
{
    const uint64_t G = r.in.n_groups;
    hipStream_t s = ctx->stream;
    TimerScope ts(ctx, CSV_K_SPLIT_FITS);
    CSV_HIP(ctx, hipMemsetAsync(r.d_big_n, 0, G * 6 * 4, s));
    CSV_HIP(ctx, hipMemsetAsync(r.d_res, 0, 16, s));
    launch_sf_fits(s, r.in, eps, min_pts, r.d_out, r.d_big_n, r.d_res);
    CSV_HIP(ctx, hipMemcpyAsync((void *)r.h_res, r.d_res, 16, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, hipMemcpyAsync(r.h_out, r.d_out, G * sizeof(csv_split_fit), hipMemcpyDeviceToHost, s));
    return CSV_OK;
}

// after the wait, when r.h_res[0] sets were too large for LDS (the page-locked block is free again: its outputs have been taken)
static int sf_big(csv_ctx *ctx, SfRun &r, double eps, int32_t min_pts, csv_split_fit *out)
{
    const uint64_t n_big = r.h_res[0], G = r.in.n_groups, B = r.B;
    hipStream_t s = ctx->stream;
    int rc;
    std::vector<uint32_t> big_n(G * 6);
    CSV_HIP(ctx, hipMemcpyAsync(big_n.data(), r.d_big_n, G * 6 * 4, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, wait_stream(s));
    if (B <= DBSCAN1D_MAX_SEG) { ctx->err = "split_fits: a set larger than its bound"; return CSV_EHIP; }
    int32_t *pts = r.pts, *ks = r.ks, *labels = r.labels;      // (carved with the run: B > DBSCAN1D_MAX_SEG)
    uint32_t *sizes = r.sizes;
    void *tmp = r.tmp;
    PinStage pin(ctx);
    uint32_t *h_flags = nullptr;
    void *h_out = nullptr;
    if ((rc = pin_reserve_for(ctx, pin, [&](PinStage &p) { h_flags = (uint32_t *)p.slot(n_big * 4); h_out = p.out(out, G * sizeof(csv_split_fit)); }))) return rc;
    memset(h_flags, 0, n_big * 4);
    {
        TimerScope ts(ctx, CSV_K_SPLIT_FITS);
        uint64_t k = 0;
        for (uint64_t item = 0; item < G * 6; item++) {
            const uint32_t n = big_n[item];
            if (!n) continue;
            if (n > B || n <= DBSCAN1D_MAX_SEG || k >= n_big) { ctx->err = "split_fits: large-set counts out of range"; return CSV_EHIP; }
            launch_sf_big_points(s, r.in, (uint32_t)item, pts);
            const uint32_t *perm = sorted_perm(ctx, pts, n, r.w);
            if (const uint32_t *flag = radix_sort_gave_up(r.w.tmp, n, 32, onesweep(ctx))) CSV_HIP(ctx, hipMemcpyAsync(h_flags + k, flag, 4, hipMemcpyDeviceToHost, s));
            launch_gather_u32(s, (const uint32_t *)pts, perm, n, (uint32_t *)ks);
            launch_dbscan_1d_big(s, ks, perm, n, eps, min_pts, labels, tmp);
            CSV_HIP(ctx, hipMemsetAsync(sizes, 0, (size_t)n * 4, s));
            launch_sf_big_reduce(s, ks, perm, labels, n, sizes, r.d_out + item / 6, (int)(item % 6));
            k++;
        }
        CSV_HIP(ctx, hipMemcpyAsync(h_out, r.d_out, G * sizeof(csv_split_fit), hipMemcpyDeviceToHost, s));
    }
    CSV_HIP(ctx, wait_stream(s));
    for (uint64_t k = 0; k < n_big; k++) if (h_flags[k]) { ctx->err = "split_fits: a radix pass's look-back gave up"; return CSV_EHIP; }
    pin.finish();
    return CSV_OK;
}

// what the fused calls share behind the chain's queue (r.in's tables set): the one sizing readback, the member lists' sort, the fits' launch and
// its records, the sets too large for LDS
static int sgf_finish(csv_ctx *ctx, SgChain &ch, SfRun &r, uint64_t n_seg, uint64_t max_len, uint64_t ns, double eps, int32_t min_pts,
                      uint64_t *seg_group_off, csv_split_fit *out, uint64_t *n_groups)
{
    int rc;
    hipStream_t s = ctx->stream;
    if ((rc = sg_wait(ctx, ch))) return rc;
    const uint64_t G = ch.n_groups, total = ch.total;
    if (total >= 0xffffffffull) { ctx->err = "split_fits: more than 2^32 - 1 entries in the groups"; return CSV_EINVAL; }
    if (G == 0) {
        for (uint64_t c = 0; c <= n_seg; c++) seg_group_off[c] = 0;
        return CSV_OK;
    }
    r.B = std::max(std::min(total, max_len), ns);
    SortWs fw;
    if ((rc = arena_reserve_for(ctx, ctx->work, "split_fits work", [&](Arena &a) { return sortws_carve(a, total, fw) && carve_sf_run(a, G, r.B, r); }))) return rc;
    r.in.n_groups = (uint32_t)G;
    PinStage pin(ctx);
    uint32_t *h_sort_err = nullptr;
    void *h_sgo = nullptr;
    if ((rc = pin_reserve_for(ctx, pin, [&](PinStage &p) {
            h_sort_err = (uint32_t *)p.slot(256);
            h_sgo = p.out(seg_group_off, (n_seg + 1) * 8);
            sf_stage(p, r, out);
        }))) return rc;
    *h_sort_err = 0;
    {
        TimerScope ts(ctx, CSV_K_SPLIT_GROUPS);
        sg_fill_launch(ctx, ch, fw);
        if (ch.sort_flag) CSV_HIP(ctx, hipMemcpyAsync(h_sort_err, ch.sort_flag, 4, hipMemcpyDeviceToHost, s));
        CSV_HIP(ctx, hipMemcpyAsync(h_sgo, ch.w.seg_group_off, (n_seg + 1) * 8, hipMemcpyDeviceToHost, s));
    }
    r.in.seg_off = ch.d_seg; r.in.seg_group_off = ch.w.seg_group_off; r.in.group_off = ch.w.group_off; r.in.members = ch.d_members;
    r.in.n_seg = n_seg;
    if ((rc = sf_queue(ctx, r, eps, min_pts))) return rc;
    CSV_HIP(ctx, wait_stream(s));
    if (*h_sort_err) { ctx->err = "split_fits: a radix pass's look-back gave up"; return CSV_EHIP; }
    pin.finish();
    *n_groups = G;
    if (r.h_res[0] == 0) return CSV_OK;
    return sf_big(ctx, r, eps, min_pts, out);
}

int csvgpu_split_fits(csv_ctx *ctx, const csv_split_tables *t, const uint64_t *seg_off, uint64_t n_seg, const uint64_t *seg_group_off,
                      const uint64_t *group_off, const uint32_t *members, double eps, int32_t min_pts, csv_split_fit *out)
{
    if (!ctx) return CSV_EINVAL;
    uint64_t max_len = 0;
    int rc = sf_check(ctx, t, seg_off, n_seg, eps, min_pts, max_len);
    if (rc) return rc;
    if (!seg_group_off || !group_off) { ctx->err = "split_fits: null array"; return CSV_EINVAL; }
    if (seg_group_off[0] != 0 || group_off[0] != 0) { ctx->err = "split_fits: group offsets must start at 0"; return CSV_EINVAL; }
    for (uint64_t c = 0; c < n_seg; c++) if (seg_group_off[c + 1] < seg_group_off[c]) { ctx->err = "split_fits: seg_group_off not ascending"; return CSV_EINVAL; }
    const uint64_t G = seg_group_off[n_seg];
    if (G > t->n_members) { ctx->err = "split_fits: more groups than members"; return CSV_EINVAL; }
    uint64_t max_group = 0;
    for (uint64_t g = 0; g < G; g++) {
        if (group_off[g + 1] < group_off[g]) { ctx->err = "split_fits: group_off not ascending"; return CSV_EINVAL; }
        max_group = std::max(max_group, group_off[g + 1] - group_off[g]);
    }
    if (G == 0) return CSV_OK;
    const uint64_t total = group_off[G];
    if (total >= 0xffffffffull) { ctx->err = "split_fits: more than 2^32 - 1 entries in the groups"; return CSV_EINVAL; }
    if (!out || (total && !members)) { ctx->err = "split_fits: null array"; return CSV_EINVAL; }
    {   // members: inside their segment, and distinct within a group (a group is a set of reads; the large-set bound below counts on it)
        std::vector<uint64_t> seen(max_len, 0);              // by member of the current segment: the last group (+ 1) that held it
        for (uint64_t c = 0; c < n_seg; c++) {
            const uint64_t len = seg_off[c + 1] - seg_off[c];
            for (uint64_t g = seg_group_off[c]; g < seg_group_off[c + 1]; g++)
                for (uint64_t q = group_off[g]; q < group_off[g + 1]; q++) {
                    if (members[q] >= len) { ctx->err = "split_fits: a member index outside its segment"; return CSV_EINVAL; }
                    if (seen[members[q]] == g + 1) { ctx->err = "split_fits: a member twice in one group"; return CSV_EINVAL; }
                    seen[members[q]] = g + 1;
                }
        }
    }
    (void)hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    const uint64_t nm = t->n_members, ns = t->n_supp;
    SfRun r;
    r.B = std::max(max_group, ns);
    uint64_t *d_seg = nullptr, *d_sgo = nullptr, *d_go = nullptr;
    uint32_t *d_mem = nullptr;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "split_fits", [&](Arena &a) {
            return carve_sf_tables(a, nm, ns, true, r.in) && take(a, d_seg, (n_seg + 1) * 8) && take(a, d_sgo, (n_seg + 1) * 8) && take(a, d_go, (G + 1) * 8) &&
                   take(a, d_mem, total * 4) && carve_sf_run(a, G, r.B, r);
        }))) return rc;
    r.in.seg_off = d_seg; r.in.seg_group_off = d_sgo; r.in.group_off = d_go; r.in.members = d_mem;
    r.in.n_seg = n_seg; r.in.n_groups = (uint32_t)G;
    Uploads up;
    sf_uploads(t, r.in, true, up);
    up.add(d_seg, seg_off, (n_seg + 1) * 8); up.add(d_sgo, seg_group_off, (n_seg + 1) * 8);
    up.add(d_go, group_off, (G + 1) * 8); up.add(d_mem, members, total * 4);
    PinStage pin(ctx);
    if ((rc = pin_reserve_for(ctx, pin, [&](PinStage &p) { stage_uploads(p, up); sf_stage(p, r, out); }))) return rc;
    if ((rc = queue_uploads(ctx, up, "split_fits: copying the tables: "))) return rc;
    if ((rc = sf_queue(ctx, r, eps, min_pts))) return rc;
    CSV_HIP(ctx, wait_stream(s));
    pin.finish();
    if (r.h_res[0] == 0) return CSV_OK;
    return sf_big(ctx, r, eps, min_pts, out);
}

namespace {
// the caller's tables beside the chain (SgExtra of csvgpu_split_groups_fits); start / end are the chain's copies
struct SfTablesExtra {
    static constexpr bool on_device = false;
    const csv_split_tables *t; SplitFitsIn &in; Uploads up;
    bool carve(Arena &a) { return carve_sf_tables(a, t->n_members, t->n_supp, false, in); }
    void carved() { sf_uploads(t, in, false, up); }
    void stage(PinStage &p) { stage_uploads(p, up); }
    int queue(SgChain &, PinStage &) { return CSV_OK; }
};
}  // namespace

int csvgpu_split_groups_fits(csv_ctx *ctx, const csv_split_tables *t, const uint64_t *seg_off, uint64_t n_seg, double eps, int32_t min_pts,
                             uint64_t *seg_group_off, csv_split_fit *out, uint64_t *n_groups)
{
    if (!ctx) return CSV_EINVAL;
    uint64_t max_len = 0;
    int rc = sf_check(ctx, t, seg_off, n_seg, eps, min_pts, max_len);
    if (rc) return rc;
    if (!seg_group_off || !n_groups) { ctx->err = "split_fits: null array"; return CSV_EINVAL; }
    const uint64_t nm = t->n_members, ns = t->n_supp;
    if (nm && !out) { ctx->err = "split_fits: null array"; return CSV_EINVAL; }
    *n_groups = 0;
    if (nm == 0 || max_len < 2) {                            // no segment can hold a group of two
        for (uint64_t c = 0; c <= n_seg; c++) seg_group_off[c] = 0;
        return CSV_OK;
    }
    hipStream_t s = ctx->stream;
    SgChain ch;
    SfRun r;
    SfTablesExtra tables{t, r.in, {}};
    if ((rc = sg_queue(ctx, t->start, t->end, seg_off, n_seg, (uint32_t)nm, max_len, ch, tables))) return rc;
    r.in.start = ch.d_start; r.in.end = ch.d_end;
    {   // the tables travel while the chain runs
        PinStage pin(ctx, ch.pin_used);
        tables.stage(pin);
        if ((rc = queue_uploads(ctx, tables.up, "split_fits: copying the tables: "))) { (void)wait_stream(s); return rc; }
    }
    return sgf_finish(ctx, ch, r, n_seg, max_len, ns, eps, min_pts, seg_group_off, out, n_groups);
}

// ---- the tables from the resident shards (kernels/splittables.hip) ------------------------------------------------------------------------
// What the two entry points share: the checks of the references (everything the kernel indexes with is bounded here), their way to the device
// and the launch.
static int sr_check(csv_ctx *ctx, uint64_t n_seg, csv_shard *const *shards, const csv_split_refs *f, const uint64_t *seg_off, uint64_t &max_len)
{
    if (!f || !seg_off || (n_seg && !shards)) { ctx->err = "split_tables_resident: null array"; return CSV_EINVAL; }
    if (ctx->split_state) { ctx->err = "split_tables_resident: a split order is pending on this context"; return CSV_EINVAL; }
    if (n_seg >= 0xffffffffull) { ctx->err = "split_tables_resident: too many segments"; return CSV_EINVAL; }
    const uint64_t nm = f->n_members, ns = f->n_supp;
    if (nm >= 0xffffffffull || ns >= 0xffffffffull) { ctx->err = "split_tables_resident: 2^32 - 1 or more members or supplementary entries"; return CSV_EINVAL; }
    if (!f->supp_off || (nm && !f->member_rec) || (ns && (!f->supp_rec || !f->supp_where))) { ctx->err = "split_tables_resident: null array in the references"; return CSV_EINVAL; }
    if (seg_off[0] != 0) { ctx->err = "split_tables_resident: seg_off[0] must be 0"; return CSV_EINVAL; }
    const int rc = check_seg_off(ctx, "split_tables_resident: seg_off not ascending", seg_off, n_seg, max_len);
    if (rc) return rc;
    if (seg_off[n_seg] != nm) { ctx->err = "split_tables_resident: seg_off does not end at the references' member count"; return CSV_EINVAL; }
    if (f->supp_off[0] != 0 || f->supp_off[nm] != ns) { ctx->err = "split_tables_resident: supp_off must run from 0 to n_supp"; return CSV_EINVAL; }
    for (uint64_t m = 0; m < nm; m++) if (f->supp_off[m + 1] < f->supp_off[m]) { ctx->err = "split_tables_resident: supp_off not ascending"; return CSV_EINVAL; }
    for (uint64_t c = 0; c < n_seg; c++) {
        const csv_shard *sh = shards[c];
        if (!sh || (sh->d.n_reads && (!sh->d.pos || !sh->d.flag || !sh->ref_end || !sh->q_start || !sh->q_end))) { ctx->err = "split_tables_resident: null shard"; return CSV_EINVAL; }
        const uint64_t n_reads = sh->d.n_reads;
        for (uint64_t m = seg_off[c]; m < seg_off[c + 1]; m++) {
            if (f->member_rec[m] >= n_reads) { ctx->err = "split_tables_resident: a member's record index beyond its shard"; return CSV_EINVAL; }
            for (uint64_t z = f->supp_off[m]; z < f->supp_off[m + 1]; z++) {
                const uint8_t w = f->supp_where[z];
                if (w != 0 && w != 2 && w != 3) { ctx->err = "split_tables_resident: supp_where must be 0, 2 or 3"; return CSV_EINVAL; }
                if (w == 0 && f->supp_rec[z] >= n_reads) { ctx->err = "split_tables_resident: a supplementary record index beyond its shard"; return CSV_EINVAL; }
            }
        }
    }
    return CSV_OK;
}

// the references and the shard table on their way to carve_sr_refs' slices, and the launch behind them. d_seg: seg_off on the device.
// in.supp_off is what the fits read afterwards.
struct SrRefs {
    std::vector<SplitTabSeg> tab;
    Uploads up;
    SplitTablesIn in;
    void uploads(uint64_t n_seg, csv_shard *const *shards, const csv_split_refs *f)       // after the carve
    {
        const uint64_t nm = f->n_members, ns = f->n_supp;
        tab.resize(n_seg);
        for (uint64_t c = 0; c < n_seg; c++) { const csv_shard *sh = shards[c]; tab[c] = SplitTabSeg{sh->d.pos, sh->d.flag, sh->ref_end, sh->q_start, sh->q_end}; }
        up.add(in.seg, tab.data(), n_seg * sizeof(SplitTabSeg)); up.add(in.member_rec, f->member_rec, nm * 4); up.add(in.supp_off, f->supp_off, (nm + 1) * 8);
        up.add(in.supp_rec, f->supp_rec, ns * 4); up.add(in.supp_where, f->supp_where, ns);
        in.n_seg = n_seg; in.n_members = (uint32_t)nm; in.n_supp = (uint32_t)ns;
    }
    int launch(csv_ctx *ctx, const uint64_t *d_seg, const SplitTablesOut &out)
    {
        const int rc = queue_uploads(ctx, up, "split_tables_resident: copying the references: ");
        if (rc) return rc;
        in.seg_off = d_seg;
        TimerScope ts(ctx, CSV_K_MISC);
        launch_st_tables(ctx->stream, in, out);
        return CSV_OK;
    }
};

int csvgpu_split_tables_resident(csv_ctx *ctx, uint64_t n_seg, csv_shard *const *shards, const csv_split_refs *f, const uint64_t *seg_off, csv_split_tables *t)
{
    if (!ctx) return CSV_EINVAL;
    uint64_t max_len = 0;
    int rc = sr_check(ctx, n_seg, shards, f, seg_off, max_len);
    if (rc) return rc;
    if (!t) { ctx->err = "split_tables_resident: null array"; return CSV_EINVAL; }
    const uint64_t nm = f->n_members, ns = f->n_supp;
    if (!t->supp_off || (nm && (!t->start || !t->end || !t->q_start || !t->q_end || !t->reverse)) ||
        (ns && (!t->supp_start || !t->supp_end || !t->supp_q_start || !t->supp_q_end || !t->supp_flags))) { ctx->err = "split_tables_resident: null array in the tables"; return CSV_EINVAL; }
    if (nm == 0) {
        t->n_members = t->n_supp = 0;
        ((uint64_t *)t->supp_off)[0] = 0;
        return CSV_OK;
    }
    (void)hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    SplitTablesOut o;
    SrRefs refs;
    uint64_t *d_seg = nullptr;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "split_tables_resident", [&](Arena &a) {
            return take(a, o.start, nm * 4) && take(a, o.end, nm * 4) && take(a, d_seg, (n_seg + 1) * 8) && take(a, o.err, 256) && sr_carve(a, nm, ns, o) &&
                   carve_sr_refs(a, n_seg, nm, ns, refs.in);
        }))) return rc;
    o.err_bit = 1;
    refs.uploads(n_seg, shards, f);
    struct Down { void *dst; const void *src; size_t bytes; void *pin; };
    Down down[] = {{(void *)t->start, o.start, nm * 4, nullptr}, {(void *)t->end, o.end, nm * 4, nullptr}, {(void *)t->q_start, o.q_start, nm * 4, nullptr},
                   {(void *)t->q_end, o.q_end, nm * 4, nullptr}, {(void *)t->reverse, o.reverse, nm, nullptr},
                   {(void *)t->supp_start, o.supp_start, ns * 4, nullptr}, {(void *)t->supp_end, o.supp_end, ns * 4, nullptr},
                   {(void *)t->supp_q_start, o.supp_q_start, ns * 4, nullptr}, {(void *)t->supp_q_end, o.supp_q_end, ns * 4, nullptr},
                   {(void *)t->supp_flags, o.supp_flags, ns, nullptr}};
    PinStage pin(ctx);
    const void *h_seg = nullptr;
    volatile uint32_t *h_err = nullptr;
    if ((rc = pin_reserve_for(ctx, pin, [&](PinStage &p) {
            h_seg = p.in(seg_off, (n_seg + 1) * 8);
            stage_uploads(p, refs.up);
            h_err = (volatile uint32_t *)p.slot(256);
            for (Down &d : down) d.pin = p.out(d.dst, d.bytes);
        }))) return rc;
    CSV_HIP(ctx, hipMemsetAsync(o.err, 0, 4, s));
    CSV_HIP(ctx, hipMemcpyAsync(d_seg, h_seg, (n_seg + 1) * 8, hipMemcpyHostToDevice, s));
    if ((rc = refs.launch(ctx, d_seg, o))) { (void)wait_stream(s); return rc; }
    CSV_HIP(ctx, hipMemcpyAsync((void *)h_err, o.err, 4, hipMemcpyDeviceToHost, s));
    for (const Down &d : down) if (d.bytes) CSV_HIP(ctx, hipMemcpyAsync(d.pin, d.src, d.bytes, hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, wait_stream(s));
    if (*h_err) { ctx->err = "split_tables_resident: a coordinate of the shards is negative or end < start"; return CSV_EINVAL; }
    pin.finish();
    memcpy((void *)t->supp_off, f->supp_off, (nm + 1) * 8);
    t->n_members = nm; t->n_supp = ns;
    return CSV_OK;
}

namespace {
// the tables built on the device in front of the chain (SgExtra of csvgpu_split_resident_fits)
struct SrFill {
    static constexpr bool on_device = true;
    csv_ctx *ctx; uint64_t n_seg; csv_shard *const *shards; const csv_split_refs *f;
    SplitFitsIn *fits_in;
    SplitTablesOut o;
    SrRefs refs;
    bool carve(Arena &a) { return sr_carve(a, f->n_members, f->n_supp, o) && carve_sr_refs(a, n_seg, f->n_members, f->n_supp, refs.in); }
    void carved() { refs.uploads(n_seg, shards, f); }
    void stage(PinStage &p) { stage_uploads(p, refs.up); }
    int queue(SgChain &c, PinStage &pin)
    {
        o.start = c.d_start; o.end = c.d_end;
        o.err = c.w.err; o.err_bit = SG_ERR_DOMAIN;
        stage(pin);
        const int rc = refs.launch(ctx, c.d_seg, o);
        if (rc) return rc;
        SplitFitsIn &r = *fits_in;
        r.start = o.start; r.end = o.end; r.q_start = o.q_start; r.q_end = o.q_end; r.reverse = o.reverse; r.supp_off = refs.in.supp_off;
        r.supp_start = o.supp_start; r.supp_end = o.supp_end; r.supp_q_start = o.supp_q_start; r.supp_q_end = o.supp_q_end; r.supp_flags = o.supp_flags;
        return CSV_OK;
    }
};
}  // namespace

int csvgpu_split_resident_fits(csv_ctx *ctx, uint64_t n_seg, csv_shard *const *shards, const csv_split_refs *f, const uint64_t *seg_off, double eps,
                               int32_t min_pts, uint64_t *seg_group_off, csv_split_fit *out, uint64_t *n_groups)
{
    if (!ctx) return CSV_EINVAL;
    int rc = check_dbscan_args(ctx, eps, min_pts, false);
    if (rc) return rc;
    uint64_t max_len = 0;
    if ((rc = sr_check(ctx, n_seg, shards, f, seg_off, max_len))) return rc;
    if (!seg_group_off || !n_groups) { ctx->err = "split_resident_fits: null array"; return CSV_EINVAL; }
    const uint64_t nm = f->n_members, ns = f->n_supp;
    if (nm && !out) { ctx->err = "split_resident_fits: null array"; return CSV_EINVAL; }
    *n_groups = 0;
    if (nm == 0 || max_len < 2) {                            // no segment can hold a group of two
        for (uint64_t c = 0; c <= n_seg; c++) seg_group_off[c] = 0;
        return CSV_OK;
    }
    SgChain ch;
    SfRun r;
    SrFill fill;
    fill.ctx = ctx; fill.n_seg = n_seg; fill.shards = shards; fill.f = f; fill.fits_in = &r.in;
    if ((rc = sg_queue(ctx, nullptr, nullptr, seg_off, n_seg, (uint32_t)nm, max_len, ch, fill))) { (void)wait_stream(ctx->stream); return rc; }
    return sgf_finish(ctx, ch, r, n_seg, max_len, ns, eps, min_pts, seg_group_off, out, n_groups);
}
