// merge_select.hip — the representative choice of mergeSVs on the device: the slot replay as a batched primitive (csvgpu_sort_slot), the
// records of one contig's representatives from host arrays (csvgpu_merge_select) and from the results a pipeline left on a shard
// (csvgpu_chr_merge_select). Kernels: kernels/mergeselect.hip; the rule: sort_select_core.hpp.
#include "glue.hpp"

namespace csv {

int merge_select_queue(csv_ctx *ctx, csv_shard *sh, const csv_sig *d_sig_del, const int32_t *d_lab_del, uint64_t n_del, const csv_sig *d_sig_ins,
                       const int32_t *d_lab_ins, uint64_t n_ins, const int64_t *max_label, uint32_t max_partitions, MergeRunWs &w)
{
    int rc;
    if (!sh) {
        if ((rc = arena_reserve_for(ctx, ctx->work, "merge select", [&](Arena &a) { return carve_merge_run(a, n_del, n_ins, w); }))) return rc;
    } else {
        // the shard's own scratch, sized by running the carve: nothing of the context's workspaces, which a job queued ahead may be using
        const size_t need = arena_plan_bytes([&](Arena &a) { return carve_merge_run(a, n_del, n_ins, w); });
        if (need > sh->sel_cap) {
            if (sh->sel_scratch) CSV_HIP(ctx, hipFree(sh->sel_scratch));
            sh->sel_scratch = nullptr; sh->sel_cap = 0;
            if (test_fail_alloc()) { ctx->err = "hipMalloc failed (select scratch)"; return CSV_ENOMEM; }
            CSV_HIP(ctx, hipMalloc((void **)&sh->sel_scratch, need + need / 4));
            sh->sel_cap = need + need / 4;
        }
        Arena sa; sa.base = sh->sel_scratch; sa.cap = sh->sel_cap; sa.used = 0;
        if (!carve_merge_run(sa, n_del, n_ins, w)) { ctx->err = "select scratch exhausted"; return CSV_ENOMEM; }
    }
    hipStream_t s = ctx->stream;
    const uint64_t bound = merge_rep_bound(n_del, n_ins);
    TimerScope ts(ctx, CSV_K_MISC);
    CSV_HIP(ctx, hipMemsetAsync(w.back, 0, sizeof(MergeBack), s));
    const csv_sig *sig[2] = {d_sig_del, d_sig_ins};
    const int32_t *lab[2] = {d_lab_del, d_lab_ins};
    const uint64_t n[2] = {n_del, n_ins};
    for (int type = 0; type < 2; type++) {
        if (n[type] == 0) continue;
        const uint32_t *flag = nullptr;
        launch_merge_select_type(s, w.ms, sig[type], lab[type], n[type], type, bits_of((uint64_t)(max_label[type] + 2)), max_partitions, onesweep(ctx),
                                 &w.back->counts, w.rep, bound, &flag);
        if (flag) CSV_HIP(ctx, hipMemcpyAsync(&w.back->gave_up[type], flag, 4, hipMemcpyDeviceToDevice, s));
    }
    return CSV_OK;
}

// The same, waited for: the counts, then exactly the records, come back in two short waits.
static int merge_select_dev(csv_ctx *ctx, csv_shard *sh, const csv_sig *d_sig_del, const int32_t *d_lab_del, uint64_t n_del, const csv_sig *d_sig_ins,
                            const int32_t *d_lab_ins, uint64_t n_ins, const int64_t *max_label, uint32_t max_partitions, csv_merge_rep *rep_out,
                            uint64_t capacity, csv_merge_counts *counts)
{
    int rc;
    MergeRunWs w;
    Transfer t(ctx);
    if ((rc = t.open("merge select"))) return rc;
    if ((rc = merge_select_queue(ctx, sh, d_sig_del, d_lab_del, n_del, d_sig_ins, d_lab_ins, n_ins, max_label, max_partitions, w))) return rc;
    MergeBack h;
    if ((rc = t.peek(&h, w.back, sizeof(MergeBack)))) return rc;
    if (h.gave_up[0] || h.gave_up[1]) { ctx->err = "merge select: a radix pass's look-back gave up"; return CSV_EHIP; }
    *counts = h.counts;
    const uint64_t n_rep = h.counts.n_rep[0] + h.counts.n_rep[1];
    if (n_rep > merge_rep_bound(n_del, n_ins)) { ctx->err = "merge select: more records than buckets"; return CSV_EHIP; }
    if (n_rep > capacity) { ctx->err = "merge select: rep_out too small"; return CSV_ECAPACITY; }
    return t.down(rep_out, w.rep, n_rep * sizeof(csv_merge_rep));
}

}  // namespace csv

using namespace csv;

int csvgpu_sort_slot(csv_ctx *ctx, const uint32_t *keys, const uint64_t *seg_off, uint64_t n_seg, const uint64_t *nth, uint32_t max_partitions,
                     uint32_t *idx_out, uint8_t *declined_out)
{
    if (!ctx) return CSV_EINVAL;
    if (ctx->split_state) { ctx->err = "sort slot: a split order is pending on this context"; return CSV_EINVAL; }
    if (n_seg == 0) return CSV_OK;
    if (!seg_off || !nth || !idx_out) { ctx->err = "sort slot: null array"; return CSV_EINVAL; }
    uint64_t max_len = 0;
    int rc;
    if ((rc = check_seg_off(ctx, "sort slot: seg_off not monotone", seg_off, n_seg, max_len))) return rc;
    if (seg_off[0] != 0) { ctx->err = "sort slot: seg_off must start at 0"; return CSV_EINVAL; }
    const uint64_t n = seg_off[n_seg];
    if (n >= (1ull << 31) || n_seg >= (1ull << 31)) { ctx->err = "sort slot: 2^31 or more keys or segments"; return CSV_EINVAL; }
    if (n && !keys) { ctx->err = "sort slot: null array"; return CSV_EINVAL; }
    for (uint64_t sg = 0; sg < n_seg; sg++)
        if (seg_off[sg + 1] > seg_off[sg] && nth[sg] >= seg_off[sg + 1] - seg_off[sg]) { ctx->err = "sort slot: a slot beyond its segment"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    // the entries as the kernels take them: (key << 32) | index inside the segment
    std::vector<uint64_t> ent(n);
    std::vector<uint32_t> off(n_seg + 1), slot(n_seg);
    for (uint64_t sg = 0; sg < n_seg; sg++) {
        off[sg] = (uint32_t)seg_off[sg];
        slot[sg] = seg_off[sg + 1] > seg_off[sg] ? (uint32_t)nth[sg] : 0u;
        for (uint64_t i = seg_off[sg]; i < seg_off[sg + 1]; i++) ent[i] = ((uint64_t)keys[i] << 32) | (uint32_t)(i - seg_off[sg]);
    }
    off[n_seg] = (uint32_t)n;
    SortSlotWs w;
    if ((rc = arena_reserve_for(ctx, ctx->work, "sort slot", [&](Arena &a) { return carve_sort_slot(a, n, n_seg, w); }))) return rc;
    Transfer t(ctx);
    if ((rc = t.open("sort slot"))) return rc;
    const uint32_t cnt[3] = {0, 0, (uint32_t)n_seg};
    if ((rc = t.up(w.ent, ent.data(), n * 8)) || (rc = t.up(w.off, off.data(), (n_seg + 1) * 4)) || (rc = t.up(w.nth, slot.data(), n_seg * 4)) ||
        (rc = t.up(w.cnt, cnt, sizeof(cnt)))) return rc;
    {
        TimerScope ts(ctx, CSV_K_MISC);
        SortSlotArgs b;
        b.off = w.off; b.n_seg = w.cnt + 2; b.nth = w.nth; b.ent = w.ent; b.list = w.list; b.mid = w.mid; b.big = w.big; b.cnt = w.cnt; b.idx = w.idx;
        b.keep = nullptr; b.max_partitions = max_partitions;
        launch_sort_slot(ctx->stream, b, n, n_seg);
    }
    CSV_HIP(ctx, hipGetLastError());
    if ((rc = t.down(idx_out, w.idx, n_seg * 4))) return rc;
    if (declined_out) for (uint64_t sg = 0; sg < n_seg; sg++) declined_out[sg] = idx_out[sg] == 0xffffffffu && seg_off[sg + 1] > seg_off[sg];
    return CSV_OK;
}

int csvgpu_merge_select(csv_ctx *ctx, const csv_sig *sig, const int32_t *labels, uint64_t n_del, uint64_t n_ins, uint32_t max_partitions,
                        csv_merge_rep *rep_out, uint64_t capacity, csv_merge_counts *counts)
{
    if (!ctx) return CSV_EINVAL;
    if (ctx->split_state) { ctx->err = "merge select: a split order is pending on this context"; return CSV_EINVAL; }
    const uint64_t n = n_del + n_ins;
    if (!counts || (capacity && !rep_out) || (n && !sig) || ((n_del >= 2 || n_ins >= 2) && !labels)) { ctx->err = "merge select: null array"; return CSV_EINVAL; }
    if (n_del >= (1ull << 31) || n_ins >= (1ull << 31)) { ctx->err = "merge select: 2^31 or more signatures of a type"; return CSV_EINVAL; }
    const uint64_t type_n[2] = {n_del, n_ins};
    int64_t max_label[2] = {-2, -2};
    for (int type = 0; type < 2; type++) {
        if (type_n[type] < 2) continue;                       // (a type that passes through has no labels: none are read)
        const int32_t *lab = labels + (type ? n_del : 0);
        for (uint64_t i = 0; i < type_n[type]; i++)
            if (lab[i] < -2 || lab[i] >= (int32_t)0x7ffffff0) { ctx->err = "merge select: a label below -2 or above 2^31 - 17"; return CSV_EINVAL; }
            else max_label[type] = std::max<int64_t>(max_label[type], lab[i]);
    }
    memset(counts, 0, sizeof(*counts));
    if (n == 0) return CSV_OK;
    (void)hipSetDevice(ctx->device);
    int rc;
    csv_sig *d_sig = nullptr;
    int32_t *d_lab = nullptr;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "merge select arrays", [&](Arena &a) { return take(a, d_sig, n * sizeof(csv_sig)) && take(a, d_lab, n * 4); }))) return rc;
    {
        Transfer t(ctx);
        if ((rc = t.open("merge select"))) return rc;
        if ((rc = t.up(d_sig, sig, n * sizeof(csv_sig)))) return rc;
        for (int type = 0; type < 2; type++)                  // (a type that passes through has no labels: none are read, none travel)
            if (type_n[type] >= 2 && (rc = t.up(d_lab + (type ? n_del : 0), labels + (type ? n_del : 0), type_n[type] * 4))) return rc;
        if ((rc = t.wait())) return rc;
    }
    return merge_select_dev(ctx, nullptr, d_sig, d_lab, n_del, d_sig + n_del, d_lab + n_del, n_ins, max_label, max_partitions, rep_out, capacity, counts);
}

int csvgpu_chr_merge_select(csv_ctx *ctx, csv_shard *shard, const csv_chr_result *result, uint32_t max_partitions, csv_merge_rep *host_rep,
                            uint64_t capacity, csv_merge_counts *counts)
{
    if (!ctx) return CSV_EINVAL;
    if (ctx->split_state) { ctx->err = "merge select: a split order is pending on this context"; return CSV_EINVAL; }
    if (!shard || !result || !counts || (capacity && !host_rep)) { ctx->err = "merge select: null argument"; return CSV_EINVAL; }
    if (result->n_del + result->n_ins != result->n_sig || (result->n_sig && (!result->sig_del || !result->sig_ins || !result->label_del || !result->label_ins))) {
        ctx->err = "merge select: not a pipeline's result";
        return CSV_EINVAL;
    }
    if (result->n_sig) {                                      // the results lie in the shard's scratch: a result of another shard, or of before the scratch grew, does not
        const char *lo = shard->scratch, *hi = shard->scratch + shard->scratch_cap;
        const char *p[4] = {(const char *)result->sig_del, (const char *)(result->sig_ins + result->n_ins), (const char *)result->label_del,
                            (const char *)(result->label_ins + result->n_ins)};
        if (!lo || p[0] < lo || p[1] > hi || p[2] < lo || p[3] > hi || result->sig_ins != result->sig_del + result->n_del ||
            result->label_ins != result->label_del + result->n_del) {
            ctx->err = "merge select: the result is not this shard's last pipeline's";
            return CSV_EINVAL;
        }
    }
    if (result->n_del >= (1ull << 31) || result->n_ins >= (1ull << 31)) { ctx->err = "merge select: 2^31 or more signatures of a type"; return CSV_EINVAL; }
    memset(counts, 0, sizeof(*counts));
    if (result->n_sig == 0) return CSV_OK;
    (void)hipSetDevice(ctx->device);
    const int64_t max_label[2] = {(int64_t)result->n_del, (int64_t)result->n_ins};          // DBSCAN's cluster ids lie below the set's size
    return merge_select_dev(ctx, shard, result->sig_del, result->label_del, result->n_del, result->sig_ins, result->label_ins, result->n_ins, max_label,
                            max_partitions, host_rep, capacity, counts);
}
