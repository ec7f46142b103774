// job.hip — one chromosome as a job in three steps, so that the caller can queue the scan + depth pass of the next chromosome before it
// waits for this one's results (the device then never idles across the host's turn-around); the one-call pipeline on top.
#include <new>
#include <optional>

#include "glue.hpp"

using namespace csv;

struct csv_job {
    csv_shard *sh = nullptr;
    uint32_t min_oplen = 50; uint8_t min_mapq = 20; double min_pts_pct = 0.1;
    hipEvent_t ev_zero = nullptr, ev_scan = nullptr, ev_depth = nullptr, ev_mid = nullptr, ev_done = nullptr, t0 = nullptr;
    bool on_gate = false;                // the pair runs on a gate's stream: this context's stream meets it only in job_cluster (ev_depth)
    char *pin = nullptr;                 // 1 KiB page-locked: [0,256) counters behind the scan, [256,512) counters at the end, [512,576) the select's MergeBack
    bool depth_queued = false, clustered = false, copied = false;
    uint64_t n = 0, n_del = 0, capacity = 0;
    csv_sig *sig_sorted = nullptr;
    int32_t *labels = nullptr;
    // csvgpu_chr_job_cluster_select: the select queued behind the DBSCAN
    bool select = false;
    csv_merge_counts *host_counts = nullptr;
    uint64_t rep_capacity = 0, rep_bound = 0;
};

// CSV_MAX_JOBS rotating 512-byte page-locked slots per context; a slot belongs to its job from begin to end / abort, so a caller
// that holds more than CSV_MAX_JOBS jobs open on one context is refused instead of aliasing another job's counters.
constexpr size_t kJobPinSlot = 1024;
static char *job_pin_slot(csv_ctx *ctx)
{
    constexpr size_t kSlots = CSV_MAX_JOBS, kSlot = kJobPinSlot;
    if (!ctx->job_pin && hipHostMalloc((void **)&ctx->job_pin, kSlots * kSlot, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    for (size_t k = 0; k < kSlots; k++) {
        const size_t i = (ctx->job_pin_next + k) % kSlots;
        if (ctx->job_pin_busy & (1u << i)) continue;
        ctx->job_pin_busy |= 1u << i;
        ctx->job_pin_next = i + 1;
        return ctx->job_pin + i * kSlot;
    }
    return nullptr;
}
static void job_pin_release(csv_ctx *ctx, char *p)
{
    if (!p || !ctx->job_pin) return;
    ctx->job_pin_busy &= ~(1u << (size_t)((p - ctx->job_pin) / kJobPinSlot));
}

// ctx->work for a shard's depth chain: reserved when the job begins (ws == nullptr), carved again — the same carve, the same arguments —
// by whichever later step queues the chain
static int depth_work(csv_ctx *ctx, const csv_shard *sh, DepthWs *ws)
{
    DepthWs w;
    if (!ws) return arena_reserve_for(ctx, ctx->work, "depth", [&](Arena &a) { return carve_depth(a, sh->d.n_reads, sh->depth_len, w); });
    ctx->work.used = 0;
    if (!carve_depth(ctx->work, sh->d.n_reads, sh->depth_len, *ws)) { ctx->err = "arena exhausted (depth)"; return CSV_ENOMEM; }
    return CSV_OK;
}

// scan (+ counters on their way to the host + depth pass, when the shard's sortedness is known). For a coordinate-sorted shard the
// device sees scan -> depth tiles back to back: the scan leaves the bucket counts and the tiles' candidate ranges behind, the
// counters travel beside the depth pass, and everything small (offsets, scatter, ranking, clustering) is queued behind it.
// With a gate, the scan + depth pairs of all attached contexts go onto the gate's one stream — back to back in queue order, no
// hand-over between queues — while each context's own (higher-priority) stream runs its small kernels beside the other lane's pair.
static int job_queue_front(csv_ctx *ctx, csv_job *job)
{
    csv_shard *sh = job->sh;
    hipStream_t s = ctx->stream;
    const ReadsView view = shard_view(sh);
    ScanCounters *cnt = view.cnt;
    int rc;
    const bool sorted = sh->unsorted == 0;
    if (!job->ev_scan) job->ev_scan = get_event(ctx);          // (handed to the timers by an earlier pass of this job)
    if (!job->ev_depth) job->ev_depth = get_event(ctx);
    if (!job->ev_scan || !job->ev_depth) { ctx->err = "job: cannot allocate events"; return CSV_ENOMEM; }
    CSV_HIP(ctx, hipMemsetAsync(cnt, 0, sorted ? sh->counters_bytes : kCntBytes, s));
    csv_gate *gate = sorted ? ctx->gate : nullptr;
    hipStream_t big = s;
    std::unique_lock<std::mutex> turn;
    if (gate) {
        turn = std::unique_lock<std::mutex>(gate->mu);
        // (stream priorities — this stream low, the contexts' own high — measured 2 % slower: a small kernel waits for a whole
        // workgroup slot of the resident big kernel either way)
        if (!gate->stream) {
            if (hipStreamCreateWithFlags(&gate->stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); gate->stream = nullptr; }
            gate->device = ctx->device;
        }
        if (gate->stream && gate->device == ctx->device) {
            big = gate->stream;
            CSV_HIP(ctx, hipEventRecord(job->ev_zero, s));                 // the pair starts behind this context's memset (and whatever it was queued behind)
            CSV_HIP(ctx, hipStreamWaitEvent(big, job->ev_zero, 0));
        }
    }
    // On the gate's stream every recorded event is a barrier packet between the big kernels of ALL lanes (~5 us each): the pair is
    // timed with the two events the job records there anyway plus one in front (scan = ev_scan - t0, depth = ev_depth - ev_scan).
    // (at level 2 only every fourth pair: the extra event in front of the scan is a barrier packet on the stream all lanes share, 2.5 % of
    // the throughput when every pair has one; the averages are over the timed pairs)
    if (job->t0) { ctx->event_pool.push_back(job->t0); job->t0 = nullptr; }          // (a re-run after the signature buffer grew)
    const bool pair_timers = big != s && ctx->timing != 0 && (ctx->timing == 1 || ctx->timing == 3 || (ctx->timer_tick++ & 3u) == 0);
    hipEvent_t t0 = nullptr;
    if (pair_timers) {
        t0 = get_event(ctx);
        if (t0) CSV_HIP(ctx, hipEventRecord(t0, big));
    }
    {
        // on the gate's stream the scan has no events of its own (a timed pair has t0 in front and the job's two behind); the gate takes
        // coordinate-sorted shards only, so the tile ranges are asked for there as well
        std::optional<TimerScope> ts;
        if (big == s) ts.emplace(ctx, CSV_K_CIGAR_SCAN, big);
        launch_cigar_scan(big, ctx->n_cu, view, ScanArgs{sh->depth_len, job->min_oplen, job->min_mapq, 1, sh->sig_raw, sh->sig_cap,
                                                         scan_extras(cnt, sh->depth_len, true, sorted ? sh->tile_range : nullptr), sh->owned ? sh->scan_split : nullptr});
    }
    job->depth_queued = false;
    if (sh->unsorted >= 0) {
        // The depth pass does not depend on the signature count, so it is queued BEFORE the host waits for the counters: the
        // device works through it while the host wakes up, sizes the ordering and clustering launches and queues them.
        job->on_gate = big != s;
        if (job->on_gate) {
            // On a gate nothing of this job touches the context's own stream until job_cluster: a caller that queues several jobs ahead must
            // not find one job's clustering kernels behind a wait for a LATER job's scan. The counters leave from the gate's stream itself,
            // between the two big kernels (256 bytes to page-locked memory), ev_scan tells the host they have landed, and job_cluster makes
            // the context's stream wait for ev_depth before min_pts. (A relay through a side stream per context was tried: three more
            // streams whose only work is to wait share the four hardware queues with everything else and stalled the caller's context.)
            CSV_HIP(ctx, hipMemcpyAsync(job->pin, cnt, sizeof(ScanCounters), hipMemcpyDeviceToHost, big));
            CSV_HIP(ctx, hipEventRecord(job->ev_scan, big));
            launch_depth_tiles(big, view, DepthArgs{sh->depth_len, sh->depth, nullptr, sh->tile_range, sh->depth_items});
            CSV_HIP(ctx, hipEventRecord(job->ev_depth, big));
            turn.unlock();
            job->t0 = pair_timers ? t0 : nullptr;            // (handed to the timers with ev_scan / ev_depth when the job ends)
        } else {
            // The counters leave on a side stream beside the depth pass.
            if (!ctx->side) CSV_HIP(ctx, hipStreamCreateWithFlags(&ctx->side, hipStreamNonBlocking));
            hipStream_t cs = ctx->side;
            CSV_HIP(ctx, hipEventRecord(job->ev_scan, big));
            CSV_HIP(ctx, hipStreamWaitEvent(cs, job->ev_scan, 0));
            CSV_HIP(ctx, hipMemcpyAsync(job->pin, cnt, sizeof(ScanCounters), hipMemcpyDeviceToHost, cs));
            CSV_HIP(ctx, hipEventRecord(job->ev_mid, cs));
            DepthWs dw;
            if ((rc = depth_work(ctx, sh, &dw))) return rc;
            if ((rc = depth_chain(ctx, dw, view, sh->unsorted != 0, DepthArgs{sh->depth_len, sh->depth, nullptr, sorted ? sh->tile_range : nullptr, sh->depth_items}))) return rc;
            launch_min_pts(s, cnt, job->min_pts_pct);
        }
        job->depth_queued = true;
    }
    return CSV_OK;
}

static void job_free(csv_ctx *ctx, csv_job *job)
{
    if (!job) return;
    job_pin_release(ctx, job->pin);
    if (job->t0 && job->ev_scan && job->ev_depth && job->on_gate && ctx->gate && ctx->gate->stream) {
        // a timed pair on the gate's stream: scan = ev_scan - t0 (the 256-byte counters copy included), depth = ev_depth - ev_scan; the
        // timers own the three events from here (folded when the times are read)
        Timer a; a.id = CSV_K_CIGAR_SCAN; a.a = job->t0; a.b = job->ev_scan; a.s = ctx->gate->stream;
        Timer b; b.id = CSV_K_DEPTH; b.a = job->ev_scan; b.b = job->ev_depth; b.s = ctx->gate->stream; b.own_a = false;
        ctx->timers.push_back(a); ctx->timers.push_back(b);
        job->t0 = nullptr; job->ev_scan = nullptr; job->ev_depth = nullptr;
    }
    if (job->t0) ctx->event_pool.push_back(job->t0);
    if (job->ev_zero) ctx->event_pool.push_back(job->ev_zero);
    if (job->ev_scan) ctx->event_pool.push_back(job->ev_scan);
    if (job->ev_depth) ctx->event_pool.push_back(job->ev_depth);
    if (job->ev_mid) ctx->event_pool.push_back(job->ev_mid);
    if (job->ev_done) ctx->event_pool.push_back(job->ev_done);
    delete job;
}

csv_job *csvgpu_chr_job_begin(csv_ctx *ctx, csv_shard *sh, uint32_t min_oplen, uint8_t min_mapq, double min_pts_pct)
{
    if (!ctx || !sh) return nullptr;
    (void)hipSetDevice(ctx->device);
    csv_job *job = new (std::nothrow) csv_job();
    if (!job) { ctx->err = "out of host memory"; return nullptr; }
    job->sh = sh; job->min_oplen = min_oplen; job->min_mapq = min_mapq; job->min_pts_pct = min_pts_pct;
    job->ev_zero = get_event(ctx); job->ev_scan = get_event(ctx); job->ev_depth = get_event(ctx); job->ev_mid = get_event(ctx); job->ev_done = get_event(ctx);
    job->pin = job_pin_slot(ctx);
    if (!job->pin && ctx->job_pin) { ctx->err = "job: more than CSV_MAX_JOBS jobs open on this context"; job_free(ctx, job); return nullptr; }
    if (!job->pin || !job->ev_zero || !job->ev_scan || !job->ev_depth || !job->ev_mid || !job->ev_done) { ctx->err = "job: cannot allocate events / page-locked memory"; job_free(ctx, job); return nullptr; }
    if (depth_work(ctx, sh, nullptr) || job_queue_front(ctx, job)) { job_free(ctx, job); return nullptr; }
    return job;
}

// what csvgpu_chr_job_cluster_select asks for on top of the clustering (nullptr: nothing — the job's carve and launches are what they were)
struct JobSelect { uint32_t max_partitions; csv_merge_rep *host_rep; uint64_t capacity; csv_merge_counts *host_counts; };

static int job_cluster(csv_ctx *ctx, csv_job *job, double eps, csv_sig *host_sig, int32_t *host_labels, uint64_t capacity, const JobSelect *sel)
{
    if (!ctx || !job || job->clustered) return CSV_EINVAL;
    if (!(eps >= 0.0) || !(eps < 1.0)) { ctx->err = "pipeline: eps must be in [0,1)"; return CSV_EINVAL; }
    if (capacity && (!host_sig || !host_labels)) { ctx->err = "pipeline: null output"; return CSV_EINVAL; }
    (void)hipSetDevice(ctx->device);
    csv_shard *sh = job->sh;
    hipStream_t s = ctx->stream;
    ScanCounters *cnt = (ScanCounters *)sh->counters;
    ScanCounters h;
    int rc;
    for (int attempt = 0;; attempt++) {
        if (job->depth_queued) {
            CSV_HIP(ctx, wait_event(job->on_gate ? job->ev_scan : job->ev_mid));
            memcpy(&h, job->pin, sizeof(ScanCounters));
        } else {
            if ((rc = read_counters(ctx, cnt, h))) return rc;             // first scan of wrapped arrays: wait, then decide
            sh->unsorted = h.unsorted != 0;
        }
        if (h.n_sig <= sh->sig_cap) break;
        if (attempt) { ctx->err = "pipeline: signature buffer overflow twice"; return CSV_ENOMEM; }
        CSV_HIP(ctx, wait_stream(s));                            // the queued depth pass reads what the re-run scan rewrites
        // the larger buffer first: if it cannot be had, the shard keeps its old buffer AND its old capacity (a later job on this
        // shard must never see a capacity without a buffer behind it — the scan's `g < sig_cap` guard would write through null)
        const uint64_t new_cap = h.n_sig + h.n_sig / 8 + 1024;
        csv_sig *bigger = nullptr;
        if (test_fail_alloc() || hipMalloc((void **)&bigger, new_cap * sizeof(csv_sig)) != hipSuccess) {
            (void)hipGetLastError();
            ctx->err = "hipMalloc failed (signature buffer)";
            return CSV_ENOMEM;
        }
        (void)hipFree(sh->sig_raw);
        sh->sig_raw = bigger; sh->sig_cap = new_cap;
        if ((rc = job_queue_front(ctx, job))) return rc;
    }
    const uint64_t n = h.n_sig, n_del = h.n_del;
    const uint32_t max_bucket = h.max_len;

    // shard scratch: sorted signatures, SoA start/end, labels, sort + dbscan workspace (grow-only)
    JobScratch js;
    const size_t need = arena_plan_bytes([&](Arena &a) { return carve_job_scratch(a, n, js); });
    if (need > sh->scratch_cap) {
        if (sh->scratch) CSV_HIP(ctx, hipFree(sh->scratch));
        sh->scratch = nullptr; sh->scratch_cap = 0;
        CSV_HIP(ctx, hipMalloc((void **)&sh->scratch, need + need / 4));
        sh->scratch_cap = need + need / 4;
    }
    Arena sa; sa.base = sh->scratch; sa.cap = sh->scratch_cap; sa.used = 0;
    if (!carve_job_scratch(sa, n, js)) { ctx->err = "shard scratch exhausted"; return CSV_ENOMEM; }
    csv_sig *sig_sorted = js.sig_sorted;
    uint32_t *st = js.st, *en = js.en;
    int32_t *labels = js.labels;
    SortWs &w = js.w;
    void *db_tmp = js.db_tmp;

    // depth map + mean coverage + min_pts (device scalar), unless already queued behind the scan
    if (!job->depth_queued) {
        DepthWs dw;
        if ((rc = depth_work(ctx, sh, &dw))) return rc;
        if ((rc = depth_chain(ctx, dw, shard_view(sh), sh->unsorted != 0, DepthArgs{sh->depth_len, sh->depth, nullptr, nullptr, sh->depth_items}))) return rc;
        launch_min_pts(s, cnt, job->min_pts_pct);
    }

    // ordering: DEL calls then INS calls, each in chr_sv_calls order
    order_signatures(ctx, sh->sig_raw, n, sh->depth_len, h.max_start, max_bucket, cnt, true, w, sig_sorted, st, en);

    // min_pts (and with it the clustering) reads what the depth pass leaves; the ordering above did not have to wait for it
    if (job->depth_queued && job->on_gate) {
        CSV_HIP(ctx, hipStreamWaitEvent(s, job->ev_depth, 0));
        launch_min_pts(s, cnt, job->min_pts_pct);
    }
    // per-type interval DBSCAN (mergeSVs walks DEL ... INS, sv_object.cpp:62-68)
    {
        TimerScope ts(ctx, CSV_K_DBSCAN);
        // DEL calls [0, n_del) and INS calls [n_del, n) are clustered side by side in the same five launches
        if (n) launch_dbscan_iv_sorted(s, st, en, nullptr, n, n_del, eps, 0, &cnt->min_pts, labels, db_tmp);
    }
    job->copied = capacity && n && n <= capacity;
    if (job->copied) {                                                   // results ride behind the last kernel, one wait for everything
        CSV_HIP(ctx, hipMemcpyAsync(host_sig, sig_sorted, n * sizeof(csv_sig), hipMemcpyDeviceToHost, s));
        CSV_HIP(ctx, hipMemcpyAsync(host_labels, labels, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    }
    if (sel && n) {
        // the representatives behind the last clustering kernel: only the counts and the records ride home. How many records there are is
        // known on the device alone, so min(capacity, bound) of them are copied; csvgpu_chr_job_end says whether that was all of them.
        MergeRunWs mw;
        const int64_t max_label[2] = {(int64_t)n_del, (int64_t)(n - n_del)};          // DBSCAN's cluster ids lie below the set's size
        if ((rc = merge_select_queue(ctx, sh, sig_sorted, labels, n_del, sig_sorted + n_del, labels + n_del, n - n_del, max_label, sel->max_partitions, mw))) return rc;
        job->rep_bound = merge_rep_bound(n_del, n - n_del);
        const uint64_t n_copy = std::min(sel->capacity, job->rep_bound);
        CSV_HIP(ctx, hipMemcpyAsync(job->pin + 512, mw.back, sizeof(MergeBack), hipMemcpyDeviceToHost, s));
        if (n_copy) CSV_HIP(ctx, hipMemcpyAsync(sel->host_rep, mw.rep, n_copy * sizeof(csv_merge_rep), hipMemcpyDeviceToHost, s));
    }
    if (sel) { job->select = true; job->host_counts = sel->host_counts; job->rep_capacity = sel->capacity; }
    CSV_HIP(ctx, hipMemcpyAsync(job->pin + 256, cnt, sizeof(ScanCounters), hipMemcpyDeviceToHost, s));
    CSV_HIP(ctx, hipEventRecord(job->ev_done, s));
    job->n = n; job->n_del = n_del; job->capacity = capacity; job->sig_sorted = sig_sorted; job->labels = labels;
    job->clustered = true;
    return CSV_OK;
}

int csvgpu_chr_job_cluster(csv_ctx *ctx, csv_job *job, double eps, csv_sig *host_sig, int32_t *host_labels, uint64_t capacity)
{
    return job_cluster(ctx, job, eps, host_sig, host_labels, capacity, nullptr);
}

int csvgpu_chr_job_cluster_select(csv_ctx *ctx, csv_job *job, double eps, uint32_t max_partitions, csv_merge_rep *host_rep, uint64_t capacity,
                                  csv_merge_counts *host_counts)
{
    if (!ctx || !job) return CSV_EINVAL;
    if (!host_counts || (capacity && !host_rep)) { ctx->err = "job select: null output"; return CSV_EINVAL; }
    if (ctx->split_state) { ctx->err = "job select: a split order is pending on this context"; return CSV_EINVAL; }
    const JobSelect sel{max_partitions, host_rep, capacity, host_counts};
    return job_cluster(ctx, job, eps, nullptr, nullptr, 0, &sel);
}

int csvgpu_chr_job_end(csv_ctx *ctx, csv_job *job, csv_chr_result *res)
{
    if (!ctx || !job) return CSV_EINVAL;
    (void)hipSetDevice(ctx->device);
    int rc = CSV_OK;
    if (!job->clustered) { ctx->err = "job_end before job_cluster"; rc = CSV_EINVAL; }
    else if (wait_event(job->ev_done) != hipSuccess) { (void)hipGetLastError(); ctx->err = "job: device error"; rc = CSV_EHIP; }
    else if (res) {
        ScanCounters h;
        memcpy(&h, job->pin + 256, sizeof(ScanCounters));
        csv_shard *sh = job->sh;
        res->n_sig = job->n; res->n_del = job->n_del; res->n_ins = job->n - job->n_del;
        res->depth_sum = h.depth_sum; res->depth_nonzero = h.depth_nonzero; res->min_pts = h.min_pts; res->mean_cov = h.mean_cov;
        res->sig_del = job->sig_sorted; res->sig_ins = job->sig_sorted + job->n_del;
        res->label_del = job->labels; res->label_ins = job->labels + job->n_del;
        res->depth = sh->depth; res->ref_end = sh->ref_end; res->q_start = sh->q_start; res->q_end = sh->q_end;
        if (job->capacity && job->n > job->capacity) { ctx->err = "pipeline_fetch: host buffers too small"; rc = CSV_ECAPACITY; }
    }
    if (rc == CSV_OK && job->clustered && job->select) {
        MergeBack mb;
        memset(&mb, 0, sizeof(mb));
        if (job->n) memcpy(&mb, job->pin + 512, sizeof(MergeBack));
        *job->host_counts = mb.counts;
        const uint64_t n_rep = mb.counts.n_rep[0] + mb.counts.n_rep[1];
        if (mb.gave_up[0] || mb.gave_up[1] || n_rep > job->rep_bound) { ctx->err = "job select: a radix pass's look-back gave up"; rc = CSV_EHIP; }
        else if (n_rep > job->rep_capacity) { ctx->err = "job select: host_rep too small"; rc = CSV_ECAPACITY; }
    }
    job_free(ctx, job);
    return rc;
}

int csvgpu_chr_job_abort(csv_ctx *ctx, csv_job *job)
{
    if (!ctx || !job) return CSV_EINVAL;
    (void)hipSetDevice(ctx->device);
    // whatever the job queued reads the shard's buffers: let it drain before the caller reuses or frees them
    (void)hipStreamSynchronize(ctx->stream);
    if (ctx->gate && ctx->gate->stream) (void)hipStreamSynchronize(ctx->gate->stream);
    if (ctx->side) (void)hipStreamSynchronize(ctx->side);
    job_free(ctx, job);                                  // ctx->err keeps the failure that led here
    return CSV_OK;
}

static int chr_pipeline(csv_ctx *ctx, csv_shard *sh, uint32_t min_oplen, uint8_t min_mapq, double eps, double min_pts_pct, csv_chr_result *res,
                        csv_sig *host_sig, int32_t *host_labels, uint64_t capacity)
{
    if (!ctx || !sh || !res) return CSV_EINVAL;
    if (!(eps >= 0.0) || !(eps < 1.0)) { ctx->err = "pipeline: eps must be in [0,1)"; return CSV_EINVAL; }
    csv_job *job = csvgpu_chr_job_begin(ctx, sh, min_oplen, min_mapq, min_pts_pct);
    if (!job) return ctx->err.find("hipMalloc") != std::string::npos ? CSV_ENOMEM : CSV_EHIP;
    const int rc = csvgpu_chr_job_cluster(ctx, job, eps, host_sig, host_labels, capacity);
    if (rc) { csvgpu_chr_job_abort(ctx, job); return rc; }
    return csvgpu_chr_job_end(ctx, job, res);
}

int csvgpu_chr_pipeline_dev(csv_ctx *ctx, csv_shard *sh, uint32_t min_oplen, uint8_t min_mapq, double eps, double min_pts_pct,
                            csv_chr_result *res)
{
    return chr_pipeline(ctx, sh, min_oplen, min_mapq, eps, min_pts_pct, res, nullptr, nullptr, 0);
}

int csvgpu_chr_pipeline_fetch(csv_ctx *ctx, csv_shard *sh, uint32_t min_oplen, uint8_t min_mapq, double eps, double min_pts_pct,
                              csv_chr_result *res, csv_sig *host_sig, int32_t *host_labels, uint64_t capacity)
{
    if (capacity && (!host_sig || !host_labels)) { if (ctx) ctx->err = "pipeline_fetch: null output"; return CSV_EINVAL; }
    return chr_pipeline(ctx, sh, min_oplen, min_mapq, eps, min_pts_pct, res, host_sig, host_labels, capacity);
}
