// glue.hpp — what more than one file of the C-ABI glue (api/*.hip) needs: the reservations of the arenas and of the page-locked block,
// the short waits, and the chains one concern's entry points borrow from another's. Not part of the ABI.
#pragma once
#include <string.h>

#include <algorithm>
#include <chrono>
#include <utility>
#include <vector>

#include "../layouts.hpp"

namespace csv {

// false in libcsvgpu.so (nohooks.hip); in libcsvgpu_testhooks.so the counting one of testhooks.hip, armed by csvgpu_test_fail_next_alloc
bool test_fail_alloc();

// Reserve `a` for a layout and carve it: carve(Arena &) -> bool runs on a planning arena (its `used` is the need), then on `a`. The carve
// writes its pointers into a workspace struct of the caller's; the planning pass's values are overwritten by the real pass.
template <class Carve>
static int arena_reserve_for(csv_ctx *ctx, Arena &a, const char *what, Carve &&carve)
{
    const int rc = arena_reserve(ctx, a, arena_plan_bytes(carve));
    if (rc) return rc;
    if (!carve(a)) { ctx->err = std::string("arena exhausted (") + what + ")"; return CSV_ENOMEM; }
    return CSV_OK;
}

// Host arrays of the host-pointer entry points travel through the context's page-locked block: the runtime stages a pageable
// hipMemcpyAsync itself, in chunks and under a lock that the other contexts' launches also take (seen as millisecond gaps in the lanes'
// big kernels whenever the caller's context copied its observation vectors). in(): bytes copied into the block, the block's address
// returned for the async copy; out(): a slot of the block the device writes to, copied to the caller's array by finish() after the wait;
// slot(): bytes of the block for the caller's own use. Built without a context it plans: the three only advance `used`.
// The block is sized like the arenas, by running the stage: pin_reserve_for plans `stage(PinStage &)`, grows the block once, then runs the
// stage on the real one. Nothing may grow the block while a PinStage over it is live.
struct PinStage {
    csv_ctx *ctx;
    size_t used = 0;
    struct Out { void *dst; const void *src; size_t bytes; };
    std::vector<Out> outs;
    explicit PinStage(csv_ctx *c = nullptr, size_t from = 0) : ctx(c), used(from) {}
    void *slot(size_t bytes) { void *p = ctx ? (char *)ctx->pinned + used : nullptr; used += align_up(bytes, 256); return p; }
    const void *in(const void *src, size_t bytes) { void *p = slot(bytes); if (ctx && bytes) memcpy(p, src, bytes); return p; }
    void *out(void *dst, size_t bytes) { void *p = slot(bytes); if (ctx) outs.push_back(Out{dst, p, bytes}); return p; }
    void finish() { for (const Out &o : outs) if (o.bytes) memcpy(o.dst, o.src, o.bytes); outs.clear(); }
};
template <class Stage>
static int pin_reserve_for(csv_ctx *ctx, PinStage &pin, Stage &&stage)
{
    PinStage plan(nullptr, pin.used);
    stage(plan);
    const int rc = ensure_pinned(ctx, plan.used);
    if (rc) return rc;
    stage(pin);
    return CSV_OK;
}
// the scalars that read_counters, check_reads_dev and dbscan_iv_chain read back through the block's first bytes: a stage whose call runs
// one of them while it is live starts with this slot, so that their ensure_pinned(kPinScalars) cannot grow the block under it
static constexpr size_t kPinScalars = 4096;

hipEvent_t get_event(csv_ctx *ctx);                      // context.hip: from the context's pool

// The waits of the per-chromosome pipeline last a fraction of a millisecond: polling for up to 100 us before blocking
// saves the tens of microseconds a blocked thread takes to be woken, during which the device has nothing queued.
constexpr std::chrono::microseconds kSpinLimit(100);
static hipError_t wait_stream(hipStream_t s)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(s);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > kSpinLimit) return hipStreamSynchronize(s);
    }
}
static hipError_t wait_event(hipEvent_t ev)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > kSpinLimit) return hipEventSynchronize(ev);
    }
}

static inline bool onesweep(const csv_ctx *ctx) { return !ctx->tuning.sort_three_launch; }

// seg_off[0 .. n_seg] must not decrease (`what`: the refusal's text, worded by the entry point); max_len: the longest segment
static inline int check_seg_off(csv_ctx *ctx, const char *what, const uint64_t *seg_off, uint64_t n_seg, uint64_t &max_len)
{
    max_len = 0;
    for (uint64_t s = 0; s < n_seg; s++) {
        if (seg_off[s + 1] < seg_off[s]) { ctx->err = what; return CSV_EINVAL; }
        max_len = std::max(max_len, seg_off[s + 1] - seg_off[s]);
    }
    return CSV_OK;
}

// the stable permutation that sorts n 32-bit keys, queued on the context's stream: iota values, one radix sort, whichever buffer it ends in
static inline const uint32_t *sorted_perm(csv_ctx *ctx, const uint32_t *keys, uint64_t n, const SortWs &w)
{
    launch_iota_keys_u32(ctx->stream, keys, n, w.k0, w.v0);
    return launch_radix_sort_u64(ctx->stream, w.k0, w.v0, w.k1, w.v1, n, 32, w.tmp, onesweep(ctx)) ? w.v1 : w.v0;
}
static inline const uint32_t *sorted_perm(csv_ctx *ctx, const int32_t *keys, uint64_t n, const SortWs &w)
{
    launch_iota_keys_i32(ctx->stream, keys, n, w.k0, w.v0);
    return launch_radix_sort_u64(ctx->stream, w.k0, w.v0, w.k1, w.v1, n, 32, w.tmp, onesweep(ctx)) ? w.v1 : w.v0;
}

// ---- defined in one file, used by others ----
// bgzf.hip: pieced copies between pageable host memory and the device through the two halves of the page-locked block
constexpr size_t kPiece = (size_t)4 << 20;               // bytes per copy: the page-locked block holds two pieces (ensure_pinned(2 * kPiece)), one in flight, one being filled / emptied
typedef std::vector<std::pair<uint64_t, uint64_t>> Runs;
int copy_up(csv_ctx *ctx, void *d_dst, const void *h_src, size_t bytes, hipEvent_t ev[2], size_t &piece_no);
int copy_down(csv_ctx *ctx, void *h_dst, const void *d_src, size_t bytes, hipEvent_t ev[2], const Runs &runs);
struct Events {                                           // two events of the context's pool, returned to it
    csv_ctx *ctx;
    hipEvent_t ev[2];
    bool done = false;                                    // set by the entry point on its way out with everything waited for
    explicit Events(csv_ctx *c) : ctx(c) { ev[0] = get_event(c); ev[1] = get_event(c); }
    // An early return (a HIP error part-way through the pieces) may leave copies queued that read or write the page-locked halves and events
    // recorded but not waited for: the stream is drained before the events go back to the pool and the block to its next user.
    ~Events()
    {
        if (!done) (void)hipStreamSynchronize(ctx->stream);
        for (hipEvent_t e : ev) if (e) ctx->event_pool.push_back(e);
    }
    bool ok() const { return ev[0] && ev[1]; }
};
// reads.hip
int check_reads(csv_ctx *ctx, const csv_reads *r);           // host arrays
int check_reads_dev(csv_ctx *ctx, const csv_reads *r);       // arrays in HBM: one small kernel
int scan_form(const csv_ctx *ctx, uint64_t n_reads, uint64_t n_cigar);
int read_counters(csv_ctx *ctx, const ScanCounters *d_cnt, ScanCounters &h);
ScanExtras scan_extras(ScanCounters *cnt, uint32_t depth_len, bool with_type, uint64_t *tile_range);
void order_signatures(csv_ctx *ctx, const csv_sig *sig_raw, uint64_t n, uint32_t depth_len, uint32_t overflow, uint32_t max_bucket,
                      ScanCounters *cnt, bool with_type, SortWs &w, csv_sig *sig_sorted, uint32_t *start_out, uint32_t *end_out);
int depth_chain(csv_ctx *ctx, const DepthWs &ws, const csv_reads &d, const int32_t *ref_end, const uint32_t *ckpt, bool unsorted, uint32_t depth_len,
                uint32_t *depth, ScanCounters *cnt, const uint64_t *ranges = nullptr, uint32_t cigar_pad = 0, void *items = nullptr,
                int form = SCAN_FORM_WAVE);
// shard.hip
void shard_release(csv_shard *sh);                            // frees what the shard owns, and the shard
csv_shard *shard_common(csv_ctx *ctx, csv_shard *sh);         // the side arrays and the scan's split of a shard whose reads are in place; releases it on failure
// cluster.hip
int check_dbscan_args(csv_ctx *ctx, double eps, int32_t min_pts, bool interval);
// split_order.hip
void split_order_epochs(uint64_t n_max, std::vector<uint64_t> &first_node, std::vector<uint64_t> &buckets);
void split_state_free(csv_ctx *ctx);

}  // namespace csv
