// glue.hpp — what more than one file of the C-ABI glue (api/*.hip) needs: the reservations of the arenas and of the page-locked block,
// the short waits, the transfer session of the pieced copies (Transfer), the device array that grows (DevBuf), and the chains one concern's
// entry points borrow from another's. Not part of the ABI.
#pragma once
#include <string.h>

#include <algorithm>
#include <chrono>
#include <functional>
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
// transfer.hip: one entry point's copies between pageable host memory and the device through the page-locked block, in pieces
constexpr size_t kPiece = (size_t)4 << 20;               // bytes per copy: the page-locked block holds two pieces, one in flight, one being filled / emptied
typedef std::vector<std::pair<uint64_t, uint64_t>> Runs;
// Holds two events of the context's pool from open() until it goes out of scope. It knows whether a copy it queued may still be in flight
// (up() and a failed member leave one; a wait that succeeded leaves none) and drains the stream on its way out then, and only then: the
// events and the block's halves never change hands under a copy. The entry point's kernels go between the calls, on ctx->stream.
struct Transfer {
    explicit Transfer(csv_ctx *c) : ctx(c) {}
    Transfer(const Transfer &) = delete;
    Transfer &operator=(const Transfer &) = delete;
    ~Transfer();
    int open(const char *who);                            // ensure_pinned(2 * kPiece), the events; "<who>: no event" without them
    // host -> device, queued: the last pieces may still be in flight on return (the stream orders them in front of the kernel). The
    // pieces are counted across calls, so consecutive arrays alternate the halves like one long one.
    int up(void *d_dst, const void *h_src, size_t bytes);
    // device -> host, complete on return; piece k + 1 travels while piece k is copied out of the block. Only the bytes inside `runs`
    // (ascending, disjoint [first, second) offsets into the range) reach the caller's memory: the rest is not the library's to write.
    int down(void *h_dst, const void *d_src, size_t bytes, const Runs &runs);
    int down(void *h_dst, const void *d_src, size_t bytes);   // the whole range; nothing to do for no bytes or a null h_dst
    // `bytes` (at most kPinScalars) through the block's first bytes, behind whatever is queued on the stream; waits
    int peek(void *dst, const void *d_src, size_t bytes);
    int wait();                                           // wait_stream(ctx->stream)
private:
    csv_ctx *ctx;
    hipEvent_t ev[2] = {nullptr, nullptr};
    size_t n_up = 0;                                      // pieces sent up so far: the next one's half, and from the third on a wait for that half's last copy
    bool pending = false;                                 // a copy of this session may be in flight
};
// context.hip: one device array that grows. `need` bytes in `b`, of which the first `used` are kept: a new block of at least 1.5x the old one
// through the guarded allocation, a copy on the device, the old block freed. CSV_ENOMEM leaves `b` as it was. `what`: whose, for the texts.
struct DevBuf {
    char *p = nullptr;
    uint64_t cap = 0;                                     // bytes allocated; the owner's counts say how many are in use
};
int devbuf_ensure(csv_ctx *ctx, DevBuf &b, uint64_t used, uint64_t need, const char *what);
// vcf.hip: the line ends of a text counted (kernels/vcfparse.hip) and the per-line workspace sized by them. carve(a, 0) lays out what the
// count needs, carve(a, n_slots) the per-line arrays behind it; first_pass queues the count (and whatever must be in place again once the
// arena has grown: it runs a second time then). w: the count's slices, as the carve set them. n_slots: the lines, a last open one included.
int count_lines(csv_ctx *ctx, Transfer &t, const char *what, const char *too_many, const uint8_t *d_text, uint32_t len, const VcfWs &w,
                const std::function<bool(Arena &, uint64_t)> &carve, const std::function<int()> &first_pass, uint32_t &n_slots);
// The SNP form of the parse with its outputs staged in the context's workspace (w.out: a record per kept line, in file order; every
// deferred line's offset), whatever their counts: for csvgpu_snp_builder_append, which reads them on the device. CSV_OK (the last kernel
// queued, not waited for; cnt filled) / 1 (declined) / CSV_E*.
int vcf_snp_stage(csv_ctx *ctx, Transfer &t, const uint8_t *d_text, uint32_t len, int dp_int, int ad_int, csv_vcf_counts &cnt, VcfWs &w);
// csvgpu_vcf_af_parse (dev_text: _dev) with sorted_pos on the device in both forms: a contig's resident column (csvgpu_snp_columns_af_parse).
// PRECONDITION: d_sorted_pos ascending. Nothing here checks it (the host form's loop over sorted_pos is skipped): the caller must hold the
// `ascending` flag that csvgpu_snp_builder_finish computed on the device, as af_parse of snp_build.hip does.
int vcf_af_parse_sorted_dev(csv_ctx *ctx, bool dev_text, const uint8_t *text, uint64_t len, const char *contig, uint32_t contig_len, const char *needle,
                            uint32_t needle_len, const uint32_t *d_sorted_pos, uint64_t n, const csv_vcf_out *out, csv_vcf_counts *counts);
// reads.hip
int check_reads(csv_ctx *ctx, const csv_reads *r);           // host arrays
int check_reads_dev(csv_ctx *ctx, const csv_reads *r);       // arrays in HBM: one small kernel
int scan_form(const csv_ctx *ctx, uint64_t n_reads, uint64_t n_cigar);
int read_counters(csv_ctx *ctx, const ScanCounters *d_cnt, ScanCounters &h);
ScanExtras scan_extras(ScanCounters *cnt, uint32_t depth_len, bool with_type, uint64_t *tile_range);
void order_signatures(csv_ctx *ctx, const csv_sig *sig_raw, uint64_t n, uint32_t depth_len, uint32_t overflow, uint32_t max_bucket,
                      ScanCounters *cnt, bool with_type, SortWs &w, csv_sig *sig_sorted, uint32_t *start_out, uint32_t *end_out);
int depth_chain(csv_ctx *ctx, const DepthWs &ws, const ReadsView &v, bool unsorted, DepthArgs a);      // (a.ord is the chain's to set)
// a resident shard as the two big kernels read it: the one place that holds the shard's form, pad and 16-bit arrays together
static inline ReadsView shard_view(const csv_shard *sh)
{
    return ReadsView{sh->d, CigarPack{sh->cig_half, sh->esc_piece, sh->esc_tab}, sh->cigar_pad, sh->form, sh->ref_end, sh->q_start, sh->q_end, sh->ckpt,
                     (ScanCounters *)sh->counters};
}
// shard.hip
void shard_release(csv_shard *sh);                            // frees what the shard owns, and the shard
csv_shard *shard_common(csv_ctx *ctx, csv_shard *sh);         // the side arrays and the scan's split of a shard whose reads are in place; releases it on failure
// snp_table.hip
// the first-hit kind from a contig's columns on the device and the population arrays of the host (csvgpu_snp_columns_table)
csv_snp_table *snp_table_hits_mixed(csv_ctx *ctx, const char *what, const uint32_t *d_pos, const double *d_baf, const uint32_t *af_pos, const double *af, uint64_t n,
                                    uint64_t n_af);
SnpTabDev snp_table_dev(const csv_snp_table *t);              // the table as the kernels see it (NULL or no records: all zero)
// cluster.hip
int check_dbscan_args(csv_ctx *ctx, double eps, int32_t min_pts, bool interval);
// merge_select.hip: both types' representatives of one contig queued on the context's stream, DEL records first — the kernels, and the
// gave-up words on their way into w.back; nothing is waited for. sh: the shard whose select scratch is carved (it grows here if it must:
// then, and only then, the device is waited for), or nullptr: the context's workspace. max_label[t]: a bound of type t's labels.
int merge_select_queue(csv_ctx *ctx, csv_shard *sh, const csv_sig *d_sig_del, const int32_t *d_lab_del, uint64_t n_del, const csv_sig *d_sig_ins,
                       const int32_t *d_lab_ins, uint64_t n_ins, const int64_t *max_label, uint32_t max_partitions, MergeRunWs &w);
// split_order.hip
void split_order_epochs(uint64_t n_max, std::vector<uint64_t> &first_node, std::vector<uint64_t> &buckets);
void split_state_free(csv_ctx *ctx);

}  // namespace csv
