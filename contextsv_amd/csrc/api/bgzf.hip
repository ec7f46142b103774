// bgzf.hip — BGZF members inflated on the device (kernels/inflate.hip): the checks of the member table, the copies through the page-locked
// block, and the count of declined members.
#include "glue.hpp"

#include <utility>
#include <vector>

using namespace csv;

namespace {

constexpr uint32_t kMaxMember = 65536;

int check_blocks(csv_ctx *ctx, const csv_bgzf_block *blocks, uint32_t n_blocks, uint64_t comp_len, uint64_t out_len)
{
    auto bad = [&](const char *msg) { ctx->err = std::string("bgzf_inflate: ") + msg; return (int)CSV_EINVAL; };
    uint64_t out_end = 0;                                // end of the output ranges so far
    for (uint32_t i = 0; i < n_blocks; i++) {
        const csv_bgzf_block &b = blocks[i];
        if (b.in_len > kMaxMember || b.out_len > kMaxMember) return bad("a member larger than 64 KiB");
        if (b.in_off > comp_len || comp_len - b.in_off < b.in_len) return bad("a member's input leaves the compressed buffer");
        if (b.out_off > out_len || out_len - b.out_off < b.out_len) return bad("a member's output leaves the output buffer");
        if (b.out_off < out_end) return bad("output ranges overlap or are out of order");
        out_end = b.out_off + b.out_len;
    }
    return CSV_OK;
}

}  // namespace

namespace csv {

// `bytes` between pageable host memory and the device through the two halves of the page-locked block (2 * kPiece, reserved by the caller).
// up: host -> device, queued; the last pieces may still be in flight on return (the stream orders them in front of the kernel).
int copy_up(csv_ctx *ctx, void *d_dst, const void *h_src, size_t bytes, hipEvent_t ev[2], size_t &piece_no)
{
    for (size_t off = 0; off < bytes; off += kPiece, piece_no++) {
        const size_t n = std::min(kPiece, bytes - off), slot = piece_no & 1;
        char *pin = (char *)ctx->pinned + slot * kPiece;
        if (piece_no >= 2) CSV_HIP(ctx, wait_event(ev[slot]));           // the copy that last read this half is done
        memcpy(pin, (const char *)h_src + off, n);
        CSV_HIP(ctx, hipMemcpyAsync((char *)d_dst + off, pin, n, hipMemcpyHostToDevice, ctx->stream));
        CSV_HIP(ctx, hipEventRecord(ev[slot], ctx->stream));
    }
    return CSV_OK;
}
// down: device -> host; piece k + 1 travels while piece k is copied out of the block. Only the bytes inside `runs` (ascending, disjoint
// [first, second) offsets into the range) reach the caller's memory: the bytes between two members are not the library's to write.
// Complete on return.
int copy_down(csv_ctx *ctx, void *h_dst, const void *d_src, size_t bytes, hipEvent_t ev[2], const Runs &runs)
{
    const size_t n_pieces = (bytes + kPiece - 1) / kPiece;
    size_t r = 0;
    for (size_t k = 0; k <= n_pieces; k++) {
        if (k < n_pieces) {
            const size_t off = k * kPiece, n = std::min(kPiece, bytes - off);
            CSV_HIP(ctx, hipMemcpyAsync((char *)ctx->pinned + (k & 1) * kPiece, (const char *)d_src + off, n, hipMemcpyDeviceToHost, ctx->stream));
            CSV_HIP(ctx, hipEventRecord(ev[k & 1], ctx->stream));
        }
        if (k > 0) {
            const size_t off = (k - 1) * kPiece, end = off + std::min(kPiece, bytes - off);
            const char *pin = (const char *)ctx->pinned + ((k - 1) & 1) * kPiece;
            CSV_HIP(ctx, wait_event(ev[(k - 1) & 1]));
            while (r < runs.size() && runs[r].second <= off) r++;
            for (size_t q = r; q < runs.size() && runs[q].first < end; q++) {
                const size_t a = std::max<size_t>(runs[q].first, off), b = std::min<size_t>(runs[q].second, end);
                if (b > a) memcpy((char *)h_dst + a, pin + (a - off), b - a);
            }
        }
    }
    return CSV_OK;
}

}  // namespace csv

namespace {

// table up, kernel, count back: what both entry points share. The page-locked block holds 2 * kPiece bytes; its first bytes take the count.
int run_members(csv_ctx *ctx, const BgzfWs &w, const uint8_t *d_comp, const csv_bgzf_block *blocks, uint32_t n_blocks, uint8_t *d_out, uint8_t *d_status,
                hipEvent_t ev[2], size_t &piece_no, unsigned int &n_declined)
{
    int rc = copy_up(ctx, w.blocks, blocks, (size_t)n_blocks * sizeof(csv_bgzf_block), ev, piece_no);
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    CSV_HIP(ctx, hipMemsetAsync(w.n_declined, 0, 4, s));
    {
        TimerScope ts(ctx, CSV_K_MISC);
        launch_bgzf_inflate(s, d_comp, w.blocks, n_blocks, d_out, d_status, w.n_declined);
    }
    CSV_HIP(ctx, hipGetLastError());
    CSV_HIP(ctx, hipMemcpyAsync(ctx->pinned, w.n_declined, 4, hipMemcpyDeviceToHost, s));      // (behind the upload's last pieces on the stream: the block's first bytes are free)
    CSV_HIP(ctx, wait_stream(s));
    n_declined = *(const unsigned int *)ctx->pinned;
    if (n_declined > n_blocks) { ctx->err = "bgzf_inflate: more members declined than there are"; return CSV_EHIP; }
    return CSV_OK;
}

}  // namespace

int csvgpu_bgzf_inflate_dev(csv_ctx *ctx, const uint8_t *d_comp, uint64_t comp_len, const csv_bgzf_block *blocks, uint32_t n_blocks,
                            uint8_t *d_out, uint64_t out_len, uint8_t *d_status)
{
    if (!ctx) return CSV_EINVAL;
    if (n_blocks == 0) return 0;
    if (!d_comp || !blocks || !d_out || !d_status) { ctx->err = "bgzf_inflate: null pointer"; return CSV_EINVAL; }
    int rc = check_blocks(ctx, blocks, n_blocks, comp_len, out_len);
    if (rc) return rc;
    (void)hipSetDevice(ctx->device);
    BgzfWs w;
    if ((rc = arena_reserve_for(ctx, ctx->work, "bgzf_inflate", [&](Arena &a) { return carve_bgzf(a, n_blocks, false, 0, 0, w); }))) return rc;
    if ((rc = ensure_pinned(ctx, 2 * kPiece))) return rc;
    Events e(ctx);
    if (!e.ok()) { ctx->err = "bgzf_inflate: no event"; return CSV_EHIP; }
    size_t piece_no = 0;
    unsigned int n_declined = 0;
    if ((rc = run_members(ctx, w, d_comp, blocks, n_blocks, d_out, d_status, e.ev, piece_no, n_declined))) return rc;
    e.done = true;                                        // run_members ends in a wait
    return (int)n_declined;
}

int csvgpu_bgzf_inflate(csv_ctx *ctx, const uint8_t *comp, uint64_t comp_len, const csv_bgzf_block *blocks, uint32_t n_blocks,
                        uint8_t *out, uint64_t out_len, uint8_t *status)
{
    if (!ctx) return CSV_EINVAL;
    if (n_blocks == 0) return 0;
    if (!comp || !blocks || !out || !status) { ctx->err = "bgzf_inflate: null pointer"; return CSV_EINVAL; }
    int rc = check_blocks(ctx, blocks, n_blocks, comp_len, out_len);
    if (rc) return rc;
    (void)hipSetDevice(ctx->device);
    // only the bytes the members span travel: [lo, hi) of comp up, [o_lo, o_hi) of out back
    uint64_t lo = comp_len, hi = 0;
    for (uint32_t i = 0; i < n_blocks; i++) { lo = std::min(lo, blocks[i].in_off); hi = std::max(hi, blocks[i].in_off + blocks[i].in_len); }
    if (hi < lo) hi = lo;
    const uint64_t o_lo = blocks[0].out_off, o_hi = blocks[n_blocks - 1].out_off + blocks[n_blocks - 1].out_len;      // out_off does not decrease
    BgzfWs w;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "bgzf_inflate", [&](Arena &a) { return carve_bgzf(a, n_blocks, true, hi - lo, o_hi - o_lo, w); }))) return rc;
    if ((rc = ensure_pinned(ctx, 2 * kPiece))) return rc;
    Events e(ctx);
    if (!e.ok()) { ctx->err = "bgzf_inflate: no event"; return CSV_EHIP; }
    size_t piece_no = 0;
    unsigned int n_declined = 0;
    if ((rc = copy_up(ctx, w.comp, comp + lo, hi - lo, e.ev, piece_no))) return rc;
    // the device copies start at lo and o_lo: the kernel's table is the caller's with its offsets moved
    std::vector<csv_bgzf_block> rel(blocks, blocks + n_blocks);
    for (csv_bgzf_block &b : rel) { b.in_off -= lo; b.out_off -= o_lo; }
    if ((rc = run_members(ctx, w, w.comp, rel.data(), n_blocks, w.out, w.status, e.ev, piece_no, n_declined))) return rc;
    if ((rc = copy_down(ctx, status, w.status, n_blocks, e.ev, Runs{{0, n_blocks}}))) return rc;
    // Only the decoded members' ranges come back (a declined member's bytes were never written on the device, and the bytes between two
    // members are the caller's): adjacent ranges as one run.
    Runs runs;
    for (uint32_t i = 0; i < n_blocks; i++) {
        if (status[i] || !rel[i].out_len) continue;
        if (!runs.empty() && runs.back().second == rel[i].out_off) runs.back().second += rel[i].out_len;
        else runs.emplace_back(rel[i].out_off, rel[i].out_off + rel[i].out_len);
    }
    if ((rc = copy_down(ctx, out + o_lo, w.out, o_hi - o_lo, e.ev, runs))) return rc;
    e.done = true;                                        // copy_down waited for its last piece
    return (int)n_declined;
}
