// bgzf.hip — BGZF members inflated on the device (kernels/inflate.hip): the checks of the member table, the copies through a Transfer
// (glue.hpp) of the host-pointer form, and the count of declined members.
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

// table up, kernel, count back: what both entry points share; ends in a wait
int run_members(csv_ctx *ctx, Transfer &t, const BgzfWs &w, const uint8_t *d_comp, const csv_bgzf_block *blocks, uint32_t n_blocks, uint8_t *d_out, uint8_t *d_status,
                unsigned int &n_declined)
{
    int rc = t.up(w.blocks, blocks, (size_t)n_blocks * sizeof(csv_bgzf_block));
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    CSV_HIP(ctx, hipMemsetAsync(w.n_declined, 0, 4, s));
    {
        TimerScope ts(ctx, CSV_K_MISC);
        launch_bgzf_inflate(s, d_comp, w.blocks, n_blocks, d_out, d_status, w.n_declined);
    }
    if ((rc = t.peek(&n_declined, w.n_declined, 4))) return rc;      // (behind the upload's last pieces on the stream: the block's first bytes are free)
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
    Transfer t(ctx);
    if ((rc = t.open("bgzf_inflate"))) return rc;
    unsigned int n_declined = 0;
    if ((rc = run_members(ctx, t, w, d_comp, blocks, n_blocks, d_out, d_status, n_declined))) return rc;
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
    Transfer t(ctx);
    if ((rc = t.open("bgzf_inflate"))) return rc;
    unsigned int n_declined = 0;
    if ((rc = t.up(w.comp, comp + lo, hi - lo))) return rc;
    // the device copies start at lo and o_lo: the kernel's table is the caller's with its offsets moved
    std::vector<csv_bgzf_block> rel(blocks, blocks + n_blocks);
    for (csv_bgzf_block &b : rel) { b.in_off -= lo; b.out_off -= o_lo; }
    if ((rc = run_members(ctx, t, w, w.comp, rel.data(), n_blocks, w.out, w.status, n_declined))) return rc;
    if ((rc = t.down(status, w.status, n_blocks))) return rc;
    // Only the decoded members' ranges come back (a declined member's bytes were never written on the device, and the bytes between two
    // members are the caller's): adjacent ranges as one run.
    Runs runs;
    for (uint32_t i = 0; i < n_blocks; i++) {
        if (status[i] || !rel[i].out_len) continue;
        if (!runs.empty() && runs.back().second == rel[i].out_off) runs.back().second += rel[i].out_len;
        else runs.emplace_back(rel[i].out_off, rel[i].out_off + rel[i].out_len);
    }
    if ((rc = t.down(out + o_lo, w.out, o_hi - o_lo, runs))) return rc;
    return (int)n_declined;
}
