// transfer.hip — Transfer (glue.hpp): the pieced copies between pageable host memory and the device through the two halves of the
// page-locked block, the read-back through the block's first bytes, and the drain that keeps the events and the halves from changing hands
// under a copy still in flight.
#include <assert.h>

#include "glue.hpp"

namespace csv {

int Transfer::open(const char *who)
{
    const int rc = ensure_pinned(ctx, 2 * kPiece);
    if (rc) return rc;
    ev[0] = get_event(ctx); ev[1] = get_event(ctx);
    if (!ev[0] || !ev[1]) { ctx->err = std::string(who) + ": no event"; return CSV_EHIP; }
    return CSV_OK;
}

// An early return (a HIP error part-way through the pieces) may leave copies queued that read or write the page-locked halves and events
// recorded but not waited for: the stream is drained before the events go back to the pool and the block to its next user.
Transfer::~Transfer()
{
    if (pending) (void)hipStreamSynchronize(ctx->stream);
    for (hipEvent_t e : ev) if (e) ctx->event_pool.push_back(e);
}

int Transfer::up(void *d_dst, const void *h_src, size_t bytes)
{
    for (size_t off = 0; off < bytes; off += kPiece, n_up++) {
        const size_t n = std::min(kPiece, bytes - off), slot = n_up & 1;
        char *pin = (char *)ctx->pinned + slot * kPiece;
        if (n_up >= 2) CSV_HIP(ctx, wait_event(ev[slot]));              // the copy that last read this half is done
        memcpy(pin, (const char *)h_src + off, n);
        pending = true;
        CSV_HIP(ctx, hipMemcpyAsync((char *)d_dst + off, pin, n, hipMemcpyHostToDevice, ctx->stream));
        CSV_HIP(ctx, hipEventRecord(ev[slot], ctx->stream));
    }
    return CSV_OK;
}

int Transfer::down(void *h_dst, const void *d_src, size_t bytes, const Runs &runs)
{
    const size_t n_pieces = (bytes + kPiece - 1) / kPiece;
    if (n_pieces == 0) return CSV_OK;
    pending = true;
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
    pending = false;                                      // the last piece's event lies behind everything this session queued
    return CSV_OK;
}

int Transfer::down(void *h_dst, const void *d_src, size_t bytes)
{
    return h_dst && bytes ? down(h_dst, d_src, bytes, Runs{{0, bytes}}) : (int)CSV_OK;
}

int Transfer::peek(void *dst, const void *d_src, size_t bytes)
{
    assert(bytes <= kPinScalars);
    CSV_HIP(ctx, hipGetLastError());
    pending = true;
    CSV_HIP(ctx, hipMemcpyAsync(ctx->pinned, d_src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    CSV_HIP(ctx, wait_stream(ctx->stream));
    pending = false;
    memcpy(dst, ctx->pinned, bytes);
    return CSV_OK;
}

int Transfer::wait()
{
    CSV_HIP(ctx, wait_stream(ctx->stream));
    pending = false;
    return CSV_OK;
}

}  // namespace csv
