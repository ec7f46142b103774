// bam.hip — BAM records unpacked on the device (kernels/bamunpack.hip): the checks of the anchors and of the output struct, the two
// read-backs (records in the stream; the kept records' counts, held against the caller's capacities before anything is written), and for the
// host-pointer form the pieced copies through the page-locked block (a Transfer, glue.hpp). Replaces, with the kernels, what the host
// reader does per record with bam1_core_t's fields, bam_get_cigar / bam_get_qname / bam_get_seq and bam_tag2cigar (host/bam_io.cpp).
#include "glue.hpp"

using namespace csv;

namespace {

int bad(csv_ctx *ctx, const char *msg) { ctx->err = std::string("bam_unpack: ") + msg; return CSV_EINVAL; }

int check_args(csv_ctx *ctx, const uint8_t *bytes, uint64_t len, const uint32_t *anchors, uint32_t n_anchors, const csv_bam_out *out, csv_bam_counts *counts)
{
    if (!out || !counts) return bad(ctx, "null pointer");
    if (len >= (1ull << 32)) return bad(ctx, "a stream of 2^32 bytes or more");
    if (len && !bytes) return bad(ctx, "null pointer");
    if (len && (!anchors || !n_anchors)) return bad(ctx, "no anchor (anchors[0] is the first record's start)");
    if (!out->pos || !out->flag || !out->mapq || !out->cigar_off || !out->cigar) return bad(ctx, "null pointer");
    if (!out->seq_off != !out->seq) return bad(ctx, "seq_off and seq are wanted together");
    if (!out->name_off != !out->name) return bad(ctx, "name_off and name are wanted together");
    for (uint32_t k = 0; k < n_anchors && len; k++) {
        if (anchors[k] >= len) return bad(ctx, "an anchor outside the stream");
        if (k && anchors[k] <= anchors[k - 1]) return bad(ctx, "anchors not strictly ascending");
    }
    return CSV_OK;
}

struct Head { uint32_t res[BU_RES_WORDS]; unsigned long long status; uint32_t bounds[2]; };
static_assert(sizeof(Head) <= BU_HEAD_BYTES, "the head is one slice");

// What both entry points share: anchors up, chain, counts, capacities, outputs. d_out: the device arrays; caps: the caller's struct.
// Returns CSV_OK (the last kernel queued, not waited for) / 1 (declined) / CSV_E*.
int run_unpack(csv_ctx *ctx, Transfer &t, const BamUnpackWs &w, const uint8_t *d_bytes, uint32_t len, const uint32_t *anchors, uint32_t n_anchors, int32_t tid,
               int64_t end, uint64_t cigar_base, uint64_t seq_base, uint64_t name_base, const BamUnpackOut &d_out, const csv_bam_out &caps, csv_bam_counts &c)
{
    hipStream_t s = ctx->stream;
    int rc = t.up(w.anchors, anchors, (size_t)n_anchors * 4);
    if (rc) return rc;
    CSV_HIP(ctx, hipMemsetAsync(w.res, 0xff, BU_HEAD_BYTES, s));          // status: none; bounds: beyond every record
    Head h;
    TimerScope ts(ctx, CSV_K_MISC);
    launch_bam_chain(s, d_bytes, len, n_anchors, w);
    if ((rc = t.peek(&h, w.res, sizeof(Head)))) return rc;
    // (the kernels order a missed anchor in front of anything else at its offset by giving it reason 0)
    auto declined = [&](unsigned long long status) { c = csv_bam_counts{}; c.status = (status & 0xff) ? status : (status | CSV_BAM_ANCHOR); return 1; };
    if (h.status != BU_STATUS_NONE) return declined(h.status);
    const uint32_t n_rec = h.res[BU_RES_NREC], consumed = h.res[BU_RES_CONSUMED];
    if (n_rec > w.rec_cap || consumed > len) { ctx->err = "bam_unpack: the chain's counts leave the stream"; return CSV_EHIP; }
    launch_bam_fields(s, d_bytes, n_rec, tid, end, w);
    if ((rc = t.peek(&h, w.res, sizeof(Head)))) return rc;
    if (h.status != BU_STATUS_NONE) return declined(h.status);
    const uint32_t n_kept = h.res[BU_RES_NKEPT], first = h.res[BU_RES_FIRST], n_cigar = h.res[BU_RES_NCIGAR], n_seq = h.res[BU_RES_NSEQ], n_name = h.res[BU_RES_NNAME];
    if ((uint64_t)first + n_kept > n_rec || n_cigar > len / 4 || n_seq > len || n_name > len) { ctx->err = "bam_unpack: the kept records' counts leave the stream"; return CSV_EHIP; }
    c = csv_bam_counts{};
    c.n_records = n_rec; c.kept_first = first; c.n_kept = n_kept; c.n_cigar = n_cigar;
    c.n_seq = d_out.seq ? n_seq : 0; c.n_name = d_out.name ? n_name : 0;
    c.consumed = consumed; c.stopped = h.res[BU_RES_STOPPED];
    if (n_kept > caps.cap_records || n_cigar > caps.cap_cigar || c.n_seq > caps.cap_seq || c.n_name > caps.cap_name) {
        ctx->err = "bam_unpack: output capacity too small";
        return CSV_ECAPACITY;
    }
    launch_bam_emit(s, d_bytes, first, n_kept, n_cigar, n_seq, n_name, cigar_base, seq_base, name_base, w, d_out);
    CSV_HIP(ctx, hipGetLastError());
    return CSV_OK;
}

BamUnpackOut dev_out(const csv_bam_out &o) { return BamUnpackOut{o.pos, o.flag, o.mapq, o.cigar_off, o.cigar, o.seq_off, o.seq, o.name_off, o.name, o.name_hash}; }

}  // namespace

int csvgpu_bam_unpack_dev(csv_ctx *ctx, const uint8_t *d_bytes, uint64_t len, const uint32_t *anchors, uint32_t n_anchors, int32_t tid, int64_t end,
                          uint64_t cigar_base, uint64_t seq_base, uint64_t name_base, const csv_bam_out *d_out, csv_bam_counts *counts)
{
    if (!ctx) return CSV_EINVAL;
    int rc = check_args(ctx, d_bytes, len, anchors, n_anchors, d_out, counts);
    if (rc) return rc;
    if (len == 0) { *counts = csv_bam_counts{}; return CSV_OK; }          // nothing to unpack, nothing written
    (void)hipSetDevice(ctx->device);
    BamUnpackWs w;
    if ((rc = arena_reserve_for(ctx, ctx->work, "bam_unpack", [&](Arena &a) { return carve_bam_unpack(a, len, n_anchors, false, 0, 0, 0, 0, false, w); }))) return rc;
    Transfer t(ctx);
    if ((rc = t.open("bam_unpack"))) return rc;
    rc = run_unpack(ctx, t, w, d_bytes, (uint32_t)len, anchors, n_anchors, tid, end, cigar_base, seq_base, name_base, dev_out(*d_out), *d_out, *counts);
    return rc == CSV_OK ? t.wait() : rc;                                  // (the caller's device arrays are complete on return)
}

int csvgpu_bam_unpack(csv_ctx *ctx, const uint8_t *bytes, uint64_t len, const uint32_t *anchors, uint32_t n_anchors, int32_t tid, int64_t end,
                      uint64_t cigar_base, uint64_t seq_base, uint64_t name_base, const csv_bam_out *out, csv_bam_counts *counts)
{
    if (!ctx) return CSV_EINVAL;
    int rc = check_args(ctx, bytes, len, anchors, n_anchors, out, counts);
    if (rc) return rc;
    if (len == 0) { *counts = csv_bam_counts{}; return CSV_OK; }          // nothing to unpack, nothing written
    (void)hipSetDevice(ctx->device);
    BamUnpackWs w;
    if ((rc = arena_reserve_for(ctx, ctx->arena, "bam_unpack", [&](Arena &a) {
            return carve_bam_unpack(a, len, n_anchors, true, out->cap_records, out->cap_cigar, out->seq ? std::max<uint64_t>(out->cap_seq, 1) : 0,
                                    out->name ? std::max<uint64_t>(out->cap_name, 1) : 0, out->name_hash != nullptr, w);
        }))) return rc;
    Transfer t(ctx);
    if ((rc = t.open("bam_unpack"))) return rc;
    if ((rc = t.up(w.bytes, bytes, len))) return rc;
    // The staged arrays hold min(capacity, what the stream can hold): a count beyond the capacity is CSV_ECAPACITY before anything is
    // written, a count within it is within the staged array.
    if ((rc = run_unpack(ctx, t, w, w.bytes, (uint32_t)len, anchors, n_anchors, tid, end, cigar_base, seq_base, name_base, w.out, *out, *counts))) return rc;
    const csv_bam_counts &c = *counts;
    if ((rc = t.down(out->pos, w.out.pos, c.n_kept * 4)) || (rc = t.down(out->flag, w.out.flag, c.n_kept * 2)) || (rc = t.down(out->mapq, w.out.mapq, c.n_kept)) ||
        (rc = t.down(out->cigar_off, w.out.cigar_off, (c.n_kept + 1) * 8)) || (rc = t.down(out->cigar, w.out.cigar, c.n_cigar * 4))) return rc;
    if (out->seq && ((rc = t.down(out->seq_off, w.out.seq_off, (c.n_kept + 1) * 8)) || (rc = t.down(out->seq, w.out.seq, c.n_seq)))) return rc;
    if (out->name && ((rc = t.down(out->name_off, w.out.name_off, (c.n_kept + 1) * 8)) || (rc = t.down(out->name, w.out.name, c.n_name)))) return rc;
    if (out->name_hash && (rc = t.down(out->name_hash, w.out.name_hash, c.n_kept * 8))) return rc;
    return t.wait();
}
