// bam_record_core.hpp — the per-record decisions of the device's BAM record unpacking (kernels/bamunpack.hip): the hop of the record chain,
// the host reader's checks in the host reader's order, the CG rule (bam_tag2cigar) with its walk over the auxiliary fields, and where a
// record's CIGAR words, sequence bytes and name lie. The same text compiles for the device (every lane runs it on a record of its own) and
// for the host with g++ (tools/fuzz/bam_record_core_check.cpp, under the sanitizers, against BamReader): no HIP construct in it.
// It replaces, per record, what BamReader::stream and BamReader::append (host/bam_io.cpp) do with bam1_core_t's fields, bam_get_cigar /
// bam_get_qname / bam_get_seq and find_cg; the values are the host's, bit for bit, and so are accept and refuse.
// What it guarantees whatever the bytes are: the buffer is only read through In::u8 / u16 / u32 at offsets whose every byte lies in
// [0, len) — the chain reads a length only where four bytes remain, a record is handed to fields() only when it lies whole inside the
// buffer, and the aux walk compares against its record's end before every read; every hop of the chain advances by at least 36 bytes.
#pragma once
#include <stdint.h>

#ifndef BRC_HD
#define BRC_HD
#endif

namespace bam_record_core {

// why a buffer is declined; the status word of the call holds the lowest failing offset with its reason
enum : uint32_t {
    R_OK = 0,
    R_SHORT = 1,          // block_size < 32                         "BAM: record shorter than its fixed fields"
    R_LONG = 2,           // block_size > 2^30                       "BAM: implausible record length"
    R_NEG_LSEQ = 3,       // l_seq < 0                               "BAM: negative sequence length"
    R_FIELDS = 4,         // fixed part longer than the record       "BAM: record fields exceed the record length"
    R_ANCHOR = 5          // a walk did not land on the next anchor  (the anchors are hints: nothing of the host's)
};

constexpr uint32_t MIN_HOP = 36;                   // 4 + the smallest block_size
constexpr uint32_t CIG_OP_S = 4;

// ---- the record chain -------------------------------------------------------------------------------------------------------------------
// Walks o += 4 + block_size from `from` while a whole record lies in front of `lim` (from <= lim <= len); sink.put(k, o) sees the k-th
// record's start. Ends at the first offset where no whole record fits (`o`; reason R_OK) or whose length is refused (reason, at `o`).
struct Walk { uint32_t o, n, reason; };
template <class In, class Sink>
BRC_HD inline Walk walk(const In &in, uint32_t from, uint32_t lim, Sink &sink)
{
    Walk w{from, 0, R_OK};
    for (;;) {
        if (lim - w.o < 4) break;
        const uint32_t bs = in.u32(w.o);
        if (bs < 32) { w.reason = R_SHORT; break; }                  // (the host's order: both length checks before "is it complete")
        if (bs > (1u << 30)) { w.reason = R_LONG; break; }
        if ((uint64_t)w.o + 4 + bs > lim) break;
        sink.put(w.n, w.o);
        w.n++;
        w.o += 4 + bs;                                               // >= MIN_HOP: the walk ends
    }
    return w;
}
struct NoSink { BRC_HD void put(uint32_t, uint32_t) {} };

// ---- one record -------------------------------------------------------------------------------------------------------------------------
struct Fields {
    int32_t tid, pos, l_seq;
    uint32_t l_name, mapq, n_cigar, flag;
    uint32_t cig_src, cig_n;          // byte offset of the CIGAR words that count (the record's own, or the CG tag's) and how many
    uint32_t seq_src, seq_n;          // bam_get_seq: byte offset, (l_seq + 1) / 2 bytes
    uint32_t name_src, name_n;        // bam_get_qname: byte offset, strnlen within l_name
};

// tid and pos alone (the contig filter looks at every record, the checks below only at the kept ones — as readContig and append do)
template <class In> BRC_HD inline int32_t rec_tid(const In &in, uint32_t o) { return (int32_t)in.u32(o + 4); }
template <class In> BRC_HD inline int32_t rec_pos(const In &in, uint32_t o) { return (int32_t)in.u32(o + 8); }

// find_cg of host/bam_io.cpp on offsets: the CG:B,I / CG:B,i array among the auxiliary fields [p, end). true: *at = offset of its first
// element, *count = its length. Anything malformed or unknown in front of it: false.
template <class In>
BRC_HD inline bool find_cg(const In &in, uint32_t p, uint32_t end, uint32_t *at, uint32_t *count)
{
    while (end - p >= 3) {
        const bool is_cg = in.u8(p) == 'C' && in.u8(p + 1) == 'G';
        const uint32_t type = in.u8(p + 2);
        p += 3;
        uint64_t len;
        switch (type) {
            case 'A': case 'c': case 'C': len = 1; break;
            case 's': case 'S': len = 2; break;
            case 'i': case 'I': case 'f': len = 4; break;
            case 'd': len = 8; break;
            case 'Z': case 'H': {
                uint32_t z = p;
                while (z < end && in.u8(z) != 0) z++;
                if (z == end) return false;
                len = (uint64_t)(z - p) + 1;
                break;
            }
            case 'B': {
                if (end - p < 5) return false;
                const uint32_t sub = in.u8(p);
                const uint32_t n = in.u32(p + 1);
                uint64_t es;
                switch (sub) { case 'c': case 'C': es = 1; break; case 's': case 'S': es = 2; break; case 'i': case 'I': case 'f': es = 4; break; default: return false; }
                if ((uint64_t)(end - p - 5) < (uint64_t)n * es) return false;
                if (is_cg) {
                    if (sub != 'I' && sub != 'i') return false;
                    *count = n;
                    *at = p + 5;
                    return true;
                }
                len = 5 + (uint64_t)n * es;
                break;
            }
            default: return false;
        }
        if (is_cg) return false;                        // a CG tag of another type is not a CIGAR
        if ((uint64_t)(end - p) < len) return false;
        p += (uint32_t)len;
    }
    return false;
}

// The record at o (its block_size field; [o, o + 4 + bs) inside the buffer, bs >= 32: the chain's doing). R_OK and f, or the host's refusal.
template <class In>
BRC_HD inline uint32_t fields(const In &in, uint32_t o, uint32_t bs, Fields &f)
{
    const uint32_t rec = o + 4;
    f.tid = (int32_t)in.u32(rec);
    f.pos = (int32_t)in.u32(rec + 4);
    f.l_name = in.u8(rec + 8);
    f.mapq = in.u8(rec + 9);
    f.n_cigar = in.u16(rec + 12);
    f.flag = in.u16(rec + 14);
    f.l_seq = (int32_t)in.u32(rec + 16);
    f.cig_src = f.cig_n = f.seq_src = f.seq_n = f.name_src = f.name_n = 0;
    if (f.l_seq < 0) return R_NEG_LSEQ;
    const uint64_t fixed = 32 + (uint64_t)f.l_name + 4ull * f.n_cigar + ((uint64_t)f.l_seq + 1) / 2 + (uint64_t)f.l_seq;
    if (fixed > bs) return R_FIELDS;
    f.name_src = rec + 32;
    while (f.name_n < f.l_name && in.u8(f.name_src + f.name_n) != 0) f.name_n++;
    f.cig_src = rec + 32 + f.l_name;
    f.cig_n = f.n_cigar;
    f.seq_src = f.cig_src + 4 * f.n_cigar;
    f.seq_n = (uint32_t)(((uint64_t)f.l_seq + 1) / 2);
    // long CIGAR in the CG tag behind a <l_seq>S<n>N placeholder (bam_tag2cigar)
    if (f.n_cigar > 0 && f.tid >= 0 && f.pos >= 0) {
        const uint32_t c0 = in.u32(f.cig_src);
        if ((c0 & 15) == CIG_OP_S && (int32_t)(c0 >> 4) == f.l_seq) {
            uint32_t at = 0, cnt = 0;
            if (find_cg(in, rec + (uint32_t)fixed, rec + bs, &at, &cnt) && cnt >= f.n_cigar && cnt < (1u << 29)) { f.cig_src = at; f.cig_n = cnt; }
        }
    }
    return R_OK;
}

// the contig filter of readContig on one record: skipped in front of the run, kept inside it (tid < 0 keeps everything)
BRC_HD inline bool flt_skip(int32_t want_tid, int32_t tid) { return want_tid >= 0 && tid >= 0 && tid < want_tid; }
BRC_HD inline bool flt_keep(int32_t want_tid, int64_t end, int32_t tid, int32_t pos) { return want_tid < 0 || (tid == want_tid && (int64_t)pos < end); }

}  // namespace bam_record_core
