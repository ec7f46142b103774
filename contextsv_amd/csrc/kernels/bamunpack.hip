// bamunpack.hip — kernel #13: BAM records unpacked where the inflate leaves them (gfx950). A decoded record stream in HBM goes in; the
// arrays the CIGAR scan takes come out — pos, flag, mapq, cigar_off, cigar with CG-tag long CIGARs restored — and, where wanted, the packed
// sequences, the query names and their std::hash values: what BamReader::stream + append (host/bam_io.cpp) make of the same bytes with
// bam1_core_t's fields, bam_get_cigar / bam_get_qname / bam_get_seq and bam_tag2cigar, bit for bit. The per-record decisions are
// bam_record_core.hpp, which the CPU check runs against the host reader.
//
//   chain    a record's start is known only from its predecessor's length, so the stream is cut at the caller's anchors (offsets claimed to be
//            record starts; anchors[0] is one): one lane per interval hops o += 4 + block_size and must land EXACTLY on the next anchor, which
//            by induction from anchors[0] makes every start a true one — a wrong anchor declines the buffer, it is never believed. Counted,
//            summed (sort.hip's exclusive sum), walked again to write rec_off[]. The last interval ends where no whole record is left: consumed.
//   filter   readContig's run — skip 0 <= tid' < tid in front, keep tid' == tid && pos < end, stop at the first other record — as two
//            atomicMins over the record indices: first not-skipped, first not-kept behind it (told from in front by its predecessor).
//   fields   one lane per kept record: the host's checks in the host's order, the CG rule, the three counts. Exclusive sums give the offsets.
//   emit     pos / flag / mapq, the three offset arrays (+ the caller's bases), the names' hashes (libstdc++'s _Hash_bytes, devutil.hpp).
//   gather   CIGAR words, sequence bytes, name bytes by one kernel, divided by OUTPUT position: a lane owns one aligned dword of the
//            destination and finds its record by a search in the offsets, so a 70 000-operation CIGAR is spread over 70 000 lanes
//            like anything else and no wave's work grows with the longest record. Sources are byte-unaligned (names have any length): a word
//            is built from two aligned words (v_alignbyte_b32), never loaded unaligned.
// Memory: every load is an aligned dword that holds a byte of [0, len) (BamIn); stores go to the kept records' output ranges alone, whole
// dwords only where all four bytes are the call's. Failed checks meet in one status word, (offset << 8 | reason, 0 for a missed anchor), lowest offset first
// (atomicMin): the lowest reported failure is a true one, since every interval in front of it landed.
#include <algorithm>

#include "../common.hpp"
#include "../devutil.hpp"

#define BRC_HD __host__ __device__
#include "../bam_record_core.hpp"

namespace csv {

namespace brc = bam_record_core;

namespace {

constexpr int BU_THREADS = 256;
constexpr uint32_t BU_MAX_BLOCKS = 4096;                 // larger calls stride

// The stream behind aligned dword loads: `w` is the buffer's address rounded down to a dword, `mis` what was cut off. A load touches the
// aligned dword(s) that hold the bytes asked for, and those are bytes of [0, len) by the caller's bounds.
struct BamIn {
    const uint32_t *w;
    uint32_t mis;
    __device__ BamIn(const uint8_t *d) : w((const uint32_t *)((uintptr_t)d & ~(uintptr_t)3)), mis((uint32_t)((uintptr_t)d & 3)) {}
    __device__ uint32_t u8(uint32_t off) const
    {
        const uint64_t q = (uint64_t)off + mis;
        return (w[q >> 2] >> ((q & 3) * 8)) & 0xffu;
    }
    __device__ uint32_t u16(uint32_t off) const
    {
        const uint64_t q = (uint64_t)off + mis;
        const uint32_t sh = (uint32_t)(q & 3), a = w[q >> 2];
        if (sh < 3) return (a >> (sh * 8)) & 0xffffu;
        return (a >> 24) | ((w[(q >> 2) + 1] & 0xffu) << 8);
    }
    __device__ uint32_t u32(uint32_t off) const
    {
        const uint64_t q = (uint64_t)off + mis;
        const uint32_t sh = (uint32_t)(q & 3), a = w[q >> 2];
        if (sh == 0) return a;
        return __builtin_amdgcn_alignbyte(w[(q >> 2) + 1], a, sh);          // bytes off .. off + 3 of {next, a}
    }
};

__device__ __forceinline__ void report(unsigned long long *status, uint32_t off, uint32_t reason)
{
    // (at one offset a missed anchor comes first: the walk that starts on a false anchor may refuse a "length" it reads right there)
    atomicMin(status, ((unsigned long long)off << 8) | (reason == brc::R_ANCHOR ? 0u : reason));
}

struct RecSink {
    uint32_t *rec_off, base, cap;
    __device__ void put(uint32_t k, uint32_t o) { if (rec_off && base + k < cap) rec_off[base + k] = o; }
};

// One lane per anchor interval. rec_off == nullptr: count[k] = records of interval k (count[n_anchors] = 0), failures reported;
// else count[] is its exclusive sum and the starts are written.
__global__ __launch_bounds__(BU_THREADS) void bu_chain_kernel(const uint8_t *__restrict__ bytes, uint32_t len, const uint32_t *__restrict__ anchors, uint32_t n_anchors,
                                                              uint32_t *__restrict__ count, uint32_t *__restrict__ rec_off, uint32_t rec_cap,
                                                              uint32_t *__restrict__ res, unsigned long long *__restrict__ status)
{
    const BamIn in(bytes);
    for (uint32_t k = blockIdx.x * BU_THREADS + threadIdx.x; k <= n_anchors; k += gridDim.x * BU_THREADS) {
        if (k == n_anchors) { if (!rec_off) count[k] = 0; else res[BU_RES_NREC] = count[k]; continue; }
        const bool last = k + 1 == n_anchors;
        const uint32_t from = anchors[k], lim = last ? len : anchors[k + 1];          // from < lim <= len: the entry point's check
        RecSink sink{rec_off, rec_off ? count[k] : 0u, rec_cap};
        const brc::Walk wk = brc::walk(in, from, lim, sink);
        if (rec_off) continue;
        count[k] = wk.n;
        if (wk.reason != brc::R_OK) report(status, wk.o, wk.reason);
        else if (!last && wk.o != lim) report(status, lim, brc::R_ANCHOR);            // no whole record ends on the next anchor
        if (last) res[BU_RES_CONSUMED] = wk.o;
    }
}

// bounds[0] = first record that is not skipped, bounds[1] = first record behind it that is not kept (both preset to n_rec)
__global__ __launch_bounds__(BU_THREADS) void bu_filter_kernel(const uint8_t *__restrict__ bytes, const uint32_t *__restrict__ rec_off, uint32_t n_rec, int32_t tid, int64_t end,
                                                               uint32_t *__restrict__ bounds)
{
    const BamIn in(bytes);
    for (uint32_t i = blockIdx.x * BU_THREADS + threadIdx.x; i < n_rec; i += gridDim.x * BU_THREADS) {
        const uint32_t o = rec_off[i];
        const int32_t t = brc::rec_tid(in, o), p = brc::rec_pos(in, o);
        const bool skip = brc::flt_skip(tid, t);
        if (!skip) atomicMin(&bounds[0], i);
        if (!brc::flt_keep(tid, end, t, p)) {
            // at or behind the first not-skipped record: that record itself, or the successor of a record that was not skipped
            bool behind = !skip;
            if (!behind && i > 0) behind = !brc::flt_skip(tid, brc::rec_tid(in, rec_off[i - 1]));
            if (behind) atomicMin(&bounds[1], i);
        }
    }
}

struct BuRec {                               // per kept record j = record bounds[0] + j; the three counts have n_rec + 1 entries (zero from n_kept on)
    uint32_t *cig_src, *cig_n, *seq_n, *name_n;
};

__global__ __launch_bounds__(BU_THREADS) void bu_fields_kernel(const uint8_t *__restrict__ bytes, const uint32_t *__restrict__ rec_off, uint32_t n_rec,
                                                               const uint32_t *__restrict__ bounds, BuRec r, unsigned long long *__restrict__ status)
{
    const BamIn in(bytes);
    const uint32_t a = min(bounds[0], n_rec), b = max(min(bounds[1], n_rec), a), n_kept = b - a;
    for (uint32_t j = blockIdx.x * BU_THREADS + threadIdx.x; j <= n_rec; j += gridDim.x * BU_THREADS) {
        uint32_t cs = 0, cn = 0, sn = 0, nn = 0;
        if (j < n_kept) {
            const uint32_t o = rec_off[a + j];
            brc::Fields f;
            const uint32_t why = brc::fields(in, o, in.u32(o), f);
            if (why != brc::R_OK) report(status, o, why);
            cs = f.cig_src; cn = f.cig_n; sn = f.seq_n; nn = f.name_n;
        }
        r.cig_src[j] = cs; r.cig_n[j] = cn; r.seq_n[j] = sn; r.name_n[j] = nn;
    }
}

// the counts of the call, behind the sums: res = {n_kept, kept_first, n_cigar, n_seq, n_name, stopped}
__global__ void bu_totals_kernel(const uint32_t *__restrict__ bounds, uint32_t n_rec, BuRec r, uint32_t *__restrict__ res)
{
    if (threadIdx.x || blockIdx.x) return;
    const uint32_t a = min(bounds[0], n_rec), b = max(min(bounds[1], n_rec), a), n_kept = b - a;
    res[0] = n_kept; res[1] = a; res[2] = r.cig_n[n_kept]; res[3] = r.seq_n[n_kept]; res[4] = r.name_n[n_kept]; res[5] = b < n_rec ? 1u : 0u;
}

__global__ __launch_bounds__(BU_THREADS) void bu_emit_kernel(const uint8_t *__restrict__ bytes, const uint32_t *__restrict__ rec_off, uint32_t first, uint32_t n_kept, BuRec r,
                                                             uint64_t cigar_base, uint64_t seq_base, uint64_t name_base, BamUnpackOut out)
{
    const BamIn in(bytes);
    for (uint32_t j = blockIdx.x * BU_THREADS + threadIdx.x; j <= n_kept; j += gridDim.x * BU_THREADS) {
        out.cigar_off[j] = cigar_base + r.cig_n[j];
        if (out.seq_off) out.seq_off[j] = seq_base + r.seq_n[j];
        if (out.name_off) out.name_off[j] = name_base + r.name_n[j];
        if (j == n_kept) continue;
        const uint32_t rec = rec_off[first + j] + 4;
        out.pos[j] = (int32_t)in.u32(rec + 4);
        out.mapq[j] = (uint8_t)in.u8(rec + 9);
        out.flag[j] = (uint16_t)in.u16(rec + 14);
        if (out.name_hash) {
            const uint32_t len = r.name_n[j + 1] - r.name_n[j];
            uint32_t p = rec + 32;
            uint64_t h = hb_init(len);
            for (uint32_t k = len >> 3; k > 0; k--, p += 8) h = hb_block(h, (uint64_t)in.u32(p) | ((uint64_t)in.u32(p + 4) << 32));
            if (len & 7u) {
                uint64_t t = 0;
                for (uint32_t k = 0; k < (len & 7u); k++) t |= (uint64_t)in.u8(p + k) << (8 * k);
                h = hb_tail(h, t);
            }
            out.name_hash[j] = hb_final(h);
        }
    }
}

// Segmented gather: dst[off[j] << shift .. off[j + 1] << shift) = bytes[src(j) ..] for the n records of the call, total = off[n] << shift
// bytes. A lane owns the aligned dword number t of the destination (dst rounded down to a dword); upper_bound in off[] finds the record of
// its first byte. src: per-record offsets (the CIGAR's), or null with rec_off and `fixed`: where the names (36) lie; the sequences sit behind
// name and CIGAR of their record (seq_mode).
struct BuGather {
    const uint32_t *off;             // [n + 1] exclusive sums, in units of 1 << shift bytes
    const uint32_t *src;             // [n] or null
    const uint32_t *rec_off;         // kept records' starts
    uint32_t n, shift, seq_mode;
};
__device__ __forceinline__ uint32_t bu_src_of(const BamIn &in, const BuGather &g, uint32_t j)
{
    if (g.src) return g.src[j];
    const uint32_t rec = g.rec_off[j] + 4;
    if (!g.seq_mode) return rec + 32;
    return rec + 32 + in.u8(rec + 8) + 4 * in.u16(rec + 12);
}
__global__ __launch_bounds__(BU_THREADS) void bu_gather_kernel(const uint8_t *__restrict__ bytes, BuGather g, uint8_t *__restrict__ dst, uint32_t total)
{
    const BamIn in(bytes);
    const uint32_t dmis = (uint32_t)((uintptr_t)dst & 3);
    const uint64_t n_words = ((uint64_t)total + dmis + 3) >> 2;
    for (uint64_t t = (uint64_t)blockIdx.x * BU_THREADS + threadIdx.x; t < n_words; t += (uint64_t)gridDim.x * BU_THREADS) {
        // destination bytes [b0, b1) of this dword, relative to dst
        const uint64_t e = t * 4 + 4 - dmis;
        const uint32_t b0 = t == 0 ? 0u : (uint32_t)(t * 4 - dmis), b1 = e < total ? (uint32_t)e : total;
        // the record of byte b0: the last j with (off[j] << shift) <= b0 among those that have bytes (off[j + 1] > off[j] is implied by the search)
        uint32_t lo = 0, hi = g.n;                                                   // invariant: off[lo] << shift <= b0 < off[hi] << shift
        while (hi - lo > 1) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (((uint64_t)g.off[mid] << g.shift) <= b0) lo = mid; else hi = mid;
        }
        uint32_t j = lo;
        uint64_t r0 = (uint64_t)g.off[j] << g.shift, r1 = (uint64_t)g.off[j + 1] << g.shift;
        uint8_t *const at = dst + b0;
        if (b1 - b0 == 4 && b1 <= r1) {                                              // a whole dword of one record: two aligned loads, one store
            *(uint32_t *)at = in.u32(bu_src_of(in, g, j) + (uint32_t)(b0 - r0));
            continue;
        }
        uint32_t v = 0, s = bu_src_of(in, g, j);
        for (uint32_t b = b0; b < b1; b++) {
            while (b >= r1) { j++; r0 = r1; r1 = (uint64_t)g.off[j + 1] << g.shift; s = bu_src_of(in, g, j); }      // (b < total = off[n]: j stays below n)
            v |= in.u8(s + (uint32_t)(b - r0)) << (8 * (b - b0));
        }
        if (b1 - b0 == 4) *(uint32_t *)at = v;
        else for (uint32_t b = b0; b < b1; b++) at[b - b0] = (uint8_t)(v >> (8 * (b - b0)));
    }
}

unsigned grid_for(uint64_t items) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((items + BU_THREADS - 1) / BU_THREADS, BU_MAX_BLOCKS)); }

BuRec rec_of(const BamUnpackWs &w) { return BuRec{w.cig_src, w.cig_n, w.seq_n, w.name_n}; }

}  // namespace

void launch_bam_chain(hipStream_t s, const uint8_t *bytes, uint32_t len, uint32_t n_anchors, const BamUnpackWs &w)
{
    const unsigned grid = grid_for((uint64_t)n_anchors + 1);
    hipLaunchKernelGGL(bu_chain_kernel, dim3(grid), dim3(BU_THREADS), 0, s, bytes, len, w.anchors, n_anchors, w.count, (uint32_t *)nullptr, 0u, w.res, w.status);
    launch_exclusive_sum_u32(s, w.count, (uint64_t)n_anchors + 1, w.es_tmp);
    hipLaunchKernelGGL(bu_chain_kernel, dim3(grid), dim3(BU_THREADS), 0, s, bytes, len, w.anchors, n_anchors, w.count, w.rec_off, w.rec_cap, w.res, w.status);
}

void launch_bam_fields(hipStream_t s, const uint8_t *bytes, uint32_t n_rec, int32_t tid, int64_t end, const BamUnpackWs &w)
{
    const BuRec r = rec_of(w);
    if (n_rec) hipLaunchKernelGGL(bu_filter_kernel, dim3(grid_for(n_rec)), dim3(BU_THREADS), 0, s, bytes, w.rec_off, n_rec, tid, end, w.bounds);
    hipLaunchKernelGGL(bu_fields_kernel, dim3(grid_for((uint64_t)n_rec + 1)), dim3(BU_THREADS), 0, s, bytes, w.rec_off, n_rec, w.bounds, r, w.status);
    launch_exclusive_sum_u32(s, w.cig_n, (uint64_t)n_rec + 1, w.es_tmp);
    launch_exclusive_sum_u32(s, w.seq_n, (uint64_t)n_rec + 1, w.es_tmp);
    launch_exclusive_sum_u32(s, w.name_n, (uint64_t)n_rec + 1, w.es_tmp);
    hipLaunchKernelGGL(bu_totals_kernel, dim3(1), dim3(WAVE), 0, s, w.bounds, n_rec, r, w.res);
}

void launch_bam_emit(hipStream_t s, const uint8_t *bytes, uint32_t first, uint32_t n_kept, uint32_t n_cigar, uint32_t n_seq, uint32_t n_name,
                     uint64_t cigar_base, uint64_t seq_base, uint64_t name_base, const BamUnpackWs &w, const BamUnpackOut &out)
{
    const BuRec r = rec_of(w);
    hipLaunchKernelGGL(bu_emit_kernel, dim3(grid_for((uint64_t)n_kept + 1)), dim3(BU_THREADS), 0, s, bytes, w.rec_off, first, n_kept, r, cigar_base, seq_base, name_base, out);
    if (n_kept == 0) return;
    const uint32_t *kept = w.rec_off + first;
    if (n_cigar) {
        const BuGather g{w.cig_n, w.cig_src, kept, n_kept, 2u, 0u};
        hipLaunchKernelGGL(bu_gather_kernel, dim3(grid_for((uint64_t)n_cigar + 1)), dim3(BU_THREADS), 0, s, bytes, g, (uint8_t *)out.cigar, n_cigar * 4u);
    }
    if (out.seq && n_seq) {
        const BuGather g{w.seq_n, nullptr, kept, n_kept, 0u, 1u};
        hipLaunchKernelGGL(bu_gather_kernel, dim3(grid_for(((uint64_t)n_seq + 7) / 4)), dim3(BU_THREADS), 0, s, bytes, g, out.seq, n_seq);
    }
    if (out.name && n_name) {
        const BuGather g{w.name_n, nullptr, kept, n_kept, 0u, 0u};
        hipLaunchKernelGGL(bu_gather_kernel, dim3(grid_for(((uint64_t)n_name + 7) / 4)), dim3(BU_THREADS), 0, s, bytes, g, out.name, n_name);
    }
}

}  // namespace csv
