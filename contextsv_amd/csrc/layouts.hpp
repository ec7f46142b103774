// layouts.hpp — every device workspace layout of the library as one carve function over an Arena (arena.hpp). The entry points in
// api/*.hip and the launchers in kernels/ reserve by planning these and then carve with them; nothing else says how large a workspace
// is. Pads that a kernel relies on are part of their slice and are named where they are taken. Free of HIP calls: the CPU-only check
// (tools/fuzz/arena_layouts_check.cpp) runs every function listed in kLayoutNames at the rounding edges.
#pragma once
#include <algorithm>

#include "common.hpp"

namespace csv {

#ifdef CSV_ARENA_LOG               // (the check program's build alone)
// the check program must cover exactly these (a carve function added here without a line there fails tests/test_arena_layouts.py)
static const char *const kLayoutNames[] = {"reads", "sortws", "depth", "dbscan_iv", "dbscan1d", "split_nodes", "split_epochs", "split_groups",
                                           "sf_tables", "sf_run", "sr_refs", "sr_tables", "job_scratch", "window", "cn_back", "cn_obs", "cn_tables", "bgzf", "bam_unpack", "vcf", "vcf_text", "dbscan_tmp", "viterbi_tmp", "sort_slot", "merge_select", "merge_run"};
constexpr size_t kLayoutCount = sizeof(kLayoutNames) / sizeof(kLayoutNames[0]);
#endif

// device scalars + the ordering pass's bucket tables, zeroed together before every scan
static constexpr size_t kCntBytes = 256 + 2 * (size_t)BK_N * 4;

// a host shard staged in the arena, with the scan's per-read outputs
struct ReadsWs {
    int32_t *pos; uint16_t *flag; uint8_t *mapq; uint64_t *coff; uint32_t *cig;
    int32_t *ref_end, *q_start, *q_end;
    ScanCounters *cnt;
    uint32_t *ckpt;
};
static inline bool carve_reads(Arena &a, uint64_t n, uint64_t m, ReadsWs &w)
{
    return take(a, w.pos, n * 4) && take(a, w.flag, n * 2) && take(a, w.mapq, n) && take(a, w.coff, (n + 1) * 8) &&
           take(a, w.cig, m * 4 + 16) &&                                  // + 16: the scan's 16-byte word loads at the last read's end
           take(a, w.ref_end, n * 4) && take(a, w.q_start, n * 4) && take(a, w.q_end, n * 4) && take(a, w.cnt, kCntBytes) && take(a, w.ckpt, ckpt_bytes(m));
}

// ordering workspace for n signatures
struct SortWs {
    uint64_t *k0, *k1;
    uint32_t *v0, *v1;
    void *tmp;
    csv_sig *sig_tmp;        // bucketed copy of the signatures (bucket ordering); aliases the radix key arrays, which that path does not use
};
static inline bool sortws_carve(Arena &a, uint64_t n, SortWs &w)
{
    const bool ok = take(a, w.k0, n * 8) && take(a, w.k1, n * 8) && take(a, w.v0, n * 4) && take(a, w.v1, n * 4) && take(a, w.tmp, radix_sort_tmp_bytes(n));
    w.sig_tmp = (csv_sig *)w.k0;                         // k0 and k1 are carved back to back: 2 x align_up(8n, 256) >= 16n bytes
    return ok && (char *)w.k1 == (char *)w.k0 + align_up(n * 8, 256);
}

// depth chain of a shard whose tile ranges the scan did not leave: prefix maximum, ranges, and (the larger branch, taken after a
// readback) the reads ordered by position
struct DepthWs {
    int32_t *pmax; void *ptmp; uint64_t *ttmp;
    uint32_t *pos_g, *end_g; SortWs w;
};
static inline bool carve_depth(Arena &a, uint64_t n, uint32_t depth_len, DepthWs &d)
{
    return take(a, d.pmax, n * 4) && take(a, d.ptmp, prefix_max_tmp_bytes(n)) && take(a, d.ttmp, depth_tiles_tmp_bytes(depth_len)) &&
           take(a, d.pos_g, n * 4) && take(a, d.end_g, n * 4) && sortws_carve(a, n, d.w);
}

// interval DBSCAN on arrays in caller order: sortedness flag, the kernels' temporaries, and (unsorted input) the sorted copies
struct DbscanIvWs {
    unsigned int *flag; void *tmp;
    uint32_t *s_s, *e_s; SortWs w;
};
static inline bool carve_dbscan_iv(Arena &a, uint64_t n, DbscanIvWs &d)
{
    return take(a, d.flag, 256) && take(a, d.tmp, dbscan_tmp_bytes(n)) && take(a, d.s_s, n * 4) && take(a, d.e_s, n * 4) && sortws_carve(a, n, d.w);
}

// batched 1-D DBSCAN: the too-large flag, and for segments beyond the LDS kernel the sorted-window path's buffers
struct Dbscan1dWs {
    unsigned int *flag;
    uint32_t *ks; void *tmp; SortWs w;
};
static inline bool carve_dbscan1d(Arena &a, uint32_t max_seg_len, Dbscan1dWs &d)
{
    if (max_seg_len <= DBSCAN1D_MAX_SEG) { d = Dbscan1dWs(); return take(a, d.flag, 256); }
    return take(a, d.flag, 256) && take(a, d.ks, (size_t)max_seg_len * 4) && take(a, d.tmp, dbscan1d_big_tmp_bytes(max_seg_len)) && sortws_carve(a, max_seg_len, d.w);
}

// split order, nodes: the filter-passing primaries of every contig (at most one per record; the supplementary hashes likewise)
struct SplitNodesWs {
    unsigned int *d_nsupp = nullptr; uint32_t *blk = nullptr; void *es_tmp = nullptr;
    uint64_t *node_hash = nullptr, *d_supp = nullptr;
    uint32_t *node_rec = nullptr, *list = nullptr;
};
static inline bool carve_split_nodes(Arena &a, uint64_t n_blocks, uint64_t total_reads, SplitNodesWs &w)
{
    return take(a, w.d_nsupp, 256) && take(a, w.blk, (n_blocks + 1) * 4) && take(a, w.es_tmp, exclusive_sum_tmp_bytes(n_blocks + 1)) &&
           take(a, w.node_hash, total_reads * 8) && take(a, w.node_rec, total_reads * 4) && take(a, w.list, total_reads * 4) && take(a, w.d_supp, total_reads * 8);
}

// split order, epochs: bucket minima, the sorts' workspace, survivors, and the D survivors-only levels
struct SplitEpochsWs {
    uint32_t *minT = nullptr;
    SortWs w;
    csv_split_survivor *d_out = nullptr;
    unsigned long long *d_count = nullptr;       // [0] survivors; 32-bit set sizes from byte 64 on
    uint32_t *bitmap[SO_TAIL_MAX] = {nullptr, nullptr, nullptr}, *set[SO_TAIL_MAX + 1] = {nullptr, nullptr, nullptr, nullptr}, *prevrank = nullptr, *filter = nullptr;
    uint8_t *is_surv = nullptr;
};
static inline bool carve_split_epochs(Arena &a, uint64_t scratch, uint64_t n_sort, uint64_t n_nodes, int D, size_t bm_words, SplitEpochsWs &w)
{
    bool ok = take(a, w.minT, scratch + 16) && sortws_carve(a, n_sort, w.w) && take(a, w.d_out, n_nodes * sizeof(csv_split_survivor)) && take(a, w.d_count, 256);
    for (int j = 0; j < D; j++) ok = ok && take(a, w.bitmap[j], bm_words * 4) && take(a, w.set[j + 1], n_nodes * 4);
    if (D > 0) ok = ok && take(a, w.is_surv, n_nodes) && take(a, w.prevrank, n_nodes * 4) && take(a, w.filter, st_filter_bytes());
    return ok;
}

// the overlap-group chain of one call: staged intervals, the (segment, start) sort, SplitGroupsWs, and the block cleared by one memset
struct SgWs {
    SplitGroupsWs w;
    SortWs sw;
    int32_t *d_start = nullptr, *d_end = nullptr;
    uint64_t *d_seg = nullptr;
    char *zero = nullptr;                      // hist | cnt | keep | state | total, err: ONE slice, cleared together
    size_t zero_bytes = 0;
    void *es_tmp = nullptr;
};
static inline bool carve_split_groups(Arena &a, uint32_t n, uint64_t n_seg, SgWs &c)
{
    SplitGroupsWs &w = c.w;
    const size_t n4 = (size_t)n * 4, nb = (size_t)n / 64 * 4 + 4;
    const size_t z4 = align_up(((size_t)n + 1) * 4, 256), z1 = align_up((size_t)n, 256);       // sub-offsets inside `zero`
    c.zero_bytes = 3 * z4 + z1 + 256;
    const bool ok = take(a, c.d_start, n4) && take(a, c.d_end, n4) && take(a, c.d_seg, (n_seg + 1) * 8) && sortws_carve(a, n, c.sw) &&
                    take(a, w.ss, n4) && take(a, w.se, n4) && take(a, w.sid, n4) && take(a, w.posof, n4) && take(a, w.plo, n4) && take(a, w.lp1, n4) &&
                    take(a, w.cstart, n4) && take(a, w.cend, n4) && take(a, w.seed_of_group, n4) && take(a, w.pm, n4) &&
                    take(a, w.blk_min_id, nb) && take(a, w.blk_max_end, nb) && take(a, w.head, n) &&
                    take(a, w.group_off, ((size_t)n + 1) * 8) && take(a, w.seg_group_off, (n_seg + 1) * 8) && take(a, w.res, 256) &&
                    take(a, c.zero, c.zero_bytes) && take(a, c.es_tmp, exclusive_sum_tmp_bytes((uint64_t)n + 1));
    if (!ok) return false;
    char *z = c.zero;
    w.hist = (uint32_t *)z; w.cnt = (uint32_t *)(z + z4); w.keep = (uint32_t *)(z + 2 * z4);
    w.state = (uint8_t *)(z + 3 * z4);
    w.total = (unsigned long long *)(z + 3 * z4 + z1); w.err = (uint32_t *)(z + 3 * z4 + z1 + 64);
    return true;
}

// the fits' tables on the device. with_start_end false: start / end are the chain's own copies (set by the caller)
static inline bool carve_sf_tables(Arena &a, uint64_t nm, uint64_t ns, bool with_start_end, SplitFitsIn &in)
{
    bool ok = true;
    if (with_start_end) ok = take(a, in.start, nm * 4) && take(a, in.end, nm * 4);
    return ok && take(a, in.q_start, nm * 4) && take(a, in.q_end, nm * 4) && take(a, in.reverse, nm) && take(a, in.supp_off, (nm + 1) * 8) &&
           take(a, in.supp_start, ns * 4) && take(a, in.supp_end, ns * 4) && take(a, in.supp_q_start, ns * 4) && take(a, in.supp_q_end, ns * 4) && take(a, in.supp_flags, ns);
}

// one run of the fits: its records and counters, and (a set can exceed the LDS kernel: B > DBSCAN1D_MAX_SEG) the buffers of the
// large-set path
struct SfRunWs {
    csv_split_fit *d_out = nullptr;
    uint32_t *d_big_n = nullptr;
    unsigned long long *d_res = nullptr;
    int32_t *pts = nullptr, *ks = nullptr, *labels = nullptr; uint32_t *sizes = nullptr; void *tmp = nullptr; SortWs w;
};
static inline bool carve_sf_run(Arena &a, uint64_t G, uint64_t B, SfRunWs &r)
{
    const bool ok = take(a, r.d_out, G * sizeof(csv_split_fit)) && take(a, r.d_big_n, G * 6 * 4) && take(a, r.d_res, 256);
    if (B <= DBSCAN1D_MAX_SEG) return ok;
    return ok && take(a, r.pts, B * 4) && take(a, r.ks, B * 4) && take(a, r.labels, B * 4) && take(a, r.sizes, B * 4) &&
           take(a, r.tmp, dbscan1d_big_tmp_bytes(B)) && sortws_carve(a, B, r.w);
}

// record references into resident shards, as the tables' kernel reads them
static inline bool carve_sr_refs(Arena &a, uint64_t n_seg, uint64_t nm, uint64_t ns, SplitTablesIn &in)
{
    return take(a, in.seg, n_seg * sizeof(SplitTabSeg)) && take(a, in.member_rec, nm * 4) && take(a, in.supp_off, (nm + 1) * 8) &&
           take(a, in.supp_rec, ns * 4) && take(a, in.supp_where, ns);
}
// the arrays of SplitTablesOut behind start / end (which the caller places)
static inline bool sr_carve(Arena &a, uint64_t nm, uint64_t ns, SplitTablesOut &o)
{
    return take(a, o.q_start, nm * 4) && take(a, o.q_end, nm * 4) && take(a, o.reverse, nm) && take(a, o.supp_start, ns * 4) && take(a, o.supp_end, ns * 4) &&
           take(a, o.supp_q_start, ns * 4) && take(a, o.supp_q_end, ns * 4) && take(a, o.supp_flags, ns);
}

// shard scratch of one chromosome job: sorted signatures, SoA start / end, labels, sort + dbscan workspace
struct JobScratch {
    csv_sig *sig_sorted; uint32_t *st, *en; int32_t *labels;
    SortWs w; void *db_tmp;
};
static inline bool carve_job_scratch(Arena &a, uint64_t n, JobScratch &j)
{
    // + 16 on start / end / labels: the clustering kernels' 16-byte loads at the arrays' ends
    return take(a, j.sig_sorted, n * sizeof(csv_sig)) && take(a, j.st, n * 4 + 16) && take(a, j.en, n * 4 + 16) && take(a, j.labels, n * 4 + 16) &&
           sortws_carve(a, n, j.w) && take(a, j.db_tmp, dbscan_tmp_bytes(n));
}

// the slot replay of a batch (kernels/mergeselect.hip): n (length, index) entries in n_seg segments, the pair lists of the streamed rounds,
// the segments' offsets and slots, the answers, the lists of the segments that take a workgroup (17 members or more: at most n / 17 of them)
struct SortSlotWs {
    uint64_t *ent = nullptr;
    uint32_t *list = nullptr, *off = nullptr, *nth = nullptr, *idx = nullptr, *mid = nullptr, *big = nullptr;
    uint32_t *cnt = nullptr;            // [0] segments of the LDS form, [1] of the streaming form, [2] the segments in all
};
static inline bool carve_sort_slot(Arena &a, uint64_t n, uint64_t n_seg, SortSlotWs &w)
{
    const uint64_t wg = std::min(n_seg, n / 17);
    return take(a, w.ent, n * 8) && take(a, w.list, n * 4) && take(a, w.off, (n_seg + 1) * 4) && take(a, w.nth, n_seg * 4) && take(a, w.idx, n_seg * 4) &&
           take(a, w.mid, wg * 4) && take(a, w.big, wg * 4) && take(a, w.cnt, 256);
}

// mergeSVs' representatives of ONE type with n signatures (csvgpu_merge_select and its kin run it once per type over the same slices):
// the bucket sort, the head marks and the kept-bucket marks with their sums, and the slot replay of up to n buckets
struct MergeSelectWs {
    SortWs sw;
    SortSlotWs ss;
    uint32_t *head = nullptr, *keep = nullptr;
    void *es_tmp = nullptr;
};
static inline bool carve_merge_select(Arena &a, uint64_t n, MergeSelectWs &w)
{
    return sortws_carve(a, n, w.sw) && carve_sort_slot(a, n, n, w.ss) && take(a, w.head, (n + 1) * 4) && take(a, w.keep, (n + 1) * 4) &&
           take(a, w.es_tmp, exclusive_sum_tmp_bytes(n + 1));
}

// One contig's select, both types over the same slices: what the call reads back behind its kernels (the counts and the two bucket sorts'
// gave-up words: each sort reuses the other's workspace, so the words are copied here before the next sort clears them) and the records.
// This is the carve of a shard's select scratch (csv_shard::sel_scratch) and, for the host-fed call, of the context's workspace.
struct MergeBack {
    csv_merge_counts counts;
    uint32_t gave_up[2];
    uint32_t pad[6];
};
struct MergeRunWs {
    MergeSelectWs ms;
    MergeBack *back = nullptr;
    csv_merge_rep *rep = nullptr;
};
// records never exceed this: one per bucket of two or more, or a type's single signature passed through
static inline uint64_t merge_rep_bound(uint64_t n_del, uint64_t n_ins) { return (n_del < 2 ? n_del : n_del / 2) + (n_ins < 2 ? n_ins : n_ins / 2); }
static inline bool carve_merge_run(Arena &a, uint64_t n_del, uint64_t n_ins, MergeRunWs &w)
{
    return carve_merge_select(a, std::max(n_del, n_ins), w.ms) && take(a, w.back, 256) && take(a, w.rep, merge_rep_bound(n_del, n_ins) * sizeof(csv_merge_rep));
}

// region tables in, windows out (csvgpu_window_log2*)
struct WindowWs { uint32_t *rs, *re; int32_t *ss; uint64_t *wo; double *l2; uint32_t *ws, *we; };
static inline bool carve_window(Arena &a, uint64_t n_regions, uint64_t nw, WindowWs &w)
{
    return take(a, w.rs, n_regions * 4) && take(a, w.re, n_regions * 4) && take(a, w.ss, n_regions * 4) && take(a, w.wo, (n_regions + 1) * 8) &&
           take(a, w.l2, nw * 8) && take(a, w.ws, nw * 4) && take(a, w.we, nw * 4);
}

// What both copy-number routes carve behind their inputs, for R regions with W windows and S SNP records in all: the windows, the per-slot
// records, the answer sized by its bound W + 3 S (a position lies in at most three distinct keys) and, for the fused call, the Viterbi
// outputs. The regions' totals (sl.tot) are each route's own take, in front of this.
struct CnBack {
    double *l2 = nullptr; uint32_t *ws = nullptr, *we = nullptr;
    CnSlots sl{};
    CnObs o{};
    int32_t *states = nullptr; double *loglik = nullptr;
};
static inline bool carve_cn_back(Arena &a, uint64_t R, uint64_t W, uint64_t S, bool decode, CnBack &b)
{
    const uint64_t bound = W + 3 * S;
    const bool ok = take(a, b.l2, W * 8) && take(a, b.ws, W * 4) && take(a, b.we, W * 4) &&
                    take(a, b.sl.fw, W * 4) && take(a, b.sl.lw, W * 4) && take(a, b.sl.lo, W * 4) && take(a, b.sl.cnt, W * 4) && take(a, b.sl.off, W * 4) &&
                    take(a, b.sl.reg, W * 4) && take(a, b.o.obs_off, (R + 1) * 8) && take(a, b.o.pos, bound * 4) &&
                    take(a, b.o.baf, bound * 8 + 8) && take(a, b.o.pfb, bound * 8 + 8) && take(a, b.o.log2_cov, bound * 8 + 8) && take(a, b.o.is_snp, bound);
    if (!decode) return ok;
    return ok && take(a, b.states, bound * 4 + 8) && take(a, b.loglik, R * 8);
}

// the copy-number observations fed from host arrays (csvgpu_cn_observations_resident_many / _cn_decode_): the tables as they come up (`in`:
// one slice, one copy; the sub-arrays at CnInLayout's offsets), the regions' totals, and the back half
struct CnInLayout {
    size_t rs, re, ss, wo, wbase, soff, spos, sbaf, spfb, small, big, bytes;
    CnInLayout(uint64_t R, uint64_t n_shards, uint64_t S)
    {
        size_t o = 0;
        auto put = [&](size_t b) { const size_t at = o; o += align_up(b, 256); return at; };
        rs = put(R * 4); re = put(R * 4); ss = put(R * 4); wo = put((R + n_shards) * 8); wbase = put((R + 1) * 4); soff = put((R + 1) * 4);
        spos = put(S * 4); sbaf = put(S * 8); spfb = put(S * 8); small = put(R * 4); big = put(R * 4);
        bytes = o;
    }
};
struct CnWs {
    char *in = nullptr;
    void *es_tmp = nullptr;
    CnBack b;
};
static inline bool carve_cn_obs(Arena &a, uint64_t R, uint64_t W, uint64_t n_shards, uint64_t S, bool decode, CnWs &w)
{
    return take(a, w.in, CnInLayout(R, n_shards, S).bytes) && take(a, w.b.sl.tot, (R + 1) * 4) && take(a, w.es_tmp, exclusive_sum_tmp_bytes(R + 1)) &&
           carve_cn_back(a, R, W, S, decode, w.b);
}

// The same pass fed by resident SNP tables (csvgpu_cn_observations_tables_many / _cn_decode_tables_many). Carved twice over the same arena:
// first with W = 0 for what the plan needs (sized by R and the shards alone: `up`, one slice and one copy with the sub-arrays at CnUpLayout's
// offsets, the plan's arrays and the regions' totals), then, once the plan's totals are back, with W and S for the compact records and the
// back half behind them. The first part does not move when W and S change.
struct CnUpLayout {
    size_t rs, re, ssf, rsh, tabs, roff, bytes;
    CnUpLayout(uint64_t R, uint64_t n_shards)
    {
        size_t o = 0;
        auto put = [&](size_t b) { const size_t at = o; o += align_up(b, 256); return at; };
        rs = put(R * 4); re = put(R * 4); ssf = put(R * 4); rsh = put(R * 4); tabs = put(n_shards * sizeof(SnpTabDev)); roff = put((n_shards + 1) * 4);
        bytes = o;
    }
};
struct CnTabWs {
    char *up = nullptr;
    CnPlan p{};
    uint32_t *spos = nullptr; uint64_t *sbaf = nullptr, *spfb = nullptr;
    CnBack b;
};
static inline bool carve_cn_tables(Arena &a, uint64_t R, uint64_t n_shards, uint64_t W, uint64_t S, bool decode, CnTabWs &w)
{
    char *head = nullptr;
    const CnUpLayout L(R, n_shards);
    const bool ok = take(a, w.up, L.bytes) && take(a, head, CN_PLAN_HEAD_BYTES + (n_shards + 1) * 4) && take(a, w.p.ss, R * 4) && take(a, w.p.wo, (R + n_shards) * 8) &&
                    take(a, w.p.wbase, (R + 1) * 4) && take(a, w.p.soff, (R + 1) * 4) && take(a, w.p.sfirst, R * 4) && take(a, w.p.hit, R * 4) &&
                    take(a, w.p.small, R * 4) && take(a, w.p.big, R * 4) && take(a, w.p.es_tmp, exclusive_sum_tmp_bytes(R + 1)) && take(a, w.b.sl.tot, (R + 1) * 4);
    if (!ok) return false;
    w.p.rs = (const uint32_t *)(w.up + L.rs); w.p.re = (const uint32_t *)(w.up + L.re); w.p.ssf = (const int32_t *)(w.up + L.ssf);
    w.p.rsh = (const uint32_t *)(w.up + L.rsh); w.p.tabs = (const SnpTabDev *)(w.up + L.tabs); w.p.reg_off = (const uint32_t *)(w.up + L.roff);
    w.p.head = (CnPlanHead *)head; w.p.shard_w0 = (uint32_t *)(head + CN_PLAN_HEAD_BYTES);
    if (!W) return true;
    return take(a, w.spos, S * 4) && take(a, w.sbaf, S * 8) && take(a, w.spfb, S * 8) && carve_cn_back(a, R, W, S, decode, w.b);
}

// BGZF members inflated on the device (csvgpu_bgzf_inflate / _dev): the member table and the count of declined members, and for the
// host-pointer form (io) the compressed bytes, the decoded bytes and the status bytes
struct BgzfWs { csv_bgzf_block *blocks = nullptr; unsigned int *n_declined = nullptr; uint8_t *comp = nullptr, *out = nullptr, *status = nullptr; };
static inline bool carve_bgzf(Arena &a, uint64_t n_blocks, bool io, uint64_t comp_len, uint64_t out_len, BgzfWs &w)
{
    const bool ok = take(a, w.blocks, n_blocks * sizeof(csv_bgzf_block)) && take(a, w.n_declined, 256);
    if (!io) return ok;
    return ok && take(a, w.comp, comp_len) && take(a, w.out, out_len) && take(a, w.status, n_blocks);
}

// BAM records unpacked on the device (csvgpu_bam_unpack / _dev) from a stream of `len` bytes cut at n_anchors anchors: the head (counts,
// status, filter bounds), the anchors and their intervals' counts, every record's start and the kept records' counts — a record takes at
// least 36 bytes, which bounds them all before anything has run — and for the host-pointer form (io) the stream itself and the outputs,
// sized by the caller's capacities where those are below what the stream can hold (n_seq / n_name 0, hash false: not wanted)
static inline uint64_t bam_unpack_max_records(uint64_t len) { return len / 36; }
static inline bool carve_bam_unpack(Arena &a, uint64_t len, uint64_t n_anchors, bool io, uint64_t n_rec, uint64_t n_cigar, uint64_t n_seq, uint64_t n_name, bool hash,
                                    BamUnpackWs &w)
{
    const uint64_t R = bam_unpack_max_records(len);
    char *head = nullptr;
    const bool ok = take(a, head, 256) && take(a, w.anchors, n_anchors * 4) && take(a, w.count, (n_anchors + 1) * 4) && take(a, w.rec_off, R * 4) &&
                    take(a, w.cig_src, (R + 1) * 4) && take(a, w.cig_n, (R + 1) * 4) && take(a, w.seq_n, (R + 1) * 4) && take(a, w.name_n, (R + 1) * 4) &&
                    take(a, w.es_tmp, exclusive_sum_tmp_bytes(std::max(R, n_anchors) + 1));
    if (!ok) return false;
    w.res = (uint32_t *)head; w.status = (unsigned long long *)(head + BU_RES_WORDS * 4); w.bounds = (uint32_t *)(head + BU_RES_WORDS * 4 + 8);
    w.rec_cap = (uint32_t)R;
    w.bytes = nullptr; w.out = BamUnpackOut{};
    if (!io) return true;
    n_rec = std::min(n_rec, R); n_cigar = std::min(n_cigar, len / 4); n_seq = std::min(n_seq, len); n_name = std::min(n_name, len);
    bool k = take(a, w.bytes, len + 4) && take(a, w.out.pos, n_rec * 4) && take(a, w.out.flag, n_rec * 2) && take(a, w.out.mapq, n_rec) &&
             take(a, w.out.cigar_off, (n_rec + 1) * 8) && take(a, w.out.cigar, n_cigar * 4);
    if (n_seq) k = k && take(a, w.out.seq_off, (n_rec + 1) * 8) && take(a, w.out.seq, n_seq);
    if (n_name) k = k && take(a, w.out.name_off, (n_rec + 1) * 8) && take(a, w.out.name, n_name);
    if (hash) k = k && take(a, w.out.name_hash, n_rec * 8);
    return k;
}

// VCF lines parsed on the device (csvgpu_vcf_*_parse / _dev). The workspace is carved twice over the same arena: first with n_slots = 0
// (the head, the tiles' line-end counts, the AF form's strings: none of these moves when n_slots changes), then, once the line ends are
// counted, with n_slots = line ends + 1 for the per-line arrays and (io: the host-pointer form) the staged outputs, which hold at most one
// record per line and no more than the caller's capacities.
static inline bool carve_vcf(Arena &a, uint64_t n_tiles, uint64_t n_strings, uint64_t n_slots, bool io, bool af, uint64_t cap, uint64_t cap_defer, VcfWs &w)
{
    char *head = nullptr;
    const bool ok = take(a, head, 256) && take(a, w.tile_cnt, (n_tiles + 1) * 4) && take(a, w.es_tmp, exclusive_sum_tmp_bytes(n_tiles + 1)) && take(a, w.strings, n_strings);
    if (!ok) return false;
    w.head = (VcfHead *)head;
    w.out = VcfOut{};
    if (!n_slots) return true;
    bool k = take(a, w.line_start, n_slots * 4) && take(a, w.kept, (n_slots + 1) * 4) && take(a, w.defer, (n_slots + 1) * 4) && take(a, w.pos, n_slots * 4) &&
             take(a, w.chrom_len, n_slots * 4) && take(a, w.value, n_slots * 8) && take(a, w.code, n_slots) && take(a, w.es_tmp2, exclusive_sum_tmp_bytes(n_slots + 1));
    if (!io) return k;
    cap = std::min(cap, n_slots); cap_defer = std::min(cap_defer, n_slots);
    k = k && take(a, w.out.line_off, cap * 4) && take(a, w.out.pos, cap * 4) && take(a, w.out.value, cap * 8) && take(a, w.out.defer_off, cap_defer * 4);
    if (!af) k = k && take(a, w.out.chrom_len, cap * 4);
    return k;
}
// the host-pointer form's inputs: the text (+ 16: the last aligned 16-byte piece) and the AF form's positions
static inline bool carve_vcf_text(Arena &a, uint64_t len, uint64_t n_sorted, VcfTextWs &w)
{
    return take(a, w.text, len + 16) && take(a, w.sorted_pos, n_sorted * 4);
}

// ---- the kernels' own temporaries (one opaque `tmp` to their callers)----------------------------------------------------------------
// dbscan.hip: core u8[n] | parent u32[n] | root_of u32[n] | is_root/cid u32[n+1] | scan tmp | tile counts, prefixes | ticket
struct DbscanTmp {
    uint8_t *core; uint32_t *parent, *root_of, *cid; void *es_tmp;
    uint32_t *tile_count, *tile_prefix; unsigned int *ticket;
    uint32_t n_tiles;                            // tiles of positions 0..n (rank[n] included)
};
static inline bool carve_dbscan_tmp(Arena &a, uint64_t n, uint64_t uf_tile, DbscanTmp &t)
{
    t.n_tiles = (uint32_t)((n + uf_tile) / uf_tile);
    return take(a, t.core, n) && take(a, t.parent, n * 4) && take(a, t.root_of, n * 4) && take(a, t.cid, (n + 1) * 4) && take(a, t.es_tmp, exclusive_sum_tmp_bytes(n + 1)) &&
           take(a, t.tile_count, ((uint64_t)t.n_tiles + 1) * 4) && take(a, t.tile_prefix, ((uint64_t)t.n_tiles + 1) * 4) && take(a, t.ticket, 256);
}
// hmm.hip: the model in device form | emission logs f64[6 n_obs] | back-pointers u8[6 n_obs]
struct ViterbiTmp { void *model; double *biot; uint8_t *psi; };
static inline bool carve_viterbi_tmp(Arena &a, uint64_t n_obs, size_t model_bytes, ViterbiTmp &t)
{
    return take(a, t.model, model_bytes) && take(a, t.biot, n_obs * 6 * sizeof(double)) && take(a, t.psi, n_obs * 6);
}

}  // namespace csv
