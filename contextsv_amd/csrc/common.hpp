// common.hpp — internals shared by the gfx950 kernels and the C-ABI glue (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/csvgpu.h"
#include "arena.hpp"

namespace csv {

constexpr int WAVE = 64;   // gfx950 wavefront

// BAM CIGAR op codes and flags (SAM spec §4.2)
enum : uint32_t { OP_M = 0, OP_I = 1, OP_D = 2, OP_N = 3, OP_S = 4, OP_H = 5, OP_P = 6, OP_EQ = 7, OP_X = 8 };
enum : uint32_t { F_UNMAP = 0x4, F_SECONDARY = 0x100, F_QCFAIL = 0x200, F_DUP = 0x400, F_SUPP = 0x800 };
constexpr uint32_t REF_OPS = (1u << OP_M) | (1u << OP_D) | (1u << OP_N) | (1u << OP_EQ) | (1u << OP_X);   // consume reference
constexpr uint32_t QRY_OPS = (1u << OP_M) | (1u << OP_I) | (1u << OP_S) | (1u << OP_EQ) | (1u << OP_X);   // consume query
constexpr uint32_t ALN_OPS = (1u << OP_M) | (1u << OP_EQ) | (1u << OP_X);                                  // count toward depth
// words allocated behind an uploaded shard's CIGAR array, so that the kernels' 1 KiB chunk loads never need a bounds test
constexpr uint32_t CIGAR_PAD_WORDS = 512;
constexpr uint32_t GAP_OPS = REF_OPS & ~ALN_OPS;                                                             // D, N: on the reference, not in the depth
constexpr uint32_t QST_OPS = (1u << OP_M) | (1u << OP_I) | (1u << OP_EQ) | (1u << OP_X);                   // open the query interval

// ---------------------------------------------------------------------------------------------
// context

struct Timer {
    hipEvent_t a, b;
    int id;
    hipStream_t s;
    bool own_a = true, own_b = true;   // returned to the event pool when the timer is folded (an event may close one group and open the next)
};

}  // namespace csv

// turn-taking of the bandwidth-bound phases of several contexts on one device (csvgpu_gate_*)
struct csv_gate {
    std::mutex  mu;                     // held while a context queues its scan + depth pair
    hipStream_t stream = nullptr;       // the ONE stream the attached contexts' big kernels run on, back to back
    int         device = -1;
};

struct csv_ctx {
    int          device = 0;
    hipStream_t  stream = nullptr;
    hipStream_t  side = nullptr;            // carries the counters to the host beside the depth pass (jobs)
    bool         own_stream = false;
    csv::Arena   arena;                     // staged inputs / outputs of the host-pointer entry points
    csv::Arena   work;                      // workspace sized after the signature count is known
    void        *pinned = nullptr;          // small pinned host block for scalar read-backs
    size_t       pinned_cap = 0;
    int          timing = 0;                // 0 off, 1 every kernel group, 2 only the two bandwidth-bound groups (scan, depth)
    uint32_t     timer_tick = 0;            // jobs seen by the pair timers (level 2 times every fourth pair on a gate's stream)
    std::vector<csv::Timer> timers;         // recorded, not yet folded
    std::vector<hipEvent_t> event_pool;
    double       t_ms[CSV_K_COUNT] = {0};
    uint64_t     t_n[CSV_K_COUNT] = {0};
    std::string  err;
    int          n_cu = 256;
    // csvgpu_host_alloc / csvgpu_host_free: page-locking is slow (hundreds of microseconds), so freed blocks are kept for reuse
    std::vector<std::pair<void *, size_t>> host_live, host_pool;
    csv_gate    *gate = nullptr;
    char        *job_pin = nullptr;         // page-locked counter slots of the jobs in flight (csvgpu_chr_job_*)
    size_t       job_pin_next = 0;
    uint32_t     job_pin_busy = 0;          // bit i: slot i belongs to a job between begin and end / abort
    struct csv_split_state *split_state = nullptr;   // between csvgpu_split_order_begin and _finish
    csv_tuning   tuning = CSV_TUNING_DEFAULTS;      // csvgpu_set_tuning
    int          cigar_packing = 1;                 // csvgpu_set_cigar_packing: read when a shard is uploaded
};

struct csv_shard {
    csv_reads d;                   // device pointers
    uint32_t  depth_len = 0;
    bool      owned = false;       // true: arrays hipMalloc'd by csvgpu_shard_upload
    uint32_t  cigar_pad = 0;       // allocated (zeroed) words behind d.cigar[n_cigar]: CIGAR_PAD_WORDS for the library's own uploads, 0 for wrapped arrays
    // The 16-bit form (cigar_pack_core.hpp) of an uploaded wave-form shard: then d.cigar is null and these hold the ops. half: the halfwords,
    // allocated to the end of the last 512-op piece + CIGAR_PAD_WORDS zeroed halfwords; esc_piece [n_pieces + 1]; esc_tab [n_esc + 1].
    uint16_t *cig_half = nullptr;
    uint32_t *esc_piece = nullptr;
    uint64_t *esc_tab = nullptr;
    uint64_t  n_esc = 0;
    int       unsorted = -1;       // pos[] not non-decreasing: 1 / 0, or -1 while unknown (wrapped device arrays before their first scan)
    // per-read side arrays + per-chromosome outputs (device, owned by the shard)
    int32_t  *ref_end = nullptr, *q_start = nullptr, *q_end = nullptr, *pmax_end = nullptr;
    uint32_t *ckpt = nullptr;      // per-256-word reference checkpoints (scan -> depth)
    uint32_t *depth = nullptr;
    csv_sig  *sig_raw = nullptr;   uint64_t sig_cap = 0;
    csv_sig  *sig_sorted = nullptr;
    int32_t  *labels = nullptr;
    uint32_t *ord = nullptr;       // read permutation by pos when the shard is not coordinate-sorted
    char     *scratch = nullptr;   size_t scratch_cap = 0;   // sort / dbscan workspace
    char     *sel_scratch = nullptr; size_t sel_cap = 0;     // the representative select's workspace (carve_merge_run; grow-only, allocated at its first use)
    uint64_t *counters = nullptr;  // device scalars (see ScanCounters) + bucket tables + the depth tiles' candidate ranges, zeroed together per chromosome
    uint64_t *tile_range = nullptr;   // inside `counters`
    uint64_t *scan_split = nullptr;   // the scan's work split for this device's grid (launch_scan_split, once per shard)
    int       form = 0;               // SCAN_FORM_*: the creating context's forced form, or chosen from the mean CIGAR words per read, when the shard is created
    void     *depth_items = nullptr;  // depth_items_bytes(depth_len): the depth tiles' work lists (depth.hip)
    uint64_t *qhash = nullptr;        // [n_reads] std::hash<std::string> of every record's query name (csvgpu_shard_set_qname_hash), or null
    size_t    counters_bytes = 0;
    // a shard built on the device (csvgpu_shard_builder_finish) also owns what the builder kept beside the reads; null / 0 otherwise
    uint64_t *seq_off = nullptr;      // [n_reads + 1] with seq [n_seq]: 4-bit packed sequences, (l_seq + 1) / 2 bytes a record (until csvgpu_shard_drop_sequences)
    uint8_t  *seq = nullptr;
    uint64_t *name_off = nullptr;     // [n_reads + 1] with name [n_name]: query names, no terminator
    uint8_t  *name = nullptr;
    uint64_t  n_seq = 0, n_name = 0;
};

// one contig's SNP records in device memory (csvgpu_snp_table_*): immutable once created, readable from every context of its device.
// One block: pos u32[n] | baf f64[n] | pfb f64[n] (per-record kind) | af_pos u32[n_af] | af f64[n_af] (first-hit kind), each 256-byte aligned.
struct csv_snp_table {
    int       device = 0;
    bool      hits = false;        // the first-hit kind
    uint64_t  n = 0, n_af = 0;
    char     *block = nullptr;
    const uint32_t *pos = nullptr, *af_pos = nullptr;
    const uint64_t *baf = nullptr, *pfb = nullptr, *af = nullptr;      // values as their bits
};

// a reference genome's bases in device memory (csvgpu_genome_*, api/fasta.hip; read by csvgpu_vcf_format, api/vcf_format.hip): immutable once
// built, readable from every context of its device. 16 spare bytes lie behind seq[total).
struct csv_genome_rec { uint64_t start; uint32_t len; uint64_t name_off; uint32_t name_len; };
struct csv_genome {
    int device = 0;
    char *seq = nullptr;
    uint64_t total = 0;                              // bases that belong to a record: seq[0 .. total)
    std::vector<csv_genome_rec> rec;                 // file order, one per named header
    std::string names;
    uint64_t n_text = 0, n_lines = 0;
};

namespace csv {

// device scalars written by the scan / depth kernels, read back once per chromosome
struct ScanCounters {
    // The three counters that every workgroup of a big kernel adds to sit in cache lines of their own: same-address device atomics
    // retire one after the other, and a workgroup's epilogue waits for its slot reservation on n_sig (returning) behind whatever
    // else is queued on that line.
    unsigned long long n_sig;        // all emitted signatures
    char               pad0[56];
    unsigned long long n_del;        // kind == DEL
    char               pad1[56];
    unsigned long long depth_sum;
    char               pad2[56];
    unsigned int       depth_nonzero;
    unsigned int       max_start;    // 0xffffffff if a signature start exceeded scan_start_limit(depth_len), else 0
    unsigned int       max_len;      // largest bucket of the ordering pass's most-significant-digit split if above BK_LOCAL_MAX, else 0 (scan epilogue)
    unsigned int       unsorted;     // != 0 if pos[] is not non-decreasing
    int                min_pts;      // written by the min_pts kernel
    int                pad;
    double             mean_cov;
    char               pad3[32];
};
static_assert(sizeof(ScanCounters) == 256, "the counters head the 256-byte block in front of the bucket tables");


#define CSV_HIP(ctx, call)                                                                       \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_);                      \
            return CSV_EHIP;                                                                     \
        }                                                                                        \
    } while (0)

int   arena_reserve(csv_ctx *ctx, Arena &a, size_t bytes);       // grow (sync + realloc) if needed, then reset
bool  timer_begin(csv_ctx *ctx, int id, hipStream_t s = nullptr);   // false: not recorded (timing off, or a group outside the selected level); s: the stream the group runs on (default: the context's)
void  timer_end(csv_ctx *ctx);
int   ensure_pinned(csv_ctx *ctx, size_t bytes);

struct TimerScope {
    csv_ctx *c;
    bool on;
    TimerScope(csv_ctx *ctx, int id, hipStream_t s = nullptr) : c(ctx), on(timer_begin(c, id, s)) {}
    ~TimerScope() { if (on) timer_end(c); }
};

static inline int bits_of(uint64_t x) { int b = 0; while (x) { b++; x >>= 1; } return b; }

// ---------------------------------------------------------------------------------------------
// launchers implemented in kernels/*.hip (all asynchronous on `s`)

// scan.hip
// What the scan can produce on the side for the passes behind it, so that nothing small has to run between the big kernels:
struct ScanExtras {
    uint64_t *tile_range = nullptr;   // [2 * n_tiles], zeroed: candidate read range of every depth tile (see DEPTH_TILE below); coordinate-sorted shards only
    uint32_t  n_tiles = 0;
    uint32_t *bucket_hist = nullptr;  // [BK_N], zeroed: counts of the ordering pass's most-significant-digit buckets; a bucket above BK_LOCAL_MAX is reported in cnt->max_len
    int       type_pos = -1, bucket_shift = 0;
};
// Forms of the scan (and of the depth pass's walk): a wave per read (long reads), or groups of 16 / 8 lanes per read (short reads)
enum { SCAN_FORM_WAVE = CSV_FORM_WAVE, SCAN_FORM_ROWS16 = CSV_FORM_ROWS16, SCAN_FORM_ROWS8 = CSV_FORM_ROWS8, SCAN_FORM_LANES = CSV_FORM_LANES };      // (LANES: the scan walks a read per lane; the depth walk takes groups of 16)
// the 16-bit form of a shard's CIGAR array as the two big kernels see it (null half: the shard is at 32 bits and d.cigar holds the words)
struct CigarPack {
    const uint16_t *half = nullptr;
    const uint32_t *piece = nullptr;
    const uint64_t *tab = nullptr;
};
// A set of reads on the device as the scan and the depth pass see it: what both kernels read of one shard, and how to read it. Made by
// shard_view (a resident shard) and stage_reads (a host-pointer call's staged arrays), nowhere else. What the two launchers rely on:
//  - form is what scan_form chose for (n_reads, n_cigar): with 2^32 - 1 ops or more that is SCAN_FORM_WAVE whatever was asked for (the
//    short-read forms index words in 32 bits), so neither launcher tests n_cigar again; a scan's `split` was built for this form.
//  - cigar_pad counts the zeroed elements allocated behind the op array, in that array's own unit, and means nothing without it.
//  - pack.half != nullptr (the 16-bit form) means d.cigar == nullptr, form == SCAN_FORM_WAVE, and a pad of cigar_pad halfwords behind the
//    END OF THE LAST 512-OP PIECE (the allocation and why it covers every load of both kernels: shard_pack_cigar in api/shard.hip);
//    otherwise d.cigar holds the 32-bit words, with cigar_pad words behind d.cigar[n_cigar], and pack is all null.
struct ReadsView {
    csv_reads     d;                   // device pointers
    CigarPack     pack;
    uint32_t      cigar_pad = 0;
    int           form = SCAN_FORM_WAVE;
    int32_t      *ref_end = nullptr, *q_start = nullptr, *q_end = nullptr;      // per read: the scan writes them, the depth pass reads ref_end
    uint32_t     *ckpt = nullptr;      // ckpt_bytes(n_cigar): the scan's reference-offset checkpoints, where the depth pass starts its walks
    ScanCounters *cnt = nullptr;
};
// what varies from one launch to the next on the same view
struct ScanArgs {
    uint32_t        depth_len, min_oplen, min_mapq;
    int             emit;              // 0: the per-read arrays and the checkpoints only
    csv_sig        *sig_out;
    uint64_t        sig_cap;
    ScanExtras      extras;
    const uint64_t *split;             // launch_scan_split's table for the same n_cu, shard and form, or null
};
struct DepthArgs {
    uint32_t        depth_len;
    uint32_t       *depth;
    const uint32_t *ord;               // null: the reads are coordinate-sorted; otherwise the tile ranges index `ord`
    const uint64_t *tile_range;
    void           *items;             // depth_items_bytes(depth_len) of scratch for the tiles' work lists, or null: every tile builds its own
};
int scan_form_for(uint64_t n_reads, uint64_t n_cigar);          // by mean CIGAR words per read: SCAN_FORM_WAVE or SCAN_FORM_ROWS16
void launch_cigar_scan(hipStream_t s, int n_cu, const ReadsView &v, const ScanArgs &a);
size_t scan_split_bytes(int n_cu, uint64_t n_reads, int form);
void launch_scan_split(hipStream_t s, int n_cu, const csv_reads &d, uint64_t *split, int form);      // once per resident shard
void launch_validate_offsets(hipStream_t s, const uint64_t *cigar_off, uint64_t n_reads, uint64_t n_cigar, uint64_t max_words, uint32_t *bad /* zeroed; set to 1 */);
uint32_t scan_start_limit(uint32_t depth_len);   // exclusive bound on signature starts that the ordering keys are sized for
// depth.hip
void launch_prefix_max(hipStream_t s, const int32_t *in, int32_t *out, uint64_t n, void *tmp /* >= 4 KiB + n/1024*4 */);
size_t prefix_max_tmp_bytes(uint64_t n);
// One workgroup of the depth pass owns DEPTH_TILE positions. tile_range[2t] = ~(first candidate read), tile_range[2t + 1] = one past
// the last: all-zero means "no read" and both halves are maintained with atomicMax, by the scan itself (ScanExtras) or by
// launch_depth_ranges.
constexpr int DEPTH_TILE_SHIFT = 14, DEPTH_TILE = 1 << DEPTH_TILE_SHIFT;
static inline uint32_t depth_n_tiles(uint32_t depth_len) { return (uint32_t)(((uint64_t)depth_len + DEPTH_TILE - 1) / DEPTH_TILE); }
size_t depth_tiles_tmp_bytes(uint32_t depth_len);
// ranges from a prefix maximum of the read ends, for shards whose ranges the scan did not produce (unsorted: in `ord` order)
void launch_depth_ranges(hipStream_t s, const int32_t *pos_s, const int32_t *pmax_end, uint64_t n_reads, uint32_t depth_len, uint64_t *tile_range);
// v.ckpt: reference offset of the owning read at every CKPT_WORDS-word CIGAR boundary (written by launch_cigar_scan); v.form: how the tiles walk their items
size_t depth_items_bytes(uint32_t depth_len);
void launch_depth_tiles(hipStream_t s, const ReadsView &v, const DepthArgs &a);
// cigarpack.hip: the 16-bit form made and undone on the device (cigar_pack_core.hpp has the rule)
void launch_cigar_esc_count(hipStream_t s, const uint32_t *cigar, uint64_t n_cigar, uint32_t *piece /* [n_pieces + 1]: escapes per piece, 0 last */);
void launch_cigar_pack(hipStream_t s, const uint32_t *cigar, uint64_t n_cigar, const uint32_t *piece /* exclusive sums */, uint16_t *half, uint64_t *tab);
void launch_cigar_unpack(hipStream_t s, const CigarPack &pack, uint64_t first, uint64_t n, uint32_t *out);      // ops [first, first + n)
// reference-offset checkpoints every CKPT_WORDS CIGAR words (scan.hip writes them, depth.hip starts its walks from them)
constexpr int CKPT_SHIFT = 6, CKPT_WORDS = 1 << CKPT_SHIFT;
static inline size_t ckpt_bytes(uint64_t n_cigar) { return ((n_cigar >> CKPT_SHIFT) + 2) * sizeof(uint32_t); }
void launch_min_pts(hipStream_t s, ScanCounters *cnt, double min_pts_pct);
void launch_depth_lookup(hipStream_t s, const uint32_t *depth, uint32_t depth_len, const uint32_t *pos, uint64_t n, int32_t *out);
// sort.hip
size_t radix_sort_tmp_bytes(uint64_t n);
// stable LSD sort of (key,val) pairs by whole 8-bit digits: key bits [0, 8 * ceil(key_bits / 8)). No pass masks its digit, so bits at
// and above key_bits inside the last digit take part in the order (every caller passes keys below 2^key_bits); bits above the last
// digit do not, and all 64 bits travel with the key. Both buffer pairs are clobbered; returns 1 when the
// result is in keys_out/vals_out, 0 when it is in keys_in/vals_in (even number of passes). onesweep: one launch per pass where n and
// key_bits allow it, else (and with onesweep == false) histogram, table scan and scatter per pass — the same order bit for bit.
int  launch_radix_sort_u64(hipStream_t s, uint64_t *keys_in, uint32_t *vals_in, uint64_t *keys_out, uint32_t *vals_out,
                           uint64_t n, int key_bits, void *tmp, bool onesweep);
// (onesweep passes only: the other passes size their table from a count the host knows)
int  launch_radix_sort_u64_devn(hipStream_t s, uint64_t *keys_in, uint32_t *vals_in, uint64_t *keys_out, uint32_t *vals_out, uint64_t n_bound,
                                const uint32_t *n_dev, int key_bits, void *tmp);
// The word (device memory inside `tmp`) that a one-launch pass sets when its bounded look-back gave up — the order is then wrong and the caller
// must fail (CSV_EHIP); nullptr when the sort with these arguments takes the three-launch passes, which cannot give up.
const uint32_t *radix_sort_gave_up(const void *tmp, uint64_t n, int key_bits, bool onesweep);
// bucket ordering: BK_N most-significant-digit buckets + one wave ranking each bucket; see sort.hip
constexpr uint32_t BK_BITS = 14, BK_N = 1u << BK_BITS, BK_LOCAL_MAX = 2048;
// (the bucket counts come from the scan: ScanExtras::bucket_hist)
void launch_bucket_sort(hipStream_t s, const csv_sig *sig_raw, uint64_t n, int type_pos, int shift, uint32_t *off /* the scan's bucket counts */, uint32_t *cur,
                        csv_sig *tmp, csv_sig *sig_sorted, uint32_t *start_out, uint32_t *end_out);
void launch_sig_make_keys(hipStream_t s, const csv_sig *sig, uint64_t n, int len_bits, int type_bit_pos,
                          uint64_t *keys, uint32_t *vals);
void launch_sig_fix_ties_gather(hipStream_t s, const csv_sig *sig_raw, const uint64_t *keys, const uint32_t *vals,
                                uint64_t n, csv_sig *sig_sorted, uint32_t *start_out, uint32_t *end_out);
void launch_iota_keys_u32(hipStream_t s, const uint32_t *k32, uint64_t n, uint64_t *keys, uint32_t *vals);
void launch_iota_keys_i32(hipStream_t s, const int32_t *k32, uint64_t n, uint64_t *keys, uint32_t *vals);   // order-preserving bias
void launch_check_sorted_u32(hipStream_t s, const uint32_t *k, uint64_t n, unsigned int *flag);
void launch_gather_u32(hipStream_t s, const uint32_t *src, const uint32_t *idx, uint64_t n, uint32_t *dst);
void launch_gather3_u32(hipStream_t s, const uint32_t *a, const uint32_t *b, const uint32_t *c, const uint32_t *idx, uint64_t n, uint32_t *da, uint32_t *db, uint32_t *dc);
void launch_exclusive_sum_u32(hipStream_t s, uint32_t *data, uint64_t n, void *tmp);   // in place
size_t exclusive_sum_tmp_bytes(uint64_t n);
// mergeselect.hip — which element libstdc++'s std::sort by length descending leaves at a slot, for a batch of segments (sort_select_core.hpp)
constexpr uint32_t SORT_SLOT_LDS_CAP = 4096;             // the largest range a workgroup replays in LDS
struct SortSlotArgs {                                    // passed to the kernels by value
    const uint32_t *off;        // [n_seg + 1] first entry of each segment
    const uint32_t *n_seg;      // the segments, a device scalar (mergeSVs' buckets are counted on the device)
    const uint32_t *nth;        // [n_seg] the slots, or nullptr: mergeSVs' slot of the segment's size, [max(1, (int)(sz * 0.2)) / 2]
    uint64_t *ent;              // [n] (length << 32) | index, in segment order; permuted inside the segments
    uint32_t *list;             // [n] scratch of the streamed rounds
    uint32_t *mid, *big, *cnt;  // the segments that take a workgroup, by form (at most n / 17 each), and cnt[0], cnt[1] how many
    uint32_t *idx;              // [n_seg] the chosen index; 0xffffffff for an empty or a declined segment
    uint32_t *keep;             // [n_seg] 1 where the segment has two members or more, or nullptr
    uint32_t max_partitions;    // 0: the library's own depth limit
};
// n: the entries in all, n_seg_bound: an upper bound of *b.n_seg (the grids are sized by them)
void launch_sort_slot(hipStream_t s, const SortSlotArgs &b, uint64_t n, uint64_t n_seg_bound);
struct MergeEmitArgs {
    const uint32_t *off, *n_buckets;
    const uint64_t *keys;       // sorted: slot = label + 2
    const uint32_t *idx, *keep;
    const csv_sig *sig;
    int type;                   // 0 DEL, 1 INS: the INS records go behind counts->n_rep[0]
    csv_merge_counts *counts;
    csv_merge_rep *rep;
    uint64_t capacity;
};
struct MergeSelectWs;
// One type's representatives behind whatever is queued: buckets by label (one radix sort), the slot replay, one record per bucket of two or
// more in slot order — or the type's 0 or 1 signatures passed through. key_bits: the bits of the largest slot (label + 2). *gave_up: the sort's flag to read back (radix_sort_gave_up), or nullptr.
void launch_merge_select_type(hipStream_t s, const MergeSelectWs &w, const csv_sig *sig, const int32_t *label, uint64_t n, int type, int key_bits,
                              uint32_t max_partitions, bool onesweep, csv_merge_counts *counts, csv_merge_rep *rep, uint64_t capacity, const uint32_t **gave_up);
// dbscan.hip
size_t dbscan_tmp_bytes(uint64_t n);
// s,e sorted by start; oid = original index of each sorted position (nullptr: identity).
// min_pts read from *d_min_pts when d_min_pts != nullptr, else the immediate.
// split: positions [0,split) and [split,n) are two independent sets clustered side by side (split == n: one set;
// only honoured when oid == nullptr).
void launch_dbscan_iv_sorted(hipStream_t s, const uint32_t *start, const uint32_t *end, const uint32_t *oid,
                             uint64_t n, uint64_t split, double eps, int min_pts, const int *d_min_pts, int32_t *labels, void *tmp);
// many small sets (caller order, at most DBSCAN_IV_SMALL_MAX points each: larger segments are skipped) in one launch, one workgroup per set
constexpr uint32_t DBSCAN_IV_SMALL_MAX = 2048;
void launch_dbscan_iv_small_batched(hipStream_t s, const uint32_t *start, const uint32_t *end, const uint64_t *seg_off, uint64_t n_seg, double eps,
                                    int min_pts, int32_t *labels, bool all_pairs /* the kernel that tests every pair instead of the start-ordered one: same labels */);
// splitorder.hip — the node order of the reference's per-chromosome qname hash map, all contigs of a batch per launch
constexpr uint32_t SO_MAX_CONTIGS = 32;
struct SplitOrderTab {                       // passed to the kernels by value
    uint32_t A = 0;                          // contigs in this table
    uint64_t blk_off[SO_MAX_CONTIGS + 1];    // compaction: first 1024-record block of each contig
    uint64_t work_off[SO_MAX_CONTIGS + 1];   // epoch: first work item (node present in the epoch) of each active contig
    uint32_t nbase[SO_MAX_CONTIGS + 1];      // global index of each contig's first node
    uint64_t rev_off[SO_MAX_CONTIGS];        // epoch: work items of the active contigs BEHIND this one (the sort key's contig part)
    uint32_t m_old[SO_MAX_CONTIGS];          // epoch: nodes that were in the list when the epoch began (the rest were inserted during it)
    uint64_t n_reads[SO_MAX_CONTIGS];
    const uint16_t *flag[SO_MAX_CONTIGS];
    const uint8_t *mapq[SO_MAX_CONTIGS];
    const uint64_t *qhash[SO_MAX_CONTIGS];
};
struct csv_split_survivor { uint32_t contig, pos, rec; };
void launch_so_count(hipStream_t s, const SplitOrderTab &tab, uint32_t n_blocks, uint32_t min_mapq, uint32_t *blk_cnt);
void launch_so_scatter(hipStream_t s, const SplitOrderTab &tab, uint32_t n_blocks, uint32_t min_mapq, const uint32_t *blk_off, uint64_t *node_hash,
                       uint32_t *node_rec);
void launch_so_mint(hipStream_t s, const SplitOrderTab &tab, uint64_t M, uint32_t B, const uint64_t *node_hash, const uint32_t *list, uint32_t *minT);
void launch_so_keys(hipStream_t s, const SplitOrderTab &tab, uint64_t M, uint32_t B, int w, const uint64_t *node_hash, const uint32_t *list,
                    const uint32_t *minT, uint64_t *keys, uint32_t *vals);
void launch_so_setlist(hipStream_t s, const SplitOrderTab &tab, uint64_t M, const uint32_t *vals, uint32_t *list);
void launch_so_survivors(hipStream_t s, const SplitOrderTab &tab, uint64_t n_nodes, const uint64_t *node_hash, const uint32_t *node_rec, const uint32_t *list,
                         const uint64_t *supp_hash, uint64_t n_supp, csv_split_survivor *out, uint64_t cap, unsigned long long *count);
// the first epochs (while nodes and buckets fit the LDS) in one launch, one workgroup per contig
constexpr uint32_t SO_SMALL_B = 5087, SO_SMALL_EPOCHS = 12;
struct SplitSmallHost {
    uint32_t A = 0, n_epochs = 0;
    uint32_t nbase[SO_MAX_CONTIGS + 1] = {0};
    int32_t  k_last[SO_MAX_CONTIGS] = {0};
    uint32_t first[SO_SMALL_EPOCHS + 1] = {0};
    uint32_t B[SO_SMALL_EPOCHS] = {0};
};
void launch_so_small_epochs(hipStream_t s, const SplitSmallHost &h, const uint64_t *node_hash, uint32_t *list);
// the last epochs for the survivors only (splitorder.hip): level j = the contig's last epoch minus j
constexpr uint32_t SO_TAIL_MAX = CSV_TAIL_MAX;
struct SplitTailHost {
    uint32_t A = 0, D = 0;
    int      wv = 0, wa = 0;
    uint32_t nbase[SO_MAX_CONTIGS + 1] = {0};
    uint32_t B[SO_TAIL_MAX][SO_MAX_CONTIGS] = {{0}};
    uint32_t F[SO_TAIL_MAX][SO_MAX_CONTIGS] = {{0}};
    uint32_t boff[SO_TAIL_MAX][SO_MAX_CONTIGS + 1] = {{0}};
};
size_t st_filter_bytes();
void launch_st_survivors(hipStream_t s, const SplitTailHost &h, uint32_t n_nodes, const uint64_t *node_hash, const uint64_t *supp_hash, uint64_t n_supp, uint32_t *filter /* st_filter_bytes(), zeroed */,
                         uint8_t *is_surv, uint32_t *bitmap);
void launch_st_member(hipStream_t s, const SplitTailHost &h, uint32_t n_nodes, int j, const uint64_t *node_hash, const uint32_t *bitmap_prev, uint32_t *bitmap_next,
                      uint32_t *set, unsigned int *count);
void launch_st_inverse(hipStream_t s, const SplitTailHost &h, uint32_t n_nodes, int j_last, const uint32_t *list, uint32_t *prevrank);
void launch_st_mint(hipStream_t s, const SplitTailHost &h, int j, const uint32_t *set, uint32_t n, const uint32_t *n_dev, const uint64_t *node_hash, const uint32_t *prevrank,
                    uint32_t *minT);
void launch_st_keys(hipStream_t s, const SplitTailHost &h, int j, const uint32_t *set, uint32_t n, const uint32_t *n_dev, const uint64_t *node_hash, const uint32_t *prevrank,
                    const uint32_t *minT, uint64_t *keys, uint32_t *vals);
void launch_st_rank(hipStream_t s, const uint32_t *vals, uint32_t n, const uint32_t *n_dev, uint32_t *prevrank);
void launch_st_emit(hipStream_t s, const SplitTailHost &h, const uint32_t *vals, uint32_t n, const uint32_t *n_dev, const uint8_t *is_surv, const uint32_t *node_rec,
                    csv_split_survivor *out, uint64_t cap, unsigned long long *count);
void launch_so_supp(hipStream_t s, const SplitOrderTab &tab, uint32_t n_blocks, uint32_t min_mapq, uint64_t *supp_hash, unsigned int *count);
// splitgroups.hip — the overlap groups that the split order seeds (interval tree + greedy seeding of the reference), all segments of a call per launch
struct SplitGroupsWs {                       // device arrays of one call, n = members of the call
    int32_t  *ss, *se;                       // [n] start / end by position in the (segment, start, rank) order
    uint32_t *sid, *posof, *plo, *lp1;       // [n] position -> member, member -> position, position -> first position of its segment, L + 1
    uint32_t *blk_min_id;                    // [n / 64 + 1] smallest member index of every 64 positions
    int32_t  *blk_max_end;                   // [n / 64 + 1] largest end
    uint8_t  *head;                          // [n] the position starts a connected component
    int32_t  *pm;                            // [n] running maximum of the ends inside a component (written for components too large for LDS only)
    uint32_t *cstart, *cend, *seed_of_group; // [n] by seed: its component; by group: its seed
    uint64_t *group_off, *seg_group_off;     // [n + 1], [n_seg + 1]
    uint64_t *res;                           // total members, groups, error word
    // zeroed together before the chain:
    uint32_t *hist, *cnt, *keep;             // [n + 1] link histogram -> its exclusive sum; group sizes -> member offsets; kept flags -> group numbers
    uint8_t  *state;                         // [n] seeds' scratch of components too large for LDS
    unsigned long long *total;
    uint32_t *err;
};
void launch_sg_keys(hipStream_t s, const int32_t *start, const uint64_t *seg_off, uint64_t n_seg, uint32_t n, uint64_t *keys, uint32_t *vals);
void launch_sg_links(hipStream_t s, const SplitGroupsWs &w, const uint64_t *keys, const uint32_t *vals, const int32_t *start, const int32_t *end,
                     const uint64_t *seg_off, uint32_t n);
void launch_sg_seeds(hipStream_t s, const SplitGroupsWs &w, uint32_t n);
void launch_sg_offsets(hipStream_t s, const SplitGroupsWs &w, const uint64_t *seg_off, uint64_t n_seg, uint32_t n, const uint32_t *sort_err);
void launch_sg_fill(hipStream_t s, const SplitGroupsWs &w, uint32_t n_groups, int pre_bits, uint64_t *keys, uint32_t *vals);
// splitfits.hip — what the reference derives from an overlap group (point sets, DBSCAN1D fits, largest clusters, medians, strand vote)
struct SplitFitsIn {                         // device arrays, passed to the kernels by value
    const int32_t *start, *end, *q_start, *q_end;        // [n_members]
    const uint8_t *reverse;
    const uint64_t *supp_off;                            // [n_members + 1]
    const int32_t *supp_start, *supp_end, *supp_q_start, *supp_q_end;   // [n_supp]
    const uint8_t *supp_flags;
    const uint64_t *seg_off, *seg_group_off;             // [n_seg + 1]
    const uint64_t *group_off;                           // [n_groups + 1]
    const uint32_t *members;                             // indices within the group's segment
    uint64_t n_seg;
    uint32_t n_groups;
};
// One wave per (group, set): out[g] complete for the sets of at most DBSCAN1D_MAX_SEG points; a larger set w = 6 g + set gets big_n[w] = its
// size (0 otherwise) and adds itself to big_res[0] (sets) and big_res[1] (points). big_n and big_res zeroed by the caller.
void launch_sf_fits(hipStream_t s, const SplitFitsIn &in, double eps, int min_pts, csv_split_fit *out, uint32_t *big_n, unsigned long long *big_res);
// the points of ONE set, in the reference's order, to global memory (the sets too large for LDS)
void launch_sf_big_points(hipStream_t s, const SplitFitsIn &in, uint32_t w, int32_t *pts);
// largest cluster and median of one labelled set: pts_sorted / oid as launch_dbscan_1d_big takes them, labels by original index; sizes[n] zeroed
void launch_sf_big_reduce(hipStream_t s, const int32_t *pts_sorted, const uint32_t *oid, const int32_t *labels, uint32_t n, uint32_t *sizes,
                          csv_split_fit *rec, int set);
// splittables.hip — the tables SplitFitsIn points to, built from record references into resident shards (csvgpu_split_tables_resident / _resident_fits)
struct SplitTabSeg { const int32_t *pos; const uint16_t *flag; const int32_t *ref_end, *q_start, *q_end; };   // one segment's shard arrays (device)
struct SplitTablesIn {                       // device arrays, passed to the kernel by value
    const SplitTabSeg *seg;                  // [n_seg]
    const uint64_t *seg_off;                 // [n_seg + 1]
    uint64_t n_seg;
    const uint32_t *member_rec;              // [n_members]
    const uint64_t *supp_off;                // [n_members + 1]
    const uint32_t *supp_rec;                // [n_supp]
    const uint8_t *supp_where;               // [n_supp]
    uint32_t n_members, n_supp;
};
struct SplitTablesOut {
    int32_t *start, *end, *q_start, *q_end;  // [n_members]
    uint8_t *reverse;
    int32_t *supp_start, *supp_end, *supp_q_start, *supp_q_end;   // [n_supp]
    uint8_t *supp_flags;
    uint32_t *err;                           // zeroed by the caller; err_bit is ORed in when a coordinate lies outside the fits' domain
    uint32_t err_bit;
};
constexpr uint32_t ST_MAX_BLOCKS = 1024;     // of 256 threads; larger calls stride
void launch_st_tables(hipStream_t s, const SplitTablesIn &in, const SplitTablesOut &out);
// cnobs.hip — the copy-number pass's observation vectors from the window kernel's output (csvgpu_cn_observations_resident_many / _cn_decode_)
constexpr uint32_t CN_MAX_WINDOWS = 5087;    // windows of a region: the last bucket count whose epoch fits the LDS (SO_SMALL_B)
constexpr uint32_t CN_SMALL_MAX = 127;       // regions of up to this many windows take the wave-per-region form (bucket counts 13 .. 127)
constexpr uint32_t CN_MAX_EPOCHS = 12;
constexpr uint32_t CN_MAX_BLOCKS_SMALL = 4096, CN_MAX_BLOCKS_BIG = 256;   // larger calls stride
constexpr uint32_t CN_SLOT_UNUSED = 0xffffffffu;
struct CnEpochs {                            // by value: epoch k holds the nodes inserted from first[k] on, in B[k] buckets; first[n] = 2^32 - 1
    uint32_t n = 0;
    uint32_t first[CN_MAX_EPOCHS + 1] = {0};
    uint32_t B[CN_MAX_EPOCHS] = {0};
};
struct CnSlots {                             // per window slot (region's first window + list position p): what the node at p contributes
    uint32_t *fw, *lw;                       // [W] first / last window of the node's run (global window index)
    uint32_t *lo, *cnt;                      // [W] its SNP slice: first record, length (0: the dummy observation; CN_SLOT_UNUSED: no node at p)
    uint32_t *off, *reg;                     // [W] first observation inside its region; the region
    uint32_t *tot;                           // [R + 1] observations per region, tot[R] = 0: the exclusive sum makes it obs_off
};
struct CnObs { uint64_t *obs_off; uint32_t *pos; double *baf, *pfb, *log2_cov; uint8_t *is_snp; };
void launch_cn_order(hipStream_t s, const uint32_t *ws, const uint32_t *we, const uint32_t *win_base, const uint32_t *snp_off, const uint32_t *snp_pos,
                     const uint32_t *regions_small, uint32_t n_small, const uint32_t *regions_big, uint32_t n_big, const CnEpochs &ep, const CnSlots &out);
void launch_cn_fill(hipStream_t s, const CnSlots &sl, uint32_t n_slots, uint32_t n_regions, const uint32_t *obs_off32, const uint32_t *ws, const uint32_t *we,
                    const double *l2, const uint32_t *snp_pos, const double *snp_baf, const double *snp_pfb, const CnObs &o);
// snptable.hip — one contig's SNP records resident in HBM (csv_snp_table), and what the copy-number pass derives from the regions' record
// counts, on the device (csvgpu_snp_table_* / csvgpu_cn_*_tables_many). The per-region rules are snp_table_core.hpp's.
struct SnpTabDev {                           // a table as the kernels see it (all zero: no records). Values as their bits.
    const uint32_t *pos; const uint64_t *baf;            // [n] ascending; baf resolved per run
    const uint64_t *pfb;                                  // [n] resolved per run (per-record kind), or null (first-hit kind)
    const uint32_t *af_pos; const uint64_t *af;           // [n_af] ascending (first-hit kind)
    uint32_t n, n_af;
};
enum : uint32_t { CN_PLAN_OVER_WINDOWS = 1 };             // CnPlanHead::flags: a region needs more than CN_MAX_WINDOWS windows
struct CnPlanHead { unsigned long long W, S; uint32_t flags, n_small, n_big, pad; };      // zeroed by the caller; [n_shards + 1] first windows follow at byte 64
constexpr size_t CN_PLAN_HEAD_BYTES = 64;
struct CnPlan {                              // device arrays of R regions on n_shards tables, passed to the kernels by value
    const uint32_t *rs, *re;                 // [R] the regions
    const int32_t *ssf;                      // [R] the window count's floor (null: 1)
    const uint32_t *rsh;                     // [R] the region's table (null: 0)
    const SnpTabDev *tabs;                   // [n_shards]
    const uint32_t *reg_off;                 // [n_shards + 1]
    int32_t *ss;                             // [R] windows per region
    uint64_t *wo;                            // [R + n_shards] window offsets relative to the region's shard (launch_window_log2)
    uint32_t *wbase, *soff;                  // [R + 1] first window / first record of each region in the flat arrays
    uint32_t *sfirst, *hit;                  // [R] first record in the table; the first-hit kind's AF record (snpcore::NO_HIT: none)
    uint32_t *small, *big;                   // [R] the regions by kernel form (launch_cn_order), in no particular order
    CnPlanHead *head; uint32_t *shard_w0;    // the readback: totals, flags, list lengths; [n_shards + 1] = wbase[reg_off[s]]
    void *es_tmp;                            // exclusive_sum_tmp_bytes(R + 1)
};
// baf_out[i] = baf[last of i's run]; pfb_out[i] = pfb of the run's last flagged member, else 0.0 (pfb_out null: not wanted; has_pfb null: none
// flagged; pfb null: 0.0). marks, pm: [n] int32; pm_tmp: prefix_max_tmp_bytes(n). Nothing for n == 0.
void launch_snp_resolve(hipStream_t s, const uint32_t *pos, const uint64_t *baf, const uint64_t *pfb, const uint8_t *has_pfb, uint32_t n, int32_t *marks, int32_t *pm,
                        void *pm_tmp, uint64_t *baf_out, uint64_t *pfb_out);
// ranges, hits, window counts, the two exclusive sums, the per-shard offsets, the lists and the head (zeroed here). R >= 1.
void launch_cn_plan(hipStream_t s, const CnPlan &p, uint32_t R, uint32_t n_shards);
// the regions' resolved records into the compact layout launch_cn_order / launch_cn_fill read: [soff[r], soff[r + 1]) for region r
void launch_snp_gather(hipStream_t s, const CnPlan &p, uint32_t R, uint32_t S, uint32_t *spos, uint64_t *sbaf, uint64_t *spfb);
// inflate.hip — BGZF members (raw DEFLATE + CRC-32), one wave per member: status[i] = 0 decoded and written, 1 declined (nothing written);
// *n_declined (zeroed by the caller) counts the declined ones
void launch_bgzf_inflate(hipStream_t s, const uint8_t *comp, const csv_bgzf_block *blocks, uint32_t n_blocks, uint8_t *out, uint8_t *status,
                         unsigned int *n_declined);
// bamunpack.hip — a decoded BAM record stream in HBM to the arrays of csv_reads (+ sequences, names, name hashes); csvgpu_bam_unpack / _dev
struct BamUnpackOut {                        // device arrays of this call's kept records, passed to the kernels by value (seq / name / hash: null = not wanted)
    int32_t *pos; uint16_t *flag; uint8_t *mapq;
    uint64_t *cigar_off; uint32_t *cigar;
    uint64_t *seq_off; uint8_t *seq;
    uint64_t *name_off; uint8_t *name;
    uint64_t *name_hash;
};
// the words of BamUnpackWs::res (preset to all-ones with status and bounds: one slice, one memset, one copy back)
enum : uint32_t { BU_RES_NKEPT = 0, BU_RES_FIRST = 1, BU_RES_NCIGAR = 2, BU_RES_NSEQ = 3, BU_RES_NNAME = 4, BU_RES_STOPPED = 5, BU_RES_CONSUMED = 6, BU_RES_NREC = 7, BU_RES_WORDS = 8 };
constexpr size_t BU_HEAD_BYTES = 64;         // res[8] | status u64 | bounds[2]
constexpr unsigned long long BU_STATUS_NONE = ~0ull;
struct BamUnpackWs {
    uint32_t *res = nullptr; unsigned long long *status = nullptr; uint32_t *bounds = nullptr;      // the head
    uint32_t *anchors = nullptr, *count = nullptr;                                                   // [n_anchors], [n_anchors + 1]
    uint32_t *rec_off = nullptr; uint32_t rec_cap = 0;                                               // [rec_cap] every record's start; rec_cap = len / 36
    uint32_t *cig_src = nullptr, *cig_n = nullptr, *seq_n = nullptr, *name_n = nullptr;              // [rec_cap + 1] per kept record
    void *es_tmp = nullptr;
    // the host-pointer form alone: the stream and the outputs staged on the device
    uint8_t *bytes = nullptr;
    BamUnpackOut out{};
};
// chain: anchors on the device, head preset; leaves rec_off[], res[BU_RES_NREC], res[BU_RES_CONSUMED] and the status
void launch_bam_chain(hipStream_t s, const uint8_t *bytes, uint32_t len, uint32_t n_anchors, const BamUnpackWs &w);
// filter, checks and CG rule of the kept records, the three sums, the counts into res[0..5]
void launch_bam_fields(hipStream_t s, const uint8_t *bytes, uint32_t n_rec, int32_t tid, int64_t end, const BamUnpackWs &w);
// the outputs, after the caller has held the counts against its capacities
void launch_bam_emit(hipStream_t s, const uint8_t *bytes, uint32_t first, uint32_t n_kept, uint32_t n_cigar, uint32_t n_seq, uint32_t n_name,
                     uint64_t cigar_base, uint64_t seq_base, uint64_t name_base, const BamUnpackWs &w, const BamUnpackOut &out);
// vcfparse.hip — VCF text lines in HBM to the kept records and the deferred lines' offsets; csvgpu_vcf_snp_parse / _af_parse / _dev
struct VcfHead {                             // one slice, preset by launch_vcf_count, copied back whole
    uint32_t n_lines;                        // non-empty lines in front of stop_off
    uint32_t stop_off;                       // lowest offset of a STOP line (all-ones: none)
    unsigned long long hash_off;             // lowest offset of a line that begins with '#' (all-ones: none)
    uint32_t n_kept, n_defer;                // the two sums' totals (launch_vcf_flags)
};
struct VcfOut { uint32_t *line_off, *chrom_len, *pos; double *value; uint32_t *defer_off; };
struct VcfParseArgs {                        // what the per-line kernel is told; contig / needle / sorted_pos on the device (AF form)
    bool af, dp_int, ad_int;
    const uint8_t *contig, *needle; uint32_t contig_len, needle_len;
    const uint32_t *sorted_pos; uint64_t n_sorted;
};
struct VcfWs {
    VcfHead *head = nullptr;
    uint32_t *tile_cnt = nullptr; void *es_tmp = nullptr;          // [n_tiles + 1] line ends per tile, then their exclusive sum
    uint8_t *strings = nullptr;                                    // contig | needle (AF form)
    // per line slot (n_slots = line ends + 1), carved once the line ends are counted
    uint32_t *line_start = nullptr, *kept = nullptr, *defer = nullptr, *pos = nullptr, *chrom_len = nullptr; double *value = nullptr; uint8_t *code = nullptr;
    void *es_tmp2 = nullptr;
    VcfOut out{};                                                  // the host-pointer form alone: the outputs staged on the device
};
struct VcfTextWs { uint8_t *text = nullptr; uint32_t *sorted_pos = nullptr; };       // the host-pointer form's inputs, staged
static inline uint32_t vcf_tiles(const uint8_t *text, uint64_t len) { return (uint32_t)((((uintptr_t)text & 15) + len + CSV_VCF_TILE_BYTES - 1) / CSV_VCF_TILE_BYTES); }
// line ends per tile and their exclusive sum: tile_cnt[n_tiles] = the text's line ends; presets the head
void launch_vcf_count(hipStream_t s, const uint8_t *text, uint32_t len, const VcfWs &w);
// line_start[0 .. n_slots); n_slots = tile_cnt[n_tiles] + 1
void launch_vcf_starts(hipStream_t s, const uint8_t *text, uint32_t len, const VcfWs &w);
// every line decided by a group of `width` lanes (8, 16 or 64; 0: chosen from the mean line length), flags, sums, the head's counts
void launch_vcf_parse(hipStream_t s, const uint8_t *text, uint32_t len, uint32_t n_slots, const VcfParseArgs &a, int width, const VcfWs &w);
// the outputs, after the caller has held the counts against its capacities
void launch_vcf_emit(hipStream_t s, uint32_t n_slots, bool af, const VcfWs &w, const VcfOut &out);
// fasta.hip — a FASTA's text in HBM to the genome's base array (csvgpu_genome_builder_*), and cuts of it (csvgpu_genome_fetch)
struct FastaCarry { uint8_t mid_line, kind; };        // the line the previous call's text left open, and its kind (fastacore::LINE_*)
struct FastaHead {                           // one slice, copied back whole
    uint32_t n_kept, n_hdr, n_name;          // the three sums' totals: residue bytes, header lines, name bytes
    uint32_t tail_len, tail_kind;            // the text's last line slot: its bytes and its kind
};
struct FastaEvents {                         // the text's header lines in file order, [n_hdr] each
    uint32_t *kept = nullptr;                // residue bytes of this text in front of the line
    uint32_t *name_off = nullptr, *name_len = nullptr;   // its name's piece in names[]: up to the first blank or the line's end
    uint8_t *blank = nullptr;                // a blank ended the piece
    uint8_t *names = nullptr;                // [n_name]
};
struct FastaWs {
    VcfWs vcf;                               // head, tile_cnt, es_tmp, line_start: what launch_vcf_count / _starts use
    FastaHead *head = nullptr;
    uint32_t *kept = nullptr, *hdr = nullptr, *nlen = nullptr;    // [n_slots + 1] per line, then their exclusive sums
    uint8_t *blank = nullptr;                // [n_slots]
    void *es_tmp = nullptr;
    FastaEvents ev;                          // sized for n_slots lines and the text's bytes
};
// per line: kind, kept bytes, name span; the sums; the header events. line_start[] must be in place (launch_vcf_starts).
void launch_fasta_lines(hipStream_t s, const uint8_t *text, uint32_t len, uint32_t n_slots, const FastaCarry &carry, const FastaWs &w);
// the residue lines' bytes to dst[0 .. n_kept), in file order
void launch_fasta_compact(hipStream_t s, const uint8_t *text, uint32_t len, const FastaWs &w, uint8_t *dst);
// item i: out[out_off[i] .. out_off[i + 1]) = seq[src[i] ..), ambiguity codes as N if mask; out_off[0] = 0, out_off[n] = total; out 16-byte aligned
void launch_fasta_cut(hipStream_t s, const uint8_t *seq, const uint64_t *src, const uint64_t *out_off, uint64_t n, uint64_t total, bool mask, uint8_t *out);
// vcfformat.hip — the VCF writer's record lines assembled on the device (csvgpu_vcf_format; the rules in vcf_format_core.hpp)
struct VfContig {                            // one contig of the batch, as the kernels see it
    uint64_t call_first;                     // its first call (call_off[t]); the table has one more entry, whose call_first is the call count
    uint64_t name_off; uint32_t name_len;    // its name in names[]
    uint32_t n_gaps; uint64_t gap_first;     // its BED rows in gap_start / gap_end
    int64_t  contig_len;                     // its length in the genome, -1: the genome has no such record
    uint64_t rec_start;                      // its first base in the genome's array
    const uint32_t *depth; uint32_t depth_len, pad;      // its resident depth map (null: no call asks for a depth)
};
struct VfHead {                              // one slice, zeroed per call (first_refused to all ones), copied back whole
    unsigned long long text_bytes, n_lines;
    unsigned long long first_refused;        // min over the refused calls of (call index << 8 | why); all ones: none
    uint32_t total, unclassified, gap_filtered, pad;
};
struct VfArgs {                              // passed to the kernels by value
    const VfContig *contig; uint32_t n_contigs;
    const void *calls; uint64_t n_calls;     // [n_calls] csv_vcf_call
    const uint64_t *alt_off; const uint8_t *alts;
    const uint8_t *names, *method; uint32_t method_len;
    const uint32_t *gap_start, *gap_end;
    const uint8_t *seq;                      // the genome's base array (16 spare bytes behind its last base)
    uint32_t *len;                           // [n_calls + 1] the lines' lengths, then their exclusive sums
    int32_t *depth;                          // [n_calls] the value at POS
    uint8_t *status;                         // [n_calls]
    VfHead *head;
    void *es_tmp;                            // exclusive_sum_tmp_bytes(n_calls + 1)
};
// a lane per call: disposition, depth, gap search, the line's length; the sums of the head; then the exclusive sum of the lengths
void launch_vcf_format_size(hipStream_t s, const VfArgs &a);
// text[0 .. total): every 16-byte piece by one lane (total = len[n_calls] < 2^32, after the caller has read the head)
void launch_vcf_format_write(hipStream_t s, const VfArgs &a, uint64_t total, uint8_t *text);
// snpbuild.hip — the kept records of VCF batches cut by contig on the device (csvgpu_snp_builder_*; the rules in snp_build_core.hpp)
constexpr uint32_t SB_MAX_BLOCKS = 256;      // of 256 threads; larger calls stride
struct SnpAppendArgs {                       // passed to the kernel by value
    uint32_t n;                              // the call's kept records
    const uint32_t *ridx;                    // [n + 1] the exclusive sums of the run flags
    const uint32_t *line_off, *chrom_len, *rec_pos; const uint64_t *rec_baf;      // [n] what launch_vcf_emit left
    uint64_t tail, text_base; uint32_t run_base;                                  // the builder's records and runs before the call
    uint32_t *pos; uint64_t *baf; uint32_t *run; uint64_t *key;                   // the builder's arrays
    uint32_t *run_first, *run_line_off, *run_chrom_len;                           // [ridx[n]] the call's run table
};
// flags[0 .. n]: 1 where kept record k starts a CHROM run, then their exclusive sums in place: flags[n] = the call's runs
void launch_snp_run_flags(hipStream_t s, const uint8_t *text, const uint32_t *line_off, const uint32_t *chrom_len, uint32_t n, uint32_t *flags, void *es_tmp);
void launch_snp_append(hipStream_t s, const SnpAppendArgs &a);
// keys[i] = contig id << shift | order key, vals[i] = i (run_contig[]: the contig of every run; host-appended records carry their own)
void launch_snp_keys(hipStream_t s, const uint32_t *run, const uint64_t *key, const uint32_t *run_contig, uint32_t n, int shift, uint64_t *keys, uint32_t *vals);
// behind the sort: pos / baf in the order; per contig id first / end slot and desc (a pos below its predecessor's); *dup: two equal keys.
// first / end / desc / dup zeroed by the caller.
void launch_snp_columns(hipStream_t s, const uint64_t *keys, const uint32_t *vals, const uint32_t *pos_in, const uint64_t *baf_in, uint32_t n, int shift,
                        uint32_t *pos_out, uint64_t *baf_out, uint32_t *first, uint32_t *end, uint32_t *desc, uint32_t *dup);
// shardbuild.hip — a resident shard built on the device (csvgpu_shard_builder_*), and the ALT strings cut from its sequences
// *unsorted |= pos[i] < pos[i - 1] for the records [first, first + n) (the first one against its predecessor, if there is one)
void launch_sb_unsorted(hipStream_t s, const int32_t *pos, uint64_t first, uint64_t n, uint32_t *unsorted);
void launch_sb_add(hipStream_t s, uint64_t *off, uint64_t n, uint64_t delta);      // off[0 .. n) += delta (modulo 2^64)
// item i: out[out_off[i] .. out_off[i + 1]) = the bases from qpos[i] on of record read[i], or N's where they leave its sequence (alt_bases_core.hpp)
void launch_alt_bases(hipStream_t s, const uint64_t *seq_off, const uint8_t *seq, const uint32_t *read, const uint32_t *qpos, const uint64_t *out_off, uint64_t n,
                      uint8_t *out);
// dbscan1d.hip
void launch_dbscan_1d_batched(hipStream_t s, const int32_t *pts, const uint64_t *seg_off, uint64_t n_seg,
                              double eps, int min_pts, int32_t *labels, unsigned int *too_large_flag);
constexpr uint32_t DBSCAN1D_MAX_SEG = 512;   // larger segments take the generic sorted path
size_t dbscan1d_big_tmp_bytes(uint64_t n);
// pts_sorted ascending (int order); oid = original index per sorted position
void launch_dbscan_1d_big(hipStream_t s, const int32_t *pts_sorted, const uint32_t *oid, uint64_t n, double eps,
                          int min_pts, int32_t *labels, void *tmp);
// hmm.hip
void launch_window_log2(hipStream_t s, const uint32_t *depth, uint32_t depth_len, const uint32_t *rs, const uint32_t *re,
                        const int32_t *ss, const uint64_t *win_off, uint64_t n_regions, uint64_t n_windows,
                        double mean_cov, double *log2_cov, uint32_t *ws, uint32_t *we);
size_t viterbi_tmp_bytes(uint64_t n_obs, uint64_t n_seq);
void launch_viterbi(hipStream_t s, const csv_hmm &hmm, const double *o1, const double *o2, const double *pfb,
                    const uint64_t *seq_off, uint64_t n_seq, uint64_t n_obs, int32_t *states, double *loglik, void *tmp);

}  // namespace csv
