/*
 * csvgpu.h — C-ABI of the MI355X (gfx950) hot path of ContextSV.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++/torch types,
 * no exceptions across it. Every entry point names the reference seam
 * (WGLab/ContextSV, file:line relative to the reference root) it replaces.
 *
 * Conventions
 *   - every call returns CSV_OK (0) or a negative csv_status; nothing throws.
 *   - the caller owns every buffer; the library owns only the opaque context
 *     (device workspace, stream, per-kernel timers).
 *   - one csv_ctx per GPU, used from one host thread at a time.
 *   - entry points without a suffix take HOST pointers (they stage H2D, run the
 *     kernels, copy the result back). Entry points ending in `_dev` take DEVICE
 *     pointers (hipMalloc'd / torch CUDA tensors), run asynchronously on the
 *     context's stream and are what the benchmark times with inputs resident
 *     in HBM.
 *   - there is no CPU fallback anywhere behind this ABI: without a usable HIP
 *     device csvgpu_create() fails with CSV_ENODEV and nothing else can be called.
 */
#ifndef CSVGPU_H
#define CSVGPU_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CSVGPU_ABI_VERSION 4   /* 4: csv_tuning, csvgpu_set_tuning (the library reads no environment variable); 3: csvgpu_split_order_begin_self; 2: CSV_K_SPLIT_ORDER, csvgpu_split_order_begin / _finish, the job / gate / batch entry points; the test hook left the product library */

typedef struct csv_ctx csv_ctx;

typedef enum csv_status {
    CSV_OK        =  0,
    CSV_EINVAL    = -1,  /* bad argument (null pointer, eps outside [0,1), min_pts < 1, ...) */
    CSV_ENODEV    = -2,  /* no usable HIP device / device ordinal out of range */
    CSV_ENOMEM    = -3,  /* device or host allocation failed */
    CSV_EHIP      = -4,  /* a HIP runtime call failed; see csvgpu_last_error() */
    CSV_ECAPACITY = -5   /* caller's output capacity too small; required count is returned */
} csv_status;

/* ---- alignment records of one shard (normally: one chromosome), struct of arrays ----
 * Mirrors exactly the fields of htslib's bam1_core_t that the reference reads on this
 * path (sv_caller.cpp:526,541-545; cnv_caller.cpp:491-502): core.pos (0-based), core.flag,
 * core.qual, core.tid, core.n_cigar and the packed CIGAR words (len<<4 | op, BAM op codes
 * M0 I1 D2 N3 S4 H5 P6 =7 X8). Records are in file (coordinate-sorted) order. */
typedef struct csv_reads {
    uint64_t        n_reads;
    uint64_t        n_cigar;    /* total CIGAR words == cigar_off[n_reads] */
    const int32_t  *pos;        /* [n_reads] 0-based leftmost reference position */
    const uint16_t *flag;       /* [n_reads] BAM FLAG */
    const uint8_t  *mapq;       /* [n_reads] MAPQ */
    const int32_t  *tid;        /* [n_reads] reference id (carried, not interpreted by kernels; may be NULL) */
    const uint64_t *cigar_off;  /* [n_reads+1] first CIGAR word of each read; non-decreasing, cigar_off[n_reads] <= n_cigar, < 2^31 words
                                 * per read — entry points return CSV_EINVAL otherwise (nothing reaches the device) */
    const uint32_t *cigar;      /* [n_cigar] packed CIGAR words */
} csv_reads;

/* One SV signature = one SVCall emitted by SVCaller::processCIGARRecord
 * (sv_caller.cpp:566-643). 16 bytes, written with a single store on device.
 *   kind: 0 = CIGARINS (I op), 1 = CIGARDEL (D op), 2 = CIGARCLIP (S op) — the SVDataType
 *         bit the reference sets (sv_types.h:60-63). SVType is DEL for kind 1, INS otherwise.
 *   qpos: query offset of the op (reference `query_pos`, sv_caller.cpp:546,653) — the host
 *         needs it to cut the inserted sequence when op_len == 50 (sv_caller.cpp:589,624). */
typedef struct csv_sig {
    uint32_t start;      /* 1-based, = pos+1 (sv_caller.cpp:584,619,636) */
    uint32_t end;        /* = start + op_len - 1 (sv_caller.cpp:585,620,637) */
    uint32_t read;       /* index of the emitting read inside the shard */
    uint32_t qpos_kind;  /* (qpos << 2) | kind */
} csv_sig;
#define CSV_SIG_KIND(s) ((s).qpos_kind & 3u)
#define CSV_SIG_QPOS(s) ((s).qpos_kind >> 2)
enum { CSV_KIND_INS = 0, CSV_KIND_DEL = 1, CSV_KIND_CLIP = 2 };

/* 6-state PennCNV-style HMM parameters = the fields ReadCHMM fills (khmm.cpp:395-553,
 * struct CHMM khmm.h:14-32). Row-major A[i*6+j] = P(i -> j). */
typedef struct csv_hmm {
    double A[36];
    double pi[6];
    double B1_mean[6];
    double B1_sd[6];
    double B1_uf;
    double B2_mean[5];
    double B2_sd[5];
    double B2_uf;
} csv_hmm;

/* Kernel ids for csvgpu_timing_get(). */
typedef enum csv_kernel_id {
    CSV_K_CIGAR_SCAN = 0,   /* signature emission + alignment intervals */
    CSV_K_DEPTH      = 1,   /* tile-owner depth map (+ sum / non-zero count) */
    CSV_K_SORT       = 2,   /* all radix-sort passes + tie fix-up */
    CSV_K_DBSCAN     = 3,   /* neighbour count + union + rank + label (interval metric) */
    CSV_K_DBSCAN1D   = 4,   /* batched 1-D DBSCAN */
    CSV_K_WINDOW     = 5,   /* window log2 coverage */
    CSV_K_VITERBI    = 6,   /* emissions + Viterbi DP + backtrack */
    CSV_K_MISC       = 7,   /* the split-read tables built from resident shards (csvgpu_split_tables_resident, csvgpu_split_resident_fits) */
    CSV_K_SPLIT_ORDER = 8,  /* hash-map node order of the split-read pass (compaction + per-epoch sorts + survivors) */
    CSV_K_SPLIT_GROUPS = 9, /* overlap groups of the split-read pass (member order, links, seeds, fill + its sorts) */
    CSV_K_SPLIT_FITS = 10,  /* point sets, 1-D DBSCAN fits, largest clusters, medians and strand vote of the overlap groups */
    CSV_K_COUNT      = 11
} csv_kernel_id;

/* ------------------------------------------------------------------------------------------ */
/* context                                                                                      */

/* Create a context on HIP device `device_ordinal`. `stream` may be NULL (the context creates
 * its own non-blocking stream) or an existing hipStream_t (e.g. torch's current stream) that
 * every kernel of this context is then launched on. Returns NULL on failure (no device, ...);
 * csvgpu_last_error(NULL) then describes why. */
csv_ctx    *csvgpu_create(int device_ordinal, void *stream);
/* The same with the context's own stream at the device's LOWEST priority: for work that should fill the gaps other contexts leave (the
 * split-read pass's ordering kernels beside the lanes' bandwidth-bound pairs) instead of sharing the compute units with them. */
csv_ctx    *csvgpu_create_background(int device_ordinal);
void        csvgpu_destroy(csv_ctx *ctx);
int         csvgpu_abi_version(void);
const char *csvgpu_last_error(const csv_ctx *ctx);
/* Block until everything queued on the context's stream has finished. */
int         csvgpu_synchronize(csv_ctx *ctx);
/* Per-kernel timers: when enabled, each launch group is bracketed by HIP events recorded on
 * the stream the group runs on (the context's; for the scan + depth pair of a job behind a gate, the gate's — there the
 * pair shares three events, and at on = 2 only every fourth pair is timed); csvgpu_timing_get() synchronises and returns the accumulated device
 * time and the number of launch groups since the last reset. on = 1: every group; on = 2: only CSV_K_CIGAR_SCAN and
 * CSV_K_DEPTH (an event is a barrier packet in the queue, ~5 us of idle device each); on = 3: those two groups, every pair timed also
 * behind a gate (for runs whose launches differ in size, where a sampled quarter would not match the bytes); on = 0: off. */
int         csvgpu_timing_enable(csv_ctx *ctx, int on);
int         csvgpu_timing_reset(csv_ctx *ctx);
int         csvgpu_timing_get(csv_ctx *ctx, int kernel_id, double *total_ms, uint64_t *launches);

/* Which of several kernels that compute the SAME result a context launches (tests and A/B measurements: no value changes an output).
 * A new context holds CSV_TUNING_DEFAULTS. */
enum { CSV_FORM_AUTO = -1, CSV_FORM_WAVE = 0, CSV_FORM_ROWS16 = 1, CSV_FORM_ROWS8 = 2, CSV_FORM_LANES = 3 };
#define CSV_TAIL_AUTO (-1)
#define CSV_TAIL_MAX  3
typedef struct csv_tuning {
    int32_t scan_form;          /* how the CIGAR scan and the depth walk take a read: CSV_FORM_AUTO = from the shard's mean CIGAR words per read
                                 * (a wave per long read, 16 lanes per short one), or one of the four forms forced. A shard of 2^32 - 1 words or more is
                                 * always walked by waves. */
    int32_t split_tail;         /* split order: how many of every contig's last epochs are ordered for the survivors only, 0 (the full chain of sorts)
                                 * .. CSV_TAIL_MAX; CSV_TAIL_AUTO = from the nodes per supplementary record. Orders too large for the
                                 * survivors' keys take the full chain whatever is set. */
    int32_t sort_three_launch;  /* radix sorts: 0 = onesweep passes (one launch per pass) where the sort's size allows them, 1 = histogram, scan and scatter
                                 * launches per pass. Sorts whose key count is still on the device when they are queued (csvgpu_split_order_begin_self)
                                 * are onesweep passes either way. */
    int32_t dbscan_all_pairs;   /* interval DBSCAN of small sets (csvgpu_dbscan_iv_batch): 0 = the kernel that meets the pairs in start order, 1 = all pairs */
    int32_t split_chain_only;   /* split order: 0 = the first epochs in one launch (nodes and buckets in LDS), 1 = through the chain's sorts like the rest */
} csv_tuning;
#define CSV_TUNING_DEFAULTS { CSV_FORM_AUTO, CSV_TAIL_AUTO, 0, 0, 0 }
/* Replace the context's record (t == NULL: the defaults); it applies to everything started on this context afterwards. CSV_EINVAL, the record
 * unchanged: a field out of range, a job open on the context (csvgpu_chr_job_begin without its _end / _abort) or a split order between _begin
 * and _finish. A resident shard keeps the scan form of the context that created it (csvgpu_shard_upload / _wrap_dev), on whichever context it is
 * run later; the host-pointer entry points take the form of the context they are called on. */
int         csvgpu_set_tuning(csv_ctx *ctx, const csv_tuning *t);
/* Whether csvgpu_shard_upload stores the CIGAR array of a long-read (CSV_FORM_WAVE) shard in 16 bits per op: 4 of op, 12 of length, the few
 * longer ops in a side table. Half the bytes the two big kernels read per step and half the resident memory; every result is the same bit for
 * bit, and csvgpu_shard_fetch_reads still returns the uploaded 32-bit words. on: 1 (the default) or 0. Read when a shard is uploaded: a shard
 * keeps the form it was uploaded with. Shards of the short-read forms, wrapped device arrays, shards of csvgpu_shard_builder_* and shards with
 * more than one op in 64 of length >= 4095 stay at 32 bits. CSV_EINVAL: on out of range, or a job or a split order open on the context. */
int         csvgpu_set_cigar_packing(csv_ctx *ctx, int on);

/* ------------------------------------------------------------------------------------------ */
/* host-pointer entry points (the seams of SURVEY.md §8b)                                       */

/* Replaces SVCaller::findCIGARSVs + processCIGARRecord + addSVCall for one chromosome
 * (sv_caller.cpp:506-537, 539-661; sv_object.cpp:22-33).
 *   filter: flag & (SECONDARY|UNMAP|DUP|QCFAIL|SUPPLEMENTARY) or mapq < min_mapq => skipped (:526).
 *   depth_len = pos_depth_map.size() (chromosome length + 1); soft clips with pos+1 >= depth_len are
 *   skipped together with their cursor update (:602-604 `continue`).
 *   min_oplen = 50 (:566), min_mapq = 20 (sv_caller.h:72) in the reference.
 * Output order == order of the reference's chr_sv_calls vector after all addSVCall()s: ascending
 * (start,end); equal (start,end) in REVERSE emission order (std::lower_bound insert, sv_object.cpp:31).
 * *n_out: in = capacity of `out` in records, out = number of signatures. If the capacity is too
 * small CSV_ECAPACITY is returned and *n_out holds the required count. */
int csvgpu_cigar_scan(csv_ctx *ctx, const csv_reads *reads, uint32_t depth_len,
                      uint32_t min_oplen, uint8_t min_mapq, csv_sig *out, uint64_t *n_out);

/* Replaces SVCaller::getAlignmentReadPositions (sv_caller.cpp:663-690) and htslib bam_endpos for
 * every record of the shard (used by findSplitSVSignatures, sv_caller.cpp:152,162):
 *   q_start = query offset of the first M/I/=/X op (0 if none), q_end = sum of M,I,S,=,X lengths,
 *   ref_end = pos + reference length of the CIGAR (pos+1 when that length is 0 or the read is unmapped). */
int csvgpu_aln_intervals(csv_ctx *ctx, const csv_reads *reads,
                         int32_t *ref_end, int32_t *q_start, int32_t *q_end);

/* Replaces the per-chromosome body of CNVCaller::calculateMeanChromosomeCoverage
 * (cnv_caller.cpp:488-543): depth[p] (1-based p, depth_len = chr_len+1 entries, entry 0 stays 0)
 * counts M/=/X bases of every record without UNMAP|SECONDARY|QCFAIL|DUP (no mapq filter,
 * supplementary included); bases at p >= depth_len are skipped. *sum = sum of depth, *nonzero =
 * #positions with depth > 0 (mean coverage = sum/nonzero, :534-538). `depth` may be NULL when only
 * the two scalars are wanted. */
int csvgpu_depth(csv_ctx *ctx, const csv_reads *reads, uint32_t depth_len,
                 uint32_t *depth, uint64_t *sum, uint32_t *nonzero);

/* Replaces DBSCAN::fit + getClusters (dbscan.cpp:9-81, dbscan.h:13-18): labels[i] for the i-th
 * interval in CALLER order: -2 noise, 0..k-1 cluster id, identical to the reference's sequential
 * visit-order labels. Metric = 1 - min reciprocal overlap evaluated in the same IEEE double
 * expression (dbscan.cpp:74-79). Requires 0 <= eps < 1 and min_pts >= 1 (CSV_EINVAL otherwise). */
int csvgpu_dbscan_iv(csv_ctx *ctx, const uint32_t *start, const uint32_t *end, uint64_t n,
                     double eps, int32_t min_pts, int32_t *labels);

/* DBSCAN::fit for a batch of independent interval sets in one call — the per-type fits of mergeSVs (sv_object.cpp:62-94) for every
 * contig of a run at once (the two final merges, sv_caller.cpp:907, :925): set s = intervals [seg_off[s], seg_off[s+1]) in CALLER
 * order, labels per set exactly as csvgpu_dbscan_iv gives them. Sets of up to 2048 intervals share one launch (one workgroup each,
 * all pairs in LDS); larger ones take the windowed path one by one. */
int csvgpu_dbscan_iv_batch(csv_ctx *ctx, const uint32_t *start, const uint32_t *end, const uint64_t *seg_off, uint64_t n_seg,
                           double eps, int32_t min_pts, int32_t *labels);

/* Replaces DBSCAN1D::fit + getClusters for a batch of independent point sets
 * (dbscan1d.cpp:8-70; the six fits per overlap group of sv_caller.cpp:270-372 become one call):
 * segment s = pts[seg_off[s] .. seg_off[s+1]); labels in caller order per segment. Metric
 * |a-b| (int) <= eps (double). Requires eps >= 0, min_pts >= 1. */
int csvgpu_dbscan_1d(csv_ctx *ctx, const int32_t *pts, const uint64_t *seg_off, uint64_t n_seg,
                     double eps, int32_t min_pts, int32_t *labels);

/* Replaces the window loop of CNVCaller::querySNPRegion (cnv_caller.cpp:76-113) for a batch of
 * regions: region r has sample_size[r] windows; window i sums depth[(uint32)(start + i*step + j)]
 * for integer j < step (step = (end-start+1)/sample_size as double), stops past `end`, skips
 * positions >= depth_len, and yields log2((sum/count)/mean_cov) (sum==0 -> 1e-9; count==0 -> 0.0).
 * win_off[r] (n_regions+1 entries) = first output window of region r. Also returns the window
 * bounds the reference uses as map keys (:80-81). */
int csvgpu_window_log2(csv_ctx *ctx, const uint32_t *depth, uint32_t depth_len,
                       const uint32_t *region_start, const uint32_t *region_end,
                       const int32_t *sample_size, const uint64_t *win_off, uint64_t n_regions,
                       double mean_cov, double *log2_cov, uint32_t *win_start, uint32_t *win_end);

/* Replaces testVit_CHMM / ViterbiLogNP_CHMM (khmm.cpp:28-56, 225-393) for a batch of observation
 * sequences: sequence s = observations [seq_off[s], seq_off[s+1]); o2 == -1 means "no BAF".
 * states[] are 1..6 (the reference's returned vector, dummy 0th element already dropped),
 * loglik[s] = max final delta. Sequences of length 0 get loglik -1e11 (VITHUGE) and no states. */
int csvgpu_viterbi(csv_ctx *ctx, const csv_hmm *hmm, const double *o1, const double *o2,
                   const double *pfb, const uint64_t *seq_off, uint64_t n_seq,
                   int32_t *states, double *loglik);

/* ------------------------------------------------------------------------------------------ */
/* device-pointer entry points (inputs resident in HBM; asynchronous on the context's stream)   */

/* Upload a shard once; the returned handle keeps pos/flag/mapq/cigar_off/cigar resident in HBM
 * together with the per-read side arrays the kernels produce (ref_end, q_start, q_end). */
typedef struct csv_shard csv_shard;
csv_shard *csvgpu_shard_upload(csv_ctx *ctx, const csv_reads *host_reads, uint32_t depth_len);
/* Wrap arrays that already live in HBM (e.g. torch tensors); nothing is copied or owned. */
csv_shard *csvgpu_shard_wrap_dev(csv_ctx *ctx, const csv_reads *dev_reads, uint32_t depth_len);
void       csvgpu_shard_free(csv_ctx *ctx, csv_shard *shard);

/* Result of one chromosome's device pipeline; pointers are device memory owned by the shard
 * and stay valid until the next csvgpu_chr_pipeline_dev() on the same shard or its free. */
typedef struct csv_chr_result {
    uint64_t        n_sig;        /* signatures emitted (all kinds) */
    uint64_t        n_del;        /* of which SVType DEL */
    uint64_t        n_ins;        /* of which SVType INS (CIGARINS + CIGARCLIP) */
    uint64_t        depth_sum;
    uint32_t        depth_nonzero;
    int32_t         min_pts;      /* ceil(mean_cov * min_pts_pct) or 5 (sv_caller.cpp:723-728) */
    double          mean_cov;
    const csv_sig  *sig_del;      /* [n_del] the DEL calls of chr_sv_calls, in vector order (std::copy_if, sv_object.cpp:80) */
    const csv_sig  *sig_ins;      /* [n_ins] the INS calls (CIGARINS + CIGARCLIP), in vector order */
    const int32_t  *label_del;    /* [n_del] DBSCAN labels of sig_del */
    const int32_t  *label_ins;    /* [n_ins] DBSCAN labels of sig_ins */
    const uint32_t *depth;        /* [depth_len] */
    const int32_t  *ref_end;      /* [n_reads] */
    const int32_t  *q_start;      /* [n_reads] */
    const int32_t  *q_end;        /* [n_reads] */
} csv_chr_result;

/* The whole per-chromosome device path of SVCaller::processChromosome up to cluster labels
 * (sv_caller.cpp:692-745 with cnv_caller.cpp:488-543 in front): CIGAR scan -> depth map and mean
 * coverage -> min_pts -> ordering -> per-type interval DBSCAN. Representative selection of
 * mergeSVs (sv_object.cpp:121-244) is host code above this ABI. (Opt-in, that choice has a device form too: csvgpu_chr_merge_select below
 * works on what this call leaves on the shard.)
 * min_pts_pct <= 0 selects the fixed min_pts = 5 (sv_caller.cpp:724-727). */
int csvgpu_chr_pipeline_dev(csv_ctx *ctx, csv_shard *shard, uint32_t min_oplen, uint8_t min_mapq,
                            double eps, double min_pts_pct, csv_chr_result *result);

/* Copy the signatures (sig_del followed by sig_ins: n_sig records) and their labels (label_del followed by
 * label_ins) of the last csvgpu_chr_pipeline_dev() on `shard` to host memory with one synchronisation. */
int csvgpu_chr_fetch(csv_ctx *ctx, csv_shard *shard, const csv_chr_result *result, csv_sig *host_sig, int32_t *host_labels);

/* csvgpu_chr_pipeline_dev + csvgpu_chr_fetch in one call with a single final synchronisation: when the chromosome's
 * n_sig <= capacity the signatures and labels are copied to host_sig / host_labels behind the last kernel and the scalars
 * ride in the same wait. With n_sig > capacity nothing is copied and CSV_ECAPACITY is returned; *result is valid (n_sig
 * says how much room is needed) and csvgpu_chr_fetch() can still fetch. Pass buffers from csvgpu_host_alloc() so that the
 * copies are true asynchronous DMA. */
int csvgpu_chr_pipeline_fetch(csv_ctx *ctx, csv_shard *shard, uint32_t min_oplen, uint8_t min_mapq, double eps, double min_pts_pct,
                              csv_chr_result *result, csv_sig *host_sig, int32_t *host_labels, uint64_t capacity);

/* The same per-chromosome path as a job in three steps, for callers that keep the device busy across their own turn-around:
 *   begin   queues the CIGAR scan, the bucket counts and (for shards whose sortedness is known) the depth pass;
 *   cluster waits for the signature count, queues ordering + DBSCAN and the copies into host_sig / host_labels (capacity records
 *           each; page-locked memory from csvgpu_host_alloc) — and returns without waiting;
 *   end     waits for the job, fills *result, frees the job; CSV_ECAPACITY when the host buffers were too small (the results
 *           are then on the device: csvgpu_chr_fetch).
 * Between cluster(i) and end(i) the caller may begin(i + 1) on the same context — also on the same shard, everything being
 * ordered by the context's stream: the next chromosome's scan then starts on the device the moment this one's last copy is done.
 * csvgpu_chr_pipeline_fetch is begin + cluster + end. */
typedef struct csv_job csv_job;
/* At most CSV_MAX_JOBS jobs may be open (between begin and end / abort) on one context: each holds one of the context's page-locked
 * counter slots. One more csvgpu_chr_job_begin returns NULL ("more than CSV_MAX_JOBS jobs open"). */
#define CSV_MAX_JOBS 16
csv_job *csvgpu_chr_job_begin(csv_ctx *ctx, csv_shard *shard, uint32_t min_oplen, uint8_t min_mapq, double min_pts_pct);
int csvgpu_chr_job_cluster(csv_ctx *ctx, csv_job *job, double eps, csv_sig *host_sig, int32_t *host_labels, uint64_t capacity);
int csvgpu_chr_job_end(csv_ctx *ctx, csv_job *job, csv_chr_result *result);
/* Give up a job after csvgpu_chr_job_cluster (or anything between begin and end) failed: waits for what the job queued, frees it,
 * and leaves csvgpu_last_error() as the failure left it (csvgpu_chr_job_end on an unclustered job would overwrite it). */
int csvgpu_chr_job_abort(csv_ctx *ctx, csv_job *job);

/* ---- mergeSVs' representatives on the device (opt-in; kernels/mergeselect.hip, the rule in contextsv_amd/csrc/sort_select_core.hpp) ----
 * mergeSVs keeps one member of every cluster (and of the noise bucket): with the members sorted by length descending through an UNSTABLE
 * std::sort, the one at slot [max(1, (int)(size * 0.2)) / 2] (sv_object.cpp:190-230). With length ties that member is whatever libstdc++'s
 * introsort leaves there; the device replays the chain of partitions that decides the slot, exactly. What it does not replay is the
 * library's heap-sort fallback (the depth limit 2 floor(log2 size) running out): such a bucket is DECLINED, never answered wrong, and the
 * caller takes the host route (csvgpu_chr_fetch and the host merge) for that contig. Timed under CSV_K_MISC. */

/* The primitive on its own, batched: idx_out[s] = the index inside segment s = keys[seg_off[s] .. seg_off[s + 1]) of the element that
 * libstdc++'s std::sort by key DESCENDING leaves at slot nth[s] of that segment. max_partitions == 0: the library's own depth limit; a
 * smaller positive value is the caller's bound on the partitions per segment. A segment whose chain needs more partitions than the bound is
 * declined: idx_out[s] = UINT32_MAX, declined_out[s] = 1 (declined_out may be NULL). Segments of up to 16 elements need no partition and
 * are never declined. An empty segment: idx_out[s] = UINT32_MAX, declined_out[s] = 0, nth[s] not read. seg_off[0] == 0.
 * CSV_EINVAL: a null array, offsets not ascending, nth[s] beyond its segment, 2^31 or more keys or segments, a split order pending on the
 * context. n_seg == 0 is valid. */
int csvgpu_sort_slot(csv_ctx *ctx, const uint32_t *keys, const uint64_t *seg_off, uint64_t n_seg, const uint64_t *nth, uint32_t max_partitions,
                     uint32_t *idx_out, uint8_t *declined_out);

typedef struct csv_merge_rep {      /* 32 bytes */
    csv_sig  sig;                   /* the chosen member, untouched (read and qpos included: the host cuts the ALT from them) */
    int32_t  label;                 /* the bucket's DBSCAN label; -2 for a pass-through record */
    uint32_t cluster_size;          /* bucket size; 0 for a pass-through record */
    uint32_t status;                /* 0 chosen, 1 pass-through (its type has < 2 signatures: sv_object.cpp:85-92), 2 declined (sig undefined) */
    uint32_t reserved;              /* 0 */
} csv_merge_rep;
typedef struct csv_merge_counts { uint64_t n_rep[2]; uint64_t n_declined[2]; } csv_merge_counts;   /* [0] DEL, [1] INS */

/* One contig's representatives from host arrays (the seam for tests and other callers): sig / labels [n_del + n_ins], the DEL signatures
 * first, each type in chr_sv_calls order with its labels as csvgpu_dbscan_iv gives them (-2 noise, 0 .. k - 1). Per type: buckets by label,
 * ascending, -2 first, members in input order; one record per bucket of two or more members, in bucket order; a type with fewer than two
 * signatures passes them through (status 1; its labels are neither read nor copied). DEL records come first. counts->n_rep: records per type;
 * n_declined: how many of them have status 2.
 * CSV_ECAPACITY: n_rep[0] + n_rep[1] > capacity; counts is valid and nothing is written to rep_out. n_sig / 2 + 2 records always suffice.
 * CSV_EINVAL: a null array, a label below -2 or above 2^31 - 17, 2^31 or more signatures of a type, a split order pending on the context.
 * CSV_EHIP also when a bounded device loop (a radix pass's look-back) gave up. */
int csvgpu_merge_select(csv_ctx *ctx, const csv_sig *sig, const int32_t *labels, uint64_t n_del, uint64_t n_ins, uint32_t max_partitions,
                        csv_merge_rep *rep_out, uint64_t capacity, csv_merge_counts *counts);
/* The same on the still-valid results of the last pipeline on `shard` (csvgpu_chr_pipeline_dev / _fetch, csvgpu_chr_job_end): the signatures
 * and labels stay on the device, 32 bytes per counts and 32 per representative come back. After CSV_ECAPACITY the caller calls again with
 * room, or fetches (csvgpu_chr_fetch) and merges on the host — as it does for a contig with a declined bucket. */
int csvgpu_chr_merge_select(csv_ctx *ctx, csv_shard *shard, const csv_chr_result *result, uint32_t max_partitions, csv_merge_rep *host_rep,
                            uint64_t capacity, csv_merge_counts *counts);

/* csvgpu_chr_job_cluster with the select queued behind the DBSCAN: nothing of the signatures or labels is copied; min(capacity, n_sig / 2 + 2)
 * records and the counts ride behind the last kernel into host_rep / host_counts (page-locked memory from csvgpu_host_alloc), valid once
 * csvgpu_chr_job_end has returned. csvgpu_chr_job_end is called as before: CSV_ECAPACITY when there are more records than `capacity`
 * (host_counts valid; *result valid: csvgpu_chr_merge_select with room, or csvgpu_chr_fetch), CSV_EHIP when a radix pass gave up. The
 * select's workspace is the shard's own (allocated at its first use, grow-only): nothing a job queued ahead uses is touched. */
int csvgpu_chr_job_cluster_select(csv_ctx *ctx, csv_job *job, double eps, uint32_t max_partitions, csv_merge_rep *host_rep, uint64_t capacity,
                                  csv_merge_counts *host_counts);

/* Several chromosomes in flight on one GPU: several contexts (one per host thread, each with its own stream) that share a gate.
 * They queue the scan + depth pair of their jobs onto the gate's ONE stream — so the bandwidth-bound kernels of all lanes run back
 * to back in queue order, with no hand-over between queues — while each context's own stream carries that lane's small kernels
 * (ordering, clustering, copies), which then run beside another lane's pair, and the host merge of one chromosome hides behind
 * the device work of the others. The reference gets its overlap from a thread pool over chromosomes (sv_caller.cpp:827-863);
 * this is the device-side counterpart. Attach the same gate to every context of ONE GPU before running pipelines concurrently;
 * detach with gate == NULL. Jobs on shards that are not coordinate-sorted ignore the gate. */
typedef struct csv_gate csv_gate;
csv_gate *csvgpu_gate_create(void);
/* Creates the gate's stream now rather than at the first job. Streams get the runtime's hardware queues in creation order and a waiting
 * stream holds up the others of its queue: open the gate before creating the lanes' contexts. Optional. */
int csvgpu_gate_open(csv_gate *gate, int device_ordinal);
void csvgpu_gate_destroy(csv_gate *gate);                 /* after every attached context is destroyed or detached */
int csvgpu_set_gate(csv_ctx *ctx, csv_gate *gate);

/* Page-locked host memory for result buffers (hipHostMalloc); NULL on failure. Freed blocks are kept by the context for reuse
 * and released by csvgpu_destroy(), which also releases blocks never freed: do not use them after the context is gone. */
void *csvgpu_host_alloc(csv_ctx *ctx, size_t bytes);
void csvgpu_host_free(csv_ctx *ctx, void *p);

/* The alignment intervals that the last csvgpu_chr_pipeline_dev() computed for every record of `shard`, copied to host. */
int csvgpu_aln_intervals_resident(csv_ctx *ctx, csv_shard *shard, int32_t *ref_end, int32_t *q_start, int32_t *q_end);

/* The same for selected records only: ref_end[i] / q_start[i] / q_end[i] of record rec[i] (the split-read pass needs the intervals of
 * the primaries that have a supplementary record and of those records — a few per cent of a contig; sv_caller.cpp:152, :162). */
int csvgpu_aln_intervals_gather_resident(csv_ctx *ctx, csv_shard *shard, const uint32_t *rec, uint64_t n, int32_t *ref_end, int32_t *q_start, int32_t *q_end);
/* ... of several shards in one call: the records of shard c are rec[rec_off[c] .. rec_off[c+1]), outputs in the same layout. */
int csvgpu_aln_intervals_gather_batch(csv_ctx *ctx, int n_shards, csv_shard *const *shards, const uint32_t *rec, const uint64_t *rec_off,
                                      int32_t *ref_end, int32_t *q_start, int32_t *q_end);

/* The query-name column of a resident shard: qname_hash[i] = std::hash<std::string> (libstdc++) of record i's query name — the value that
 * decides where the reference's unordered_map<std::string, PrimaryAlignment> puts the read (sv_caller.cpp:152). Copied to HBM, owned by the shard. */
int csvgpu_shard_set_qname_hash(csv_ctx *ctx, csv_shard *shard, const uint64_t *qname_hash);

/* §8f-4: which primary alignments survive, and in which order the reference iterates them — for up to 32 contigs in one call.
 * For every contig the reference fills an unordered_map keyed by query name with every record that passes the filter of sv_caller.cpp:145
 * (not SECONDARY/UNMAP/DUP/QCFAIL, mapq >= min_mapq) and is not supplementary, in file order (:137-172); erases the names without a
 * supplementary record (:183-202); then iterates the map (:216, :224). Given the (sorted, distinct) name hashes of the run's supplementary
 * records, this returns per contig the record indices of the surviving primaries in that iteration order: out_rec[out_off[c] .. out_off[c+1]).
 * A record "survives" here when its name HASH is in supp_hash — the caller confirms the names (a 64-bit collision is the only difference).
 * Precondition (caller's to check when it stages the shard): within a contig no two non-supplementary records share a name hash
 * (no repeated query names, no 64-bit collisions) — otherwise the map would hold one node for two records and the host form
 * (host/umap_order.h) has to be used for that contig. CSV_ECAPACITY: out_rec too small, out_off[n_contigs] holds the required count. */
int csvgpu_split_order(csv_ctx *ctx, int n_contigs, csv_shard *const *shards, uint8_t min_mapq, const uint64_t *supp_hash, uint64_t n_supp,
                       uint32_t *out_rec, uint64_t capacity, uint64_t *out_off);
/* The same in two calls, so that the part that needs no supplementary record — the nodes and all but the last epochs of every contig's map:
 * most of the device's work — runs while the caller is still collecting the supplementary records (sv_caller.cpp:146-165 does both in one loop
 * over the file). _begin queues that work on the context's stream and returns; _finish takes the hashes and returns what csvgpu_split_order
 * returns. No other entry point may be called on this context between the two (they share its workspaces); one pending order per context;
 * after CSV_ECAPACITY _finish may be called again with a larger out_rec. */
int csvgpu_split_order_begin(csv_ctx *ctx, int n_contigs, csv_shard *const *shards, uint8_t min_mapq);
/* _begin for a call that holds EVERY contig of the run (sv_caller.cpp:137-172 fills supp_map from the same records): the supplementary
 * records' name hashes are then taken from these shards on the device (same filter, flag 0x800 set), and the whole order — nodes, epochs,
 * survivors — is queued by this call; _finish(ctx, NULL, 0, ...) only waits for it. A caller whose run has supplementary records on contigs
 * that are not in this call must use _begin and pass all hashes to _finish. */
int csvgpu_split_order_begin_self(csv_ctx *ctx, int n_contigs, csv_shard *const *shards, uint8_t min_mapq);
int csvgpu_split_order_finish(csv_ctx *ctx, const uint64_t *supp_hash, uint64_t n_supp, uint32_t *out_rec, uint64_t capacity, uint64_t *out_off);

/* §8f-4, second half: replaces the interval tree and the greedy overlap groups of findSplitSVSignatures (sv_caller.cpp:215-238,
 * insert :964-980, findOverlaps :948-962) for a batch of contigs. Segment c = members [seg_off[c], seg_off[c+1])
 * in the iteration order of that contig's qname map (what csvgpu_split_order returns); member = closed interval
 * [start, end] (start = pos + 1, end = bam_endpos). Output: the groups with more than one member, per segment in
 * seed order; members[] holds indices WITHIN the segment, in findOverlaps' traversal order:
 *   groups of segment c = [seg_group_off[c], seg_group_off[c+1]); members of group g = members[group_off[g] .. group_off[g+1]).
 * Only group_off[0 .. seg_group_off[n_seg]] is written. Any int32_t coordinates are valid (no arithmetic is done on them).
 * *n_members: in = capacity of members[] in entries, out = entries required. CSV_ECAPACITY when the capacity is too small (members shared
 * between groups make the total quadratic in the worst case: k disjoint seeds under L long intervals give k * L entries); nothing but
 * *n_members is then written. CSV_EINVAL: end < start anywhere, offsets not ascending, more than 2^32 - 1 members in the call or
 * entries in the answer. Empty segments and n_seg == 0 are valid. */
int csvgpu_split_groups(csv_ctx *ctx, const int32_t *start, const int32_t *end, const uint64_t *seg_off, uint64_t n_seg,
                        uint64_t *seg_group_off,   /* [n_seg + 1]: first group of each segment */
                        uint64_t *group_off,       /* [seg_off[n_seg] + 1]: there are never more groups than members */
                        uint32_t *members, uint64_t *n_members /* in: capacity of members[], out: count required */);

/* §8f-4, third part: what the reference derives from every overlap group before it makes calls (sv_caller.cpp:248-416): the strand vote
 * (:248-265), the six point sets (:270-347), their DBSCAN1D(eps, min_pts) fits, getLargestCluster (dbscan1d.cpp:72-90) and the medians
 * of the largest clusters — on the device, one 64-byte record per group back.
 * The members (primary alignments that have a supplementary record) and their supplementary records, host pointers, for a batch of
 * contigs: segment c = members [seg_off[c], seg_off[c+1]), as in csvgpu_split_groups. */
typedef struct csv_split_tables {
    uint64_t n_members, n_supp;
    const int32_t *start, *end, *q_start, *q_end;   /* [n_members]: pos + 1, bam_endpos, query_start, query_end of each member (a primary alignment), map iteration order per segment */
    const uint8_t *reverse;                         /* [n_members]: 1 = FLAG 0x10 */
    const uint64_t *supp_off;                       /* [n_members + 1]: member m's supplementary records, file order */
    const int32_t *supp_start, *supp_end, *supp_q_start, *supp_q_end;   /* [n_supp] */
    const uint8_t *supp_flags;                      /* [n_supp]: bit 0 reverse strand, bit 1 on another tid than the primary (then only the flags are read) */
} csv_split_tables;
/* Coordinates (of members, and of the supplementary records on the primary's tid) must lie in [0, 2^31 - 1] with end >= start
 * (q_end may be below q_start); CSV_EINVAL otherwise, nothing reaching the device. Every int difference the reference forms to BUILD
 * the sets (:322-345), and every distance of its DBSCAN1D (dbscan1d.cpp:68-70) on sets 0-3 and 5, is then free of overflow. Set 4 is
 * NOT covered: it holds read distances of both signs, and the distance of two of them, |a - b| in int, overflows once they differ by
 * more than 2^31 - 1 — query coordinates beyond 2^30, which no read has. The reference's own expression is undefined there, and so is
 * the record's set-4 pair (nothing else of the record is affected). */

/* One group's evidence. Sets: 0 primary starts, 1 primary ends, 2 supplementary starts, 3 supplementary ends, 4 signed read distances,
 * 5 reference distances (sets 2, 3: the supplementary records on the primary's tid; 4, 5: those of them on the primary's strand).
 * Points of a set are in the reference's order — members in the group's findOverlaps order, a member's supplementary records in supp_off
 * order — which decides the cluster ids and so, among clusters of equal size, the largest (the lowest id). */
typedef struct csv_split_fit {
    int32_t  median[6];    /* sorted largest cluster [size / 2]; 0 when size == 0 */
    uint32_t size[6];      /* points in the largest cluster (getLargestCluster, dbscan1d.cpp:72-90); 0 = none */
    uint32_t n_members, n_opposite;   /* group size; members with a same-tid supplementary record on the other strand (sv_caller.cpp:248-265) */
    uint32_t reserved[2];  /* 0 */
} csv_split_fit;
/* The inversion vote stays the caller's double expression: (double)n_opposite / (double)n_members > 0.5 (:265). */

/* The fits of given groups — seg_group_off / group_off / members exactly as csvgpu_split_groups (or the host's tree) returns them;
 * out[g] for g < seg_group_off[n_seg]. Requires eps >= 0 and min_pts >= 1 (as csvgpu_dbscan_1d). Sets of more than 512 points are
 * solved by the large-segment path of csvgpu_dbscan_1d inside this call, with the same result. CSV_EINVAL: a null array, offsets not
 * ascending or not ending at the tables' counts, a member index outside its segment or twice in one group, a coordinate out of range, a split order pending on
 * the context. CSV_EHIP also when a bounded device loop (a radix pass's look-back) gave up. Empty segments and n_seg == 0 are valid. */
int csvgpu_split_fits(csv_ctx *ctx, const csv_split_tables *tables, const uint64_t *seg_off, uint64_t n_seg, const uint64_t *seg_group_off,
                      const uint64_t *group_off, const uint32_t *members, double eps, int32_t min_pts, csv_split_fit *out);
/* csvgpu_split_groups and csvgpu_split_fits in one call: the groups are computed by the chain of csvgpu_split_groups from the tables'
 * start / end and consumed where they lie — the member lists never reach the host, so there is no capacity to guess: the workspace is
 * sized from the chain's one readback. seg_group_off[n_seg + 1] and *n_groups = seg_group_off[n_seg] are returned with the records;
 * out has room for tables->n_members records (there are never more groups than members). */
int csvgpu_split_groups_fits(csv_ctx *ctx, const csv_split_tables *tables, const uint64_t *seg_off, uint64_t n_seg, double eps, int32_t min_pts,
                             uint64_t *seg_group_off, csv_split_fit *out, uint64_t *n_groups);

/* §8f-4, the step in front: the tables themselves from the RESIDENT shards — pos, flag and the scan's ref_end / q_start / q_end of the records
 * that take part lie in HBM already (csvgpu_chr_pipeline_dev / the jobs ran on every shard named here), so the caller passes record references
 * instead of gathering the intervals, building the tables and sending them back. Segment c = members [seg_off[c], seg_off[c+1]), all of them
 * records of shards[c]. */
typedef struct csv_split_refs {
    uint64_t n_members, n_supp;
    const uint32_t *member_rec;   /* [n_members]: record index in its segment's shard */
    const uint64_t *supp_off;     /* [n_members + 1] */
    const uint32_t *supp_rec;     /* [n_supp]: record index in the SAME shard (ignored when supp_where != 0) */
    const uint8_t  *supp_where;   /* [n_supp]: 0 same shard; 2 / 3 = on another tid, forward / reverse: the flags byte itself */
} csv_split_refs;
/* The tables of csv_split_tables for these references, copied to the host (the seam for tests and integrators): with S = shards[c] and
 * r = member_rec[m], start = S.pos[r] + 1, end = S.ref_end[r], q_start = S.q_start[r], q_end = S.q_end[r], reverse = FLAG 0x10 of S.flag[r];
 * supp_off as given; an entry with supp_where == 0 the same five from record supp_rec[z] of S (supp_flags = its FLAG 0x10), any other entry
 * supp_flags = supp_where and the four coordinates 0. `out`: the caller sets the eleven pointers to writable arrays of the stated sizes, the call
 * sets n_members / n_supp. One page-locked block each way, one launch, one wait.
 * CSV_EINVAL (nothing written): a null array or shard, offsets not starting at 0, not ascending or not ending at the counts, a record index
 * beyond its shard, supp_where outside {0, 2, 3}, 2^32 - 1 or more members or entries, a split order pending on the context — and a coordinate
 * outside the domain of csvgpu_split_fits (negative, or end < start; members and same-shard entries), which the kernel itself finds: a shard
 * whose coordinates all lie below 2^31 cannot hold one. Empty segments, n_seg == 0 and n_supp == 0 are valid. */
int csvgpu_split_tables_resident(csv_ctx *ctx, uint64_t n_seg, csv_shard *const *shards, const csv_split_refs *refs, const uint64_t *seg_off,
                                 csv_split_tables *out);
/* The product path: those tables built where csvgpu_split_groups_fits' chain reads them and that chain run on them — neither the intervals, the
 * tables nor the groups reach the host; seg_group_off, *n_groups and one record per group come back, byte for byte what
 * csvgpu_split_groups_fits returns on the tables of csvgpu_split_tables_resident. out has room for refs->n_members records. The same CSV_EINVAL
 * cases (the domain is checked wherever the chain runs: a call in which no segment has two members has no group and launches nothing), eps / min_pts
 * as csvgpu_dbscan_1d; CSV_EHIP also when a bounded device loop gave up. */
int csvgpu_split_resident_fits(csv_ctx *ctx, uint64_t n_seg, csv_shard *const *shards, const csv_split_refs *refs, const uint64_t *seg_off,
                               double eps, int32_t min_pts, uint64_t *seg_group_off, csv_split_fit *out, uint64_t *n_groups);

/* csvgpu_window_log2 on the depth map that the last csvgpu_chr_pipeline_dev() left resident in `shard`
 * (region tables and outputs are host memory; the depth map never leaves HBM). */
int csvgpu_window_log2_resident(csv_ctx *ctx, csv_shard *shard, const uint32_t *region_start, const uint32_t *region_end,
                                const int32_t *sample_size, const uint64_t *win_off, uint64_t n_regions, double mean_cov,
                                double *log2_cov, uint32_t *win_start, uint32_t *win_end);

/* csvgpu_window_log2_resident for several shards in one call (the copy-number pass of a whole run: one region table per contig, each
 * evaluated on its own resident depth map; cnv_caller.cpp:76-113): table c has n_regions[c] regions, its win_off[c] starts at 0, its
 * outputs go to log2_cov[c] / win_start[c] / win_end[c]. One transfer in, one launch per shard, one transfer out, one wait. */
int csvgpu_window_log2_resident_many(csv_ctx *ctx, int n_shards, csv_shard *const *shards, const uint32_t *const *region_start,
                                     const uint32_t *const *region_end, const int32_t *const *sample_size, const uint64_t *const *win_off,
                                     const uint64_t *n_regions, const double *mean_cov, double *const *log2_cov, uint32_t *const *win_start,
                                     uint32_t *const *win_end);

/* The copy-number pass's observation vectors on the device (kernels/cnobs.hip; CNVCaller::querySNPRegion, cnv_caller.cpp:65-164): the
 * regions' windows are evaluated as by csvgpu_window_log2_resident_many and consumed where they lie. Regions [reg_off[c], reg_off[c+1])
 * lie on shards[c] and are evaluated against mean_cov[c]; region r has max(sample_size[r], snp_off[r+1] - snp_off[r]) windows, and
 * snp_pos / snp_baf / snp_pfb [snp_off[r], snp_off[r+1]) are its SNP records as SNPSource::queryFlat returns them (the two hash maps'
 * values already resolved per record). */
typedef struct csv_cn_regions {
    int32_t n_shards;
    csv_shard *const *shards;     /* [n_shards] */
    const double   *mean_cov;     /* [n_shards] */
    const uint64_t *reg_off;      /* [n_shards + 1], reg_off[0] == 0; R = reg_off[n_shards] */
    const uint32_t *region_start, *region_end;   /* [R] */
    const int32_t  *sample_size;  /* [R] */
    const uint64_t *snp_off;      /* [R + 1], snp_off[0] == 0; S = snp_off[R] */
    const uint32_t *snp_pos;      /* [S] */
    const double   *snp_baf, *snp_pfb;           /* [S] */
} csv_cn_regions;
/* The seam for tests and integrators: obs_off[R + 1] and, for region r at [obs_off[r], obs_off[r+1]), the observations in the order the
 * reference's unordered_map<std::string,double> of "ws-we" keys iterates its windows (a libstdc++ container: the order is replayed from the
 * library's own rehash policy and std::hash<std::string>): per window in that order the region's SNPs inside [ws, we], both ends inclusive,
 * else one dummy observation (pos = (ws + we) / 2, baf = -1, pfb = 0.5, is_snp = 0); log2_cov is the window's — of the LAST window with that
 * key. *n_obs: in, the capacity of the five arrays in observations; out, the exact count (never above sum of windows + 3 S).
 * CSV_ECAPACITY (obs_off and the arrays untouched, *n_obs set): the capacity is too small — call again with room for *n_obs.
 * CSV_EINVAL (nothing written): a null array, offsets not starting at 0 or not ascending, sample_size <= 0, start > end, a region's end at or
 * above 2^31 - 1 (a window coordinate could reach 2^31: the reference parses its keys back with std::stoi), SNP positions decreasing inside a
 * region, more than 5087 windows in a region, 2^32 - 1 or more windows, records or observations in all, a split order pending on the context.
 * One page-locked block each way; R == 0 is valid. */
int csvgpu_cn_observations_resident_many(csv_ctx *ctx, const csv_cn_regions *regions, uint64_t *obs_off, uint32_t *pos, double *baf, double *pfb,
                                         double *log2_cov, uint8_t *is_snp, uint64_t *n_obs);
/* The product path: windows -> observations -> emissions -> Viterbi without a return to the host in between (csvgpu_viterbi on o1 = log2_cov,
 * o2 = baf, pfb, seq_off = obs_off, bit for bit). Returns obs_off, pos, states[n_obs], loglik[R]; baf / pfb / log2_cov / is_snp only where
 * the pointer is not NULL. *n_obs, CSV_ECAPACITY and CSV_EINVAL as above. One 8-byte readback of the count sizes the Viterbi workspace,
 * then one wait. */
int csvgpu_cn_decode_resident_many(csv_ctx *ctx, const csv_cn_regions *regions, const csv_hmm *hmm, uint64_t *obs_off, uint32_t *pos,
                                   int32_t *states, double *loglik, double *baf, double *pfb, double *log2_cov, uint8_t *is_snp, uint64_t *n_obs);

/* ------------------------------------------------------------------------------------------ */
/* Resident SNP tables (opt-in: the copy-number pass looks its SNPs up on the device; kernels/snptable.hip, the rules in
 * contextsv_amd/csrc/snp_table_core.hpp). A csv_snp_table holds one contig's records in device memory. It is immutable once created; any
 * context of the same device may read it, several at a time. The creators wait for their own kernels before they return; NULL on failure
 * (csvgpu_last_error). Values are copied as bits: a NaN stays that NaN. n == 0 is a valid table.
 * NULL with a message: positions not ascending (checked on the device; the host forms tolerate disorder by scanning, which is outside the
 * device's domain), n or n_af at or above 2^32 - 1, a null array with a count, no memory.
 * What a region [start, end] yields: the records from lower_bound(pos, start) up to the first pos > end, every member of a run of equal
 * positions with the baf of the run's last member (SNPSource::queryFlat, the values the reference's hash maps hold). */
typedef struct csv_snp_table csv_snp_table;
/* The per-record kind (the host mirror's SNPTable): every member of a run carries the pfb of the run's last member with has_pfb, or 0.0 if
 * the run has none. pfb NULL: 0.0 everywhere; has_pfb NULL: no record has one. */
csv_snp_table *csvgpu_snp_table_create(csv_ctx *ctx, const uint32_t *pos, const double *baf, const double *pfb, const uint8_t *has_pfb, uint64_t n);
/* The first-hit kind (the host mirror's SNPFileTable): pfb is decided per region. With lo / hi the first and last position of the region's
 * records and g = lower_bound(af_pos, lo): if g < n_af and af_pos[g] <= hi, every record with pos == af_pos[g] gets af[g]; all others 0.0. */
csv_snp_table *csvgpu_snp_table_create_hits(csv_ctx *ctx, const uint32_t *pos, const double *baf, const uint32_t *af_pos, const double *af,
                                            uint64_t n, uint64_t n_af);
/* The same from device arrays (what csvgpu_vcf_snp_parse_dev leaves, cut to one contig), copied device to device. */
csv_snp_table *csvgpu_snp_table_create_dev(csv_ctx *ctx, const uint32_t *d_pos, const double *d_baf, const double *d_pfb, const uint8_t *d_has_pfb,
                                           uint64_t n);
csv_snp_table *csvgpu_snp_table_create_hits_dev(csv_ctx *ctx, const uint32_t *d_pos, const double *d_baf, const uint32_t *d_af_pos,
                                                const double *d_af, uint64_t n, uint64_t n_af);
/* Waits for ctx's stream, then frees; the caller sees to it that no other context still reads the table. */
void csvgpu_snp_table_free(csv_ctx *ctx, csv_snp_table *table);
uint64_t csvgpu_snp_table_size(const csv_snp_table *table);      /* n; 0 for NULL */
/* The seam for tests and integrators: what queryFlat would append for each of R regions, back to back: region r at
 * [snp_off[r], snp_off[r + 1]) of pos / baf / pfb; a region with start > end yields nothing. *n: in, the capacity of the three arrays in
 * records; out, the exact count. CSV_ECAPACITY (*n set, nothing written, snp_off included): the capacity is too small. CSV_EINVAL: a null
 * array, a table of another device, 2^32 - 1 or more regions or records. */
int csvgpu_snp_table_query(csv_ctx *ctx, const csv_snp_table *table, const uint32_t *region_start, const uint32_t *region_end, uint64_t n_regions,
                           uint64_t *snp_off, uint32_t *pos, double *baf, double *pfb, uint64_t *n);

/* csv_cn_regions without the SNP arrays: tables[c] is shard c's table (NULL: no SNPs), sample_size[r] the floor of region r's window count
 * (it has max(sample_size[r], its records) windows). */
typedef struct csv_cn_table_regions {
    int32_t n_shards;
    csv_shard *const *shards;     /* [n_shards] */
    const csv_snp_table *const *tables;          /* [n_shards] */
    const double   *mean_cov;     /* [n_shards] */
    const uint64_t *reg_off;      /* [n_shards + 1], reg_off[0] == 0; R = reg_off[n_shards] */
    const uint32_t *region_start, *region_end;   /* [R] */
    const int32_t  *sample_size;  /* [R] */
} csv_cn_table_regions;
/* The twins of csvgpu_cn_observations_resident_many / csvgpu_cn_decode_resident_many: byte for byte what those return when they are fed
 * the host's queryFlat arrays for the same regions, with no SNP array going up. The record ranges, the window counts, every offset table,
 * the lists of the two kernel forms and the regions' records in the compact layout are made on the device; one small readback (windows W,
 * records S, per-shard window totals, the decline flag) sizes the workspace and the window launches.
 * *n_obs: in, the capacity; out on CSV_OK, the exact count. A capacity below W + 3 S returns CSV_ECAPACITY right after that readback with
 * *n_obs = W + 3 S, which is always enough, and nothing else is launched.
 * Returns 1 = declined, nothing written, the reason in csvgpu_last_error — what only the device can know: a region whose records call for
 * more than 5087 windows, 2^32 - 1 or more windows, records or observations in all. CSV_EINVAL as above for what the host can see (null
 * arrays, reg_off, sample_size <= 0 or above 5087, start > end, an end at or above 2^31 - 1, a pending split order) and for a table of
 * another device. */
int csvgpu_cn_observations_tables_many(csv_ctx *ctx, const csv_cn_table_regions *regions, uint64_t *obs_off, uint32_t *pos, double *baf, double *pfb,
                                       double *log2_cov, uint8_t *is_snp, uint64_t *n_obs);
int csvgpu_cn_decode_tables_many(csv_ctx *ctx, const csv_cn_table_regions *regions, const csv_hmm *hmm, uint64_t *obs_off, uint32_t *pos,
                                 int32_t *states, double *loglik, double *baf, double *pfb, double *log2_cov, uint8_t *is_snp, uint64_t *n_obs);

/* depth_out[i] = depth[pos[i]] on the depth map resident in `shard`, or -1 where pos[i] >= depth_len: the VCF writer's
 * SUPPORT / DP lookups (SVCaller::getReadDepth, sv_caller.cpp:1332-1344, called at :1306) without moving the map. */
int csvgpu_depth_lookup_resident(csv_ctx *ctx, csv_shard *shard, const uint32_t *pos, uint64_t n, int32_t *depth_out);

/* Copy `bytes` from device memory returned by this library (csv_chr_result pointers) to host memory;
 * synchronous with respect to the context's stream. For host code above the ABI that does not link HIP. */
int csvgpu_download(csv_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes);
/* Device memory for a caller that links the C-ABI alone and chains `_dev` entry points (the host mirror's BAM reader keeps a batch's decoded
 * bytes and the unpacked arrays in such buffers between csvgpu_bgzf_inflate_dev and csvgpu_bam_unpack_dev). alloc: NULL on failure
 * (csvgpu_last_error); free waits for the context's stream first. csvgpu_upload copies host bytes (pageable: through the context's page-locked
 * block, in pieces) to device memory and waits. */
void *csvgpu_dev_alloc(csv_ctx *ctx, size_t bytes);
void  csvgpu_dev_free(csv_ctx *ctx, void *dev_ptr);
int   csvgpu_upload(csv_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes);

/* Device-pointer twins of the clustering / HMM entry points (same semantics as above). */
int csvgpu_dbscan_iv_dev(csv_ctx *ctx, const uint32_t *d_start, const uint32_t *d_end, uint64_t n,
                         double eps, int32_t min_pts, int32_t *d_labels);
int csvgpu_dbscan_1d_dev(csv_ctx *ctx, const int32_t *d_pts, const uint64_t *d_seg_off,
                         uint64_t n_seg, uint64_t n_pts, uint32_t max_seg_len,
                         double eps, int32_t min_pts, int32_t *d_labels);
int csvgpu_window_log2_dev(csv_ctx *ctx, const uint32_t *d_depth, uint32_t depth_len,
                           const uint32_t *d_region_start, const uint32_t *d_region_end,
                           const int32_t *d_sample_size, const uint64_t *d_win_off, uint64_t n_regions,
                           uint64_t n_windows, double mean_cov, double *d_log2_cov,
                           uint32_t *d_win_start, uint32_t *d_win_end);
int csvgpu_viterbi_dev(csv_ctx *ctx, const csv_hmm *hmm, const double *d_o1, const double *d_o2,
                       const double *d_pfb, const uint64_t *d_seq_off, uint64_t n_seq,
                       uint64_t n_obs, int32_t *d_states, double *d_loglik);

/* ------------------------------------------------------------------------------------------ */
/* BGZF members inflated on the device (opt-in: the from-file path decodes on the host by default) */
/* One member (SAMv1 §4.1): the raw DEFLATE stream comp[in_off .. in_off + in_len), which decodes to out_len bytes at out[out_off ..] whose
 * CRC-32 (the member's trailer) is crc32. in_len and out_len are at most 65536. */
typedef struct csv_bgzf_block {
    uint64_t in_off;
    uint64_t out_off;
    uint32_t in_len;
    uint32_t out_len;
    uint32_t crc32;
    uint32_t reserved;
} csv_bgzf_block;  /* 32 bytes */

/* Inflates n_blocks members. status[i] = 0: member i decoded to exactly out_len bytes, its stream was consumed to the last byte (only
 * that byte's padding bits left) and the CRC-32 of the bytes equals crc32 — the bytes are in place. status[i] = 1: declined — the bytes
 * at out_off are unspecified and the caller decodes the member itself (zlib). The decoder declines whatever it does not recognise as a
 * plain, well-formed stream of exactly the announced sizes, so the result never depends on it being right about a corner of the format;
 * whatever the input, it reads nothing outside [in_off, in_off + in_len) and writes nothing outside [out_off, out_off + out_len).
 * Returns the number of declined members (>= 0), or a CSV_E* code: CSV_EINVAL for a null pointer, a member whose ranges leave
 * comp_len / out_len, in_len or out_len above 65536, or output ranges that overlap in the order given (out_off may not decrease).
 * n_blocks == 0 does nothing and returns 0. Timed under CSV_K_MISC.
 * Host pointers: the compressed bytes travel up and the decoded bytes and status back through the context's page-locked block, in pieces
 * (comp may be a mapped file). */
int csvgpu_bgzf_inflate(csv_ctx *ctx, const uint8_t *comp, uint64_t comp_len, const csv_bgzf_block *blocks, uint32_t n_blocks,
                        uint8_t *out, uint64_t out_len, uint8_t *status);
/* Device pointers for comp / out / status (blocks from the host): the decoded bytes stay on the device — the seam for a later
 * record-unpacking kernel. Waits for the kernel (the return value is its count of declined members). */
int csvgpu_bgzf_inflate_dev(csv_ctx *ctx, const uint8_t *d_comp, uint64_t comp_len, const csv_bgzf_block *blocks, uint32_t n_blocks,
                            uint8_t *d_out, uint64_t out_len, uint8_t *d_status);

/* ------------------------------------------------------------------------------------------ */
/* BAM records unpacked on the device (opt-in: the from-file path parses on the host by default) */
/* A decoded BAM record stream bytes[0, len) (what the members of a BGZF file decode to, behind the header; len < 2^32) to the arrays of
 * csv_reads: what the host reader makes of the same bytes from bam1_core_t's fields, bam_get_cigar / bam_get_qname / bam_get_seq and
 * bam_tag2cigar (a CIGAR of more than 65 535 operations is taken from its CG:B,I tag), bit for bit.
 * The outputs of ONE call: every pointer is where this call's first kept record goes (a caller that appends behind an earlier call
 * advances them). pos / flag / mapq [cap_records]; cigar_off [cap_records + 1], cigar [cap_cigar] words. Optional, null = not wanted:
 * seq_off [cap_records + 1] with seq [cap_seq] (4-bit packed, (l_seq + 1) / 2 bytes a record), name_off [cap_records + 1] with name
 * [cap_name] (strnlen within l_name bytes a record, no terminator), name_hash [cap_records] (libstdc++'s std::hash<std::string> of the
 * name: what csvgpu_shard_set_qname_hash takes). An offset array and its data are wanted together. */
typedef struct csv_bam_out {
    int32_t  *pos;
    uint16_t *flag;
    uint8_t  *mapq;
    uint64_t *cigar_off;
    uint32_t *cigar;
    uint64_t *seq_off;
    uint8_t  *seq;
    uint64_t *name_off;
    uint8_t  *name;
    uint64_t *name_hash;
    uint64_t  cap_records, cap_cigar, cap_seq, cap_name;
} csv_bam_out;

/* reasons in csv_bam_counts::status (bits 0-7; bits 8-39: the offset the check failed at) */
enum { CSV_BAM_SHORT = 1,        /* block_size < 32 */
       CSV_BAM_LONG = 2,         /* block_size > 2^30 */
       CSV_BAM_NEG_LSEQ = 3,     /* l_seq < 0 (a kept record) */
       CSV_BAM_FIELDS = 4,       /* name + CIGAR + sequence + qualities longer than the record (a kept record) */
       CSV_BAM_ANCHOR = 5 };     /* anchor missed: no record starts at this anchor */

typedef struct csv_bam_counts {
    uint64_t n_records;          /* whole records in the stream */
    uint64_t kept_first;         /* index of the first kept record among them */
    uint64_t n_kept;             /* records written */
    uint64_t n_cigar, n_seq, n_name;   /* CIGAR words, sequence bytes, name bytes of the kept records */
    uint64_t consumed;           /* offset of the first incomplete record: [consumed, len) is the caller's carry */
    uint64_t status;             /* 0, or why the stream was declined: (offset << 8) | reason, the lowest failing offset */
    uint32_t stopped;            /* a record behind the kept run exists: the contig has ended */
    uint32_t reserved;
} csv_bam_counts;

/* anchors[0 .. n_anchors): strictly ascending offsets in [0, len) that are claimed to be record starts (a BAI's chunk begins and linear-index
 * offsets mapped into the buffer, or a walk of the caller's); anchors[0] IS the first record's start. They only divide the walk along the
 * record chain among the lanes and are never believed: a walk that does not land exactly on the next anchor declines the stream
 * (CSV_BAM_ANCHOR). One anchor is a walk by one lane: correct, and slow.
 * tid >= 0: the records of that contig as the host reader's readContig selects them — a leading run with 0 <= refID < tid is skipped,
 * records are kept while refID == tid and pos < end, the first other record ends the run (counts->stopped). tid < 0: every record.
 * The host reader's checks apply in its order (block_size on every record; l_seq and the fixed part on the kept ones); offsets written are
 * cigar_base / seq_base / name_base + the exclusive sums of the kept records' counts, so that a second call appends behind a first.
 * Returns CSV_OK with the counts filled and the arrays written; 1 when the stream is declined: counts->status says why and where,
 * consumed and the other counts are 0, the outputs are unspecified (nothing outside their capacities is ever written) and the caller parses
 * the bytes itself; CSV_ECAPACITY when a capacity is too small: the exact counts are filled in, nothing is written; CSV_EINVAL for a null
 * pointer, len >= 2^32, no anchor for a non-empty stream (len == 0 does nothing and returns CSV_OK with zero counts), anchors that are not strictly ascending or lie outside [0, len), an offset
 * array without its data — nothing reaches the device then. Whatever the bytes are, nothing outside [0, len) is read beyond the aligned
 * 4-byte word that holds a byte of it. Timed under CSV_K_MISC.
 * _dev: bytes and the outputs are device pointers (anchors and counts the host's): behind csvgpu_bgzf_inflate_dev the bytes never leave
 * the device, and the arrays are what csvgpu_shard_wrap_dev takes. Host pointers: the stream travels up and the arrays back through the
 * context's page-locked block, in pieces. Both wait for their kernels. */
int csvgpu_bam_unpack_dev(csv_ctx *ctx, const uint8_t *d_bytes, uint64_t len, const uint32_t *anchors, uint32_t n_anchors, int32_t tid, int64_t end,
                          uint64_t cigar_base, uint64_t seq_base, uint64_t name_base, const csv_bam_out *d_out, csv_bam_counts *counts);
int csvgpu_bam_unpack(csv_ctx *ctx, const uint8_t *bytes, uint64_t len, const uint32_t *anchors, uint32_t n_anchors, int32_t tid, int64_t end,
                      uint64_t cigar_base, uint64_t seq_base, uint64_t name_base, const csv_bam_out *out, csv_bam_counts *counts);

/* ------------------------------------------------------------------------------------------ */
/* SNP and population-frequency VCF records parsed on the device (opt-in: the host reader parses every line itself by default) */
/* Replaces, with kernels/vcfparse.hip, the per-line work of SNPFile::load and SNPFile::table (host/snp_io.cpp: snp_record_of_line,
 * af_record_of_line) on one batch of whole text lines. The rules of one line are csrc/vcf_record_core.hpp; a line whose decision hangs on
 * a number that the device cannot convert with libc's exact result, or that has more than one sample column, is not decided here but
 * DEFERRED: its offset comes back and the caller parses it with the host function. Kept records and deferred offsets are in file order,
 * duplicates kept. */
#define CSV_VCF_TILE_BYTES 4096u   /* the text is searched for line ends in 16-byte-aligned tiles of this many bytes */
typedef struct csv_vcf_out {
    uint32_t *line_off;      /* [cap] offset of the kept record's line (CHROM starts there) */
    uint32_t *chrom_len;     /* [cap] SNP form only; NULL for the AF form */
    uint32_t *pos;           /* [cap] */
    double   *value;         /* [cap] baf (SNP form) or af (AF form) */
    uint32_t *defer_off;     /* [cap_defer] offsets of the lines the caller parses itself, ascending */
    uint64_t  cap, cap_defer;
} csv_vcf_out;
enum { CSV_VCF_HEADER_LINE = 1 };   /* reason in csv_vcf_counts::status (bits 0-7; bits 8-39: the line's offset): a '#' line */
typedef struct csv_vcf_counts {
    uint64_t n_lines;        /* non-empty lines in front of stop_off */
    uint64_t n_kept, n_deferred;
    uint64_t stop_off;       /* AF form: offset of the first line the device found to be behind the last position, UINT64_MAX if none */
    uint64_t status;         /* 0, or (offset << 8) | reason when declined */
} csv_vcf_counts;

/* text[0 .. len): lines ended by '\n' (the last one may lack it); a '\r' in front of the '\n' is stripped, empty lines are skipped.
 * snp: dp_int / ad_int say whether the header declared FORMAT/DP and FORMAT/AD as Integer. af: the records of `contig` whose POS is in
 * sorted_pos[0 .. n) (ascending, duplicates allowed; n == 0 is taken as a last position of 0) and whose INFO holds needle (the key with its
 * '=', at the field's start or behind ';'); the first line of the contig with POS beyond sorted_pos[n - 1] is the STOP line: its offset is
 * counts->stop_off and nothing at or behind it is reported. A deferred line in front of it may be a STOP line too: the caller finds out.
 * Header lines are the caller's to consume before the call: a line in front of stop_off that begins with '#' declines the batch.
 * Returns CSV_OK; 1 = declined, outputs unspecified, counts->status says why and where; CSV_ECAPACITY = out->cap or out->cap_defer too
 * small, the exact counts filled in, nothing written; CSV_EINVAL, nothing reaching the device: a null pointer, len >= 2^32, sorted_pos not
 * ascending (host-pointer form; the _dev form trusts it), needle_len 0 or above 64, a needle with a tab or a line end in it. The AF form
 * ignores out->chrom_len. len == 0: CSV_OK with zero counts. Whatever the bytes are, nothing outside [0, len) is read beyond the
 * aligned 16-byte piece that holds a byte of it, and nothing is written outside the capacities. Timed under CSV_K_MISC.
 * _dev: text, sorted_pos and the arrays of d_out are device pointers (text at any alignment: what csvgpu_bgzf_inflate_dev left); contig,
 * needle and counts are the host's. Host pointers: the text goes up and the arrays come back through the page-locked block, in pieces. */
int csvgpu_vcf_snp_parse(csv_ctx *ctx, const uint8_t *text, uint64_t len, int dp_int, int ad_int, const csv_vcf_out *out, csv_vcf_counts *counts);
int csvgpu_vcf_snp_parse_dev(csv_ctx *ctx, const uint8_t *d_text, uint64_t len, int dp_int, int ad_int, const csv_vcf_out *d_out, csv_vcf_counts *counts);
int csvgpu_vcf_af_parse(csv_ctx *ctx, const uint8_t *text, uint64_t len, const char *contig, uint32_t contig_len, const char *needle, uint32_t needle_len,
                        const uint32_t *sorted_pos, uint64_t n, const csv_vcf_out *out, csv_vcf_counts *counts);
int csvgpu_vcf_af_parse_dev(csv_ctx *ctx, const uint8_t *d_text, uint64_t len, const char *contig, uint32_t contig_len, const char *needle, uint32_t needle_len,
                            const uint32_t *d_sorted_pos, uint64_t n, const csv_vcf_out *d_out, csv_vcf_counts *counts);

/* ------------------------------------------------------------------------------------------ */
/* Resident shards built on the device from BAM batches (opt-in: the from-file path fills host arrays and uploads them by default) */
/* A builder owns device arrays that grow: batches are appended behind its tail, and csvgpu_shard_builder_finish hands the arrays to a
 * csv_shard of the kind csvgpu_shard_upload makes (padded CIGAR array, sortedness known) — without the host arrays of the reader's BamShard
 * (host/bam_io.cpp readContig) and their upload (host/sv_caller.cpp run). `want`: what is kept beside the reads — the 4-bit packed
 * sequences (for csvgpu_alt_bases_resident), the query names (for the split-read pass, which fetches them), their hashes (what
 * csvgpu_shard_set_qname_hash would upload). One builder is used from one host thread at a time, on contexts of one device. */
typedef struct csv_shard_builder csv_shard_builder;
enum { CSV_SB_SEQ = 1, CSV_SB_NAMES = 2, CSV_SB_NAME_HASH = 4 };
typedef struct csv_shard_sizes { uint64_t n_reads, n_cigar, n_seq, n_name; } csv_shard_sizes;   /* records, CIGAR words, sequence bytes, name bytes */

/* reserve (may be NULL or zeros): room allocated now, as readContig sizes its arrays from the compressed span. NULL on failure. */
csv_shard_builder *csvgpu_shard_builder_create(csv_ctx *ctx, uint32_t want, const csv_shard_sizes *reserve);
/* csvgpu_bam_unpack_dev writing at the builder's tail (BamReader::append per record, host/bam_io.cpp): a sizing pass gives the exact counts,
 * every array that is too small grows (a new block of at least 1.5x the old size, a device-to-device copy, the old block freed), a second
 * pass writes in place with the builder's totals as cigar_base / seq_base / name_base. d_bytes, anchors, tid, end, counts and the return
 * values are that function's: CSV_OK; 1 = declined, NOTHING appended, the builder's sizes unchanged, counts->status says why (the caller
 * parses the bytes itself and appends them with _append_host); CSV_E*. CSV_ECAPACITY never leaves this function; after CSV_ENOMEM (a
 * failed growth) the builder is valid with its old contents, and the same append may be tried again. The CIGAR array always keeps the
 * pad words of an uploaded shard allocated behind its tail. Waits for its kernels. */
int  csvgpu_shard_builder_append_bam(csv_ctx *ctx, csv_shard_builder *b, const uint8_t *d_bytes, uint64_t len, const uint32_t *anchors, uint32_t n_anchors,
                                     int32_t tid, int64_t end, csv_bam_counts *counts);
/* A batch the host parser read (BamReader::append; a batch the device declined): HOST arrays, appended behind the tail. batch->cigar_off,
 * seq_off and name_off are relative to the batch's own arrays (any first value; the span [off[0], off[n_reads]) is taken) and are rebased by
 * the builder's totals. Arrays the builder does not want are ignored; CSV_EINVAL, nothing changed: a wanted one that is null, offsets not
 * monotone, and what csvgpu_shard_upload refuses of a csv_reads. */
int  csvgpu_shard_builder_append_host(csv_ctx *ctx, csv_shard_builder *b, const csv_reads *batch, const uint64_t *seq_off, const uint8_t *seq,
                                      const uint64_t *name_off, const uint8_t *name, const uint64_t *name_hash);
int  csvgpu_shard_builder_sizes(csv_ctx *ctx, const csv_shard_builder *b, csv_shard_sizes *out);
/* The shard csvgpu_shard_upload would make of the appended records (with no record: of zero reads), the arrays handed over, not copied.
 * Both appends keep "pos[i] < pos[i - 1]" in a device word (each batch's first record against the previous tail), so the shard's sortedness
 * is known, as after an upload (the upload's loop over pos, api/shard.hip). With CSV_SB_NAME_HASH the hashes are in place as after
 * csvgpu_shard_set_qname_hash. Consumes the builder, also on failure (NULL). The arrays are plain device memory: once this has returned the
 * shard may be used and freed through another context of the same device, like an uploaded one. */
csv_shard *csvgpu_shard_builder_finish(csv_ctx *ctx, csv_shard_builder *b, uint32_t depth_len);
void csvgpu_shard_builder_destroy(csv_ctx *ctx, csv_shard_builder *b);

/* What a resident shard holds, copied to the host (any shard; n_seq / n_name are 0 where it holds no sequences / names): the BamShard's
 * pos / flag / mapq and query names for the split-read pass (host/split_caller.cpp), which are small. Any output may be NULL.
 * fetch_names: CSV_EINVAL when name_off / name are asked of a shard without names, or name_hash of one without hashes. */
int  csvgpu_shard_sizes(csv_ctx *ctx, const csv_shard *shard, csv_shard_sizes *out);
/* Bytes of device memory the shard's CIGAR array takes, padding and (16-bit form) the escape tables included: 4 (n_cigar + pad) at 32 bits;
 * 2 (n_cigar rounded up to 512 + pad) + 4 (pieces + 1) + 8 (escapes + 1) at 16 bits. n_cigar of csvgpu_shard_sizes counts ops either way. */
uint64_t csvgpu_shard_cigar_bytes(const csv_shard *shard);
int  csvgpu_shard_fetch_reads(csv_ctx *ctx, csv_shard *shard, int32_t *pos, uint16_t *flag, uint8_t *mapq, uint64_t *cigar_off, uint32_t *cigar);
int  csvgpu_shard_fetch_names(csv_ctx *ctx, csv_shard *shard, uint64_t *name_off, uint8_t *name, uint64_t *name_hash);
/* Frees the packed sequences of a built shard (the largest of its arrays: half a byte per base). csvgpu_alt_bases_resident returns
 * CSV_EINVAL afterwards. CSV_OK also when there is none. */
int  csvgpu_shard_drop_sequences(csv_ctx *ctx, csv_shard *shard);
/* Replaces the base loop of SVCaller::toSVCall (host/sv_caller.cpp:47-62; the reference's sv_caller.cpp:572-590, :607-625) on the
 * sequences a built shard holds: item i, len = out_off[i + 1] - out_off[i], writes len characters at out + out_off[i] — when
 * ((uint64_t)qpos[i] + len + 1) / 2 <= the BYTES of record read[i]'s packed sequence, the bases from query offset qpos[i] on through the
 * table "=ACMGRSVTWYHKDBN" with R Y K M S W B D H V turned into N (for an odd l_seq the last byte's pad nibble is inside the bound and
 * decodes to whatever it holds, as on the host); otherwise len times N. out_off has n + 1 entries.
 * CSV_EINVAL, nothing launched or written: read[i] >= the shard's records, out_off not non-decreasing, a shard without sequences (uploaded,
 * wrapped, built without CSV_SB_SEQ, or dropped). Indices and offsets go up and the characters come back through the page-locked block;
 * one launch, one wait. Timed under CSV_K_MISC. */
int  csvgpu_alt_bases_resident(csv_ctx *ctx, csv_shard *shard, const uint32_t *read, const uint32_t *qpos, const uint64_t *out_off, uint64_t n, char *out);

/* ------------------------------------------------------------------------------------------ */
/* The reference genome loaded and queried on the device (opt-in: the host loader keeps every contig as a string by default) */
/* Replaces, with kernels/fasta.hip, the line loop of ReferenceGenome::setFilepath and the cut of ::query (host/fasta_query.cpp). The rules
 * are csrc/fasta_core.hpp: lines end at '\n' only (a '\r' stays), a non-empty line that begins with '>' is a header whose name runs to the
 * first blank, every other line's bytes are kept in file order in ONE device array, and a record per named header owns the run of kept
 * bytes that the host loader would store under it (residues in front of the first header or under an empty-named header fall to the next
 * named one; kept bytes that no named header follows are dropped). Records are in file order, duplicates of a name kept: a lookup by name
 * takes the LAST record of that name, as the loader's map does. One builder or genome is used from one host thread at a time, on
 * contexts of one device. */
typedef struct csv_genome_builder csv_genome_builder;
typedef struct csv_genome csv_genome;
typedef struct csv_genome_counts {
    uint64_t n_records;      /* named headers */
    uint64_t n_name_bytes;   /* their names, back to back */
    uint64_t total_bases;    /* bytes that belong to a record */
    uint64_t n_text_bytes;   /* what was appended */
    uint64_t n_lines;        /* ... and its line ends */
} csv_genome_counts;

/* reserve_bytes: room for that many bases allocated now (the file's size: the array never grows then). NULL on failure. */
csv_genome_builder *csvgpu_genome_builder_create(csv_ctx *ctx, uint64_t reserve_bytes);
/* The next len < 2^32 bytes of the FASTA text. A call's text may be cut ANYWHERE — inside a header line, inside a name, between '\r' and
 * '\n': what crosses the cut (whether the text is inside a line, that line's kind, the partial name, whether the open header is named)
 * is carried by the builder. The array grows as csvgpu_shard_builder's do; after CSV_ENOMEM (a failed growth) or any other failure the
 * builder is valid with its old contents and the same append may be tried again. CSV_EINVAL, nothing reaching the device: a null pointer,
 * len >= 2^32, 2^32 line ends or more in one call. len == 0 does nothing. Whatever the bytes are, nothing outside [0, len) is read beyond
 * the aligned 16-byte piece that holds a byte of it. Timed under CSV_K_MISC; waits for its kernels.
 * _dev: text is a device pointer at any alignment (what csvgpu_bgzf_inflate_dev left). Host pointer: the text goes up through the
 * page-locked block, in pieces. */
int  csvgpu_genome_builder_append(csv_ctx *ctx, csv_genome_builder *b, const uint8_t *text, uint64_t len);
int  csvgpu_genome_builder_append_dev(csv_ctx *ctx, csv_genome_builder *b, const uint8_t *d_text, uint64_t len);
/* The text has ended (a final unterminated line counts). The array is handed over, not copied. Consumes the builder, also on failure
 * (NULL): a contig of 2^32 bytes or more is refused, as the loader's uint32 length could not hold it. */
csv_genome *csvgpu_genome_builder_finish(csv_ctx *ctx, csv_genome_builder *b);
void csvgpu_genome_builder_destroy(csv_ctx *ctx, csv_genome_builder *b);
void csvgpu_genome_free(csv_ctx *ctx, csv_genome *g);
/* counts is always filled. Record i's name is names[name_off[i] .. name_off[i + 1]) (name_off [cap_records + 1], names [cap_name_bytes]),
 * its bases length[i] (length [cap_records]). CSV_ECAPACITY, nothing written, when a capacity is too small: a first call with zero
 * capacities sizes the second. */
int  csvgpu_genome_describe(csv_ctx *ctx, const csv_genome *g, uint64_t cap_records, uint64_t cap_name_bytes, uint64_t *name_off, char *names, uint32_t *length,
                            csv_genome_counts *counts);
/* Item i: the cut [pos_start[i], pos_end[i]] of record record[i] (1-based inclusive, both decremented with uint32 wrap; empty when
 * pos_end >= length or pos_start > pos_end — ReferenceGenome::query) written at out + out_off[i]; mask != 0 turns R Y K M S W B D H V of
 * either case into N (the VCF writer's REF rule). out_off has n + 1 entries, and out_off[i + 1] - out_off[i] must be the cut's length, which
 * the caller knows from the lengths. CSV_EINVAL, nothing launched or written: a record index beyond the genome, out_off decreasing, an
 * item whose room is not its cut's length. Nothing outside the genome's array is read and nothing outside [out_off[0], out_off[n]) is
 * written. Items and offsets go up and the bytes come back through the page-locked block; one launch, one wait. Timed under CSV_K_MISC. */
int  csvgpu_genome_fetch(csv_ctx *ctx, const csv_genome *g, const uint32_t *record, const uint32_t *pos_start, const uint32_t *pos_end, const uint64_t *out_off,
                         uint64_t n, int mask, char *out);

/* ------------------------------------------------------------------------------------------ */
/* Resident SNP columns built on the device from VCF text (opt-in: the host reader merges the parsed records per contig by default) */
/* A builder takes batches of whole VCF data lines, decides them as csvgpu_vcf_snp_parse does and keeps the records in device arrays that
 * grow as csvgpu_shard_builder's do. The parsed records of a batch interleave contigs: the builder cuts them into CHROM RUNS on the device
 * (a kept record starts a run when it is the call's first kept record or its CHROM — the chrom_len bytes at line_off — differs in length
 * or in a byte from the previous KEPT record's; skipped and deferred lines between two kept records break nothing) and hands back one
 * small table of runs, whose names the caller maps to contig ids below 2^16. _finish orders every record by (contig id, order key), the
 * key of a device record being text_base + line_off, and leaves per-contig pos / baf columns in device memory, from which tables and the
 * population parse are made without the host arrays going up again. Replaces the `keep` lambda and the merge loop of SNPFile::load and
 * the `sorted` copy of SNPFile::table (host/snp_io.cpp); rules in csrc/snp_build_core.hpp, kernels in kernels/snpbuild.hip. One builder is
 * used from one host thread at a time, on contexts of one device. Launches are timed under CSV_K_MISC. */
typedef struct csv_snp_builder csv_snp_builder;
typedef struct csv_snp_columns csv_snp_columns;
typedef struct csv_snp_runs {            /* the caller's HOST arrays */
    uint32_t *run_first;                 /* [cap_runs] the run's first kept record, counted inside the call */
    uint32_t *run_line_off;              /* [cap_runs] that record's line offset: the run's CHROM starts there */
    uint32_t *run_chrom_len;             /* [cap_runs] */
    uint32_t *defer_off;                 /* [cap_defer] offsets of the lines the caller parses itself, ascending */
    uint64_t  cap_runs, cap_defer;
} csv_snp_runs;
typedef struct csv_snp_append_counts {
    uint64_t n_lines, n_kept, n_deferred;        /* as csv_vcf_counts */
    uint64_t n_runs;                             /* the call's runs */
    uint64_t first_run;                          /* the builder's run count before the call: run r of the call is global run first_run + r */
    uint64_t status;                             /* 0, or (offset << 8) | reason when declined, as csv_vcf_counts */
} csv_snp_append_counts;

/* reserve_records: room allocated now (0: the arrays grow from nothing). NULL on failure. */
csv_snp_builder *csvgpu_snp_builder_create(csv_ctx *ctx, uint64_t reserve_records);
/* One batch (text, dp_int, ad_int as csvgpu_vcf_snp_parse). Returns CSV_OK: the kept records are behind the builder's tail, the run table
 * and the deferred offsets in *out; 1 = declined (a '#' line behind data; counts->status as csv_vcf_counts), nothing appended, the run
 * count unchanged: the caller parses the batch and uses _append_host; CSV_ECAPACITY: cap_runs or cap_defer too small, the exact counts
 * filled in, nothing appended or written; CSV_ENOMEM: a growth failed, the builder keeps its contents and the same append may be
 * repeated; CSV_EINVAL, nothing reaching the device: a null pointer, len >= 2^32, text_base + len > 2^48. A call that would bring the
 * builder to 2^31 runs or more is CSV_EINVAL too, but only the device can count the runs: the batch has been parsed by then, and nothing
 * is appended.
 * len == 0: CSV_OK with zero counts. Calls may come in any order of text_base: the key orders the records. Waits for its kernels.
 * _dev: text is a device pointer at any alignment (what csvgpu_bgzf_inflate_dev left); out and counts are the host's. */
int  csvgpu_snp_builder_append(csv_ctx *ctx, csv_snp_builder *b, const uint8_t *text, uint64_t len, uint64_t text_base, int dp_int, int ad_int,
                               const csv_snp_runs *out, csv_snp_append_counts *counts);
int  csvgpu_snp_builder_append_dev(csv_ctx *ctx, csv_snp_builder *b, const uint8_t *d_text, uint64_t len, uint64_t text_base, int dp_int, int ad_int,
                                   const csv_snp_runs *out, csv_snp_append_counts *counts);
/* Records the host parser kept (snp_record_of_line on a deferred line; a declined batch): HOST arrays, each record with its own contig id
 * and order key (its line's offset in the file). CSV_EINVAL, nothing changed: an id at or above 2^16, a key at or above 2^48, a null array
 * with a count. CSV_ENOMEM as above. */
int  csvgpu_snp_builder_append_host(csv_ctx *ctx, csv_snp_builder *b, uint64_t n, const uint32_t *contig_id, const uint64_t *order_key, const uint32_t *pos,
                                    const double *baf);
/* run_contig[r]: the contig id of global run r (HOST array, n_runs == the builder's run count). One stable order by (contig id, order
 * key): one radix sort of the packed key over the bits that vary, a gather of pos / baf; then per contig its count, its offset and whether
 * it is ascending (pos[i] >= pos[i - 1] inside the contig), all on the device. Consumes the builder, also on failure. NULL with a message:
 * n_runs is not the builder's run count, a run_contig at or above 2^16, two records of a contig with one order key (found on the device
 * behind the sort: the caller broke the contract), 2^32 - 1 records or more, no memory. A contig that is not ascending is no error: it is
 * flagged and can be fetched; csvgpu_snp_columns_table and _af_parse refuse it, and the host route serves it. */
csv_snp_columns *csvgpu_snp_builder_finish(csv_ctx *ctx, csv_snp_builder *b, const uint32_t *run_contig, uint64_t n_runs);
void csvgpu_snp_builder_destroy(csv_ctx *ctx, csv_snp_builder *b);

/* The contigs that hold a record, by ascending id: *n_contigs is always set; CSV_ECAPACITY, nothing written, when cap is below it. Any
 * array may be NULL. */
int  csvgpu_snp_columns_describe(const csv_snp_columns *cols, uint64_t cap, uint32_t *contig_id, uint64_t *count, uint8_t *ascending, uint64_t *n_contigs);
/* One contig's columns to the host, in file order (count entries each; either may be NULL). CSV_EINVAL: an id that holds no record. */
int  csvgpu_snp_columns_fetch(csv_ctx *ctx, const csv_snp_columns *cols, uint32_t contig_id, uint32_t *pos, double *baf);
/* csvgpu_vcf_af_parse / _dev with sorted_pos = the contig's resident pos (an ascending contig's file order is its sorted order), nothing
 * going up but the text: counts, decline, capacity and deferral are that function's. CSV_EINVAL also for an id that holds no record, a
 * contig that is not ascending, columns of another device. */
int  csvgpu_snp_columns_af_parse(csv_ctx *ctx, const csv_snp_columns *cols, uint32_t contig_id, const uint8_t *text, uint64_t len, const char *contig,
                                 uint32_t contig_len, const char *needle, uint32_t needle_len, const csv_vcf_out *out, csv_vcf_counts *counts);
int  csvgpu_snp_columns_af_parse_dev(csv_ctx *ctx, const csv_snp_columns *cols, uint32_t contig_id, const uint8_t *d_text, uint64_t len, const char *contig,
                                     uint32_t contig_len, const char *needle, uint32_t needle_len, const csv_vcf_out *d_out, csv_vcf_counts *counts);
/* csvgpu_snp_table_create_hits of the contig's columns (copied device to device) and the caller's HOST af arrays. NULL with a message as
 * there, and for an id that holds no record or a contig that is not ascending. The table does not depend on the columns afterwards. */
csv_snp_table *csvgpu_snp_columns_table(csv_ctx *ctx, const csv_snp_columns *cols, uint32_t contig_id, const uint32_t *af_pos, const double *af, uint64_t n_af);
/* Plain device memory: any context of the device may read the columns. Waits for ctx's stream, then frees. */
void csvgpu_snp_columns_free(csv_ctx *ctx, csv_snp_columns *cols);

/* ------------------------------------------------------------------------------------------ */
/* VCF records formatted on the device (opt-in: the host writer assembles them by default) */
/* The record lines of the reference's SVCaller::saveToVCF (sv_caller.cpp:1067-1330) with the SUPPORT / DP values of ::getReadDepth
 * (:1332-1344), assembled where their inputs lie: REF from the genome's base array, the depth from the contigs' resident depth maps
 * (csvgpu_depth_lookup_resident's value at POS), ALT from the caller's bytes. Replaces the record loop of writeVCF (host/vcf_writer.cpp);
 * the header stays the host's. Rules in csrc/vcf_format_core.hpp, kernels in kernels/vcfformat.hip: a lane per call sizes its line, an
 * exclusive sum places the lines, and every 16-byte piece of the text has one owning lane, so a REF of 1 MB costs what 1 MB of short lines
 * costs. The text is the concatenation of the contigs' lines in the order given, byte for byte the host writer's.
 *   calls       contig t's are calls[call_off[t] .. call_off[t + 1]); call i's ALT string is alts[alt_off[i] .. alt_off[i + 1]).
 *   line_status [call_off[n_contigs]] the core's status byte of every call (disposition in bits 0-1: 0 written, 1 skipped as UNKNOWN /
 *               NEUTRAL, 2 an INS at the first position: counted, no line; 4 REF was empty: N and <DEL> / <INS>; 8 assembly-gap filtered;
 *               16 POS outside the depth map: 0 printed), from which the caller replays the host's warnings. May be NULL.
 *   counts      always filled on CSV_OK, 1 and CSV_ECAPACITY.
 * Returns CSV_OK; 1 = declined, nothing written to text, counts->declined_why names the rule (vcffmt::Why: a likelihood of 2^63 or more,
 * a DEL whose length does not fit a positive int or that starts at 2^31, an enum outside its table, a REF asked of a contig the genome has
 * not — for these the host throws or is undefined — or a text of 2^32 bytes or more): the caller runs the host writer;
 * CSV_ECAPACITY = cap < text_bytes, nothing written, call again with room; CSV_EINVAL, nothing launched: a null array, offsets that
 * decrease or do not start at 0, a record index beyond the genome, a method string above 64 bytes, a genome of another device, a contig
 * with a call to write and no shard or no depth map in it. Nothing outside [0, text_bytes) is written, and nothing outside the genome's
 * array, the ALT bytes and the depth maps is read. Launches are timed under CSV_K_MISC; one readback sizes the text, one brings it down.
 * _dev: text is a device pointer (the seam a device BGZF writer starts from); every other array is the host's. */
typedef struct csv_vcf_call { uint32_t start, end; int32_t sv_type, cluster_size; double hmm_likelihood; int64_t id;
                              uint32_t aln_flags; int32_t genotype, cn_state, aln_offset; } csv_vcf_call;      /* 48 bytes: csvhost_call's layout */
typedef struct csv_vcf_contig { const char *name; uint32_t name_len; int64_t genome_record;  /* -1: the genome has none */
                                csv_shard *shard;                                             /* its depth map; NULL only with no call to write */
                                const uint32_t *gap_start, *gap_end; uint32_t n_gaps; } csv_vcf_contig;  /* BED rows as loaded, file order */
typedef struct csv_vcf_format_counts { uint64_t text_bytes, n_lines; uint32_t total, unclassified, gap_filtered, declined_why; } csv_vcf_format_counts;

int  csvgpu_vcf_format(csv_ctx *ctx, const csv_genome *g, const csv_vcf_contig *contigs, uint32_t n_contigs, const uint64_t *call_off, const csv_vcf_call *calls,
                       const uint64_t *alt_off, const char *alts, const char *method, uint32_t method_len, uint64_t cap, char *text, uint8_t *line_status,
                       csv_vcf_format_counts *counts);
int  csvgpu_vcf_format_dev(csv_ctx *ctx, const csv_genome *g, const csv_vcf_contig *contigs, uint32_t n_contigs, const uint64_t *call_off, const csv_vcf_call *calls,
                           const uint64_t *alt_off, const char *alts, const char *method, uint32_t method_len, uint64_t cap, char *d_text, uint8_t *line_status,
                           csv_vcf_format_counts *counts);

#ifdef CSV_TEST_HOOKS
/* Test build only (libcsvgpu_testhooks.so, -DCSV_TEST_HOOKS; libcsvgpu.so does not export it): the next n guarded device allocations
 * inside the library fail as if HBM were exhausted (error-path tests of the signature-buffer growth in csvgpu_chr_job_cluster and of the
 * array growth in csvgpu_shard_builder_append_bam). */
void csvgpu_test_fail_next_alloc(int n);

/* Test build only: the device primitives under every kernel chain (kernels/sort.hip, launch_prefix_max of kernels/depth.hip), called
 * unchanged on host arrays that are staged through the context's arena and stream as the chains stage theirs. Every device buffer a
 * primitive may write is followed by CSVGPU_TEST_GUARD elements filled with a sentinel byte; the workspace is filled with it too.
 *
 * csvgpu_test_radix_sort: launch_radix_sort_u64 of n (key, val) pairs (onesweep != 0: the one-launch passes where the launcher takes
 *   them). keys_out / vals_out [n]: the buffer pair the launcher names as the result. *gave_up: the word of radix_sort_gave_up, 0 where
 *   that returns null. *tail_ok: 1 if the guards of all four ping-pong buffers and of the workspace still hold the sentinel.
 * csvgpu_test_radix_sort_devn: launch_radix_sort_u64_devn queued with n_bound, the count n (<= n_bound) in a device word; only the n
 *   pairs are staged. *tail_ok: 1 if slots [n, n_bound + guard) of all four buffers and the workspace's guard still hold the sentinel.
 *   CSV_EINVAL when the launcher refuses n_bound (it is asked before anything is staged when n_bound >= 2^30: nothing is launched).
 * csvgpu_test_exclusive_sum: launch_exclusive_sum_u32 on data[n], in place. csvgpu_test_prefix_max: launch_prefix_max, in[n] -> out[n].
 *   Both return CSV_EHIP ("wrote past n") when a guard lost its sentinel. */
#define CSVGPU_TEST_GUARD 4096
int csvgpu_test_radix_sort(csv_ctx *ctx, const uint64_t *keys, const uint32_t *vals, uint64_t n, int32_t key_bits, int32_t onesweep,
                           uint64_t *keys_out, uint32_t *vals_out, uint32_t *gave_up, int32_t *tail_ok);
int csvgpu_test_radix_sort_devn(csv_ctx *ctx, const uint64_t *keys, const uint32_t *vals, uint64_t n, uint64_t n_bound, int32_t key_bits,
                                uint64_t *keys_out, uint32_t *vals_out, uint32_t *gave_up, int32_t *tail_ok);
int csvgpu_test_exclusive_sum(csv_ctx *ctx, uint32_t *data, uint64_t n);
int csvgpu_test_prefix_max(csv_ctx *ctx, const int32_t *in, uint64_t n, int32_t *out);
#endif

#ifdef __cplusplus
}
#endif
#endif /* CSVGPU_H */
