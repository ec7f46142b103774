// sv_caller.h — host mirror of the per-chromosome CIGAR path of the reference's SVCaller
// (src/sv_caller.cpp:506-537 findCIGARSVs, :539-661 processCIGARRecord, :692-745 processChromosome) and of
// the depth pass in front of it (src/cnv_caller.cpp:415-556), working on a decoded struct-of-arrays
// shard instead of an htslib iterator. All per-read and per-signature work runs on the GPU behind the
// C-ABI; the host keeps only the order-defining representative choice (mergeSVs) and the string fields.
#pragma once
#include <cstdint>
#include <memory>
#include <functional>
#include <string>
#include <vector>

#include "../../../include/csvgpu.h"
#include <unordered_map>

#include "cnv_caller.h"
#include "khmm.h"
#include "split_caller.h"
#include "sv_object.h"
#include "vcf_writer.h"

// 4-bit packed read sequences (BAM encoding, two bases per byte, high nibble first); optional.
// The device form: `resident` is a shard built with its sequences (csvgpu_shard_builder_finish, CSV_SB_SEQ) and the host arrays are null.
// toSVCall then cannot cut the bases: it leaves a note (read, query offset, length) in the call's ALT field, and patchResidentAlts replaces the
// notes of a contig's merged calls with the bases in one csvgpu_alt_bases_resident call. Only processResidentChromosome (and so
// processChromosome's callers and run()) takes this form; the pipelined passes over many shards take host arrays or none.
struct SeqStore {
    const uint64_t *seq_off = nullptr;   // [n_reads+1] byte offset of each read's packed sequence
    const uint8_t *seq = nullptr;
    csv_shard *resident = nullptr;
};

struct ChrStats {
    uint64_t n_signatures = 0, n_del = 0, n_ins = 0;
    uint64_t depth_sum = 0;
    uint32_t depth_nonzero = 0;
    double mean_chr_cov = 0.0;
    int dbscan_min_pts = 0;
    double ms_device = 0.0, ms_host_merge = 0.0;
};

// One contig of a run: decoded records (+ optional sequences and query names for the split-read pass) and its SNPs.
struct ChromosomeInput {
    std::string name;
    csv_reads reads{};                      // host arrays, file order
    csv_shard *resident = nullptr;          // not null: the contig's records are this resident shard already (BamReadOptions::device_shard) — run() takes it
                                            // (and frees it) instead of uploading; reads.pos / flag / mapq are the host's, reads.cigar_off and reads.cigar null;
                                            // seq, when given, is the SeqStore's device form over the same shard. OWNERSHIP passes with the struct: whoever
                                            // receives it from ContigSource::next frees the shard (csvgpu_shard_free on a context of its device) — run() does,
                                            // from the moment next() has returned, on every way out
    const SeqStore *seq = nullptr;
    uint32_t depth_len = 0;                 // contig length + 1
    const std::vector<std::string> *qnames = nullptr;   // [n_reads]; nullptr: this contig takes no part in the split-read pass
    const SNPSource *snps = nullptr;        // nullptr: no SNPs (every window gets the dummy observation)
};

// Contigs one at a time: next() fills `out` and returns false at the end. The arrays behind `out` (reads, sequences, query
// names) only have to stay valid until the following call — run() uploads them and keeps what it needs; `out.snps` must live
// until run() returns.
struct ContigSource {
    virtual ~ContigSource() = default;
    virtual bool next(ChromosomeInput &out) = 0;
};

// A contig whose records are already resident in HBM (csvgpu_shard_upload / csvgpu_shard_wrap_dev) together with the small
// per-record host arrays the host-side passes read: the decoded, staged form of one chromosome. `split` carries pos / flag / mapq
// and the query names (hash + identity, see split_caller.h); its ref_end / q_start / q_end are filled by the run from the scan
// kernel's per-read outputs. split.qhash == nullptr: the contig takes no part in the split-read pass.
struct ResidentContig {
    std::string name;
    csv_shard *shard = nullptr;
    uint32_t depth_len = 0;                 // contig length + 1
    const SeqStore *seq = nullptr;          // for the 50-bp insertion ALT strings (may be null: N's)
    const SNPSource *snps = nullptr;        // nullptr: no SNPs
    SplitContig split;
};

// Wall time of each pass of one run (the order of SVCaller::run, sv_caller.cpp:804-945) and what went through it.
struct RunStageTimes {
    double ms_cigar = 0;        // depth + CIGAR scan + ordering + DBSCAN + mergeSVs, all contigs
    double ms_cigar_cn = 0;     // runCIGARCopyNumberPrediction, all contigs (with lanes: beside the split-read chain, on a lane's context)
    double ms_split_fetch = 0;  // alignment intervals device -> host
    double ms_split = 0;        // findSplitSVSignatures (its second half when the first ran beside the CIGAR pass)
    double ms_split_prepare = 0; // its first half — primaries / supplementaries, the qname map's order, survivors; inside ms_cigar's wall time when lanes are used
    double ms_split_cn = 0;     // runSplitReadCopyNumberPredictions
    double ms_merge_split = 0;  // mergeSVs(0.1, 2, true) on the split calls + concatenation
    double ms_merge_final = 0;  // mergeSVs(0.1, 2, true) on the union
    double ms_vcf = 0;
    double ms_total = 0;
    uint64_t n_reads = 0, n_signatures = 0, n_cigar_calls = 0, n_cigar_cn_regions = 0, n_split_calls = 0, n_final_calls = 0;
};

// How runResident schedules its work around the CIGAR pass. Results never depend on these fields: the defaults are the production
// schedule, and the others exist so that tests can force each branch that timing otherwise decides.
struct RunSchedule {
    // The copy-number predictions and every later step of the contigs merged so far, in batches inside the CIGAR pass (with lanes):
    // Timed — one when the split pass's first half is done, another whenever three more contigs are merged, while eight or more are still
    // to come; None; AllAtOnce — one batch of every contig, once all are merged; EveryThree — whenever three more are merged, to the last.
    enum class EarlyBatches { Timed, None, AllAtOnce, EveryThree };
    EarlyBatches early_batches = EarlyBatches::Timed;
    bool split_beside_pass = true;          // contigs that go through no early batch get their split chain beside the pass (false: behind it)
    bool split_order_self = true;           // a run's split order in one call when it holds every contig (false: _begin + the collected hashes)
    int prepare_delay_ms = 0;               // the split pass's first half starts this much later (makes it outlast the CIGAR pass)
};

struct RunParams {
    double dbscan_epsilon = 0.1;            // --eps          (input_data.cpp:18-37)
    double dbscan_min_pts_pct = 0.1;        // --min-pts-pct
    int sample_size = 20;                   // --sample-size
    uint32_t min_cnv_length = 2000;         // --min-cnv
    bool cigar_svs = true, cigar_cn = true, split_svs = true, merge_split_svs = true, merge_final_svs = true;   // sv_caller.cpp:749-753
    bool split_order_on_device = true;      // contigs staged with unique query-name hashes (SplitContig::unique_names) get the qname map's order from csvgpu_split_order
    bool split_groups_on_device = false;    // the overlap groups of the split-read pass (interval tree + greedy seeding, sv_caller.cpp:215-238) from csvgpu_split_groups, one
                                            // call per batch of contigs, instead of the host tree on one pool thread per contig; the calls do not depend on it
    bool split_fits_on_device = false;      // what the split-read pass derives from every overlap group (point sets, DBSCAN1D fits, largest clusters, medians, strand vote;
                                            // sv_caller.cpp:248-416) from csvgpu_split_fits — with split_groups_on_device from csvgpu_split_groups_fits, the groups then staying
                                            // on the device — instead of the host's sets and one DBSCAN1D batch; the calls do not depend on it
    bool split_tables_on_device = false;    // the members' and supplementary records' tables of the split-read pass built on the device from the resident shards
                                            // (csvgpu_split_resident_fits): no interval gather, no members on the pool, no upload; groups and fits then come from the
                                            // device too, whatever the two switches above say; the calls do not depend on it
    bool cn_observations_on_device = false; // the copy-number passes' observation vectors built on the device from the window kernel's output and decoded there
                                            // (csvgpu_cn_decode_resident_many) instead of windows back, assembleRegion on the pool and observations up again; the
                                            // calls do not depend on it
    bool inflate_on_device = false;         // runBam: the BAM's BGZF blocks inflated on the device (csvgpu_bgzf_inflate on a context of the reader's own, created on
    int inflate_device = 0;                 // device `inflate_device` — the run's — for the run's length) instead of on the host's threads; whatever the device declines is
                                            // decoded on the host, every block is CRC-checked either way; the records, and so the calls, do not depend on it
    bool unpack_on_device = false;          // runBam: every batch's records unpacked on the device (csvgpu_bam_unpack, BamReadOptions::device_unpack) on the reader's own
                                            // context — the inflate's when both are set — instead of by the host parser; a batch the device declines goes through
                                            // the host parser, so the records, and so the calls, do not depend on it
    bool shard_on_device = false;           // runBam (implies unpack_on_device): every contig's resident shard is built on the device from the unpacked batches
                                            // (BamReadOptions::device_shard) and handed to the run — no host arrays, no csvgpu_shard_upload; the 50-base ALT strings
                                            // are cut from the shard's own sequences (csvgpu_alt_bases_resident), which are dropped afterwards; the calls do not
                                            // depend on it
    bool overlap_split_prepare = true;      // runResident with lanes: the split-read pass's first half (qname map order on the device, survivors) beside the CIGAR pass
                                            // (false: after it — the big kernels then have the device to themselves: depth 0.53 of peak instead of 0.48, the step 10 % longer)
    int host_threads = 0;                   // host threads of the split-read and copy-number passes over contigs / regions (0: the hardware's); results do not depend on it
    bool save_cnv = false;                  // --save-cnv: <vcf.output_dir>/CNVCalls.json (main.cpp:109-118, sv_caller.cpp:929-931)
    std::string snp_vcf;                    // --snp: the sample's SNP VCF (runBam; "" = no SNPs, every window gets the dummy observation)
    std::string pfb_table;                  // --pfb: "<chr>=<gnomAD VCF>" table
    std::string ethnicity;                  // --eth: AF_<eth> instead of AF
    const ReferenceGenome *ref_genome = nullptr;   // with vcf.output_dir set: write <output_dir>/output.vcf at the end (sv_caller.cpp:943-945)
    VCFOptions vcf;
    RunSchedule schedule;
};

struct BamRunStats {
    uint64_t n_contigs = 0, n_reads = 0, n_cigar = 0, bam_bytes = 0;
    double ms_decode = 0.0;          // wall time spent waiting for decoded contigs (decode not hidden behind the device)
    double ms_total = 0.0;
    // RunParams::unpack_on_device: batches the device unpacked / the host parser read, anchors given to the device, batches whose decoded
    // bytes never came to the host (BamReader::UnpackStats, summed over the contigs)
    uint64_t unpack_batches_device = 0, unpack_batches_host = 0, unpack_anchors = 0, unpack_batches_kept_on_device = 0;
    // RunParams::shard_on_device: contigs that reached the run as resident shards; batches that went into them from the host parser's arrays
    uint64_t contigs_resident = 0, unpack_batches_appended_host = 0;
};

// A SplitGroupSource that asks csvgpu_split_groups on `ctx` (SplitParams::device_groups); the caller keeps the context alive and uses it from the
// thread that runs the split pass only.
std::unique_ptr<SplitGroupSource> makeDeviceGroupSource(csv_ctx *ctx);
// A SplitFitSource that asks csvgpu_split_fits / csvgpu_split_groups_fits on `ctx` (SplitParams::device_fits); same conditions.
std::unique_ptr<SplitFitSource> makeDeviceFitSource(csv_ctx *ctx);

class SVCaller {
public:
    explicit SVCaller(csv_ctx *ctx) : ctx(ctx) {}
    int min_mapq = 20;       // sv_caller.h:72 of the reference
    // Opt-in: the representative choice of the CIGAR merge made on the device (csvgpu_chr_job_cluster_select): only the representatives' records
    // come back and the merge threads materialise SVCalls from them. A contig with a declined bucket, or whose records overflowed twice, takes
    // the host route (csvgpu_chr_fetch + mergeOrdered): the call set is the same either way. merge_max_partitions: the device's bound on the
    // partitions per bucket (0: the library's own depth limit).
    bool merge_on_device = false;
    // Opt-in, runBam: the SNP VCF (and the population files) parsed on the device (SNPDeviceOptions of host/snp_io.h, on a context of the
    // run's own); with snp_tables_on_device the contigs' SNP tables are built there and stay resident, so that the copy-number pass takes
    // the table route by itself. Beside merge_on_device, not in RunParams: csvhost_run_options is pinned.
    bool snp_parse_on_device = false, snp_tables_on_device = false;
    // The run's output.vcf with its record lines assembled on the device (VCFOptions::format_on_device; host/vcf_writer.h): one
    // csvgpu_vcf_format call where the reference genome is on the device, the host loop otherwise. Same file. Beside the switches above.
    bool vcf_format_on_device = false;
    uint32_t merge_max_partitions = 0;
    // which route the contigs of this process took since the last reset (all callers, all lanes), and the buckets the device declined
    struct MergeRouteStats { uint64_t contigs_device = 0, contigs_host_declined = 0, contigs_host_overflow = 0, buckets_declined = 0; };
    static MergeRouteStats mergeRouteStats(bool reset = false);
    int min_oplen = 50;      // sv_caller.cpp:566

    // Depth pass + CIGAR pass + CIGAR merge of one chromosome. `reads` are host arrays; they are uploaded,
    // the device pipeline runs, labels and signatures come back, and mergeSVs' representative choice runs
    // here. On return chr_sv_calls == the reference's vector after mergeSVs(chr_sv_calls, eps, min_pts, false).
    // If keep_shard != nullptr the resident shard (depth map etc.) is handed to the caller, who frees it.
    void processChromosome(const std::string &chr, const csv_reads &reads, const SeqStore *seq, uint32_t depth_len,
                           double dbscan_epsilon, double dbscan_min_pts_pct, std::vector<SVCall> &chr_sv_calls,
                           ChrStats &stats, csv_shard **keep_shard = nullptr);

    // Same, for a shard that is already resident (benchmark / multi-pass use).
    void processResidentChromosome(const std::string &chr, csv_shard *shard, const SeqStore *seq, double dbscan_epsilon,
                                   double dbscan_min_pts_pct, std::vector<SVCall> &chr_sv_calls, ChrStats &stats);

    // Many resident shards back to back, software-pipelined the way a whole-genome run is: while the device runs shard
    // i+1 (scan -> depth -> ordering -> DBSCAN), a host worker thread does shard i's representative choice. The reference
    // gets this overlap from its chromosome thread pool (sv_caller.cpp:827-863); here one GPU stream + one merge thread.
    // calls[i] / stats[i] correspond to shards[i] (the same shard may appear several times).
    void processResidentChromosomesPipelined(const std::vector<csv_shard *> &shards, const SeqStore *seq, double dbscan_epsilon,
                                             double dbscan_min_pts_pct, std::vector<std::vector<SVCall>> &calls,
                                             std::vector<ChrStats> &stats);
    // (seqs[i] belongs to shards[i]; an empty vector = no sequences)
    void processResidentChromosomesPipelined(const std::vector<csv_shard *> &shards, const std::vector<const SeqStore *> &seqs, double dbscan_epsilon,
                                             double dbscan_min_pts_pct, std::vector<std::vector<SVCall>> &calls,
                                             std::vector<ChrStats> &stats);

    // Several chromosomes in flight on one GPU: every lane is a context of its own (own stream; attach one csv_gate to all of them so
    // that their scan + depth pairs run back to back on the gate's stream) and runs processResidentChromosomesPipelined on its shards in its own pair of threads.
    struct Lane {
        csv_ctx *ctx; std::vector<csv_shard *> shards; std::vector<const SeqStore *> seqs; /* per shard, or empty */
        bool merge_on_device = false; uint32_t merge_max_partitions = 0;       // the lane's caller takes them
    };
    // Which rank of `world` takes which shard: longest processing time first over the weights (read counts), ties by index — the partition
    // `contextsv_amd.parallel.assign_shards` makes for bench.py --gpus N (the reference runs the chromosomes as independent pool tasks,
    // sv_caller.cpp:827-863; a rank's shards are what it stages and passes to runResident, the merged calls are gathered once at the end).
    static std::vector<int> assignShards(const std::vector<double> &weights, int world);

    static void processResidentLanes(const std::vector<Lane> &lanes, const SeqStore *seq, double dbscan_epsilon, double dbscan_min_pts_pct,
                                     std::vector<std::vector<std::vector<SVCall>>> &calls, std::vector<std::vector<ChrStats>> &stats,
                                     const std::function<void(size_t lane, size_t k)> &on_merged = {}, int min_mapq = 20, int min_oplen = 50,
                                     const std::function<void(size_t lane, size_t k)> &on_device = {});
    // called by processResidentChromosomesPipelined's merge threads when shard i's calls and statistics are final (any thread; may be empty)
    std::function<void(size_t)> on_merged;
    // called by processResidentChromosomesPipelined when shard i's device chain is over — depth map, alignment intervals and its statistics
    // (mean coverage) are final, its calls not yet: the host merge follows (the calling thread; may be empty)
    std::function<void(size_t)> on_device;

    // Pass ordering of SVCaller::run (sv_caller.cpp:747-946) over in-memory contigs: depth + CIGAR pass + CIGAR merge per
    // contig -> CIGAR copy-number predictions -> split-read signatures -> their copy-number predictions ->
    // mergeSVs(0.1, 2, keep_noise) on the split calls -> concatenation -> final mergeSVs(0.1, 2, keep_noise).
    // Every contig's shard (reads, depth map) stays resident in HBM until the run ends; the VCF writer's SUPPORT / DP values are
    // gathered from those resident maps.
    void run(const std::vector<ChromosomeInput> &contigs, const CHMM &hmm, const RunParams &params,
             std::unordered_map<std::string, std::vector<SVCall>> &whole_genome_sv_calls);
    void run(ContigSource &source, const CHMM &hmm, const RunParams &params,
             std::unordered_map<std::string, std::vector<SVCall>> &whole_genome_sv_calls);

    // The same run over contigs that are already resident in HBM — one *step* of the whole-genome benchmark: the CIGAR pass of all
    // contigs through `lanes` (contexts of this GPU that share a gate; the contigs are spread over them by read count, longest
    // processing time first; one lane = this caller's own context when `lanes` is empty), then the passes of run() in the
    // reference's order. Nothing is uploaded or freed; the contigs can be run again.
    void runResident(const std::vector<ResidentContig> &contigs, const std::vector<csv_ctx *> &lanes, const CHMM &hmm, const RunParams &params,
                     std::unordered_map<std::string, std::vector<SVCall>> &whole_genome_sv_calls, std::vector<ChrStats> *stats = nullptr,
                     RunStageTimes *times = nullptr);

    // The same run fed from a coordinate-sorted, indexed BAM (reference: SVCaller::run(const InputData&) opening the file three
    // times per contig, sv_caller.cpp:747-863): each contig is decoded once by BamReader (threads = inflate threads) while the
    // previous one is on the device. chromosomes empty = every contig of the header (the reference's default), else the listed
    // ones (--chr). The contig length is the BAM header's (cnv_caller.cpp:482).
    void runBam(const std::string &bam_path, const std::vector<std::string> &chromosomes, int threads, const CHMM &hmm, const RunParams &params,
                std::unordered_map<std::string, std::vector<SVCall>> &whole_genome_sv_calls, struct BamRunStats *bam_stats = nullptr);

    // signature -> SVCall with the reference's field values (sv_caller.cpp:569-643)
    static SVCall toSVCall(const csv_sig &s, const SeqStore *seq);
    // the ALT notes toSVCall left in `calls` for a SeqStore in its device form -> the bases, cut on the device from `shard`'s sequences
    static void patchResidentAlts(csv_ctx *ctx, csv_shard *shard, std::vector<SVCall> &calls);
    static void mergeSignaturesWithLabels(const csv_sig *sig, const int32_t *labels, uint64_t n, const SeqStore *seq, std::vector<SVCall> &merged);
    // The host half of processChromosome on its own: ordered signatures (DEL block then INS block) + their labels -> merged calls.
    static void mergeOrdered(const csv_sig *sig, const int32_t *labels, uint64_t n_del, uint64_t n_ins, const SeqStore *seq, std::vector<SVCall> &chr_sv_calls, bool share_pool = true);

private:
    csv_ctx *ctx;
    struct SplitSetup;
    struct PassOverlap;                      // runResident's work beside the CIGAR pass
    std::unique_ptr<SplitSetup> makeSplitSetup(std::vector<ResidentContig> &contigs, const RunParams &P);
    // everything of run() behind the CIGAR pass: CIGAR copy-number predictions, split-read signatures + their predictions, the two
    // final merges, the VCF (sv_caller.cpp:865-945). stats[i] belongs to contigs[i]; `overlap`: what was done beside the pass (or null).
    void finishRun(std::vector<ResidentContig> &contigs, const std::vector<ChrStats> &stats, const CHMM &hmm, const RunParams &P,
                   std::unordered_map<std::string, std::vector<SVCall>> &whole_genome_sv_calls, RunStageTimes &T, PassOverlap *overlap = nullptr);
    struct DeviceOut {                       // what the device chain of one shard hands to the host merge: page-locked result buffers
        csv_ctx *ctx = nullptr;
        csv_sig *sig = nullptr;
        int32_t *lab = nullptr;
        uint64_t cap = 0, n_del = 0, n_ins = 0;
        // merge_on_device: the representatives' records and their counts (page-locked); use_rep: the merge reads them, not sig / lab
        csv_merge_rep *rep = nullptr;
        csv_merge_counts *cnt = nullptr;
        uint64_t rep_cap = 0, n_rep = 0;
        bool use_rep = false;
        DeviceOut() = default;
        DeviceOut(const DeviceOut &) = delete;
        DeviceOut &operator=(const DeviceOut &) = delete;
        ~DeviceOut() { release(); releaseRep(); }
        void release() { if (ctx) { csvgpu_host_free(ctx, sig); csvgpu_host_free(ctx, lab); } sig = nullptr; lab = nullptr; cap = 0; }
        void releaseRep() { if (rep_ctx) { csvgpu_host_free(rep_ctx, rep); csvgpu_host_free(rep_ctx, cnt); } rep = nullptr; cnt = nullptr; rep_cap = 0; }
        void reserve(csv_ctx *c, uint64_t n);
        void reserveRep(csv_ctx *c, uint64_t n);
        csv_ctx *rep_ctx = nullptr;
    };
    void runDeviceChain(const std::string &chr, csv_shard *shard, double eps, double pct, DeviceOut &out, ChrStats &st);
    // behind csvgpu_chr_job_end of a select job (rc: what it returned): the records are in place, or selected again with room, or — a declined
    // bucket, a second overflow — the signatures and labels are fetched for the host merge
    void finishSelect(csv_shard *shard, const csv_chr_result &res, int rc, DeviceOut &out);
    static void hostMerge(const std::string &chr, const DeviceOut &in, const SeqStore *seq, std::vector<SVCall> &chr_sv_calls, ChrStats &st, bool share_pool = true);
};
