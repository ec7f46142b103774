// run.cpp — whole runs: SVCaller::run over host arrays, runResident over a staged genome, runBam from a file. What the caller may set of a
// run arrives as one csvhost_run_options (csvhost_abi.h), decoded by run_params_from and passed on as it is.
#include <atomic>
#include <mutex>

#include "abi.hpp"
#include "../dbscan.h"
#include "../log.h"
#include "../par.h"
#include "../umap_order.h"

// v's calls flat at out[k ..] while there is room, each with `tid`; k counts them all
static void append_flat(const std::vector<SVCall> &v, int32_t tid, csvhost_call *out, int32_t *out_tid, uint64_t cap, uint64_t &k)
{
    for (const SVCall &c : v) {
        if (k < cap) { out[k] = flat_call(c); out_tid[k] = tid; }
        k++;
    }
}

extern "C" {

const char *csvhost_last_error(void) { return csvhost_abi::last_error().c_str(); }
void csvhost_set_context(csv_ctx *ctx) { csvhost::set_context(ctx); }
void csvhost_set_quiet(int q) { csvhost::set_quiet(q != 0); }

// ---- whole run (SVCaller::run mirror) over concatenated contig arrays -----------------------------
// reads of contig t = [read_off[t], read_off[t+1]); cigar_off is global over the concatenated cigar array; SNPs of contig t =
// [snp_off[t], snp_off[t+1]); qname of read i = "r<qname_id[i]>". Output: merged calls with contig id, contigs ascending.
int csvhost_run(csv_ctx *ctx, int n_contigs, const uint64_t *read_off, const uint32_t *depth_len, const int32_t *pos, const uint16_t *flag,
                const uint8_t *mapq, const uint64_t *cigar_off, const uint32_t *cigar, const uint32_t *qname_id,
                const uint64_t *snp_off, const uint32_t *snp_pos, const double *snp_baf, const double *snp_pfb, const uint8_t *snp_has,
                const csv_hmm *hmm, const csvhost_run_options *opt,
                csvhost_call *out, int32_t *out_tid, uint64_t cap, uint64_t *n_out,
                const csvhost_fasta *fasta, const char *vcf_dir, const char *gap_path, const char *file_date,
                char *alt_buf, uint64_t alt_cap, uint64_t *alt_off)
{
    GUARD({
        std::vector<ChromosomeInput> contigs((size_t)n_contigs);
        std::vector<std::vector<uint64_t>> local_off((size_t)n_contigs);
        std::vector<std::vector<std::string>> qn((size_t)n_contigs);
        std::vector<SNPTable> tabs((size_t)n_contigs);
        for (int t = 0; t < n_contigs; t++) {
            const uint64_t r0 = read_off[t], r1 = read_off[t + 1], n = r1 - r0;
            local_off[t].resize(n + 1);
            for (uint64_t i = 0; i <= n; i++) local_off[t][i] = cigar_off[r0 + i] - cigar_off[r0];
            qn[t].resize(n);
            for (uint64_t i = 0; i < n; i++) qn[t][i] = "r" + std::to_string(qname_id[r0 + i]);
            tabs[t] = snp_table(snp_pos + snp_off[t], snp_baf + snp_off[t], snp_pfb + snp_off[t], snp_has + snp_off[t], snp_off[t + 1] - snp_off[t]);
            ChromosomeInput &c = contigs[t];
            c.name = "contig" + std::to_string(t);
            c.reads.n_reads = n; c.reads.n_cigar = local_off[t][n];
            c.reads.pos = pos + r0; c.reads.flag = flag + r0; c.reads.mapq = mapq + r0; c.reads.tid = nullptr;
            c.reads.cigar_off = local_off[t].data(); c.reads.cigar = cigar + cigar_off[r0];
            c.depth_len = depth_len[t]; c.qnames = &qn[t]; c.snps = &tabs[t];
        }
        RunParams P = run_params_from(*opt);
        set_vcf_output(P, fasta, vcf_dir, gap_path, file_date);
        SVCaller caller(ctx);
        std::unordered_map<std::string, std::vector<SVCall>> calls;
        caller.run(contigs, chmm_from_pod(hmm), P, calls);
        uint64_t k = 0, alt_used = 0;
        if (alt_off) alt_off[0] = 0;
        for (int t = 0; t < n_contigs; t++) {
            for (const SVCall &c : calls[contigs[t].name]) {
                if (k < cap) {
                    out[k] = flat_call(c); out_tid[k] = t;
                    if (alt_off) {                     // ALT strings, concatenated; truncated once alt_cap is reached
                        const uint64_t len = std::min<uint64_t>(c.alt_allele.size(), alt_cap - alt_used);
                        if (alt_buf && len) memcpy(alt_buf + alt_used, c.alt_allele.data(), len);
                        alt_used += len;
                        alt_off[k + 1] = alt_used;
                    }
                }
                k++;
            }
        }
        *n_out = k;
    })
}

// ---- a staged genome: contigs resident in HBM + the host arrays of the host-side passes (SVCaller::runResident) -----------
struct csvhost_genome {
    bool merge_on_device = false;               // csvhost_genome_merge_on_device
    uint32_t merge_max_partitions = 0;
    struct Contig {
        std::string name;
        int32_t global_tid = 0;
        csv_ctx *ctx = nullptr;                 // the context the shard was uploaded with (frees it)
        csv_shard *shard = nullptr;
        uint32_t depth_len = 0;
        uint64_t n_reads = 0, n_cigar = 0;
        std::vector<int32_t> pos; std::vector<uint16_t> flag; std::vector<uint8_t> mapq;
        std::vector<uint64_t> qhash, name_id;
        bool unique_names = false;
        SNPTable snps;
    };
    std::vector<std::unique_ptr<Contig>> contigs;
    ~csvhost_genome() { for (auto &c : contigs) { c->snps.dropResident(); if (c->shard) csvgpu_shard_free(c->ctx, c->shard); } }
};

csvhost_genome *csvhost_genome_create(void) { return new csvhost_genome(); }
void csvhost_genome_free(csvhost_genome *g) { delete g; }

// Stage one contig: upload the records (the shard stays resident), keep pos / flag / mapq and the query-name hash + identity of
// every record on the host. Record i's query name is "r<global_tid>_<qname_id[i]>" (what the synthetic BAM writer calls it), so a
// contig hashes the same whichever rank or lane it lands on (name_style 0: "r<id>", the naming of csvhost_run). SNPs: snp_pos / snp_baf (n_snp, sorted; no population frequency).
int csvhost_genome_add(csvhost_genome *g, csv_ctx *ctx, const char *name, int32_t global_tid, const csv_reads *reads, uint32_t depth_len,
                       const uint32_t *qname_id, int name_style /* 0: "r<id>" (names shared across contigs), 1: "r<tid>_<id>" */,
                       const uint32_t *snp_pos, const double *snp_baf, const double *snp_pfb /* nullable: 0.0 */, const uint8_t *snp_has_pfb /* nullable: none */,
                       uint64_t n_snp)
{
    GUARD({
        std::unique_ptr<csvhost_genome::Contig> c(new csvhost_genome::Contig());
        c->name = name; c->global_tid = global_tid; c->ctx = ctx; c->depth_len = depth_len;
        c->n_reads = reads->n_reads; c->n_cigar = reads->n_cigar;
        c->shard = csvgpu_shard_upload(ctx, reads, depth_len);
        if (!c->shard) throw std::runtime_error(std::string("genome_add: ") + csvgpu_last_error(ctx));
        const uint64_t n = reads->n_reads;
        c->pos.assign(reads->pos, reads->pos + n); c->flag.assign(reads->flag, reads->flag + n); c->mapq.assign(reads->mapq, reads->mapq + n);
        if (qname_id) {
            c->qhash.resize(n); c->name_id.resize(n);
            char buf[48];
            const int pre = name_style ? snprintf(buf, sizeof buf, "r%d_", (int)global_tid) : snprintf(buf, sizeof buf, "r");
            for (uint64_t i = 0; i < n; i++) {
                const int len = pre + snprintf(buf + pre, sizeof buf - (size_t)pre, "%u", qname_id[i]);
                c->qhash[i] = csvhost::std_string_hash(buf, (size_t)len);
                c->name_id[i] = (name_style ? ((uint64_t)(uint32_t)global_tid << 32) : 0) | qname_id[i];
            }
            // the query-name column goes to HBM with the shard; and, once, is any name hash shared by two non-supplementary records?
            // (then the reference's map holds ONE node for them and the contig's order is replayed on the host instead of the device)
            if (csvgpu_shard_set_qname_hash(ctx, c->shard, c->qhash.data()) != CSV_OK) throw std::runtime_error(std::string("genome_add: ") + csvgpu_last_error(ctx));
            std::vector<uint64_t> h;
            h.reserve(n);
            for (uint64_t i = 0; i < n; i++) if (!(reads->flag[i] & 0x800)) h.push_back(c->qhash[i]);
            std::sort(h.begin(), h.end());
            c->unique_names = std::adjacent_find(h.begin(), h.end()) == h.end();
        }
        if (n_snp) {
            c->snps.pos.assign(snp_pos, snp_pos + n_snp); c->snps.baf.assign(snp_baf, snp_baf + n_snp);
            if (snp_pfb) c->snps.pfb.assign(snp_pfb, snp_pfb + n_snp); else c->snps.pfb.assign(n_snp, 0.0);
            if (snp_has_pfb) c->snps.has_pfb.assign(snp_has_pfb, snp_has_pfb + n_snp); else c->snps.has_pfb.assign(n_snp, 0);
        }
        g->contigs.push_back(std::move(c));
    })
}

// the same from a generated shard (+ generated SNPs when with_snps)
int csvhost_genome_add_synth(csvhost_genome *g, csv_ctx *ctx, const char *name, int32_t global_tid, const csvhost_synth *syn, uint64_t snp_seed, int with_snps)
{
    const SynthShard &sh = syn->sh;
    std::vector<uint32_t> sp; std::vector<double> sb;
    if (with_snps) synth_snps(snp_seed, sh.depth_len - 1, sp, sb);
    const csv_reads r = sh.view();
    return csvhost_genome_add(g, ctx, name, global_tid, &r, sh.depth_len, sh.qname_id.data(), 1, sp.data(), sb.data(), nullptr, nullptr, sp.size());
}

// Opt-in: every contig's SNP table resident on its own context's device (on != 0: created, a refusal leaves that contig host-only; 0: freed).
// While they are there the copy-number passes of csvhost_genome_run look the SNPs up on the device. Returns the number of resident tables.
int csvhost_genome_snp_tables_resident(csvhost_genome *g, int on)
{
    int n = 0;
    for (auto &c : g->contigs) {
        if (!on) c->snps.dropResident();
        else if (c->snps.resident || c->snps.makeResident(c->ctx)) n++;
    }
    return n;
}

// Opt-in: the CIGAR merge's representatives of csvhost_genome_run chosen on the device (SVCaller::merge_on_device; max_partitions: the
// device's bound per bucket, 0 = the library's). Same calls and statistics either way; csvhost_merge_route_stats says which route the contigs took.
int csvhost_genome_merge_on_device(csvhost_genome *g, int on, uint32_t max_partitions)
{
    g->merge_on_device = on != 0; g->merge_max_partitions = max_partitions;
    return 0;
}

uint64_t csvhost_genome_n_contigs(const csvhost_genome *g) { return g->contigs.size(); }
void csvhost_genome_contig_info(const csvhost_genome *g, uint64_t i, uint64_t *n_reads, uint64_t *n_cigar, uint32_t *depth_len, int32_t *global_tid, csv_shard **shard)
{
    const auto &c = *g->contigs[i];
    if (n_reads) *n_reads = c.n_reads;
    if (n_cigar) *n_cigar = c.n_cigar;
    if (depth_len) *depth_len = c.depth_len;
    if (global_tid) *global_tid = c.global_tid;
    if (shard) *shard = c.shard;
}

// One step: SVCaller::runResident over every staged contig, as `opt` says (its schedule fields change no result). Calls come back grouped
// by contig in staging order with the contig's GLOBAL tid in out_tid; stats[i] per contig.
int csvhost_genome_run(csvhost_genome *g, csv_ctx *ctx, int n_lanes, csv_ctx *const *lane_ctxs, const csv_hmm *hmm, const csvhost_run_options *opt,
                       csvhost_call *out, int32_t *out_tid, uint64_t cap, uint64_t *n_out, csvhost_stage_times *times, csvhost_chr_stats *stats)
{
    GUARD({
        std::vector<ResidentContig> rc(g->contigs.size());
        for (size_t i = 0; i < rc.size(); i++) {
            auto &c = *g->contigs[i];
            rc[i].name = c.name; rc[i].shard = c.shard; rc[i].depth_len = c.depth_len; rc[i].snps = &c.snps;
            rc[i].split.n = c.n_reads; rc[i].split.pos = c.pos.data(); rc[i].split.flag = c.flag.data(); rc[i].split.mapq = c.mapq.data();
            if (!c.qhash.empty()) { rc[i].split.qhash = c.qhash.data(); rc[i].split.name_id = c.name_id.data(); rc[i].split.unique_names = c.unique_names; }
        }
        const RunParams P = run_params_from(*opt);
        std::vector<csv_ctx *> lanes(lane_ctxs, lane_ctxs + (n_lanes > 0 ? n_lanes : 0));
        SVCaller caller(ctx);
        caller.merge_on_device = g->merge_on_device; caller.merge_max_partitions = g->merge_max_partitions;
        // the call map of a genome is 3e4 records with strings in them: it is torn down beside whatever the caller does next — the next run,
        // in a loop of runs: the previous run's teardown is waited for when this run hands over its own map, not before it starts
        static std::mutex teardown_mu;                                          // (runs of different genomes may come from different threads)
        static csvhost::WorkerThreads::Ticket teardown = nullptr;
        auto swap_teardown = [](csvhost::WorkerThreads::Ticket next) {
            csvhost::WorkerThreads::Ticket prev;
            { std::lock_guard<std::mutex> l(teardown_mu); prev = teardown; teardown = next; }
            if (prev) csvhost::WorkerThreads::instance().wait(prev);
        };
        auto calls_p = std::make_shared<std::unordered_map<std::string, std::vector<SVCall>>>();
        std::unordered_map<std::string, std::vector<SVCall>> &calls = *calls_p;
        struct Hand {                                                           // (also when runResident throws)
            std::shared_ptr<std::unordered_map<std::string, std::vector<SVCall>>> &p;
            decltype(swap_teardown) &swap;
            ~Hand() { auto dead = std::move(p); swap(csvhost::WorkerThreads::instance().start([dead]() mutable { dead.reset(); })); }
        } hand{calls_p, swap_teardown};
        std::vector<ChrStats> cs;
        RunStageTimes T;
        {
            csvhost::TraceScope tr_run("genome_run: runResident (with its locals' teardown)");
            caller.runResident(rc, lanes, chmm_from_pod(hmm), P, calls, &cs, &T);
        }
        csvhost::TraceScope tr_flat("genome_run: calls -> flat records");
        uint64_t k = 0;
        for (size_t i = 0; i < rc.size(); i++) {
            const std::vector<SVCall> &v = calls[rc[i].name];
            append_flat(v, g->contigs[i]->global_tid, out, out_tid, cap, k);
            if (stats) fill(stats[i], cs[i], v.size());
        }
        *n_out = k;
        if (times) {
            times->ms_cigar = T.ms_cigar; times->ms_cigar_cn = T.ms_cigar_cn; times->ms_split_fetch = T.ms_split_fetch; times->ms_split = T.ms_split;
            times->ms_split_cn = T.ms_split_cn; times->ms_merge_split = T.ms_merge_split; times->ms_merge_final = T.ms_merge_final; times->ms_vcf = T.ms_vcf;
            times->ms_total = T.ms_total; times->ms_split_prepare = T.ms_split_prepare; times->n_reads = T.n_reads; times->n_signatures = T.n_signatures; times->n_cigar_calls = T.n_cigar_calls;
            times->n_cigar_cn_regions = T.n_cigar_cn_regions; times->n_split_calls = T.n_split_calls; times->n_final_calls = T.n_final_calls;
        }
    })
}

// The switches of the SVCaller behind csvhost_run_bam (process-wide, off by default, like csvhost_set_merge_on_device):
// SVCaller::snp_parse_on_device, snp_tables_on_device. csvhost_run_options is untouched.
static std::atomic<int> g_snp_parse_on_device{0}, g_snp_tables_on_device{0};
void csvhost_set_snp_on_device(int parse, int tables) { g_snp_parse_on_device = parse != 0; g_snp_tables_on_device = tables != 0; }
// SVCaller::vcf_format_on_device of the same caller: the run's output.vcf through csvgpu_vcf_format where the genome is on the device
static std::atomic<int> g_vcf_on_device{0};
void csvhost_set_vcf_on_device(int on) { g_vcf_on_device = on != 0; }
// out[2]: copy-number decode calls that took the table route (every job's SNPs resident: "cn: decode on resident tables") / that ran the
// host's SNP queries, since the process began or the last reset
void csvhost_cn_route_stats(uint64_t *out, int reset) { cnRouteStats(out, reset != 0); }

// SVCaller::runBam: chrs = '\n'-separated contig names or null (all). snp_vcf / pfb_table / ethnicity: RunParams' fields of those names (null: none —
// every window then gets the dummy observation). Calls come back grouped by contig in header order, with their contig index in out_tid.
int csvhost_run_bam(csv_ctx *ctx, const char *bam_path, const char *chrs, int threads, const csv_hmm *hmm, const csvhost_run_options *opt,
                    const csvhost_fasta *fasta, const char *vcf_dir, const char *gap_path,
                    const char *file_date, csvhost_call *out, int32_t *out_tid, uint64_t cap, uint64_t *n_out, csvhost_bam_stats *stats,
                    const char *snp_vcf, const char *pfb_table, const char *ethnicity)
{
    GUARD({
        RunParams P = run_params_from(*opt);
        P.snp_vcf = snp_vcf ? snp_vcf : ""; P.pfb_table = pfb_table ? pfb_table : ""; P.ethnicity = ethnicity ? ethnicity : "";
        set_vcf_output(P, fasta, vcf_dir, gap_path, file_date);
        SVCaller caller(ctx);
        caller.snp_parse_on_device = g_snp_parse_on_device.load() != 0; caller.snp_tables_on_device = g_snp_tables_on_device.load() != 0;
        caller.vcf_format_on_device = g_vcf_on_device.load() != 0;
        std::unordered_map<std::string, std::vector<SVCall>> calls;
        BamRunStats bs;
        caller.runBam(bam_path, split_lines(chrs), threads, chmm_from_pod(hmm), P, calls, &bs);
        BamReader hdr_reader;
        if (!hdr_reader.open(bam_path)) throw std::runtime_error(hdr_reader.error());
        uint64_t k = 0;
        for (size_t t = 0; t < hdr_reader.header().names.size(); t++) {
            auto it = calls.find(hdr_reader.header().names[t]);
            if (it != calls.end()) append_flat(it->second, (int32_t)t, out, out_tid, cap, k);
        }
        *n_out = k;
        if (stats) { stats->n_contigs = bs.n_contigs; stats->n_reads = bs.n_reads; stats->n_cigar = bs.n_cigar; stats->bam_bytes = bs.bam_bytes;
                     stats->ms_decode = bs.ms_decode; stats->ms_total = bs.ms_total;
                     stats->unpack_batches_device = bs.unpack_batches_device; stats->unpack_batches_host = bs.unpack_batches_host;
                     stats->unpack_anchors = bs.unpack_anchors; stats->unpack_batches_kept_on_device = bs.unpack_batches_kept_on_device;
                     stats->contigs_resident = bs.contigs_resident; stats->unpack_batches_appended_host = bs.unpack_batches_appended_host; }
    })
}

}  // extern "C"
