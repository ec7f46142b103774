// reference.cpp — reference genome + VCF writer (fasta_query.cpp, saveToVCF)
#include <fstream>

#include "abi.hpp"

// csvgpu_vcf_format takes the mirror's calls as they are: csv_vcf_call (include/csvgpu.h) and csvhost_call (csvhost_abi.h) are one layout
#define SAME_FIELD(f) (offsetof(csv_vcf_call, f) == offsetof(csvhost_call, f) && sizeof(((csv_vcf_call *)0)->f) == sizeof(((csvhost_call *)0)->f))
static_assert(sizeof(csv_vcf_call) == sizeof(csvhost_call) && sizeof(csvhost_call) == 48 && SAME_FIELD(start) && SAME_FIELD(end) && SAME_FIELD(sv_type) &&
              SAME_FIELD(cluster_size) && SAME_FIELD(hmm_likelihood) && SAME_FIELD(id) && SAME_FIELD(aln_flags) && SAME_FIELD(genotype) && SAME_FIELD(cn_state) &&
              SAME_FIELD(aln_offset), "csv_vcf_call and csvhost_call are one layout");
#undef SAME_FIELD

extern "C" {

csvhost_fasta *csvhost_fasta_open(const char *path)
{
    try {
        csvhost_fasta *h = new csvhost_fasta();
        if (h->g.setFilepath(path ? path : "") != 0) { delete h; set_error("No FASTA filepath provided"); return nullptr; }
        return h;
    } catch (const std::exception &e) { set_error(e.what()); return nullptr; }
}
// The same with the sequences on ctx's device (ReferenceGenome::setFilepath with FastaDeviceOptions): the file goes up in windows of
// window_bytes (0 = the default), queries are fetches on ctx. The handle is what csvhost_fasta_open returns, for every function that takes one.
csvhost_fasta *csvhost_fasta_open_device(const char *path, csv_ctx *ctx, uint64_t window_bytes)
{
    if (!ctx) { set_error("csvhost_fasta_open_device: no context"); return nullptr; }
    try {
        csvhost_fasta *h = new csvhost_fasta();
        FastaDeviceOptions opt;
        opt.ctx = ctx; opt.window_bytes = window_bytes;
        if (h->g.setFilepath(path ? path : "", opt) != 0) { delete h; set_error("No FASTA filepath provided"); return nullptr; }
        return h;
    } catch (const std::exception &e) { set_error(e.what()); return nullptr; }
}
// out[8]: on the device (0 / 1), bytes uploaded, lines, records, bases, fetch calls, items fetched, fallback to the host loader (0 / 1)
void csvhost_fasta_device_stats(const csvhost_fasta *h, uint64_t *out)
{
    const FastaDeviceStats s = h->g.deviceStats();
    out[0] = h->g.onDevice() ? 1 : 0; out[1] = s.bytes_uploaded; out[2] = s.lines; out[3] = s.records; out[4] = s.bases;
    out[5] = s.fetch_calls; out[6] = s.items_fetched; out[7] = s.fallback;
}
void csvhost_fasta_free(csvhost_fasta *h) { delete h; }

// length of the view, -1 on error (unknown contig); at most cap bytes are copied to buf
int64_t csvhost_fasta_query(const csvhost_fasta *h, const char *chr, uint32_t pos_start, uint32_t pos_end, char *buf, uint64_t cap)
{
    try {
        std::string_view v = h->g.query(chr, pos_start, pos_end);
        if (buf && cap) memcpy(buf, v.data(), (size_t)std::min<uint64_t>(cap, v.size()));
        return (int64_t)v.size();
    } catch (const std::exception &e) { set_error(e.what()); return -1; }
}
int csvhost_fasta_compare(const csvhost_fasta *h, const char *chr, uint32_t pos_start, uint32_t pos_end, const char *seq, float threshold)
{
    try { return h->g.compare(chr, pos_start, pos_end, seq, threshold) ? 1 : 0; } catch (const std::exception &e) { set_error(e.what()); return -1; }
}
uint32_t csvhost_fasta_length(const csvhost_fasta *h, const char *chr) { return h->g.getChromosomeLength(chr); }
// contig header and the sorted contig list ('\n'-joined) as text; returns the full length
int64_t csvhost_fasta_contig_header(const csvhost_fasta *h, char *buf, uint64_t cap) { return (int64_t)copy_text(h->g.getContigHeader(), buf, cap); }
int64_t csvhost_fasta_chromosomes(const csvhost_fasta *h, char *buf, uint64_t cap)
{
    std::string s;
    for (const std::string &c : h->g.getChromosomes()) { if (!s.empty()) s += '\n'; s += c; }
    return (int64_t)copy_text(s, buf, cap);
}

// csvhost_save_vcf and csvhost_save_vcf_device: one body
static int save_vcf(csv_ctx *ctx, const char *out_dir, const csvhost_fasta *fasta, const char *gap_path, const char *file_date, int n_contigs,
                    const char *const *chr_names, const uint64_t *call_off, const csvhost_call *calls, const char *const *alts,
                    csv_shard *const *shards, const uint32_t *const *depth, const uint64_t *depth_len, int map_order, int32_t *counts, bool format_on_device)
{
    GUARD({
        std::vector<std::pair<std::string, std::vector<SVCall>>> per((size_t)n_contigs);
        std::unordered_map<std::string, std::vector<uint32_t>> host_depth;
        ShardDepthSource shard_src(ctx);
        for (int t = 0; t < n_contigs; t++) {
            per[t].first = chr_names[t];
            for (uint64_t i = call_off[t]; i < call_off[t + 1]; i++) {
                SVCall c = from_pod(calls[i]);
                c.alt_allele = alts[i];
                per[t].second.push_back(c);
            }
            if (shards) { if (shards[t]) shard_src.add(chr_names[t], shards[t]); }
            else if (depth[t]) host_depth[chr_names[t]].assign(depth[t], depth[t] + depth_len[t]);
        }
        HostDepthSource host_src(host_depth);
        const DepthSource &src = shards ? (const DepthSource &)shard_src : (const DepthSource &)host_src;
        VCFOptions opt;
        opt.assembly_gaps = gap_path ? gap_path : "";
        opt.output_dir = out_dir;
        opt.file_date = file_date ? file_date : "";
        opt.format_on_device = format_on_device; opt.ctx = ctx;
        VCFCounts c;
        if (map_order) {
            std::unordered_map<std::string, std::vector<SVCall>> m;
            for (auto &e : per) m[e.first] = e.second;
            if (!saveToVCF(m, opt, fasta->g, src, &c)) throw std::runtime_error("saveToVCF returned early");
        } else {
            std::unordered_map<std::string, std::vector<std::pair<uint32_t, uint32_t>>> gaps;
            if (!opt.assembly_gaps.empty() && !loadAssemblyGaps(opt.assembly_gaps, gaps)) throw std::runtime_error("cannot open assembly gap file");
            std::ofstream f(opt.output_dir + "/output.vcf");
            if (!f.is_open()) throw std::runtime_error("cannot open output.vcf");
            std::vector<std::pair<std::string, const std::vector<SVCall> *>> order;
            for (auto &e : per) order.emplace_back(e.first, &e.second);
            c = writeVCF(f, order, opt, gaps, fasta->g, src);
        }
        if (counts) { counts[0] = c.total; counts[1] = c.unclassified; counts[2] = c.assembly_gap_filtered; }
    })
}

// Calls of contig t = calls[call_off[t] .. call_off[t+1]) with ALT strings alts[i]. Depth comes from resident shards
// (shards != nullptr, ShardDepthSource) or from host arrays depth[t][0..depth_len[t]) (a null depth[t] = contig without a map).
// map_order != 0 goes through saveToVCF's unordered_map iteration; otherwise contigs are written in the order given.
// counts = {total, unclassified, assembly-gap filtered}.
int csvhost_save_vcf(csv_ctx *ctx, const char *out_dir, const csvhost_fasta *fasta, const char *gap_path, const char *file_date, int n_contigs,
                     const char *const *chr_names, const uint64_t *call_off, const csvhost_call *calls, const char *const *alts,
                     csv_shard *const *shards, const uint32_t *const *depth, const uint64_t *depth_len, int map_order, int32_t *counts)
{
    return save_vcf(ctx, out_dir, fasta, gap_path, file_date, n_contigs, chr_names, call_off, calls, alts, shards, depth, depth_len, map_order, counts, false);
}
// The same with VCFOptions::format_on_device: the record lines from one csvgpu_vcf_format call on ctx where the genome is on the device and
// the depth comes from shards; the host loop otherwise, and for a batch the device declines. The file is the same either way.
int csvhost_save_vcf_device(csv_ctx *ctx, const char *out_dir, const csvhost_fasta *fasta, const char *gap_path, const char *file_date, int n_contigs,
                            const char *const *chr_names, const uint64_t *call_off, const csvhost_call *calls, const char *const *alts,
                            csv_shard *const *shards, const uint32_t *const *depth, const uint64_t *depth_len, int map_order, int32_t *counts,
                            int format_on_device)
{
    return save_vcf(ctx, out_dir, fasta, gap_path, file_date, n_contigs, chr_names, call_off, calls, alts, shards, depth, depth_len, map_order, counts,
                    format_on_device != 0);
}
// out[3]: batches of writeVCF formatted on the device / that ran the host loop with the option on / of those, declined by the device; since
// the process began or the last reset
void csvhost_vcf_route_stats(uint64_t *out, int reset) { vcfRouteStats(out, reset != 0); }

}  // extern "C"
