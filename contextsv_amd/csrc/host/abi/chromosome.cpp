// chromosome.cpp — the per-chromosome CIGAR path (SVCaller::processChromosome mirror) on resident shards
#include <atomic>

#include "abi.hpp"

// csvhost_set_merge_on_device: what the SVCallers behind csvhost_process_resident_* take (SVCaller::merge_on_device, off by default)
static std::atomic<int> g_merge_on_device{0};
static std::atomic<uint32_t> g_merge_max_partitions{0};
static void configure(SVCaller &c) { c.merge_on_device = g_merge_on_device.load() != 0; c.merge_max_partitions = g_merge_max_partitions.load(); }

static SeqStore host_seqs(const uint64_t *seq_off, const uint8_t *seq) { SeqStore ss; ss.seq_off = seq_off; ss.seq = seq; return ss; }

// the merged calls (POD) of one step, at most cap; their ALT strings are not returned: tags[i] = alt_tag
static void flatten(const std::vector<SVCall> &calls, csvhost_call *out, uint8_t *tags, uint64_t cap)
{
    for (size_t i = 0; i < calls.size() && i < cap; i++) {
        out[i] = flat_call(calls[i]);
        if (tags) tags[i] = alt_tag(calls[i]);
    }
}

// processResidentChromosome -> "<start>\t<end>\t<ALT>\n" per merged call
static void chromosome_alts(csv_ctx *ctx, csv_shard *shard, const SeqStore *ss, double eps, double min_pts_pct, char *buf, uint64_t cap, uint64_t *len)
{
    SVCaller caller(ctx);
    configure(caller);
    std::vector<SVCall> calls;
    ChrStats cs;
    caller.processResidentChromosome("chr", shard, ss, eps, min_pts_pct, calls, cs);
    *len = copy_text(alt_lines(calls), buf, cap);
}

extern "C" {

// The switch of the SVCallers behind csvhost_process_resident_* (process-wide; off / 0 by default): SVCaller::merge_on_device, merge_max_partitions.
void csvhost_set_merge_on_device(int on, uint32_t max_partitions) { g_merge_on_device = on != 0; g_merge_max_partitions = max_partitions; }
// SVCaller::mergeRouteStats: out[0] contigs whose representatives the device chose, [1] contigs that took the host route for a declined bucket,
// [2] for records that overflowed twice, [3] buckets the device declined; reset != 0 clears them.
void csvhost_merge_route_stats(uint64_t *out, int reset)
{
    const SVCaller::MergeRouteStats r = SVCaller::mergeRouteStats(reset != 0);
    out[0] = r.contigs_device; out[1] = r.contigs_host_declined; out[2] = r.contigs_host_overflow; out[3] = r.buckets_declined;
}

// Runs the whole path on a resident shard and writes the merged calls (POD) + alt_tag[i] (0 "<DEL>", 1 "<INS>", 2 literal sequence).
int csvhost_process_resident_chromosome(csv_ctx *ctx, csv_shard *shard, const uint64_t *seq_off, const uint8_t *seq, double eps,
                                        double min_pts_pct, csvhost_call *out, uint8_t *alt_tag, uint64_t cap, csvhost_chr_stats *st)
{
    GUARD({
        SVCaller caller(ctx);
        configure(caller);
        const SeqStore ss = host_seqs(seq_off, seq);
        std::vector<SVCall> calls;
        ChrStats cs;
        caller.processResidentChromosome("chr", shard, seq ? &ss : nullptr, eps, min_pts_pct, calls, cs);
        fill(*st, cs, calls.size());
        flatten(calls, out, alt_tag, cap);
    })
}

// ALT strings only: SVCaller::toSVCall for n signatures ('\n'-joined into buf, at most cap bytes; returns the full length through *len).
// Host only — the 50-bp insertion ALT is cut from the 4-bit sequences here (sv_caller.cpp:572-590, :607-625 of the reference).
int csvhost_sig_alts(const csv_sig *sig, uint64_t n, const uint64_t *seq_off, const uint8_t *seq, char *buf, uint64_t cap, uint64_t *len)
{
    GUARD({
        const SeqStore ss = host_seqs(seq_off, seq);
        std::string t;
        for (uint64_t i = 0; i < n; i++) { t += SVCaller::toSVCall(sig[i], seq ? &ss : nullptr).alt_allele; t += '\n'; }
        *len = copy_text(t, buf, cap);
    })
}

// processChromosome on a resident shard, returning "<start>\t<end>\t<ALT>\n" per merged call (the string fields the POD view drops)
int csvhost_process_resident_chromosome_alts(csv_ctx *ctx, csv_shard *shard, const uint64_t *seq_off, const uint8_t *seq, double eps, double min_pts_pct,
                                             char *buf, uint64_t cap, uint64_t *len)
{
    GUARD({
        const SeqStore ss = host_seqs(seq_off, seq);
        chromosome_alts(ctx, shard, seq ? &ss : nullptr, eps, min_pts_pct, buf, cap, len);
    })
}

// The same with the ALT strings cut on the device from the sequences the shard itself holds (a shard built by csvgpu_shard_builder_finish with
// CSV_SB_SEQ): SeqStore's device form.
int csvhost_process_resident_chromosome_alts_resident(csv_ctx *ctx, csv_shard *shard, double eps, double min_pts_pct, char *buf, uint64_t cap, uint64_t *len)
{
    GUARD({
        SeqStore ss; ss.resident = shard;
        chromosome_alts(ctx, shard, &ss, eps, min_pts_pct, buf, cap, len);
    })
}

// n_steps passes over the same resident shard, software-pipelined (device chain of step i+1 overlaps the host merge of
// step i). Returns the merged calls of the LAST step and its stats; ms_total = wall time of all steps.
int csvhost_process_resident_pipelined(csv_ctx *ctx, csv_shard *shard, uint64_t n_steps, const uint64_t *seq_off, const uint8_t *seq,
                                       double eps, double min_pts_pct, csvhost_call *out, uint8_t *alt_tag, uint64_t cap,
                                       csvhost_chr_stats *st, double *ms_total, uint64_t *total_calls)
{
    GUARD({
        SVCaller caller(ctx);
        configure(caller);
        const SeqStore ss = host_seqs(seq_off, seq);
        std::vector<csv_shard *> shards(n_steps, shard);
        std::vector<std::vector<SVCall>> calls;
        std::vector<ChrStats> stats;
        const auto t0 = std::chrono::steady_clock::now();
        caller.processResidentChromosomesPipelined(shards, seq ? &ss : nullptr, eps, min_pts_pct, calls, stats);
        *ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        uint64_t tot = 0;
        for (auto &c : calls) tot += c.size();
        *total_calls = tot;
        if (n_steps) {
            fill(*st, stats.back(), calls.back().size());
            double dev = 0, hm = 0;
            for (auto &x : stats) { dev += x.ms_device; hm += x.ms_host_merge; }
            st->ms_device = dev / n_steps; st->ms_host_merge = hm / n_steps;
            flatten(calls.back(), out, alt_tag, cap);
        }
    })
}

// n_lanes contexts of one GPU, lane l runs steps[l] passes over its own resident shard concurrently with the others.
// Returns lane 0's last merged calls + stats averaged over every step of every lane; ms_total = wall time of the whole job.
int csvhost_process_resident_lanes(int n_lanes, csv_ctx *const *ctxs, csv_shard *const *shards, const uint64_t *steps, double eps, double min_pts_pct,
                                   csvhost_call *out, uint64_t cap, csvhost_chr_stats *st, double *ms_total, uint64_t *total_calls)
{
    GUARD({
        std::vector<SVCaller::Lane> lanes((size_t)n_lanes);
        for (int l = 0; l < n_lanes; l++) { lanes[l].ctx = ctxs[l]; lanes[l].shards.assign(steps[l], shards[l]);
                                           lanes[l].merge_on_device = g_merge_on_device.load() != 0; lanes[l].merge_max_partitions = g_merge_max_partitions.load(); }
        std::vector<std::vector<std::vector<SVCall>>> calls;
        std::vector<std::vector<ChrStats>> stats;
        const auto t0 = std::chrono::steady_clock::now();
        SVCaller::processResidentLanes(lanes, nullptr, eps, min_pts_pct, calls, stats);
        *ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        uint64_t tot = 0, n_steps = 0;
        double dev = 0, hm = 0;
        for (auto &lane : calls) for (auto &c : lane) tot += c.size();
        for (auto &lane : stats) for (auto &x : lane) { dev += x.ms_device; hm += x.ms_host_merge; n_steps++; }
        *total_calls = tot;
        if (n_steps && !stats[0].empty()) {
            const std::vector<SVCall> &last = calls[0].back();
            fill(*st, stats[0].back(), last.size());
            st->ms_device = dev / n_steps; st->ms_host_merge = hm / n_steps;
            for (size_t i = 0; i < last.size() && i < cap; i++) out[i] = to_pod(last[i]);
        }
    })
}

}  // extern "C"
