#include "sv_caller.h"
#include <cstddef>
#include <cstring>

#include <deque>

#include <algorithm>
#include <cstdio>
#include <chrono>
#include <condition_variable>
#include <exception>
#include <mutex>
#include <thread>
#include <stdexcept>
#include <atomic>

#include <memory>

#include "dbscan.h"
#include "log.h"
#include "par.h"
#include "sort_select.h"
#include "umap_order.h"

namespace {
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

void check(csv_ctx *ctx, int rc, const char *what)
{
    if (rc != CSV_OK) throw std::runtime_error(std::string(what) + ": " + csvgpu_last_error(ctx));
}
}  // namespace

namespace { constexpr char kAltNote = '\x01'; }   // first byte of an ALT field that holds toSVCall's note instead of bases (no ALT string starts with it)

// Field values of the SVCall the reference builds per op (sv_caller.cpp:569-643): INS from I (CIGARINS) or
// from a soft clip (CIGARCLIP), DEL from D (CIGARDEL); ALT is the inserted sequence only when op_len <= 50
// (i.e. exactly 50, ambiguity codes RYKMSWBDHV in either case -> N), otherwise "<INS>"; DEL -> "<DEL>".
SVCall SVCaller::toSVCall(const csv_sig &s, const SeqStore *seq)
{
    const uint32_t kind = CSV_SIG_KIND(s);
    SVEvidenceFlags flags;
    if (kind == CSV_KIND_DEL) {
        flags.set((size_t)SVDataType::CIGARDEL);
        return SVCall(s.start, s.end, SVType::DEL, "<DEL>", flags, Genotype::UNKNOWN, 0.0, 0, 0, 0);
    }
    flags.set((size_t)(kind == CSV_KIND_INS ? SVDataType::CIGARINS : SVDataType::CIGARCLIP));
    const uint32_t op_len = s.end - s.start + 1;
    std::string alt = "<INS>";
    if (op_len <= 50) {
        alt.assign(op_len, 'N');
        const uint32_t q0 = CSV_SIG_QPOS(s);
        if (seq && seq->resident && !seq->seq) {
            // the sequences are on the device: the call carries (read, query offset) in the place of its bases until patchResidentAlts
            // has run — nothing in between reads an ALT field (the representative rule compares lengths of start .. end only)
            alt.assign(1, kAltNote);
            alt.append((const char *)&s.read, 4);
            alt.append((const char *)&q0, 4);
            alt.append((const char *)&op_len, 4);
            return SVCall(s.start, s.end, SVType::INS, alt, flags, Genotype::UNKNOWN, 0.0, 0, 0, 0);
        }
        // a record stored without its sequence ("*", l_seq = 0) has nothing to copy from: the ALT stays N's
        if (seq && seq->seq && seq->seq_off && ((uint64_t)q0 + op_len + 1) / 2 <= seq->seq_off[s.read + 1] - seq->seq_off[s.read]) {
            static const char nt16[] = "=ACMGRSVTWYHKDBN";              // BAM 4-bit code table (SAM spec §4.2.3)
            const uint8_t *p = seq->seq + seq->seq_off[s.read];
            for (uint32_t j = 0; j < op_len; j++) {
                const uint32_t q = q0 + j;
                const char b = nt16[(p[q >> 1] >> ((~q & 1u) << 2)) & 0xf];
                switch (b) {
                    case 'R': case 'Y': case 'K': case 'M': case 'S': case 'W': case 'B': case 'D': case 'H': case 'V': alt[j] = 'N'; break;
                    default: alt[j] = b;
                }
            }
        }
    }
    return SVCall(s.start, s.end, SVType::INS, alt, flags, Genotype::UNKNOWN, 0.0, 0, 0, 0);
}

void SVCaller::patchResidentAlts(csv_ctx *ctx, csv_shard *shard, std::vector<SVCall> &calls)
{
    std::vector<size_t> which;
    std::vector<uint32_t> read, qpos;
    std::vector<uint64_t> off(1, 0);
    for (size_t i = 0; i < calls.size(); i++) {
        const std::string &a = calls[i].alt_allele;
        if (a.size() != 13 || a[0] != kAltNote) continue;
        uint32_t r, q, len;
        memcpy(&r, a.data() + 1, 4); memcpy(&q, a.data() + 5, 4); memcpy(&len, a.data() + 9, 4);
        // (the note holds the operation's own length: a merge that moved the call's ends must not change what is cut)
        if (len != calls[i].end - calls[i].start + 1) throw std::logic_error("patchResidentAlts: a call's ends changed between toSVCall and the patch");
        which.push_back(i); read.push_back(r); qpos.push_back(q);
        off.push_back(off.back() + len);
    }
    if (which.empty()) return;
    std::string bases((size_t)off.back(), 'N');
    check(ctx, csvgpu_alt_bases_resident(ctx, shard, read.data(), qpos.data(), off.data(), which.size(), &bases[0]), "patchResidentAlts");
    for (size_t k = 0; k < which.size(); k++) calls[which[k]].alt_allele.assign(bases, (size_t)off[k], (size_t)(off[k + 1] - off[k]));
}

// mergeTypeWithLabels (sv_object.cpp) specialised to raw CIGAR signatures, keep_noise = false: same bucket order,
// same std::sort comparator on an index vector, same top-20 % / middle element rule, cluster_size = bucket size.
void SVCaller::mergeSignaturesWithLabels(const csv_sig *sig, const int32_t *labels, uint64_t n, const SeqStore *seq, std::vector<SVCall> &merged)
{
    // members of every label, in input order, as (length, index) pairs: the representative rule only compares lengths, and the
    // selection below streams over this compact array instead of chasing indices into the 16-byte records
    struct Ent { uint32_t len, idx; };
    static thread_local std::vector<uint32_t> head, cur;
    static thread_local std::vector<Ent> member;
    int32_t max_label = -2;
    for (uint64_t i = 0; i < n; i++) max_label = std::max(max_label, labels[i]);
    const size_t n_slots = (size_t)(max_label + 3);
    head.assign(n_slots + 1, 0);
    for (uint64_t i = 0; i < n; i++) head[(size_t)(labels[i] + 2) + 1]++;
    for (size_t s = 0; s < n_slots; s++) head[s + 1] += head[s];
    cur.assign(head.begin(), head.end() - 1);
    if (member.size() < n) member.resize(n);
    for (uint64_t i = 0; i < n; i++) member[cur[(size_t)(labels[i] + 2)]++] = Ent{sig[i].end - sig[i].start, (uint32_t)i};
    for (size_t s = 0; s < n_slots; s++) {
        const size_t sz = head[s + 1] - head[s];
        if (sz < 2) continue;
        Ent *m = member.data() + head[s];
        // the slot std::sort(by length desc) would fill at [top/2] — selected in O(sz), see sort_select.h
        const size_t top = (size_t)std::max(1, (int)(sz * 0.2));
        auto by_len_desc = [](const Ent &a, const Ent &b) { return a.len > b.len; };
        const uint32_t pick = csvhost::std_sort_select(m, m + sz, (std::ptrdiff_t)(top / 2), by_len_desc)->idx;
        SVCall rep = toSVCall(sig[pick], seq);
        rep.cluster_size = (int)sz;
        merged.push_back(rep);
    }
}

// How many signatures did the chromosomes of this process need room for so far? New result buffers start at that size: a buffer that
// turns out too small costs a CSV_ECAPACITY round trip (grow + synchronous fetch), and a driver that is called once per batch of
// chromosomes would pay it again for every buffer of every call (3 lanes x 3 buffers x ~1 ms per call of the benchmark).
namespace {
std::atomic<uint64_t> g_result_hint{0};
uint64_t result_capacity_hint(const csv_ctx *) { return std::max<uint64_t>(1 << 16, g_result_hint.load(std::memory_order_relaxed)); }
void note_result_size(const csv_ctx *, uint64_t n_sig)
{
    uint64_t h = g_result_hint.load(std::memory_order_relaxed);
    while (n_sig > h && !g_result_hint.compare_exchange_weak(h, n_sig, std::memory_order_relaxed)) {}
}
}  // namespace

void SVCaller::DeviceOut::reserve(csv_ctx *c, uint64_t n)
{
    if (n <= cap && c == ctx) return;
    release();
    ctx = c;
    const uint64_t want = n + n / 4 + 4096;
    sig = (csv_sig *)csvgpu_host_alloc(c, want * sizeof(csv_sig));
    lab = (int32_t *)csvgpu_host_alloc(c, want * sizeof(int32_t));
    if (!sig || !lab) { release(); throw std::runtime_error("cannot allocate page-locked result buffers"); }
    cap = want;
}

void SVCaller::DeviceOut::reserveRep(csv_ctx *c, uint64_t n)
{
    if (n <= rep_cap && c == rep_ctx && cnt) return;
    releaseRep();
    rep_ctx = c;
    const uint64_t want = n + n / 4 + 4096;
    rep = (csv_merge_rep *)csvgpu_host_alloc(c, want * sizeof(csv_merge_rep));
    cnt = (csv_merge_counts *)csvgpu_host_alloc(c, sizeof(csv_merge_counts));
    if (!rep || !cnt) { releaseRep(); throw std::runtime_error("cannot allocate page-locked record buffers"); }
    memset(cnt, 0, sizeof(*cnt));
    rep_cap = want;
}

namespace {
std::atomic<uint64_t> g_route_device{0}, g_route_declined{0}, g_route_overflow{0}, g_buckets_declined{0};
}
SVCaller::MergeRouteStats SVCaller::mergeRouteStats(bool reset)
{
    MergeRouteStats r;
    r.contigs_device = g_route_device.load(); r.contigs_host_declined = g_route_declined.load(); r.contigs_host_overflow = g_route_overflow.load();
    r.buckets_declined = g_buckets_declined.load();
    if (reset) { g_route_device = 0; g_route_declined = 0; g_route_overflow = 0; g_buckets_declined = 0; }
    return r;
}

void SVCaller::finishSelect(csv_shard *shard, const csv_chr_result &res, int rc, DeviceOut &out)
{
    out.use_rep = false;
    bool overflow = false;
    if (rc == CSV_ECAPACITY) {                         // more records than room: once more with room for what the counts say
        out.reserveRep(ctx, out.cnt->n_rep[0] + out.cnt->n_rep[1]);
        rc = csvgpu_chr_merge_select(ctx, shard, &res, merge_max_partitions, out.rep, out.rep_cap, out.cnt);
        if (rc == CSV_ECAPACITY) { overflow = true; rc = CSV_OK; }
    }
    check(ctx, rc, "processChromosome (select)");
    const uint64_t declined = out.cnt->n_declined[0] + out.cnt->n_declined[1];
    g_buckets_declined += declined;
    if (overflow || declined) {                        // today's route for this contig: everything comes down, the host picks
        out.reserve(ctx, res.n_sig);
        check(ctx, csvgpu_chr_fetch(ctx, shard, &res, out.sig, out.lab), "processChromosome (fetch behind a declined select)");
        (declined ? g_route_declined : g_route_overflow)++;
        return;
    }
    out.n_rep = out.cnt->n_rep[0] + out.cnt->n_rep[1];
    out.use_rep = true;
    g_route_device++;
}

void SVCaller::runDeviceChain(const std::string &chr, csv_shard *shard, double eps, double pct, DeviceOut &out, ChrStats &st)
{
    const double t0 = now_ms();
    csv_chr_result res;
    int rc;
    out.use_rep = false;
    if (merge_on_device) {
        if (!out.rep_cap) out.reserveRep(ctx, 1 << 14);
        csv_job *job = csvgpu_chr_job_begin(ctx, shard, (uint32_t)min_oplen, (uint8_t)min_mapq, pct);
        if (!job) throw std::runtime_error(std::string("processChromosome: ") + csvgpu_last_error(ctx));
        rc = csvgpu_chr_job_cluster_select(ctx, job, eps, merge_max_partitions, out.rep, out.rep_cap, out.cnt);
        if (rc) { csvgpu_chr_job_abort(ctx, job); check(ctx, rc, "processChromosome"); }
        rc = csvgpu_chr_job_end(ctx, job, &res);
        if (rc != CSV_ECAPACITY) check(ctx, rc, "processChromosome");
        finishSelect(shard, res, rc, out);
        rc = CSV_OK;
    } else {
        if (!out.cap) out.reserve(ctx, result_capacity_hint(ctx));
        rc = csvgpu_chr_pipeline_fetch(ctx, shard, (uint32_t)min_oplen, (uint8_t)min_mapq, eps, pct, &res, out.sig, out.lab, out.cap);
        if (rc == CSV_ECAPACITY) {                     // first contig of this size: grow the buffers, fetch what the device already holds
            out.reserve(ctx, res.n_sig);
            rc = csvgpu_chr_fetch(ctx, shard, &res, out.sig, out.lab);
        }
    }
    check(ctx, rc, "processChromosome");
    note_result_size(ctx, res.n_sig);
    st.n_signatures = res.n_sig; st.n_del = res.n_del; st.n_ins = res.n_ins;
    st.depth_sum = res.depth_sum; st.depth_nonzero = res.depth_nonzero; st.mean_chr_cov = res.mean_cov; st.dbscan_min_pts = res.min_pts;
    if (pct > 0.0)
        printMessage(chr + ": Mean chr. cov.: " + std::to_string(res.mean_cov) + " (DBSCAN min. pts.= " + std::to_string(res.min_pts) +
                     ", min. pts. pct.= " + std::to_string(pct) + ")");
    out.n_del = res.n_del; out.n_ins = res.n_ins;
    st.ms_device = now_ms() - t0;
}

// mergeSVs(chr_sv_calls, eps, min_pts, keep_noise=false) with the labels already computed on device.
// Every CIGAR call has hmm_likelihood == 0, so only the length-ranked branch of the representative choice
// can run (sv_object.cpp:187-244 of the reference); it is evaluated on the 16-byte signatures and an SVCall
// (with its strings) is materialised for the chosen member only.
void SVCaller::mergeOrdered(const csv_sig *sig, const int32_t *labels, uint64_t n_del, uint64_t n_ins, const SeqStore *seq, std::vector<SVCall> &chr_sv_calls, bool share_pool)
{
    const uint64_t n_sig = n_del + n_ins;
    chr_sv_calls.clear();
    if (n_sig < 2) {                                   // mergeSVs returns early (:49-51)
        for (uint64_t i = 0; i < n_sig; i++) chr_sv_calls.push_back(toSVCall(sig[i], seq));
        return;
    }
    const uint64_t type_n[2] = {n_del, n_ins};
    auto one_type = [&](int t, std::vector<SVCall> &dst) {
        const uint64_t base = t ? n_del : 0;
        if (type_n[t] < 2) for (uint64_t i = 0; i < type_n[t]; i++) dst.push_back(toSVCall(sig[base + i], seq));
        else mergeSignaturesWithLabels(sig + base, labels + base, type_n[t], seq, dst);
    };
    // (share_pool = false: a pass over many contigs — the other lanes' merges hide this one, and the host pool belongs to the split-read and
    // copy-number sections running beside the pass: a merge that took it made those run inline, 1 ms sections became 6 ms ones)
    if (n_sig < 40000 || !share_pool) {
        one_type(0, chr_sv_calls);
        one_type(1, chr_sv_calls);
        return;
    }
    // (a type with few signatures — the deletions of a synthetic ONT contig — goes through the sequential form, the other through the sections)
    const bool big[2] = {n_del >= 20000, n_ins >= 20000};
    // A large contig (a rank that holds chr1 alone waited 2.85 ms here, its device chain takes 1.9): the same bucket order and the same
    // selections as mergeSignaturesWithLabels, in sections the host pool can share — per-chunk label counts, the members scattered chunk by
    // chunk (a chunk's members of a label go behind the earlier chunks': input order kept), then the buckets: each type's noise bucket
    // (93 % of the signatures; its selection is one sequential replay) as an item of its own beside ranges of clusters. When the pool is
    // taken (a whole-genome pass: the lanes' other merges hide this one) the sections run inline, one after the other.
    struct Ent { uint32_t len, idx; };
    struct TypeWork {
        uint64_t base = 0, n = 0;
        size_t n_slots = 0;
        std::vector<std::vector<uint32_t>> cnt;      // per chunk: members per slot, then the chunk's first position per slot
        std::vector<uint32_t> head;
        std::vector<Ent> member;
        std::vector<std::vector<SVCall>> part;       // per bucket item, in slot order
    } W[2];
    constexpr size_t kChunks = 8;
    std::unique_ptr<csvhost::TraceScope> tr(new csvhost::TraceScope("merge: label counts + scatter"));
    for (int t = 0; t < 2; t++) { W[t].base = t ? n_del : 0; W[t].n = big[t] ? type_n[t] : 0; W[t].cnt.assign(kChunks, {}); W[t].member.resize(W[t].n); }
    auto chunk = [&](const TypeWork &w, size_t c, uint64_t &a, uint64_t &b) { a = w.n * c / kChunks; b = w.n * (c + 1) / kChunks; };
    csvhost::parallel_for(2 * kChunks, 0, [&](size_t it) {
        TypeWork &w = W[it / kChunks];
        uint64_t a, b; chunk(w, it % kChunks, a, b);
        const int32_t *lab = labels + w.base;
        int32_t mx = -2;
        for (uint64_t i = a; i < b; i++) mx = std::max(mx, lab[i]);
        std::vector<uint32_t> &c = w.cnt[it % kChunks];
        c.assign((size_t)(mx + 3), 0);
        for (uint64_t i = a; i < b; i++) c[(size_t)(lab[i] + 2)]++;
    });
    for (int t = 0; t < 2; t++) {
        TypeWork &w = W[t];
        for (auto &c : w.cnt) w.n_slots = std::max(w.n_slots, c.size());
        w.head.assign(w.n_slots + 1, 0);
        for (auto &c : w.cnt) { c.resize(w.n_slots, 0); for (size_t s2 = 0; s2 < w.n_slots; s2++) w.head[s2 + 1] += c[s2]; }
        for (size_t s2 = 0; s2 < w.n_slots; s2++) w.head[s2 + 1] += w.head[s2];
        std::vector<uint32_t> run(w.head.begin(), w.head.end() - 1);
        for (auto &c : w.cnt) for (size_t s2 = 0; s2 < w.n_slots; s2++) { const uint32_t k = c[s2]; c[s2] = run[s2]; run[s2] += k; }
    }
    csvhost::parallel_for(2 * kChunks, 0, [&](size_t it) {
        TypeWork &w = W[it / kChunks];
        uint64_t a, b; chunk(w, it % kChunks, a, b);
        const int32_t *lab = labels + w.base;
        const csv_sig *sg = sig + w.base;
        std::vector<uint32_t> &cur = w.cnt[it % kChunks];
        for (uint64_t i = a; i < b; i++) w.member[cur[(size_t)(lab[i] + 2)]++] = Ent{sg[i].end - sg[i].start, (uint32_t)i};
    });
    // bucket items per type: [0, 1) = the noise bucket, then the clusters in kRanges ranges
    constexpr size_t kRanges = 7;
    tr.reset(new csvhost::TraceScope("merge: buckets (noise bucket + cluster ranges)"));
    for (int t = 0; t < 2; t++) W[t].part.assign(1 + kRanges, {});
    csvhost::parallel_for(2 * (1 + kRanges), 0, [&](size_t it) {
        TypeWork &w = W[it / (1 + kRanges)];
        const size_t item = it % (1 + kRanges);
        if (!big[it / (1 + kRanges)]) { if (item == 0) one_type((int)(it / (1 + kRanges)), w.part[0]); return; }
        size_t s0 = 0, s1 = std::min<size_t>(1, w.n_slots);
        if (item > 0) {
            const size_t rest = w.n_slots > 1 ? w.n_slots - 1 : 0;
            s0 = 1 + rest * (item - 1) / kRanges; s1 = 1 + rest * item / kRanges;
        }
        std::vector<SVCall> &dst = w.part[item];
        const csv_sig *sg = sig + w.base;
        for (size_t s2 = s0; s2 < s1; s2++) {
            const size_t sz = w.head[s2 + 1] - w.head[s2];
            if (sz < 2) continue;
            Ent *m = w.member.data() + w.head[s2];
            const size_t top = (size_t)std::max(1, (int)(sz * 0.2));
            auto by_len_desc = [](const Ent &x, const Ent &y) { return x.len > y.len; };
            const uint32_t pick = csvhost::std_sort_select(m, m + sz, (std::ptrdiff_t)(top / 2), by_len_desc)->idx;
            SVCall rep = toSVCall(sg[pick], seq);
            rep.cluster_size = (int)sz;
            dst.push_back(std::move(rep));
        }
    });
    tr.reset();
    for (int t = 0; t < 2; t++)
        for (auto &v : W[t].part) chr_sv_calls.insert(chr_sv_calls.end(), std::make_move_iterator(v.begin()), std::make_move_iterator(v.end()));
}

void SVCaller::hostMerge(const std::string &chr, const DeviceOut &in, const SeqStore *seq, std::vector<SVCall> &chr_sv_calls, ChrStats &st, bool share_pool)
{
    const double t1 = now_ms();
    csvhost::TraceScope tr("lane: host merge");
    printMessage(chr + ": Merging CIGAR...");
    if (in.use_rep) {                                  // the device chose: the records' calls, DEL records first, as mergeOrdered orders them
        chr_sv_calls.clear();
        chr_sv_calls.reserve(in.n_rep);
        for (uint64_t i = 0; i < in.n_rep; i++) {
            SVCall c = toSVCall(in.rep[i].sig, seq);
            if (in.rep[i].status == 0) c.cluster_size = (int)in.rep[i].cluster_size;      // (a pass-through record stays untouched)
            chr_sv_calls.push_back(std::move(c));
        }
    } else mergeOrdered(in.sig, in.lab, in.n_del, in.n_ins, seq, chr_sv_calls, share_pool);
    st.ms_host_merge = now_ms() - t1;
    printMessage(chr + ": Found " + std::to_string(getSVCount(chr_sv_calls)) + " SV candidates in the CIGAR string");
}

void SVCaller::processResidentChromosome(const std::string &chr, csv_shard *shard, const SeqStore *seq, double eps, double pct,
                                         std::vector<SVCall> &chr_sv_calls, ChrStats &st)
{
    DeviceOut d;
    runDeviceChain(chr, shard, eps, pct, d, st);
    hostMerge(chr, d, seq, chr_sv_calls, st);
    if (seq && seq->resident && !seq->seq) patchResidentAlts(ctx, seq->resident, chr_sv_calls);
}

void SVCaller::processResidentChromosomesPipelined(const std::vector<csv_shard *> &shards, const SeqStore *seq, double eps, double pct,
                                                   std::vector<std::vector<SVCall>> &calls, std::vector<ChrStats> &stats)
{
    processResidentChromosomesPipelined(shards, seq ? std::vector<const SeqStore *>(shards.size(), seq) : std::vector<const SeqStore *>(), eps, pct, calls, stats);
}

void SVCaller::processResidentChromosomesPipelined(const std::vector<csv_shard *> &shards, const std::vector<const SeqStore *> &seqs, double eps, double pct,
                                                   std::vector<std::vector<SVCall>> &calls, std::vector<ChrStats> &stats)
{
    const size_t n = shards.size();
    if (!seqs.empty() && seqs.size() != n) throw std::invalid_argument("processResidentChromosomesPipelined: one SeqStore per shard, or none");
    for (const SeqStore *q : seqs) if (q && q->resident && !q->seq) throw std::invalid_argument("processResidentChromosomesPipelined: a SeqStore in its device form (host arrays, or none)");
    calls.assign(n, {});
    stats.assign(n, ChrStats());
    // The representative choice of one chromosome (~0.5 ms for chr22: a sequential selection over the noise bucket) takes about as
    // long as its device chain, so two merge threads take alternate chromosomes; three result slots rotate between the device
    // thread (filling one) and the two merges in progress.
    constexpr size_t kMergers = 2, kSlots = kMergers + 1;
    DeviceOut slot[kSlots];
    std::mutex mu;
    std::condition_variable cv;
    std::vector<char> ready(n, 0), merged(n, 0);          // guarded by mu
    bool failed = false;
    std::exception_ptr worker_err;
    csvhost::WorkerThreads &pool = csvhost::WorkerThreads::instance();
    std::vector<csvhost::WorkerThreads::Ticket> workers;
    for (size_t w = 0; w < kMergers; w++) {
        workers.push_back(pool.start([&, w] {
            try {
                for (size_t i = w; i < n; i += kMergers) {
                    { std::unique_lock<std::mutex> l(mu); cv.wait(l, [&] { return ready[i] || failed; }); if (failed) return; }
                    hostMerge("shard" + std::to_string(i), slot[i % kSlots], seqs.empty() ? nullptr : seqs[i], calls[i], stats[i], n <= 2);
                    { std::lock_guard<std::mutex> l(mu); merged[i] = 1; }
                    cv.notify_all();
                    if (on_merged) on_merged(i);
                }
            } catch (...) {
                std::lock_guard<std::mutex> l(mu);
                if (!worker_err) worker_err = std::current_exception();
                failed = true;
                cv.notify_all();
            }
        }));
    }
    auto stop_workers = [&] {
        { std::lock_guard<std::mutex> l(mu); failed = true; }
        cv.notify_all();
        for (auto &t : workers) pool.wait(t);
    };
    // The scan + depth pair of the next shard is queued ahead of the shard whose results are being fetched. More than one ahead was measured
    // and is no better (25.7 / 26.7 ms per genome step with one, 26.4 / 26.9 with three): the gaps between the big kernels were not a starved
    // gate but a lane's stream sharing the gate's hardware queue — see csvgpu_gate_open.
    constexpr size_t kAhead = 1;
    std::deque<csv_job *> ahead;                          // jobs whose scan + depth pass is already queued, oldest first
    size_t next_begin = 0;
    auto begin_one = [&] {
        csv_job *j = csvgpu_chr_job_begin(ctx, shards[next_begin], (uint32_t)min_oplen, (uint8_t)min_mapq, pct);
        if (!j) throw std::runtime_error(std::string("processChromosome: ") + csvgpu_last_error(ctx));
        ahead.push_back(j);
        next_begin++;
    };
    auto abort_all = [&] { for (csv_job *j : ahead) csvgpu_chr_job_abort(ctx, j); ahead.clear(); };
    // (a job works in its shard's own buffers: a shard that is listed again — the benchmark's repeated passes over one contig — is only
    // begun again once the job before it on that shard has queued its clustering)
    std::vector<csv_shard *> open_shards;                 // shards of the jobs in `ahead`, same order
    auto shard_free = [&](csv_shard *sh) { return std::find(open_shards.begin(), open_shards.end(), sh) == open_shards.end(); };
    auto top_up = [&] {
        while (next_begin < n && ahead.size() < kAhead && shard_free(shards[next_begin])) { open_shards.push_back(shards[next_begin]); begin_one(); }
    };
    try {
        top_up();
        for (size_t i = 0; i < n; i++) {
            // slot i % kSlots is free once shard i - kSlots has been merged
            if (i >= kSlots) {
                std::unique_lock<std::mutex> l(mu);
                cv.wait(l, [&] { return merged[i - kSlots] || failed; });
                if (failed) break;
            }
            const double t0 = now_ms();
            DeviceOut &out = slot[i % kSlots];
            ChrStats &st = stats[i];
            if (merge_on_device) { if (!out.rep_cap) out.reserveRep(ctx, 1 << 14); }
            else if (!out.cap) out.reserve(ctx, result_capacity_hint(ctx));
            if (ahead.empty()) top_up();                   // (a repeated shard: its next pass could not be queued ahead)
            csv_job *job = ahead.front();
            ahead.pop_front();
            int rc = merge_on_device ? csvgpu_chr_job_cluster_select(ctx, job, eps, merge_max_partitions, out.rep, out.rep_cap, out.cnt)
                                     : csvgpu_chr_job_cluster(ctx, job, eps, out.sig, out.lab, out.cap);
            if (rc) { csvgpu_chr_job_abort(ctx, job); check(ctx, rc, "processChromosome"); }      // abort keeps the failure's own message
            open_shards.erase(open_shards.begin());       // this shard's clustering is queued: a later pass over it may follow on the stream
            // more scan + depth passes go into the queue now, behind this shard's clustering and copies
            try { top_up(); } catch (...) { csvgpu_chr_job_abort(ctx, job); throw; }
            csv_chr_result res;
            rc = csvgpu_chr_job_end(ctx, job, &res);
            out.use_rep = false;
            if (merge_on_device) {
                if (rc != CSV_ECAPACITY) check(ctx, rc, "processChromosome");
                finishSelect(shards[i], res, rc, out);
                rc = CSV_OK;
            } else if (rc == CSV_ECAPACITY) {              // first contig of this size: grow the buffers, fetch what the device still holds
                out.reserve(ctx, res.n_sig);
                rc = csvgpu_chr_fetch(ctx, shards[i], &res, out.sig, out.lab);
            }
            check(ctx, rc, "processChromosome");
            note_result_size(ctx, res.n_sig);
            st.n_signatures = res.n_sig; st.n_del = res.n_del; st.n_ins = res.n_ins;
            st.depth_sum = res.depth_sum; st.depth_nonzero = res.depth_nonzero; st.mean_chr_cov = res.mean_cov; st.dbscan_min_pts = res.min_pts;
            out.n_del = res.n_del; out.n_ins = res.n_ins;
            st.ms_device = now_ms() - t0;
            if (on_device) on_device(i);
            { std::lock_guard<std::mutex> l(mu); ready[i] = 1; }
            cv.notify_all();
        }
        abort_all();                                      // (only after a merge-thread failure cut the loop short)
    } catch (...) {
        abort_all();
        stop_workers();
        throw;
    }
    for (auto &t : workers) pool.wait(t);
    if (worker_err) std::rethrow_exception(worker_err);
}

std::vector<int> SVCaller::assignShards(const std::vector<double> &weights, int world)
{
    if (world < 1) throw std::invalid_argument("assignShards: world < 1");
    std::vector<size_t> order(weights.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return weights[a] != weights[b] ? weights[a] > weights[b] : a < b; });
    std::vector<double> load((size_t)world, 0.0);
    std::vector<int> rank_of(weights.size(), 0);
    for (size_t i : order) {
        int r = 0;
        for (int k = 1; k < world; k++) if (load[(size_t)k] < load[(size_t)r]) r = k;      // (least loaded, lowest rank on ties)
        rank_of[i] = r;
        load[(size_t)r] += weights[i];
    }
    return rank_of;
}

void SVCaller::processResidentLanes(const std::vector<Lane> &lanes, const SeqStore *seq, double eps, double pct,
                                    std::vector<std::vector<std::vector<SVCall>>> &calls, std::vector<std::vector<ChrStats>> &stats,
                                    const std::function<void(size_t lane, size_t k)> &on_merged, int min_mapq, int min_oplen,
                                    const std::function<void(size_t lane, size_t k)> &on_device)
{
    calls.assign(lanes.size(), {});
    stats.assign(lanes.size(), {});
    std::vector<std::exception_ptr> errs(lanes.size());
    csvhost::WorkerThreads &pool = csvhost::WorkerThreads::instance();
    std::vector<csvhost::WorkerThreads::Ticket> threads;
    for (size_t l = 0; l < lanes.size(); l++) {
        threads.push_back(pool.start([&, l] {
            try {
                SVCaller caller(lanes[l].ctx);
                caller.min_mapq = min_mapq; caller.min_oplen = min_oplen;
                caller.merge_on_device = lanes[l].merge_on_device; caller.merge_max_partitions = lanes[l].merge_max_partitions;
                if (on_merged) caller.on_merged = [&on_merged, l](size_t k) { on_merged(l, k); };
                if (on_device) caller.on_device = [&on_device, l](size_t k) { on_device(l, k); };
                if (!lanes[l].seqs.empty()) caller.processResidentChromosomesPipelined(lanes[l].shards, lanes[l].seqs, eps, pct, calls[l], stats[l]);
                else caller.processResidentChromosomesPipelined(lanes[l].shards, seq, eps, pct, calls[l], stats[l]);
            } catch (...) { errs[l] = std::current_exception(); }
        }));
    }
    for (auto &t : threads) pool.wait(t);
    for (auto &e : errs) if (e) std::rethrow_exception(e);
}

void SVCaller::processChromosome(const std::string &chr, const csv_reads &reads, const SeqStore *seq, uint32_t depth_len, double eps,
                                 double pct, std::vector<SVCall> &chr_sv_calls, ChrStats &stats, csv_shard **keep_shard)
{
    printMessage(chr + ": CIGAR SVs...");
    csv_shard *sh = csvgpu_shard_upload(ctx, &reads, depth_len);
    if (!sh) throw std::runtime_error(std::string("processChromosome: ") + csvgpu_last_error(ctx));
    try {
        processResidentChromosome(chr, sh, seq, eps, pct, chr_sv_calls, stats);
    } catch (...) {
        csvgpu_shard_free(ctx, sh);
        throw;
    }
    if (keep_shard) *keep_shard = sh; else csvgpu_shard_free(ctx, sh);
}


namespace {
// alignment intervals of selected records of resident shards (csvgpu_aln_intervals_gather_batch): shard_of[c] is the resident shard of
// split-pass contig c
struct ShardIntervals : IntervalSource {
    ShardIntervals(csv_ctx *ctx, std::vector<csv_shard *> shard_of) : ctx(ctx), shard_of(std::move(shard_of)) {}
    void gather(const std::vector<size_t> &which, const std::vector<uint32_t> &rec, const std::vector<uint64_t> &rec_off, int32_t *ref_end, int32_t *q_start,
                int32_t *q_end) const override
    {
        std::vector<csv_shard *> sh(which.size());
        for (size_t k = 0; k < which.size(); k++) sh[k] = shard_of[which[k]];
        check(ctx, csvgpu_aln_intervals_gather_batch(ctx, (int)sh.size(), sh.data(), rec.data(), rec_off.data(), ref_end, q_start, q_end), "alignment intervals");
    }
    csv_ctx *ctx;
    std::vector<csv_shard *> shard_of;
};

// the iteration order of the reference's per-chromosome qname map from the device (csvgpu_split_order): shard_of[c] is the resident
// shard of split-pass contig c (its query-name hashes were attached when it was staged). self_ok = false: a complete run takes the two-call
// form too (RunSchedule::split_order_self)
struct ShardOrderSource : SplitOrderSource {
    ShardOrderSource(csv_ctx *ctx, std::vector<csv_shard *> shard_of, bool self_ok) : ctx(ctx), shard_of(std::move(shard_of)), self_ok(self_ok) {}
    void begin(const std::vector<size_t> &which, int min_mapq, bool complete) const override
    {
        pending.clear();
        if (which.empty() || which.size() > 32) return;                           // (more than one batch: the one-call form below)
        std::vector<csv_shard *> sh(which.size());
        for (size_t k = 0; k < which.size(); k++) sh[k] = shard_of[which[k]];
        // every contig of the run in this one call: the supplementary hashes are the shards' own and the whole order is queued now
        pending_self = complete && self_ok;
        check(ctx, pending_self ? csvgpu_split_order_begin_self(ctx, (int)sh.size(), sh.data(), (uint8_t)min_mapq)
                                : csvgpu_split_order_begin(ctx, (int)sh.size(), sh.data(), (uint8_t)min_mapq), "split-read order (begin)");
        pending = which; pending_mapq = min_mapq;
    }
    void survivors(const std::vector<size_t> &which, int min_mapq, const std::vector<uint64_t> &supp_hash, std::vector<std::vector<uint32_t>> &recs) const override
    {
        recs.assign(which.size(), {});
        if (!pending.empty() && pending == which && pending_mapq == min_mapq) {      // the head start was taken: only the last epochs are left
            pending.clear();
            const size_t nb = which.size();
            std::vector<uint64_t> off(nb + 1, 0);
            std::vector<uint32_t> out(std::max<size_t>(supp_hash.size() * 2, 1024));
            const uint64_t *sh_p = pending_self ? nullptr : supp_hash.data();
            const uint64_t sh_n = pending_self ? 0 : supp_hash.size();
            int rc = csvgpu_split_order_finish(ctx, sh_p, sh_n, out.data(), out.size(), off.data());
            if (rc == CSV_ECAPACITY) {
                out.resize(off[nb]);
                rc = csvgpu_split_order_finish(ctx, sh_p, sh_n, out.data(), out.size(), off.data());
            }
            check(ctx, rc, "split-read order");
            for (size_t k = 0; k < nb; k++) recs[k].assign(out.begin() + (std::ptrdiff_t)off[k], out.begin() + (std::ptrdiff_t)off[k + 1]);
            return;
        }
        pending.clear();
        for (size_t b0 = 0; b0 < which.size(); b0 += 32) {                       // the entry point takes up to 32 contigs per call
            const size_t nb = std::min<size_t>(32, which.size() - b0);
            std::vector<csv_shard *> sh(nb);
            for (size_t k = 0; k < nb; k++) sh[k] = shard_of[which[b0 + k]];
            std::vector<uint64_t> off(nb + 1, 0);
            std::vector<uint32_t> out(std::max<size_t>(supp_hash.size() * 2, 1024));
            int rc = csvgpu_split_order(ctx, (int)nb, sh.data(), (uint8_t)min_mapq, supp_hash.data(), supp_hash.size(), out.data(), out.size(), off.data());
            if (rc == CSV_ECAPACITY) {
                out.resize(off[nb]);
                rc = csvgpu_split_order(ctx, (int)nb, sh.data(), (uint8_t)min_mapq, supp_hash.data(), supp_hash.size(), out.data(), out.size(), off.data());
            }
            check(ctx, rc, "split-read order");
            for (size_t k = 0; k < nb; k++) recs[b0 + k].assign(out.begin() + (std::ptrdiff_t)off[k], out.begin() + (std::ptrdiff_t)off[k + 1]);
        }
    }
    csv_ctx *ctx;
    std::vector<csv_shard *> shard_of;
    bool self_ok;
    mutable std::vector<size_t> pending;          // the contigs csvgpu_split_order_begin was called for, until _finish
    mutable int pending_mapq = 0;
    mutable bool pending_self = false;            // ... by csvgpu_split_order_begin_self: _finish takes no hashes
};

// the overlap groups from the device (csvgpu_split_groups), on the context that the same thread's interval gather (ShardIntervals) and DBSCAN1D
// batch use: the split pass's calls come one after the other from one thread, and a context is one arena and one stream
struct ShardGroupSource : SplitGroupSource {
    explicit ShardGroupSource(csv_ctx *ctx) : ctx(ctx) {}
    void groups(const std::vector<int32_t> &start, const std::vector<int32_t> &end, const std::vector<uint64_t> &seg_off, std::vector<uint64_t> &seg_group_off,
                std::vector<uint64_t> &group_off, std::vector<uint32_t> &members) const override
    {
        const uint64_t n_seg = seg_off.size() - 1;
        seg_group_off.assign(n_seg + 1, 0);
        group_off.assign(start.size() + 1, 0);
        members.resize(std::max<size_t>(start.size() * 2, 1024));            // (events of a few dozen reads: about one entry per member)
        uint64_t n = members.size();
        int rc = csvgpu_split_groups(ctx, start.data(), end.data(), seg_off.data(), n_seg, seg_group_off.data(), group_off.data(), members.data(), &n);
        if (rc == CSV_ECAPACITY) {
            members.resize(n);
            rc = csvgpu_split_groups(ctx, start.data(), end.data(), seg_off.data(), n_seg, seg_group_off.data(), group_off.data(), members.data(), &n);
        }
        check(ctx, rc, "split-read overlap groups");
        members.resize(n);
        group_off.resize(seg_group_off[n_seg] + 1);
    }
    csv_ctx *ctx;
};

// the groups' evidence from the device (csvgpu_split_fits on given groups, csvgpu_split_groups_fits when the device computes the groups too), on the same
// context and from the same thread as the sources above
static_assert(sizeof(SplitFit) == sizeof(csv_split_fit) && sizeof(SplitFit) == 64 && offsetof(SplitFit, median) == offsetof(csv_split_fit, median) &&
              offsetof(SplitFit, size) == offsetof(csv_split_fit, size) && offsetof(SplitFit, n_members) == offsetof(csv_split_fit, n_members) &&
              offsetof(SplitFit, n_opposite) == offsetof(csv_split_fit, n_opposite) && offsetof(SplitFit, reserved) == offsetof(csv_split_fit, reserved),
              "SplitFit (split_caller.h, which does not see the C-ABI header) is csv_split_fit field for field");
struct ShardFitSource : SplitFitSource {
    explicit ShardFitSource(csv_ctx *ctx) : ctx(ctx) {}
    void fits(const SplitFitTables &T, const std::vector<uint64_t> &seg_off, const Groups *groups, double eps, int min_pts,
              std::vector<uint64_t> &seg_group_off, std::vector<SplitFit> &out) const override
    {
        const uint64_t n_seg = seg_off.size() - 1;
        csv_split_tables t;
        t.n_members = T.start.size(); t.n_supp = T.supp_start.size();
        t.start = T.start.data(); t.end = T.end.data(); t.q_start = T.q_start.data(); t.q_end = T.q_end.data(); t.reverse = T.reverse.data();
        t.supp_off = T.supp_off.data();
        t.supp_start = T.supp_start.data(); t.supp_end = T.supp_end.data(); t.supp_q_start = T.supp_q_start.data(); t.supp_q_end = T.supp_q_end.data();
        t.supp_flags = T.supp_flags.data();
        if (groups) {
            seg_group_off = *groups->seg_group_off;
            out.assign(std::max<size_t>(seg_group_off.back(), 1), SplitFit());
            check(ctx, csvgpu_split_fits(ctx, &t, seg_off.data(), n_seg, seg_group_off.data(), groups->group_off->data(), groups->members->data(), eps, min_pts,
                                         (csv_split_fit *)out.data()), "split-read group fits");
            out.resize(seg_group_off.back());
            return;
        }
        seg_group_off.assign(n_seg + 1, 0);
        out.assign(std::max<size_t>(T.start.size(), 1), SplitFit());
        uint64_t n_groups = 0;
        check(ctx, csvgpu_split_groups_fits(ctx, &t, seg_off.data(), n_seg, eps, min_pts, seg_group_off.data(), (csv_split_fit *)out.data(), &n_groups),
              "split-read overlap groups and fits");
        out.resize(n_groups);
    }
    csv_ctx *ctx;
};

// tables, groups and fits from the device, given record references into the resident shards (csvgpu_split_resident_fits); shard_of[c] is the
// resident shard of split-pass contig c, as for ShardIntervals, and the context and thread are theirs
struct ShardTableSource : SplitTableSource {
    ShardTableSource(csv_ctx *ctx, std::vector<csv_shard *> shard_of) : ctx(ctx), shard_of(std::move(shard_of)) {}
    void fits(const std::vector<size_t> &which, const SplitRefTables &R, const std::vector<uint64_t> &seg_off, double eps, int min_pts,
              std::vector<uint64_t> &seg_group_off, std::vector<SplitFit> &out) const override
    {
        std::vector<csv_shard *> sh(which.size());
        for (size_t k = 0; k < which.size(); k++) sh[k] = shard_of.at(which[k]);
        csv_split_refs f;
        f.n_members = R.member_rec.size(); f.n_supp = R.supp_rec.size();
        f.member_rec = R.member_rec.data(); f.supp_off = R.supp_off.data(); f.supp_rec = R.supp_rec.data(); f.supp_where = R.supp_where.data();
        seg_group_off.assign(which.size() + 1, 0);
        out.assign(std::max<size_t>(R.member_rec.size(), 1), SplitFit());
        uint64_t n_groups = 0;
        check(ctx, csvgpu_split_resident_fits(ctx, which.size(), sh.data(), &f, seg_off.data(), eps, min_pts, seg_group_off.data(), (csv_split_fit *)out.data(), &n_groups),
              "split-read tables, overlap groups and fits");
        out.resize(n_groups);
    }
    csv_ctx *ctx;
    std::vector<csv_shard *> shard_of;
};

}  // namespace

std::unique_ptr<SplitGroupSource> makeDeviceGroupSource(csv_ctx *ctx) { return std::unique_ptr<SplitGroupSource>(new ShardGroupSource(ctx)); }
std::unique_ptr<SplitFitSource> makeDeviceFitSource(csv_ctx *ctx) { return std::unique_ptr<SplitFitSource>(new ShardFitSource(ctx)); }

// what the split-read pass of a run works on (built once per run; prepare() may already be running while the CIGAR pass is on the device)
struct SVCaller::SplitSetup {
    std::vector<SplitContig> blocks;
    std::vector<int> block_of;                          // per contig of the run: its index in `blocks`, or -1
    std::vector<std::string> names;
    std::unique_ptr<ShardOrderSource> dev_order;
    std::unique_ptr<ShardIntervals> intervals;
    std::unique_ptr<ShardGroupSource> dev_groups;
    std::unique_ptr<ShardFitSource> dev_fits;
    std::unique_ptr<ShardTableSource> dev_tables;
    SplitParams sp;
    std::unique_ptr<SplitPass> pass;
    double ms_prepare = 0.0;
};

namespace {
struct EmptySnps : SNPSource {
    void query(uint32_t, uint32_t, std::vector<uint32_t> &, std::unordered_map<uint32_t, double> &, std::unordered_map<uint32_t, double> &) const override {}
};

struct VectorSource : ContigSource {
    explicit VectorSource(const std::vector<ChromosomeInput> &v) : v(v) {}
    bool next(ChromosomeInput &out) override { if (i >= v.size()) return false; out = v[i++]; return true; }
    const std::vector<ChromosomeInput> &v;
    size_t i = 0;
};

using CallMap = std::unordered_map<std::string, std::vector<SVCall>>;

CNVCaller makeCnv(csv_ctx *ctx, const RunParams &P)
{
    CNVCaller cn(ctx);
    cn.sample_size = P.sample_size; cn.min_cnv_length = P.min_cnv_length; cn.host_threads = P.host_threads;
    cn.device_observations = P.cn_observations_on_device;
    return cn;
}

struct ThreadContext {                                  // this thread's context for the host passes' clustering calls, while in scope
    explicit ThreadContext(csv_ctx *c) { csvhost::set_thread_context(c); }
    ~ThreadContext() { csvhost::set_thread_context(nullptr); }
};

// The contigs of a run as the passes behind the CIGAR merge see them: resident data, mean coverage and CIGAR calls (the lanes' result
// vectors during the CIGAR pass, the call map behind it). Its steps are what the run does with a set of contigs behind their CIGAR
// copy-number predictions (sv_caller.cpp:885-927 of the reference): split-read signatures -> their copy-number predictions -> mergeSVs of
// the split calls -> concatenation -> final mergeSVs. Nothing in them reaches across contigs (supplementary records on another contig only
// answer tid tests, :352-354), so any partition of the contigs gives the same calls: an early batch takes every step inside the CIGAR pass
// (splitChain), the split chain beside the pass the first two, finishRun whatever is left behind the pass.
struct RunContigs {
    RunContigs(const std::vector<ResidentContig> &contigs, const CHMM &hmm, const RunParams &P)
        : contigs(contigs), hmm(hmm), P(P), mean_cov(contigs.size(), 0.0), calls(contigs.size(), nullptr)
    {
        for (size_t i = 0; i < contigs.size(); i++) index_of[contigs[i].name] = i;
    }
    const std::vector<ResidentContig> &contigs;
    const CHMM &hmm;
    const RunParams &P;
    std::unordered_map<std::string, size_t> index_of;
    std::vector<double> mean_cov;                       // per contig
    std::vector<std::vector<SVCall> *> calls;           // per contig: its CIGAR calls

    // the copy-number job of contig i over `v` (its CIGAR or its split-read calls)
    CNVCaller::ContigJob job(size_t i, std::vector<SVCall> &v) const
    {
        static const EmptySnps no_snps;
        CNVCaller::ContigJob j;
        j.chr = contigs[i].name; j.calls = &v; j.mean_chr_cov = mean_cov[i]; j.shard = contigs[i].shard;
        j.snps = contigs[i].snps ? contigs[i].snps : (const SNPSource *)&no_snps; j.depth_len = contigs[i].depth_len;
        return j;
    }
    // the jobs of the contigs of `m` that have calls and are not in `skip`, in the map's own order (the reference walks its map)
    std::vector<CNVCaller::ContigJob> jobs(CallMap &m, const std::vector<char> *skip = nullptr) const
    {
        std::vector<CNVCaller::ContigJob> out;
        for (auto &entry : m) {
            if (entry.second.empty()) continue;
            const size_t i = index_of.at(entry.first);
            if (skip && (*skip)[i]) continue;
            out.push_back(job(i, entry.second));
        }
        return out;
    }
    // split-read signatures of the contigs `idx` (their scans are over: the alignment intervals exist)
    CallMap findSplit(SplitPass &pass, const std::vector<int> &block_of, const std::vector<size_t> &idx) const
    {
        std::vector<size_t> blocks;
        for (size_t i : idx) if (block_of[i] >= 0) blocks.push_back((size_t)block_of[i]);
        CallMap split;
        pass.finishFor(blocks, split);
        return split;
    }
    void predictSplit(const CNVCaller &cn, CallMap &split) const { std::vector<CNVCaller::ContigJob> j = jobs(split); cn.runSplitReadCopyNumberPredictionsAll(j, hmm); }
    void mergeSplit(CallMap &split) const
    {
        std::vector<std::vector<SVCall> *> sets;
        for (auto &entry : split) sets.push_back(&entry.second);
        if (P.merge_split_svs) mergeSVsMany(sets, 0.1, 2, true, P.host_threads);
    }
    // the split calls behind each contig's CIGAR calls; -> how many
    size_t appendSplit(const CallMap &split) const
    {
        size_t k = 0;
        for (const auto &entry : split) {
            k += entry.second.size();
            std::vector<SVCall> &dst = *calls[index_of.at(entry.first)];
            dst.insert(dst.end(), entry.second.begin(), entry.second.end());
        }
        return k;
    }
    void mergeFinal(const std::vector<size_t> &idx) const
    {
        std::vector<std::vector<SVCall> *> sets;
        for (size_t i : idx) sets.push_back(calls[i]);
        if (P.merge_final_svs) mergeSVsMany(sets, 0.1, 2, true, P.host_threads);
    }
    // every step for the contigs `idx`, whose CIGAR copy-number predictions are made; -> the number of split-read calls
    size_t splitChain(SplitPass &pass, const std::vector<int> &block_of, const std::vector<size_t> &idx, const CNVCaller &cn) const
    {
        CallMap split = findSplit(pass, block_of, idx);
        predictSplit(cn, split);
        mergeSplit(split);
        const size_t k = appendSplit(split);
        mergeFinal(idx);
        return k;
    }
};
}  // namespace

// runResident's work beside the CIGAR pass. With lanes, the caller's own context is idle during the pass, and the first half of the
// split-read pass needs nothing the pass produces (flags, name hashes -> the qname map's iteration order): a task runs it there, on another
// thread (prepare). When it is done the pass is a little over half way, and the task goes on with
//  - early batches: the CIGAR copy-number predictions of the contigs whose calls are final by then, and every later step of the run for
//    them (RunContigs::splitChain), in place on the lanes' result vectors; another batch whenever a few more contigs are merged. What is
//    left when the pass ends is done behind it;
//  - then, or instead (a rank with few contigs, or short reads: a first half as long as the pass, takes no batch), the split chain beside
//    the pass: it needs the scans' alignment intervals and, for its copy-number pass, the depth maps and mean coverages — all there when a
//    contig's device chain is over, before its host merge. The task runs it for every contig that went through no early batch, beside the
//    rest of the pass and the CIGAR copy-number pass; finishRun meets it in front of the split chain.
// Which of these the task does is decided by timing, within what RunSchedule allows; the calls never depend on it.
struct SVCaller::PassOverlap {
    PassOverlap(SVCaller &caller, std::vector<ResidentContig> &contigs, const std::vector<csv_ctx *> &lane_ctxs, const CHMM &hmm, const RunParams &P)
        : ctx(caller.ctx), P(P), R(contigs, hmm, P), n(contigs.size()),
          task(P.split_svs && P.cigar_svs && n && lane_ctxs.size() > 1 && P.overlap_split_prepare),
          early(task && P.cigar_cn && !P.save_cnv && P.schedule.early_batches != RunSchedule::EarlyBatches::None),
          forced(P.schedule.early_batches == RunSchedule::EarlyBatches::AllAtOnce || P.schedule.early_batches == RunSchedule::EarlyBatches::EveryThree),
          beside(task && !P.save_cnv && !forced && P.schedule.split_beside_pass),
          side_ctx(lane_ctxs.size() > 1 ? lane_ctxs[0] : nullptr), finished(n, 0)
    {
        if (P.split_svs) split = caller.makeSplitSetup(contigs, P);
        if (task) ticket = csvhost::WorkerThreads::instance().start([this] { work(); });
    }
    ~PassOverlap() { { std::lock_guard<std::mutex> l(mu); pass_over = true; } wait(); }     // (also when the pass throws: the task refers to the run's frame)

    // from the lanes (any thread): contig i's device chain is over (its depth map, alignment intervals and statistics are final) / its calls are final
    void deviceDone(size_t i, const ChrStats &st) { R.mean_cov[i] = st.mean_chr_cov; std::lock_guard<std::mutex> l(mu); device_done.push_back(i); }
    void merged(size_t i, std::vector<SVCall> &calls) { R.calls[i] = &calls; std::lock_guard<std::mutex> l(mu); merged_.push_back(i); }
    // The CIGAR pass has returned: the task takes no batch any more (early batches work on the lanes' vectors in place: they must be over
    // before those move). The run goes on without waiting for a task still inside prepare() — the CIGAR copy-number pass needs nothing of
    // it — or running the split chain beside the pass, and meets it in front of the split chain (join). Any other task is over on return.
    // (With save_cnv the copy-number passes run on the caller's context, which a task still running would use: the run waits.)
    void passOver()
    {
        bool later;
        { std::lock_guard<std::mutex> l(mu); pass_over = true; later = ticket && (!prepare_over || split_only) && !forced && !P.save_cnv; }
        if (!later) join();
    }
    void join() { wait(); if (err) std::rethrow_exception(err); }

    csv_ctx *const ctx;
    const RunParams &P;
    RunContigs R;
    const size_t n;
    // what does not depend on timing, decided once: whether the task starts; whether it may take early batches; whether the schedule forces
    // them (tests: no split chain beside the pass and no late join then); whether it may run the split chain beside the pass
    const bool task, early, forced, beside;
    csv_ctx *const side_ctx;                           // a lane's context, idle behind the pass (finishRun's CIGAR copy-number pass)
    std::unique_ptr<SplitSetup> split;
    // read by finishRun after join()
    std::vector<char> finished;                        // per contig: every step of the run made in an early batch (its calls are final)
    size_t regions = 0, n_split_calls = 0;             // of the early batches
    CallMap pre_split;                                 // the split chain beside the pass: the split-read calls, copy-number predictions made ...
    bool pre_ready = false;                            // ... of every contig that went through no early batch

private:
    void wait() { if (ticket) { csvhost::WorkerThreads::instance().wait(ticket); ticket = nullptr; } }
    void work()
    {
        prepare();
        bool late;                                     // prepare() outlasted the CIGAR pass (short reads): the run has gone on without waiting
        { std::lock_guard<std::mutex> l(mu); prepare_over = true; late = pass_over && !forced; }
        if (err) return;
        try {
            if (late) {
                if (beside) splitBesidePass();
                return;
            }
            if (early) earlyBatches();
            if (beside && takeSplitOnly()) splitBesidePass();
        } catch (...) { err = std::current_exception(); }
    }
    void prepare()
    {
        const double t0 = now_ms();
        if (P.schedule.prepare_delay_ms > 0) std::this_thread::sleep_for(std::chrono::milliseconds(P.schedule.prepare_delay_ms));
        try { split->pass->prepare(); } catch (...) { err = std::current_exception(); }
        split->ms_prepare = now_ms() - t0;
    }
    // One batch now (a little over half the genome is merged), then another whenever a few more contigs are: what is left for the end of the
    // pass is the last contigs' share. The pass's end ends the loop; whatever was not taken here is done behind the pass.
    void earlyBatches()
    {
        const RunSchedule::EarlyBatches mode = P.schedule.early_batches;
        if (mode == RunSchedule::EarlyBatches::AllAtOnce)               // every contig through this path, whatever the timing
            for (int spin = 0; spin < 200000; spin++) {
                { std::lock_guard<std::mutex> l(mu); if (merged_.size() >= n) break; }
                std::this_thread::sleep_for(std::chrono::microseconds(50));
            }
        size_t taken = 0;
        for (bool first = true;; first = false) {
            std::vector<size_t> batch;
            bool over;
            size_t unmerged;
            { std::lock_guard<std::mutex> l(mu); batch.assign(merged_.begin() + (std::ptrdiff_t)taken, merged_.end()); over = pass_over; unmerged = n - merged_.size(); }
            // (a batch takes a few milliseconds beside the pass: with fewer than eight contigs still to come the pass could be over first and
            // the run would wait for the batch — those go with the rest; a rank with a handful of contigs never takes one)
            if (mode == RunSchedule::EarlyBatches::Timed && unmerged < 8) return;
            if (mode == RunSchedule::EarlyBatches::EveryThree && first && batch.size() < 3 && !over) { std::this_thread::sleep_for(std::chrono::microseconds(100)); continue; }
            if (!first && over) return;
            if (!first && batch.size() < 3) { std::this_thread::sleep_for(std::chrono::microseconds(100)); continue; }
            taken += batch.size();
            takeBatch(batch);
            if (mode == RunSchedule::EarlyBatches::AllAtOnce) return;
        }
    }
    void takeBatch(const std::vector<size_t> &batch)
    {
        std::vector<CNVCaller::ContigJob> jobs;
        for (size_t i : batch) if (!R.calls[i]->empty()) jobs.push_back(R.job(i, *R.calls[i]));
        csvhost::TraceScope tr(jobs.empty() ? "cn: early batch (nothing merged yet)" : "cn: early batch");
        ThreadContext tc(ctx);
        const CNVCaller cn = makeCnv(ctx, P);
        if (!jobs.empty()) regions += cn.runCIGARCopyNumberPredictionAll(jobs, R.hmm);
        csvhost::TraceScope tr2("run: early split chain + merges");
        n_split_calls += R.splitChain(*split->pass, split->block_of, batch, cn);
        for (size_t i : batch) finished[i] = 1;
    }
    // the task takes no (more) early batches: the split chain beside the pass, unless the pass is over already
    bool takeSplitOnly() { std::lock_guard<std::mutex> l(mu); split_only = !pass_over; return split_only; }
    // whatever is ready goes now, the rest as it comes (a rank of six contigs has two ready when the first half is over and the last one when
    // the pass ends: what runs behind the pass is that one's chain, not all six)
    void splitBesidePass()
    {
        size_t taken = 0;
        for (;;) {
            std::vector<size_t> ready;
            bool over;
            { std::lock_guard<std::mutex> l(mu); ready.assign(device_done.begin() + (std::ptrdiff_t)taken, device_done.end()); over = pass_over; }
            if (ready.empty()) {
                if (taken >= n || over) break;                           // (over with contigs missing: the pass failed)
                std::this_thread::sleep_for(std::chrono::microseconds(50));
                continue;
            }
            taken += ready.size();
            csvhost::TraceScope tr("run: split chain beside the pass");
            std::vector<size_t> todo;                                    // (a contig that went through an early batch has its split calls merged in)
            for (size_t i : ready) if (!finished[i] && split->block_of[i] >= 0) todo.push_back(i);
            if (todo.empty()) continue;
            ThreadContext tc(ctx);
            CallMap part = R.findSplit(*split->pass, split->block_of, todo);
            R.predictSplit(makeCnv(ctx, P), part);
            for (auto &entry : part) pre_split[entry.first] = std::move(entry.second);
        }
        pre_ready = taken >= n;
    }

    std::mutex mu;                                     // guards what follows
    std::vector<size_t> device_done, merged_;          // contigs, in the order the lanes reported them
    bool pass_over = false;                            // the CIGAR pass has returned: no batch may be taken any more
    bool prepare_over = false;                         // the task is past prepare()
    bool split_only = false;                           // the task runs the split chain beside the pass; the run meets it in front of the split chain
    std::exception_ptr err;
    csvhost::WorkerThreads::Ticket ticket = nullptr;
};

void SVCaller::run(const std::vector<ChromosomeInput> &contigs, const CHMM &hmm, const RunParams &P,
                   std::unordered_map<std::string, std::vector<SVCall>> &whole_genome_sv_calls)
{
    VectorSource src(contigs);
    run(src, hmm, P, whole_genome_sv_calls);
}

void SVCaller::run(ContigSource &source, const CHMM &hmm, const RunParams &P,
                   std::unordered_map<std::string, std::vector<SVCall>> &whole_genome_sv_calls)
{
    csvhost::set_context(ctx);
    // what outlives a contig's host arrays: its shard (reads, depth map, alignment intervals in HBM), its statistics, its SNP
    // source, and per record the 7 bytes + query name (hash + bytes) that the split-read pass groups by
    struct Kept {
        std::vector<int32_t> pos; std::vector<uint16_t> flag; std::vector<uint8_t> mapq;
        std::vector<uint64_t> qhash, name_off; std::string names;
    };
    std::vector<std::unique_ptr<Kept>> kept;
    std::vector<ResidentContig> contigs;
    std::vector<ChrStats> stats;
    auto free_all = [&] { for (ResidentContig &c : contigs) if (c.shard) csvgpu_shard_free(ctx, c.shard); };
    try {
        // depth pass + CIGAR pass + CIGAR merge (sv_caller.cpp:794-863); the reference pre-seeds the map with every contig
        ChromosomeInput c;
        while (source.next(c)) {
            const size_t i = contigs.size();
            // a resident shard is this run's from the moment next() returned it: held here until contigs[i] (and with it free_all) has it
            struct Taken { csv_ctx *x; csv_shard *s; ~Taken() { if (s) csvgpu_shard_free(x, s); } } taken{ctx, c.resident};
            contigs.emplace_back();
            stats.emplace_back();
            kept.emplace_back(new Kept());
            contigs[i].name = c.name; contigs[i].depth_len = c.depth_len; contigs[i].snps = c.snps;
            contigs[i].seq = nullptr;                                 // the sequences are only valid until the next contig: ALT strings are cut now
            contigs[i].split.tid = (int32_t)i;
            std::vector<SVCall> calls;
            if (c.resident) {
                // the reader built the shard on the device (another context of this device; its finish has synchronised): nothing to upload
                contigs[i].shard = c.resident;                        // (owned from here: free_all)
                taken.s = nullptr;
                if (P.cigar_svs) {
                    printMessage(c.name + ": CIGAR SVs...");
                    processResidentChromosome(c.name, c.resident, c.seq, P.dbscan_epsilon, P.dbscan_min_pts_pct, calls, stats[i]);
                }
                // the ALT strings are cut: the packed sequences, the largest of the shard's arrays, go
                check(ctx, csvgpu_shard_drop_sequences(ctx, c.resident), "run: drop_sequences");
                if (!P.cigar_svs) { csvgpu_shard_free(ctx, c.resident); contigs[i].shard = nullptr; }
            } else if (P.cigar_svs) processChromosome(c.name, c.reads, c.seq, c.depth_len, P.dbscan_epsilon, P.dbscan_min_pts_pct, calls, stats[i], &contigs[i].shard);
            whole_genome_sv_calls[c.name] = std::move(calls);
            if (P.split_svs && c.qnames && contigs[i].shard) {                          // inputs of the split-read pass (:133-175)
                const uint64_t n = c.reads.n_reads;
                Kept &K = *kept[i];
                K.pos.assign(c.reads.pos, c.reads.pos + n); K.flag.assign(c.reads.flag, c.reads.flag + n); K.mapq.assign(c.reads.mapq, c.reads.mapq + n);
                K.qhash.resize(n); K.name_off.resize(n + 1);
                size_t bytes = 0;
                for (uint64_t r = 0; r < n; r++) bytes += (*c.qnames)[r].size();
                K.names.reserve(bytes);
                for (uint64_t r = 0; r < n; r++) {
                    const std::string &q = (*c.qnames)[r];
                    K.qhash[r] = csvhost::std_string_hash(q.data(), q.size());
                    K.name_off[r] = K.names.size();
                    K.names += q;
                }
                K.name_off[n] = K.names.size();
                SplitContig &sc = contigs[i].split;
                sc.n = n; sc.pos = K.pos.data(); sc.flag = K.flag.data(); sc.mapq = K.mapq.data();
                sc.qhash = K.qhash.data(); sc.name_bytes = K.names.data(); sc.name_off = K.name_off.data();
            }
        }
        RunStageTimes T;
        finishRun(contigs, stats, hmm, P, whole_genome_sv_calls, T);
    } catch (...) {
        free_all();
        throw;
    }
    free_all();
}

void SVCaller::runResident(const std::vector<ResidentContig> &contigs_in, const std::vector<csv_ctx *> &lane_ctxs, const CHMM &hmm, const RunParams &P,
                           std::unordered_map<std::string, std::vector<SVCall>> &whole_genome_sv_calls, std::vector<ChrStats> *stats_out, RunStageTimes *times)
{
    csvhost::set_context(ctx);
    const double t_begin = now_ms();
    RunStageTimes T;
    // The caller's own context works on another thread while the lanes run the CIGAR pass (PassOverlap): a context is one arena + one stream
    // + one set of timers and belongs to one thread at a time.
    for (csv_ctx *lc : lane_ctxs)
        if (lc == ctx) throw std::invalid_argument("runResident: the caller's context must not be one of the lanes (each lane needs a context of its own)");
    for (size_t a = 0; a < lane_ctxs.size(); a++)
        for (size_t b = 0; b < a; b++)
            if (lane_ctxs[a] == lane_ctxs[b]) throw std::invalid_argument("runResident: the same context given for two lanes");
    std::vector<ResidentContig> contigs = contigs_in;
    const size_t n = contigs.size();
    std::vector<ChrStats> stats(n);
    std::vector<std::vector<SVCall>> per(n);
    // contigs over the lanes: longest processing time first by read count, every lane works down its list
    const size_t L = std::max<size_t>(1, lane_ctxs.size());
    std::vector<Lane> lanes(L);
    std::vector<std::vector<size_t>> which(L);
    std::vector<std::vector<std::vector<SVCall>>> lane_calls;
    std::vector<std::vector<ChrStats>> lane_stats;
    if (P.cigar_svs && n) {
        for (size_t l = 0; l < L; l++) { lanes[l].ctx = lane_ctxs.empty() ? ctx : lane_ctxs[l]; lanes[l].merge_on_device = merge_on_device; lanes[l].merge_max_partitions = merge_max_partitions; }
        std::vector<size_t> order(n);
        for (size_t i = 0; i < n; i++) order[i] = i;
        std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return contigs[a].split.n != contigs[b].split.n ? contigs[a].split.n > contigs[b].split.n : contigs[a].depth_len != contigs[b].depth_len ? contigs[a].depth_len > contigs[b].depth_len : a < b; });
        std::vector<double> load(L, 0.0);
        for (size_t i : order) {
            size_t l = 0;
            for (size_t k = 1; k < L; k++) if (load[k] < load[l]) l = k;
            lanes[l].shards.push_back(contigs[i].shard);
            lanes[l].seqs.push_back(contigs[i].seq);
            which[l].push_back(i);
            load[l] += (double)std::max<uint64_t>(contigs[i].split.n, contigs[i].depth_len / 400);
        }
    }
    PassOverlap overlap(*this, contigs, lane_ctxs, hmm, P);
    if (P.cigar_svs && n) {
        csvhost::TraceScope tr_pass("run: CIGAR pass");
        if (L == 1) {
            lane_calls.resize(1); lane_stats.resize(1);
            SVCaller one(lanes[0].ctx);
            one.min_mapq = min_mapq; one.min_oplen = min_oplen;
            one.merge_on_device = merge_on_device; one.merge_max_partitions = merge_max_partitions;
            one.processResidentChromosomesPipelined(lanes[0].shards, lanes[0].seqs, P.dbscan_epsilon, P.dbscan_min_pts_pct, lane_calls[0], lane_stats[0]);
        } else {
            std::function<void(size_t, size_t)> on_merged, on_device;
            if (overlap.early) on_merged = [&](size_t l, size_t k) { overlap.merged(which[l][k], lane_calls[l][k]); };
            if (overlap.task) on_device = [&](size_t l, size_t k) { overlap.deviceDone(which[l][k], lane_stats[l][k]); };
            processResidentLanes(lanes, nullptr, P.dbscan_epsilon, P.dbscan_min_pts_pct, lane_calls, lane_stats, on_merged, min_mapq, min_oplen, on_device);
        }
        T.ms_cigar = now_ms() - t_begin;
        overlap.passOver();
        for (size_t l = 0; l < L; l++)
            for (size_t k = 0; k < which[l].size(); k++) { per[which[l][k]] = std::move(lane_calls[l][k]); stats[which[l][k]] = lane_stats[l][k]; }
    } else T.ms_cigar = now_ms() - t_begin;
    for (size_t i = 0; i < n; i++) {                                   // the map is filled in contig order, as run() does
        T.n_signatures += stats[i].n_signatures; T.n_cigar_calls += per[i].size(); T.n_reads += contigs[i].split.n;
        whole_genome_sv_calls[contigs[i].name] = std::move(per[i]);
    }
    T.n_cigar_cn_regions += overlap.regions;                           // (a task the run meets later takes no batch after the pass)
    T.n_split_calls += overlap.n_split_calls;
    finishRun(contigs, stats, hmm, P, whole_genome_sv_calls, T, &overlap);
    T.ms_total = now_ms() - t_begin;
    if (stats_out) *stats_out = stats;
    if (times) *times = T;
}

std::unique_ptr<SVCaller::SplitSetup> SVCaller::makeSplitSetup(std::vector<ResidentContig> &contigs, const RunParams &P)
{
    std::unique_ptr<SplitSetup> S(new SplitSetup());
    std::vector<csv_shard *> shard_of;
    for (size_t i = 0; i < contigs.size(); i++) {
        ResidentContig &c = contigs[i];
        S->names.push_back(c.name);
        S->block_of.push_back(-1);
        if (!c.split.qhash || !c.shard || !c.split.n) continue;
        S->block_of.back() = (int)S->blocks.size();
        c.split.tid = (int32_t)i;
        c.split.ref_end = c.split.q_start = c.split.q_end = nullptr;     // the scan kernel's per-read intervals (the reference's third BAM pass, :137-172) stay in the shards
        S->blocks.push_back(c.split);
        shard_of.push_back(c.shard);
    }
    S->sp.min_mapq = min_mapq; S->sp.threads = P.host_threads;
    S->dev_order.reset(new ShardOrderSource(ctx, shard_of, P.schedule.split_order_self));
    S->intervals.reset(new ShardIntervals(ctx, shard_of));
    S->sp.intervals = S->intervals.get();
    if (P.split_order_on_device) S->sp.device_order = S->dev_order.get();          // only contigs staged with unique_names take it
    S->dev_groups.reset(new ShardGroupSource(ctx));
    if (P.split_groups_on_device) S->sp.device_groups = S->dev_groups.get();
    S->dev_fits.reset(new ShardFitSource(ctx));
    if (P.split_fits_on_device) S->sp.device_fits = S->dev_fits.get();
    S->dev_tables.reset(new ShardTableSource(ctx, shard_of));
    if (P.split_tables_on_device) S->sp.device_tables = S->dev_tables.get();
    S->pass.reset(new SplitPass(S->blocks, S->names, S->sp));
    return S;
}

void SVCaller::finishRun(std::vector<ResidentContig> &contigs, const std::vector<ChrStats> &stats, const CHMM &hmm, const RunParams &P,
                         std::unordered_map<std::string, std::vector<SVCall>> &whole_genome_sv_calls, RunStageTimes &T, PassOverlap *overlap)
{
    csvhost::WorkerThreads::Ticket teardown = nullptr;
    struct JoinTeardown {
        csvhost::WorkerThreads::Ticket &t;
        ~JoinTeardown() { if (t) csvhost::WorkerThreads::instance().wait(t); }
    } join_teardown{teardown};
    RunContigs R(contigs, hmm, P);
    for (size_t i = 0; i < contigs.size(); i++) { R.mean_cov[i] = stats[i].mean_chr_cov; R.calls[i] = &whole_genome_sv_calls[contigs[i].name]; }
    const std::vector<char> *finished = overlap ? &overlap->finished : nullptr;     // (every step made while the CIGAR pass was still running)
    CNVCaller cnv = makeCnv(ctx, P);
    if (P.save_cnv && !P.vcf.output_dir.empty()) {                                 // main.cpp:109-118
        cnv.save_cnv_data = true;
        cnv.cnv_output_file = P.vcf.output_dir + "/CNVCalls.json";
        std::remove(cnv.cnv_output_file.c_str());
        printMessage("Saving CNV data to: " + cnv.cnv_output_file);
    }
    double t0 = now_ms();
    // The CIGAR copy-number pass (:865-881) and the split-read chain (:885-917) do not depend on each other: with a second context
    // at hand (`side_ctx`: a lane's, idle by now) the former runs on another thread — its own context, its own host pool — while
    // this thread goes on with the latter; they meet in front of the final merge.
    csv_ctx *side_ctx = overlap ? overlap->side_ctx : nullptr;
    csvhost::WorkerThreads::Ticket cn_task = nullptr;
    std::exception_ptr cn_err;
    struct JoinCn {
        csvhost::WorkerThreads::Ticket &t;
        ~JoinCn() { if (t) csvhost::WorkerThreads::instance().wait(t); }
    } join_cn{cn_task};
    if (P.cigar_svs && P.cigar_cn) {
        printMessage("Running copy number predictions on CIGAR SVs...");
        if (side_ctx && side_ctx != ctx && P.split_svs && !cnv.save_cnv_data) {
            cn_task = csvhost::WorkerThreads::instance().start([&, t0] {
                csvhost::HostPool::second_pool_flag() = true;
                try {
                    ThreadContext tc(side_ctx);
                    std::vector<CNVCaller::ContigJob> jobs = R.jobs(whole_genome_sv_calls, finished);
                    T.n_cigar_cn_regions += makeCnv(side_ctx, P).runCIGARCopyNumberPredictionAll(jobs, hmm);
                } catch (...) { cn_err = std::current_exception(); }
                csvhost::HostPool::second_pool_flag() = false;
                T.ms_cigar_cn = now_ms() - t0;
            });
        } else {
            std::vector<CNVCaller::ContigJob> jobs = R.jobs(whole_genome_sv_calls, finished);
            T.n_cigar_cn_regions += cnv.runCIGARCopyNumberPredictionAll(jobs, hmm);
            T.ms_cigar_cn = now_ms() - t0;
        }
    }
    if (P.split_svs) {                                                             // :885-917
        t0 = now_ms();
        std::unique_ptr<SplitSetup> own;
        SplitSetup *split = overlap ? overlap->split.get() : nullptr;
        if (!split) { own = makeSplitSetup(contigs, P); split = own.get(); }
        T.ms_split_fetch = 0.0;
        if (overlap) overlap->join();                                              // (prepare() or the split chain still running beside the pass: meet it here)
        const bool pre = overlap && overlap->pre_ready;                            // (the split chain and its copy-number pass ran beside the CIGAR pass)
        CallMap split_calls;
        if (pre) split_calls = std::move(overlap->pre_split);
        else split->pass->finish(split_calls);                                     // (runs prepare() first when nobody has)
        T.ms_split_prepare = split->ms_prepare;
        {   // the pass's working set (1e5 small vectors for a genome) is torn down beside the next stages, not between them
            std::shared_ptr<SplitPass> dead(split->pass.release());
            teardown = csvhost::WorkerThreads::instance().start([dead]() mutable { dead.reset(); });
        }
        T.ms_split = now_ms() - t0;
        t0 = now_ms();
        if (!pre) R.predictSplit(cnv, split_calls);
        T.ms_split_cn = now_ms() - t0;
        t0 = now_ms();
        R.mergeSplit(split_calls);
        if (cn_task) { csvhost::WorkerThreads::instance().wait(cn_task); cn_task = nullptr; }          // the CIGAR calls are final from here on
        if (cn_err) std::rethrow_exception(cn_err);
        T.n_split_calls += R.appendSplit(split_calls);
        T.ms_merge_split = now_ms() - t0;
    }
    if (cn_task) { csvhost::WorkerThreads::instance().wait(cn_task); cn_task = nullptr; }
    if (cn_err) std::rethrow_exception(cn_err);
    t0 = now_ms();
    std::vector<size_t> rest;                                                      // :919-927, the map's own order
    for (const auto &entry : whole_genome_sv_calls) {
        const size_t i = R.index_of.at(entry.first);
        if (!(finished && (*finished)[i])) rest.push_back(i);
    }
    R.mergeFinal(rest);
    T.ms_merge_final = now_ms() - t0;
    if (cnv.save_cnv_data) CNVCaller::closeJSON(cnv.cnv_output_file);                                       // :929-931
    uint32_t total = 0;
    for (const auto &entry : whole_genome_sv_calls) {
        total += getSVCount(entry.second);
        printMessage("Total SVs detected for " + entry.first + ": " + std::to_string(getSVCount(entry.second)));
    }
    T.n_final_calls = total;
    printMessage("Total SVs detected: " + std::to_string(total));
    if (P.ref_genome && !P.vcf.output_dir.empty()) {                               // :943-945
        t0 = now_ms();
        printMessage("Saving SVs to VCF...");
        ShardDepthSource depth(ctx);
        for (const ResidentContig &c : contigs) if (c.shard) depth.add(c.name, c.shard);
        VCFOptions vcf = P.vcf;
        vcf.format_on_device = vcf_format_on_device; vcf.ctx = ctx;
        saveToVCF(whole_genome_sv_calls, vcf, *P.ref_genome, depth);
        T.ms_vcf = now_ms() - t0;
    }
}

// ---- the run fed from a BAM file ----------------------------------------------------------------------------------
#include <future>

#include "bam_io.h"
#include "snp_io.h"

namespace {
// Contigs decoded one ahead: while run() has contig i on the device, the inflate pool works on contig i + 1.
struct BamSource : ContigSource {
    BamReader reader;
    std::vector<std::string> chrs;
    BamReadOptions opt;
    BamShard cur, ahead;
    std::future<bool> pending;
    SeqStore seq;
    size_t i = 0;
    BamRunStats st;
    SNPFile *snp_file = nullptr;                                  // loaded SNP VCF, or nullptr
    SNPDeviceOptions snp_dev;                                     // how it was loaded (ctx null: the host parser); table() takes the same
    const AlleleFreqFiles *af_files = nullptr;
    std::string ethnicity;

    void launch(size_t k) { pending = std::async(std::launch::async, [this, k] { return reader.readContig(chrs[k], opt, ahead); }); }

    bool next(ChromosomeInput &out) override
    {
        if (i >= chrs.size()) return false;
        const double t0 = now_ms();
        if (!pending.valid()) launch(i);
        const bool ok = pending.get();
        st.ms_decode += now_ms() - t0;
        if (!ok) throw std::runtime_error(reader.error());
        {   // (the reader is between two contigs here: the counters are this contig's)
            const BamReader::UnpackStats &u = reader.unpackStats();
            st.unpack_batches_device += u.batches_device; st.unpack_batches_host += u.batches_host; st.unpack_anchors += u.anchors;
            st.unpack_batches_kept_on_device += u.batches_kept_on_device;
            st.unpack_batches_appended_host += u.batches_appended_host;
        }
        std::swap(cur, ahead);
        if (i + 1 < chrs.size()) launch(i + 1);
        seq = SeqStore();
        seq.seq_off = cur.seq_off.data();
        seq.seq = cur.seq.data();
        out = ChromosomeInput();
        out.name = cur.name;
        out.reads = cur.view();
        uint64_t n_cigar = cur.cigar.size();
        if (cur.resident) {
            // the contig is a resident shard: the run takes it; the host has the small per-record arrays only
            n_cigar = cur.resident_cigar;
            out.resident = cur.resident.release();
            out.reads.cigar_off = nullptr; out.reads.cigar = nullptr; out.reads.n_cigar = n_cigar;
            seq.seq_off = nullptr; seq.seq = nullptr; seq.resident = out.resident;
            st.contigs_resident++;
        }
        out.seq = opt.want_seq ? &seq : nullptr;
        out.depth_len = cur.target_len + 1;                       // cnv_caller.cpp:482
        out.qnames = opt.want_qnames ? &cur.qnames : nullptr;
        if (snp_file) out.snps = &snp_file->table(cur.name, af_files ? af_files->get(cur.name) : std::string(), ethnicity, opt.threads, snp_dev.ctx ? &snp_dev : nullptr);
        st.n_contigs++; st.n_reads += cur.n_reads(); st.n_cigar += n_cigar;
        i++;
        return true;
    }
    ~BamSource() override { if (pending.valid()) pending.wait(); }
};
}  // namespace

void SVCaller::runBam(const std::string &bam_path, const std::vector<std::string> &chromosomes, int threads, const CHMM &hmm, const RunParams &P,
                      std::unordered_map<std::string, std::vector<SVCall>> &whole_genome_sv_calls, BamRunStats *bam_stats)
{
    const double t0 = now_ms();
    // With RunParams::inflate_on_device the reader inflates one contig ahead on a thread of its own, beside this run on the device: its context is
    // its own (two threads must not share one), on the same device, for the length of the run — declared in front of the source, so that it
    // outlives a read that is still in flight when the source goes.
    struct OwnCtx { csv_ctx *c = nullptr; ~OwnCtx() { if (c) csvgpu_destroy(c); } } inflate_ctx, snp_ctx;
    // (snp_file in front of the source and behind its context: the source's tables point into it, and its resident tables are freed on snp_ctx)
    SNPFile snp_file;
    BamSource src;
    if (!src.reader.open(bam_path)) throw std::runtime_error("ERROR failed to open BAM file " + bam_path + ": " + src.reader.error());
    if (!src.reader.loadIndex()) throw std::runtime_error("ERROR failed to load index for " + bam_path);
    src.chrs = chromosomes.empty() ? src.reader.header().names : chromosomes;      // sv_caller.cpp:766-774
    for (const std::string &chr : src.chrs) {
        if (src.reader.header().tid(chr) < 0) throw std::runtime_error("ERROR: Could not find chromosome " + chr + " in BAM file.");
        if (P.ref_genome && P.ref_genome->getChromosomeLength(chr) == 0) {        // :795-800: the reference gives up on the whole run
            printError("Chromosome " + chr + " not found in reference genome");
            return;
        }
    }
    src.opt.threads = std::max(1, threads);
    if (P.inflate_on_device || P.unpack_on_device || P.shard_on_device) {
        inflate_ctx.c = csvgpu_create(P.inflate_device, nullptr);
        if (!inflate_ctx.c) throw std::runtime_error(std::string("ERROR: no device context for the BAM reader: ") + csvgpu_last_error(nullptr));
        if (P.inflate_on_device) src.opt.device_inflate = inflate_ctx.c;
        if (P.unpack_on_device || P.shard_on_device) src.opt.device_unpack = inflate_ctx.c;         // (one context for both: the reader's thread is its only user)
        src.opt.device_shard = P.shard_on_device;
    }
    AlleleFreqFiles af_files;
    if (!P.snp_vcf.empty()) {
        std::string e;
        if (!af_files.load(P.pfb_table, &e)) throw std::runtime_error(e);          // the reference exits (input_data.cpp:221-225, :278-283)
        if (snp_parse_on_device || snp_tables_on_device) {
            // a context of the file's own on the run's device, for the length of the run: load() and every table() of the source use it from
            // the thread that feeds the run, never beside a lane's
            snp_ctx.c = csvgpu_create(P.inflate_device, nullptr);
            if (!snp_ctx.c) throw std::runtime_error(std::string("ERROR: no device context for the SNP reader: ") + csvgpu_last_error(nullptr));
            src.snp_dev.ctx = snp_ctx.c; src.snp_dev.tables_on_device = snp_tables_on_device;
        }
        if (snp_file.load(P.snp_vcf, src.opt.threads, &e, src.snp_dev.ctx ? &src.snp_dev : nullptr)) {
            src.snp_file = &snp_file; src.af_files = &af_files; src.ethnicity = P.ethnicity;
        } else {
            printError(e);                                                         // as there: every region then has no SNPs (cnv_caller.cpp:586-591)
        }
    }
    src.opt.want_seq = true;                                      // 50-bp insertion ALT strings (sv_caller.cpp:589-600)
    src.opt.want_qnames = P.split_svs;
    run(src, hmm, P, whole_genome_sv_calls);
    if (bam_stats) {
        *bam_stats = src.st;
        bam_stats->bam_bytes = src.reader.bytes();
        bam_stats->ms_total = now_ms() - t0;
    }
}
