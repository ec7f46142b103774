// vcf_format_core_check.cpp — the per-record rule of the device's VCF formatter (contextsv_amd/csrc/vcf_format_core.hpp) against the host
// writer (host/vcf_writer.cpp: writeVCF over a HostDepthSource and a host-backed ReferenceGenome), on the CPU under AddressSanitizer +
// UBSan. A program of its own: `make -C contextsv_amd/csrc vcf-format-check` links it with host/vcf_writer.cpp and host/fasta_query.cpp;
// tests/test_vcf_format_core.py runs it.
//   vcf_format_core_check <generated doubles> <batches> <seed>
// Checked:
//   (a) fmt_f6 against snprintf("%f"): directed values (ties, the carry, -0.0, denormals, inf, nan by sign, the 2^63 edge), uniform bit
//       patterns, and k / 2^s for s = 1..30 around the ties of the sixth decimal. Every value is equal or refused by f6_refused.
//   (b) dec_digits_u32 / dec_chars_i32 at every power of ten, one below and one above, INT_MIN + 1, -1, 0.
//   (c) whole lines: generated call sets (the kind tests/test_vcf_writer.py draws, plus starts at 0, 1, 2, L - 1, L, L + 1, 2^31 - 1, 2^31,
//       2^31 + 1, 2^32 - 1, end < start, every cn_state, every evidence mask, gap rows that touch, contain and miss a call) assembled by the
//       core into a heap block of EXACTLY the computed length, against writeVCF's text behind its header, with the three counts. A batch
//       the rule refuses is not compared; where the host throws for it (an enum outside its table, a contig the genome has not) it must.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "../../contextsv_amd/csrc/host/vcf_writer.h"
#include "../../contextsv_amd/csrc/vcf_format_core.hpp"

// the C-ABI calls of the two host files' opt-in device routes; this program never takes them
extern "C" {
csv_genome_builder *csvgpu_genome_builder_create(csv_ctx *, uint64_t) { abort(); }
int csvgpu_genome_builder_append(csv_ctx *, csv_genome_builder *, const uint8_t *, uint64_t) { abort(); }
csv_genome *csvgpu_genome_builder_finish(csv_ctx *, csv_genome_builder *) { abort(); }
void csvgpu_genome_builder_destroy(csv_ctx *, csv_genome_builder *) { abort(); }
void csvgpu_genome_free(csv_ctx *, csv_genome *) { abort(); }
int csvgpu_genome_describe(csv_ctx *, const csv_genome *, uint64_t, uint64_t, uint64_t *, char *, uint32_t *, csv_genome_counts *) { abort(); }
int csvgpu_genome_fetch(csv_ctx *, const csv_genome *, const uint32_t *, const uint32_t *, const uint32_t *, const uint64_t *, uint64_t, int, char *) { abort(); }
int csvgpu_depth_lookup_resident(csv_ctx *, csv_shard *, const uint32_t *, uint64_t, int32_t *) { abort(); }
int csvgpu_vcf_format(csv_ctx *, const csv_genome *, const csv_vcf_contig *, uint32_t, const uint64_t *, const csv_vcf_call *, const uint64_t *, const char *, const char *,
                      uint32_t, uint64_t, char *, uint8_t *, csv_vcf_format_counts *) { abort(); }
const char *csvgpu_last_error(const csv_ctx *) { abort(); }
}

void printError(const std::string &m) { (void)m; }
void printMessage(const std::string &m) { (void)m; }

using namespace vcffmt;

namespace {

long g_fail = 0;
void fail(const char *what, long a, long b)
{
    if (g_fail++ < 20) fprintf(stderr, "FAIL %s (%ld, %ld)\n", what, a, b);
}

// ---- (a)
long g_doubles = 0, g_refused = 0;
void check_f6(double x)
{
    g_doubles++;
    if (f6_refused(x)) { g_refused++; return; }
    char want[64];
    const int n = snprintf(want, sizeof want, "%f", x);
    CountSink cs;
    fmt_f6(cs, x);
    std::unique_ptr<uint8_t[]> got(new uint8_t[cs.at]);   // exactly the counted bytes
    WindowSink ws{got.get(), 0, 0, cs.at};
    fmt_f6(ws, x);
    if ((uint64_t)n != cs.at || ws.at != cs.at || memcmp(want, got.get(), (size_t)n) != 0) {
        uint64_t b;
        memcpy(&b, &x, 8);
        fail("fmt_f6", (long)(b >> 32), (long)(b & 0xffffffff));
    }
}
double from_bits(uint64_t b) { double x; memcpy(&x, &b, 8); return x; }

void check_doubles(long n_random, std::mt19937_64 &rng)
{
    const double directed[] = {0.0, -0.0, 1.0 / 128, 3.0 / 128, 0.9999995, 0.99999949999999, 0.9999994, 1.9999995, 999999.9999995, -0.9999995, 0.5, 0.0000005, 0.00000049,
                               0.0000015, 0.0000025, 4.76837158203125e-07, 4.7683715820312494e-07, 1e-300, -1e-300, 5e-324, -5e-324, 2.2250738585072014e-308,
                               -2533.541937, -12.5, 123456789.123456789, 9007199254740992.0, 9007199254740993.0, 4503599627370495.5, 4503599627370496.5,
                               9223372036854774784.0, -9223372036854774784.0, 9223372036854775808.0, -9223372036854775808.0, 1e19, 1e300, -1e300, 1e-7, -1e-7,
                               2251799813685247.75, 1125899906842623.875, 0.1, 0.2, 0.3, 1e15 + 0.3, 123456.7890125, 0.0078125, 0.0234375};
    for (double x : directed) check_f6(x);
    check_f6(from_bits(0x7ff0000000000000ull)); check_f6(from_bits(0xfff0000000000000ull));                       // inf, -inf
    check_f6(from_bits(0x7ff8000000000000ull)); check_f6(from_bits(0xfff8000000000000ull));                       // nan, -nan
    check_f6(from_bits(0x7ff0000000000001ull)); check_f6(from_bits(0xfff0000000000001ull));                       // signalling
    check_f6(from_bits(0x000fffffffffffffull)); check_f6(from_bits(0x8000000000000001ull));                       // denormals
    for (int e = -30; e <= 64; e++)                                                                                // every binade's edges near the rule's
        for (int d = -1; d <= 1; d++) { check_f6(from_bits(((uint64_t)(1023 + e) << 52) + (uint64_t)d)); check_f6(-from_bits(((uint64_t)(1023 + e) << 52) + (uint64_t)d)); }
    for (long i = 0; i < n_random; i++) {
        uint64_t b = rng();
        // uniform bit patterns below 2^63 in magnitude; half of them where the digits are
        b = (b & ~(0x7ffull << 52)) | ((uint64_t)(i & 1 ? 1023 - 24 + rng() % 87 : rng() % (1023 + 63)) << 52);
        check_f6(from_bits(b));
    }
    // k / 2^s near the ties of the sixth decimal: the nearest k to (j + 1/2) * 1e-6 * 2^s and its neighbours
    for (int s = 1; s <= 30; s++)
        for (int r = 0; r < 4000; r++) {
            const uint64_t j = rng() % 4000000;
            const double t = ((double)j + 0.5) * 1e-6 * (double)(1ull << s);
            const int64_t k = (int64_t)t;
            for (int64_t d = -1; d <= 2; d++) { check_f6((double)(k + d) / (double)(1ull << s)); check_f6(-(double)(k + d) / (double)(1ull << s)); }
        }
}

// ---- (b)
void check_digits()
{
    std::vector<uint32_t> u = {0, 1, 9, UINT_MAX, UINT_MAX - 1, (uint32_t)INT_MAX, (uint32_t)INT_MAX + 1};
    for (uint64_t p = 10; p <= UINT_MAX; p *= 10) { u.push_back((uint32_t)p - 1); u.push_back((uint32_t)p); u.push_back((uint32_t)p + 1); }
    for (uint32_t v : u) {
        char t[16];
        if (dec_digits_u32(v) != (uint32_t)snprintf(t, sizeof t, "%u", v)) fail("dec_digits_u32", (long)v, 0);
    }
    std::vector<int32_t> s = {0, -1, 1, INT_MIN + 1, INT_MIN, INT_MAX, -9, -10, 9, 10};
    for (int64_t p = 10; p <= INT_MAX; p *= 10)
        for (int d = -1; d <= 1; d++) { s.push_back((int32_t)(p + d)); s.push_back((int32_t)-(p + d)); }
    for (int32_t v : s) {
        char t[16];
        const int n = snprintf(t, sizeof t, "%d", v);
        if (dec_chars_i32(v) != (uint32_t)n) fail("dec_chars_i32", (long)v, 0);
        CountSink cs;
        put_i32(cs, v);
        uint8_t got[16];
        WindowSink ws{got, 0, 0, 16};
        put_i32(ws, v);
        if (cs.at != (uint64_t)n || memcmp(got, t, (size_t)n) != 0) fail("put_i32", (long)v, 0);
    }
}

// ---- (c)
struct Contig {
    std::string name, seq;                                // seq empty + in_genome false: the genome has no such contig
    bool in_genome = true;
    std::vector<SVCall> calls;
    std::vector<std::pair<uint32_t, uint32_t>> gaps;
    std::vector<uint32_t> depth;
};

std::string random_seq(std::mt19937_64 &rng, size_t n)
{
    static const char pool[] = "ACGTACGTACGTACGTACGTacgtacgtNnRYKMSWBDHVrykmswbdhv";
    std::string s(n, 'A');
    for (char &c : s) c = pool[rng() % (sizeof pool - 1)];
    return s;
}

SVCall random_call(std::mt19937_64 &rng, uint32_t L)
{
    static const int types[] = {-1, 0, 0, 0, 1, 2, 3, 3, 3, 4, 5, 6};
    SVCall c;
    const int t = types[rng() % 12];
    c.sv_type = (SVType)t;
    c.start = (uint32_t)(rng() % (L + 5));
    c.end = c.start + (rng() % 10 < 3 ? 0 : (uint32_t)(rng() % 120));
    c.cluster_size = (int)(rng() % 50);
    static const double scale[] = {1, 10, 100, 1e3, 1e4, 1e5};
    c.hmm_likelihood = rng() % 10 < 3 ? 0.0 : -(double)(rng() % 1000000007) / 1000000007.0 * scale[rng() % 6];
    c.aln_type = SVEvidenceFlags(rng() % 1024);
    c.genotype = (Genotype)(rng() % 4);
    c.cn_state = (int)(rng() % 7);
    c.aln_offset = (int)(rng() % 600) - 300;
    if (t == 3) c.alt_allele = rng() % 10 < 4 ? "<INS>" : random_seq(rng, 1 + rng() % 60);
    else c.alt_allele = t == 0 ? "<DEL>" : t == 1 ? "<DUP>" : t == 2 ? "<INV>" : t == 4 ? "<BND>" : ".";
    return c;
}

long g_batches = 0, g_lines = 0, g_declined = 0, g_threw = 0, g_calls = 0;

Call to_core(const SVCall &s)
{
    Call c;
    c.start = s.start; c.end = s.end; c.sv_type = (int32_t)s.sv_type; c.cluster_size = s.cluster_size; c.hmm_likelihood = s.hmm_likelihood; c.id = -1;
    c.aln_flags = (uint32_t)s.aln_type.to_ulong(); c.genotype = (int32_t)s.genotype; c.cn_state = s.cn_state; c.aln_offset = s.aln_offset;
    return c;
}

void check_batch(const std::vector<Contig> &contigs)
{
    g_batches++;
    const std::string method = svMethodString();
    // the core: decide every call, then assemble a block of exactly the summed length
    struct Item { Call c; Line L; const Contig *ct; const SVCall *sv; uint64_t len; };
    std::vector<Item> items;
    uint32_t why = 0;
    VCFCounts want_counts;
    uint64_t total = 0;
    for (const Contig &ct : contigs) {
        std::vector<uint32_t> gs, ge;
        for (const auto &g : ct.gaps) { gs.push_back(g.first); ge.push_back(g.second); }
        for (const SVCall &sv : ct.calls) {
            g_calls++;
            Item it{to_core(sv), Line(), &ct, &sv, 0};
            it.L = decide(it.c, ct.in_genome ? (int64_t)ct.seq.size() : -1, gs.data(), ge.data(), (uint32_t)gs.size(), (const uint8_t *)sv.alt_allele.data(), sv.alt_allele.size());
            if (it.L.why) { if (!why) why = it.L.why; continue; }
            const uint8_t disp = it.L.status & DISPOSITION;
            if (disp == SKIP_UNCLASSIFIED) want_counts.unclassified++; else want_counts.total++;
            if (it.L.gap_hit) want_counts.assembly_gap_filtered++;
            if (disp == WRITTEN) {
                set_depth(it.L, it.L.pos < ct.depth.size() ? (int32_t)ct.depth[it.L.pos] : -1);
                Layout lay;
                it.len = line_length(it.c, it.L, (uint32_t)ct.name.size(), sv.alt_allele.size(), (uint32_t)method.size(), &lay);
                if (lay.len != it.len || !(lay.pos < lay.ref && lay.ref < lay.alt && lay.alt < lay.filter && lay.filter < lay.info && lay.info < lay.format && lay.format < lay.len))
                    fail("layout order", (long)items.size(), (long)it.len);
                if (lay.ref != ref_offset(it.L, (uint32_t)ct.name.size()) || !asks_depth(it.c)) fail("ref_offset / asks_depth", (long)items.size(), (long)lay.ref);
                if (it.len > ct.name.size() + it.L.ref_len + sv.alt_allele.size() + method.size() + kShortMax) fail("kShortMax", (long)items.size(), (long)it.len);
                total += it.len;
            }
            items.push_back(it);
        }
    }
    ReferenceGenome genome;
    std::unordered_map<std::string, std::vector<uint32_t>> depth;
    std::unordered_map<std::string, std::vector<std::pair<uint32_t, uint32_t>>> gaps;
    std::vector<std::pair<std::string, const std::vector<SVCall> *>> order;
    for (const Contig &ct : contigs) {
        if (ct.in_genome) genome.addContig(ct.name, ct.seq);
        depth[ct.name] = ct.depth;
        if (!ct.gaps.empty()) gaps[ct.name] = ct.gaps;
        order.emplace_back(ct.name, &ct.calls);
    }
    VCFOptions opt;
    opt.file_date = "20250926";
    if (why) {
        g_declined++;
        if (why == WHY_ENUM || why == WHY_NO_RECORD) {                          // the host throws for these; the others it cannot run defined
            bool threw = false;
            std::ostringstream out;
            try { (void)writeVCF(out, order, opt, gaps, genome, HostDepthSource(depth)); } catch (const std::exception &) { threw = true; }
            if (!threw) fail("declined, but the host wrote it", (long)why, 0); else g_threw++;
        }
        return;
    }
    std::unique_ptr<uint8_t[]> block(new uint8_t[total]);
    uint64_t at = 0;
    for (const Item &it : items) {
        if ((it.L.status & DISPOSITION) != WRITTEN) continue;
        WindowSink ws{block.get(), at, at, at + it.len};
        const uint8_t *ref = it.L.ref_kind == REF_GENOME ? (const uint8_t *)it.ct->seq.data() + it.L.ref_first : nullptr;
        emit_line(ws, it.c, it.L, (const uint8_t *)it.ct->name.data(), (uint32_t)it.ct->name.size(), ref, (const uint8_t *)it.sv->alt_allele.data(), it.sv->alt_allele.size(),
                  (const uint8_t *)method.data(), (uint32_t)method.size());
        if (ws.at != at + it.len) fail("emitted length", (long)ws.at, (long)(at + it.len));
        at += it.len;
        g_lines++;
    }
    std::ostringstream out;
    const VCFCounts got = writeVCF(out, order, opt, gaps, genome, HostDepthSource(depth));
    const std::string text = out.str();
    static const char last_header[] = "FORMAT\tSAMPLE\n";
    const size_t body = text.find(last_header) + sizeof last_header - 1;
    if (text.size() - body != total || memcmp(text.data() + body, block.get(), (size_t)total) != 0) {
        size_t k = 0;
        while (k < total && body + k < text.size() && text[body + k] == (char)block[k]) k++;
        fail("text", (long)g_batches, (long)k);
    }
    if (got.total != want_counts.total || got.unclassified != want_counts.unclassified || got.assembly_gap_filtered != want_counts.assembly_gap_filtered)
        fail("counts", (long)got.total, (long)want_counts.total);
}

Contig make_contig(std::mt19937_64 &rng, int k, bool with_gaps)
{
    Contig ct;
    static const char *names[] = {"c", "chr2", "chrA", "chr10_random", "chrUn_KI270742v1", "chrB"};
    ct.name = names[k % 6];
    ct.seq = random_seq(rng, 300 + rng() % 600);
    const uint32_t L = (uint32_t)ct.seq.size();
    ct.depth.resize(k % 3 == 2 ? L / 2 : L + 1);
    for (uint32_t &d : ct.depth) d = (uint32_t)(rng() % 5 == 0 ? rng() % 3000000000u : rng() % 90);
    if (with_gaps)
        for (int g = 0; g < 6; g++) { const uint32_t a = (uint32_t)(rng() % L); ct.gaps.emplace_back(a, a + 1 + (uint32_t)(rng() % 200)); }
    return ct;
}

void check_lines(long n_batches, std::mt19937_64 &rng)
{
    // generated sets
    for (long b = 0; b < n_batches; b++) {
        std::vector<Contig> cs;
        const int nc = 1 + (int)(rng() % 4);
        for (int k = 0; k < nc; k++) {
            Contig ct = make_contig(rng, (int)(b + k), b % 2 == 1);
            const int n = (int)(rng() % 80);
            for (int i = 0; i < n; i++) ct.calls.push_back(random_call(rng, (uint32_t)ct.seq.size()));
            cs.push_back(std::move(ct));
        }
        if (b % 7 == 3) { Contig e; e.name = "chrEmpty"; e.in_genome = false; cs.push_back(e); }      // no calls, no genome record, no depth
        check_batch(cs);
    }
    // directed starts and ends, per type, each a batch of its own among generated calls (so that a refusal hides nothing else)
    for (int type = 0; type <= 6; type++) {
        if (type == 5) continue;
        Contig base = make_contig(rng, type, true);
        const uint32_t L = (uint32_t)base.seq.size();
        const uint32_t starts[] = {0, 1, 2, 3, L - 1, L, L + 1, L + 2, 0x7fffffffu, 0x80000000u, 0x80000001u, 0xfffffffeu, 0xffffffffu};
        for (uint32_t st : starts)
            for (int64_t de : {-3, -2, -1, 0, 1, 5, 100, 1000, 0x7ffffffe, 0x7fffffff}) {
                Contig ct = base;
                for (int i = 0; i < 5; i++) { SVCall c = random_call(rng, L); if (c.sv_type == SVType::DEL && c.start > L) c.start = L; ct.calls.push_back(c); }
                SVCall c = random_call(rng, L);
                c.sv_type = (SVType)type; c.start = st; c.end = (uint32_t)(st + de);
                if (type == 3) c.alt_allele = de % 2 ? "<INS>" : "acgtn";
                ct.calls.insert(ct.calls.begin() + 2, c);
                check_batch({ct});
            }
    }
    // every cn_state, genotype and type; every evidence mask
    {
        Contig ct = make_contig(rng, 1, false);
        for (int t = -1; t <= 6; t++) for (int g = 0; g < 4; g++) for (int cn = 0; cn < 7; cn++) {
            SVCall c = random_call(rng, (uint32_t)ct.seq.size());
            c.sv_type = (SVType)t; c.genotype = (Genotype)g; c.cn_state = cn;
            if (c.start < 2) c.start = 2;
            ct.calls.push_back(c);
        }
        for (int m = 0; m < 1024; m++) { SVCall c = random_call(rng, (uint32_t)ct.seq.size()); c.aln_type = SVEvidenceFlags((unsigned long long)m); ct.calls.push_back(c); }
        check_batch({ct});
    }
    // enums outside their tables, a contig the genome has not (with and without a call that asks for REF), refused likelihoods
    for (int k = 0; k < 10; k++) {
        Contig ct = make_contig(rng, k, false);
        for (int i = 0; i < 10; i++) ct.calls.push_back(random_call(rng, (uint32_t)ct.seq.size()));
        SVCall &c = ct.calls[5];
        switch (k) {
        case 0: c.sv_type = (SVType)7; break;
        case 1: c.sv_type = (SVType)-2; break;
        case 2: c.genotype = (Genotype)4; break;
        case 3: c.genotype = (Genotype)-1; c.sv_type = SVType::UNKNOWN; break;      // looked up in front of the skip
        case 4: c.cn_state = 7; break;
        case 5: c.cn_state = -1; c.sv_type = SVType::NEUTRAL; break;
        case 6: ct.in_genome = false; c.sv_type = SVType::DEL; c.start = 10; c.end = 20; break;
        case 7: ct.in_genome = false; for (SVCall &x : ct.calls) if (x.sv_type == SVType::DEL || x.sv_type == SVType::INS) x.sv_type = SVType::DUP; break;   // written
        case 8: c.sv_type = SVType::DUP; c.hmm_likelihood = 9223372036854775808.0; break;
        case 9: c.sv_type = SVType::UNKNOWN; c.hmm_likelihood = -1e300; break;       // never printed: written
        }
        const long before = g_declined;
        check_batch({ct});
        if ((g_declined != before) != (k != 7 && k != 9)) fail("directed refusal", k, 0);
    }
    // the likelihoods of (a) in whole lines
    {
        Contig ct = make_contig(rng, 2, false);
        for (double x : {1.0 / 128, 3.0 / 128, 0.9999995, -0.0, 5e-324, 9223372036854774784.0, -123456.7890125}) {
            SVCall c = random_call(rng, (uint32_t)ct.seq.size());
            c.sv_type = SVType::DUP; c.hmm_likelihood = x;
            ct.calls.push_back(c);
        }
        {                                                 // every short field at its longest
            SVCall c = random_call(rng, 10);
            c.sv_type = SVType::NEUTRAL; c.sv_type = SVType::LOH; c.start = 0; c.end = 0x80000000u; c.aln_type = SVEvidenceFlags(1023ull); c.cluster_size = INT_MIN + 1;
            c.aln_offset = INT_MIN; c.hmm_likelihood = -9223372036854774784.0; c.cn_state = 4; c.genotype = Genotype::UNKNOWN;
            ct.depth[0] = 4294967295u;
            ct.gaps = {{0, 0x7fffffffu}};
            ct.calls.push_back(c);
        }
        for (uint64_t b : {0x7ff0000000000000ull, 0xfff0000000000000ull, 0x7ff8000000000000ull, 0xfff8000000000000ull}) {
            SVCall c = random_call(rng, (uint32_t)ct.seq.size());
            c.sv_type = SVType::INV; c.hmm_likelihood = from_bits(b);
            ct.calls.push_back(c);
        }
        check_batch({ct});
    }
    // gap rows that touch, contain and miss a call; exactly 20 % and one base more; two matching rows
    {
        Contig ct = make_contig(rng, 3, false);
        auto add = [&](uint32_t s, uint32_t e, int type) { SVCall c = random_call(rng, 200); c.sv_type = (SVType)type; c.start = s; c.end = e; if (type == 3) c.alt_allele = "<INS>"; ct.calls.push_back(c); };
        ct.gaps = {{99, 119}, {150, 150}, {400, 500}, {104, 110}, {0xfffffffeu, 0xffffffffu}, {0xffffffffu, 5}};
        for (int type : {0, 1, 3}) {
            add(100, 199, type);                          // [100, 120] of 100 bases: 21 %
            add(101, 200, type);                          // 20 bases: exactly 20 %
            add(121, 220, type); add(120, 219, type); add(151, 151, type); add(152, 160, type); add(390, 510, type); add(1, 1, type); add(0, 0, type); add(5, 4, type); add(500, 100, type);
            add(0xffffffffu, 0xffffffffu, type); add(0, 0xffffffffu, type);
        }
        std::vector<SVCall> all = ct.calls;
        ct.calls.clear();
        for (const SVCall &c : all) { ct.calls.push_back(c); }
        // (a DEL over the whole uint32 range is refused: one batch per call keeps the others compared)
        for (const SVCall &c : all) { Contig one = ct; one.calls = {c}; check_batch({one}); }
    }
}

}  // namespace

int main(int argc, char **argv)
{
    const long n_doubles = argc > 1 ? atol(argv[1]) : 10000000, n_batches = argc > 2 ? atol(argv[2]) : 300;
    std::mt19937_64 rng(argc > 3 ? (uint64_t)atoll(argv[3]) : 7);
    std::cerr.rdbuf(nullptr);                             // the writer's warnings are not what this program reports (failures go to stderr through stdio)
    check_doubles(n_doubles, rng);
    check_digits();
    check_lines(n_batches, rng);
    printf("vcf_format_core_check: %ld doubles (%ld refused), %ld batches, %ld calls, %ld lines, %ld declined (%ld thrown by the host), %ld failures\n", g_doubles, g_refused,
           g_batches, g_calls, g_lines, g_declined, g_threw, g_fail);
    return g_fail ? 1 : 0;
}
