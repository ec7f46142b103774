// vcf_record_core_check.cpp — the per-line decisions of the device VCF parser (contextsv_amd/csrc/vcf_record_core.hpp) against the host
// reader's two functions (host/snp_io.cpp: snp_record_of_line, af_record_of_line), on the CPU under AddressSanitizer + UBSan. A program of
// its own: `make -C contextsv_amd/csrc vcf-check` links it with host/snp_io.cpp and the BGZF reader that file needs; tests/test_vcf_record_core.py
// writes the corpus and runs it.
//   vcf_record_core_check <corpus> <mutations per text> <seed>
// corpus: "VCFC", u32 texts, then per text: u32 kind (0 SNP, 1 AF), u32 len, bytes; AF: u32 contig_len, bytes, u32 needle_len, bytes,
// u32 n, u32 sorted_pos[n]. Every text and every byte-mutated copy of it lies in a heap block of exactly its size; every line of it goes
// through both. KEEP / SKIP / STOP must agree with the host field for field; DEFER must be one the rule allows: a second sample column, or
// a number outside the integer / real rule at the first check that cannot be decided without it (restated here in the host's order), and
// exactly then.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <string_view>
#include <vector>

#include "../../contextsv_amd/csrc/host/snp_io.h"
#include "../../contextsv_amd/csrc/vcf_record_core.hpp"
#include "../../include/csvgpu.h"

// host/snp_io.cpp's opt-in device path calls these; this program never takes it
extern "C" {
int csvgpu_vcf_snp_parse(csv_ctx *, const uint8_t *, uint64_t, int, int, const csv_vcf_out *, csv_vcf_counts *) { abort(); }
int csvgpu_vcf_af_parse(csv_ctx *, const uint8_t *, uint64_t, const char *, uint32_t, const char *, uint32_t, const uint32_t *, uint64_t, const csv_vcf_out *,
                        csv_vcf_counts *) { abort(); }
const char *csvgpu_last_error(const csv_ctx *) { abort(); }
// ... and its tables_on_device path these (csvgpu_snp_builder_* / csvgpu_snp_columns_*); never taken here either
csv_snp_builder *csvgpu_snp_builder_create(csv_ctx *, uint64_t) { abort(); }
int csvgpu_snp_builder_append(csv_ctx *, csv_snp_builder *, const uint8_t *, uint64_t, uint64_t, int, int, const csv_snp_runs *, csv_snp_append_counts *) { abort(); }
int csvgpu_snp_builder_append_host(csv_ctx *, csv_snp_builder *, uint64_t, const uint32_t *, const uint64_t *, const uint32_t *, const double *) { abort(); }
csv_snp_columns *csvgpu_snp_builder_finish(csv_ctx *, csv_snp_builder *, const uint32_t *, uint64_t) { abort(); }
void csvgpu_snp_builder_destroy(csv_ctx *, csv_snp_builder *) { abort(); }
int csvgpu_snp_columns_describe(const csv_snp_columns *, uint64_t, uint32_t *, uint64_t *, uint8_t *, uint64_t *) { abort(); }
int csvgpu_snp_columns_fetch(csv_ctx *, const csv_snp_columns *, uint32_t, uint32_t *, double *) { abort(); }
int csvgpu_snp_columns_af_parse(csv_ctx *, const csv_snp_columns *, uint32_t, const uint8_t *, uint64_t, const char *, uint32_t, const char *, uint32_t,
                                const csv_vcf_out *, csv_vcf_counts *) { abort(); }
csv_snp_table *csvgpu_snp_columns_table(csv_ctx *, const csv_snp_columns *, uint32_t, const uint32_t *, const double *, uint64_t) { abort(); }
void csvgpu_snp_columns_free(csv_ctx *, csv_snp_columns *) { abort(); }
void csvgpu_snp_table_free(csv_ctx *, csv_snp_table *) { abort(); }
}

// SNPFileTable's base class keeps this one function (and with it its vtable) in host/cnv_caller.cpp, which is not linked; no table is queried here
void SNPSource::queryFlat(uint32_t, uint32_t, std::vector<uint32_t> &, std::vector<double> &, std::vector<double> &) const { abort(); }

void printError(const std::string &m) { fprintf(stderr, "%s\n", m.c_str()); }     // (the mirror's logger is not linked either)

using sv = std::string_view;
using namespace vcfcore;

namespace {

struct Text {
    uint32_t kind = 0;
    std::vector<uint8_t> bytes;
    std::string contig, needle;
    std::vector<uint32_t> sorted;
};

long g_kept = 0, g_skipped = 0, g_deferred = 0, g_fail = 0;

void fail(const char *what, sv line)
{
    if (g_fail++ < 20) fprintf(stderr, "FAIL %s: %.*s\n", what, (int)std::min<size_t>(line.size(), 300), line.data());
}

bool same(double a, double b) { return (std::isnan(a) && std::isnan(b)) || memcmp(&a, &b, 8) == 0; }

std::vector<sv> split(sv s, char c)
{
    std::vector<sv> out;
    size_t a = 0;
    for (;;) {
        const size_t e = s.find(c, a);
        out.push_back(s.substr(a, e == sv::npos ? sv::npos : e - a));
        if (e == sv::npos) return out;
        a = e + 1;
    }
}
bool int_ok(sv t) { int64_t v; return tok_int((const uint8_t *)t.data(), (uint32_t)t.size(), v); }
bool real_ok(sv t) { double v; return tok_real((const uint8_t *)t.data(), (uint32_t)t.size(), v); }

// The defer rule restated on string views, in the host's order of checks: a line is deferred exactly when the FIRST check that cannot be
// decided without a conversion outside the integer / real rule (or with a second sample column in reach) comes before any check that
// skips the line. Nothing of the core's control flow is reused: only its two token rules.
bool allele_ok(sv a) { return (a.size() == 1 && a[0] != '*') || a == "<X>" || a == "<*>"; }
bool snp_alleles(sv ref, sv alt)
{
    if (!allele_ok(ref)) return false;
    if (alt == ".") return true;
    for (sv a : split(alt, ',')) if (!allele_ok(a)) return false;
    return true;
}
int first_key(const std::vector<sv> &keys, sv key) { for (size_t k = 0; k < keys.size(); k++) if (keys[k] == key) return (int)k; return -1; }
// one integer FORMAT value: 0 outside the rule, 1 missing, 2 a number (v)
int fmt_int(sv t, int64_t &v) { if (t.empty() || t == ".") return 1; return tok_int((const uint8_t *)t.data(), (uint32_t)t.size(), v) ? 2 : 0; }

bool snp_must_defer(sv line, bool dp_int, bool ad_int)
{
    const std::vector<sv> f = split(line, '\t');
    if (f.size() < 9 || !snp_alleles(f[3], f[4]) || f[5] == ".") return false;
    double q;
    if (!tok_real((const uint8_t *)f[5].data(), (uint32_t)f[5].size(), q)) return true;
    if ((float)q <= 30 || !dp_int) return false;
    const std::vector<sv> keys = split(f[8], ':'), vals = split(f.size() > 9 ? f[9] : sv(), ':');
    const int dp = first_key(keys, "DP");
    if (dp < 0) return false;
    if (f.size() > 10) return true;
    int64_t v = 0;
    const int kind = fmt_int(split((size_t)dp < vals.size() ? vals[dp] : sv(), ',')[0], v);
    if (kind == 0) return true;
    if (kind == 1 || v <= 10) return false;
    if (f[6] != "." && f[6] != "PASS") {
        bool pass = false;
        for (sv x : split(f[6], ';')) pass |= x == "PASS";
        if (!pass) return false;
    }
    const int ad = first_key(keys, "AD");
    if (!ad_int || ad < 0) return false;
    const std::vector<sv> t = split((size_t)ad < vals.size() ? vals[ad] : sv(), ',');
    if (t.size() < 2) return false;
    if (fmt_int(t[0], v) == 0 || fmt_int(t[1], v) == 0) return true;
    return !int_ok(f[1]);
}

bool af_must_defer(sv line, const Text &t, uint32_t last)
{
    const std::vector<sv> f = split(line, '\t');
    if (f.size() < 8 || f[0] != sv(t.contig)) return false;
    int64_t v;
    if (!tok_int((const uint8_t *)f[1].data(), (uint32_t)f[1].size(), v)) return true;
    const uint32_t pos = (uint32_t)v;
    if (pos > last || !std::binary_search(t.sorted.begin(), t.sorted.end(), pos) || !snp_alleles(f[3], f[4])) return false;
    const sv info = f[7], needle = t.needle;
    size_t k = info.find(needle);
    while (k != sv::npos && k != 0 && info[k - 1] != ';') k = info.find(needle, k + 1);
    if (k == sv::npos) return false;
    const size_t a = k + needle.size(), e = info.find_first_of(";,", a);
    const sv val = info.substr(a, e == sv::npos ? sv::npos : e - a);
    return !val.empty() && val != "." && !real_ok(val);
}

void check_line(const Text &t, const uint8_t *p, uint32_t len, bool dp_int, bool ad_int)
{
    const sv line((const char *)p, len);
    Rec r;
    if (t.kind == 0) {
        const int c = vcf_snp_line(p, len, dp_int, ad_int, r);
        if ((c == VCF_DEFER) != snp_must_defer(line, dp_int, ad_int)) fail(c == VCF_DEFER ? "DEFER outside the rule" : "a line the rule defers was decided", line);
        SnpLineRecord h;
        const bool kept = snp_record_of_line(line, dp_int, ad_int, h);
        if (c == VCF_KEEP) {
            g_kept++;
            if (!kept || h.chrom.size() != r.chrom_len || h.chrom.data() != line.data() || h.pos != r.pos || !same(h.baf, r.value)) fail("KEEP differs from the host", line);
        } else if (c == VCF_SKIP) {
            g_skipped++;
            if (kept) fail("SKIP of a line the host keeps", line);
        } else if (c == VCF_DEFER) {
            g_deferred++;
        } else fail("a code the SNP form does not have", line);
        return;
    }
    const uint32_t last = t.sorted.empty() ? 0 : t.sorted.back();
    const int c = vcf_af_line(p, len, (const uint8_t *)t.contig.data(), (uint32_t)t.contig.size(), (const uint8_t *)t.needle.data(), (uint32_t)t.needle.size(),
                              t.sorted.data(), t.sorted.size(), last, r);
    uint32_t pos = 0;
    double af = 0;
    const AfLine h = af_record_of_line(line, t.contig, t.needle, t.sorted, last, pos, af);
    if ((c == VCF_DEFER) != af_must_defer(line, t, last)) fail(c == VCF_DEFER ? "DEFER outside the rule" : "a line the rule defers was decided", line);
    if (c == VCF_KEEP) {
        g_kept++;
        if (h != AfLine::Keep || pos != r.pos || !same(af, r.value)) fail("KEEP differs from the host", line);
    } else if (c == VCF_SKIP || c == VCF_STOP) {
        g_skipped++;
        if (h != (c == VCF_STOP ? AfLine::Stop : AfLine::Skip)) fail("SKIP / STOP differs from the host", line);
    } else if (c == VCF_DEFER) {
        g_deferred++;
    } else fail("a code that must not leave vcf_af_line", line);
}

// every line of a text held in a heap block of exactly its size (the host's for_lines: '\r' stripped, empty and '#' lines passed over)
void check_text(const Text &t, const std::vector<uint8_t> &bytes, bool dp_int, bool ad_int)
{
    uint8_t *block = (uint8_t *)malloc(bytes.size() ? bytes.size() : 1);
    if (!bytes.empty()) memcpy(block, bytes.data(), bytes.size());
    size_t a = 0;
    while (a < bytes.size()) {
        const void *nl = memchr(block + a, '\n', bytes.size() - a);
        size_t e = nl ? (size_t)((const uint8_t *)nl - block) : bytes.size();
        size_t end = e;
        if (end > a && block[end - 1] == '\r') end--;
        if (end > a && block[a] != '#') check_line(t, block + a, (uint32_t)(end - a), dp_int, ad_int);
        a = e + 1;
    }
    free(block);
}

bool read_u32(FILE *f, uint32_t &v) { return fread(&v, 4, 1, f) == 1; }
bool read_bytes(FILE *f, std::string &s) { uint32_t n; if (!read_u32(f, n)) return false; s.resize(n); return n == 0 || fread(&s[0], 1, n, f) == n; }

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 4) { fprintf(stderr, "usage: vcf_record_core_check <corpus> <mutations per text> <seed>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    char magic[4];
    uint32_t n_texts = 0;
    if (!f || fread(magic, 1, 4, f) != 4 || memcmp(magic, "VCFC", 4) != 0 || !read_u32(f, n_texts)) { fprintf(stderr, "cannot read the corpus %s\n", argv[1]); return 2; }
    std::vector<Text> texts(n_texts);
    for (Text &t : texts) {
        std::string b;
        bool ok = read_u32(f, t.kind) && read_bytes(f, b);
        t.bytes.assign(b.begin(), b.end());
        if (ok && t.kind == 1) {
            uint32_t n = 0;
            ok = read_bytes(f, t.contig) && read_bytes(f, t.needle) && read_u32(f, n);
            t.sorted.resize(n);
            ok = ok && (n == 0 || fread(t.sorted.data(), 4, n, f) == n);
        }
        if (!ok) { fprintf(stderr, "the corpus ends inside a text\n"); return 2; }
    }
    fclose(f);
    const int n_mut = atoi(argv[2]);
    std::mt19937_64 rng(strtoull(argv[3], nullptr, 10));
    static const char kBytes[] = {'\t', '0', '1', '2', '3', '4', '5', '6', '7', '8', '9', ':', ',', ';', '.', 'e', '-', '\0'};
    for (const Text &t : texts) {
        check_text(t, t.bytes, true, true);
        if (t.kind == 0) { check_text(t, t.bytes, false, true); check_text(t, t.bytes, true, false); }
        for (int m = 0; m < n_mut && !t.bytes.empty(); m++) {
            std::vector<uint8_t> b = t.bytes;
            // a copy's share of changed bytes grows with its number: from one byte to one in thirty
            const size_t changes = 1 + (size_t)((double)b.size() / 30 * m / std::max(1, n_mut - 1));
            for (size_t k = 0; k < changes; k++) b[rng() % b.size()] = (uint8_t)kBytes[rng() % sizeof(kBytes)];
            check_text(t, b, true, true);
        }
    }
    printf("vcf_record_core_check: %u texts, %ld kept, %ld skipped, %ld deferred, %ld failures\n", n_texts, g_kept, g_skipped, g_deferred, g_fail);
    return g_fail ? 1 : 0;
}
