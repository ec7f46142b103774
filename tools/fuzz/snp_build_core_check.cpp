// snp_build_core_check.cpp — the rules of the SNP table builder (contextsv_amd/csrc/snp_build_core.hpp: the run rule, the key packing) and a
// literal restatement of csvgpu_snp_builder_append + _finish on the CPU, against SNPFile::load (host/snp_io.cpp: the `keep` lambda and its
// per-record loop), under AddressSanitizer + UBSan. A program of its own: `make -C contextsv_amd/csrc snp-build-check` links it with
// host/snp_io.cpp and the BGZF reader that file needs; tests/test_snp_build_core.py writes the corpus and runs it.
//   snp_build_core_check <corpus> <mutations per text> <seed> <scratch file>
// corpus: "SNPB", u32 header_len, header bytes, u32 texts, then per text: u32 len, bytes (whole data lines). Every text and every
// byte-mutated copy of it is cut into three batches at line ends, each batch in a heap block of exactly its size, and appended out of
// order: the lines decided by vcf_record_core.hpp as the device decides them, the kept records cut into runs by snpbuild::starts_run, the
// deferred lines (and a batch with a '#' line behind data, which the device declines) through snp_record_of_line; finish orders by
// snpbuild::pack_key. The per-contig columns must be the tables SNPFile::load builds from the same bytes in a file (header + text).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <random>
#include <string>
#include <string_view>
#include <vector>

#include "../../contextsv_amd/csrc/host/snp_io.h"
#include "../../contextsv_amd/csrc/snp_build_core.hpp"
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
// SNPFileTable's base class keeps this one function (and with it its vtable) in host/cnv_caller.cpp, which is not linked; no region is queried here
void SNPSource::queryFlat(uint32_t, uint32_t, std::vector<uint32_t> &, std::vector<double> &, std::vector<double> &) const { abort(); }
void printError(const std::string &m) { fprintf(stderr, "%s\n", m.c_str()); }     // (the mirror's logger is not linked either)

using sv = std::string_view;

namespace {

long g_records = 0, g_runs = 0, g_host = 0, g_declined = 0, g_contigs = 0, g_fail = 0;

void fail(const char *what, const std::string &detail)
{
    if (g_fail++ < 20) fprintf(stderr, "FAIL %s: %s\n", what, detail.c_str());
}

struct Builder {                                      // csv_snp_builder, and the caller's map of names
    std::vector<uint32_t> pos, run; std::vector<double> baf; std::vector<uint64_t> key;
    std::vector<uint32_t> run_contig;
    uint64_t max_key = 0;
    std::map<std::string, uint32_t> ids;
    uint32_t id_of(sv name) { return ids.emplace(std::string(name), (uint32_t)ids.size()).first->second; }
    void host_record(const SnpLineRecord &r, uint64_t key_)
    {
        pos.push_back(r.pos); baf.push_back(r.baf); run.push_back(snpbuild::HOST_TAG | id_of(r.chrom)); key.push_back(key_);
        max_key = std::max(max_key, key_);
        g_host++;
    }
};

// the non-empty lines of a block, '\r' stripped: (offset, length)
std::vector<std::pair<uint32_t, uint32_t>> lines_of(const uint8_t *p, size_t n)
{
    std::vector<std::pair<uint32_t, uint32_t>> out;
    size_t a = 0;
    while (a < n) {
        const void *nl = memchr(p + a, '\n', n - a);
        const size_t e = nl ? (size_t)((const uint8_t *)nl - p) : n;
        size_t end = e;
        if (end > a && p[end - 1] == '\r') end--;
        if (end > a) out.push_back({(uint32_t)a, (uint32_t)(end - a)});
        a = e + 1;
    }
    return out;
}

// csvgpu_snp_builder_append on one batch, and what the caller does with its report
void append(Builder &b, const std::vector<uint8_t> &bytes, uint64_t text_base)
{
    if (bytes.empty()) return;
    uint8_t *text = (uint8_t *)malloc(bytes.size());          // exactly its size: a load outside a CHROM field's bytes would be seen
    memcpy(text, bytes.data(), bytes.size());
    const auto lines = lines_of(text, bytes.size());
    bool declined = false;
    for (auto [off, len] : lines) declined |= text[off] == '#';
    if (declined) {                                           // the whole batch through the host parser and append_host
        g_declined++;
        for (auto [off, len] : lines) {
            SnpLineRecord r;
            if (text[off] != '#' && snp_record_of_line(sv((const char *)text + off, len), true, true, r)) b.host_record(r, text_base + off);
        }
        free(text);
        return;
    }
    std::vector<uint32_t> line_off, chrom_len, pos, defer_off;
    std::vector<double> value;
    for (auto [off, len] : lines) {
        vcfcore::Rec r;
        const int c = vcfcore::vcf_snp_line(text + off, len, true, true, r);
        if (c == vcfcore::VCF_KEEP) { line_off.push_back(off); chrom_len.push_back(r.chrom_len); pos.push_back(r.pos); value.push_back(r.value); }
        else if (c == vcfcore::VCF_DEFER) defer_off.push_back(off);
    }
    const uint32_t K = (uint32_t)line_off.size(), run_base = (uint32_t)b.run_contig.size();
    std::vector<uint32_t> ridx(K + 1, 0);                     // the flags, then their exclusive sums
    for (uint32_t k = 0; k < K; k++) ridx[k] = snpbuild::starts_run(text, line_off.data(), chrom_len.data(), k) ? 1 : 0;
    uint32_t sum = 0;
    for (uint32_t k = 0; k <= K; k++) { const uint32_t f = ridx[k]; ridx[k] = sum; sum += f; }
    const uint32_t R = ridx[K];
    std::vector<uint32_t> run_line_off(R), run_chrom_len(R);
    for (uint32_t k = 0; k < K; k++) {
        const uint32_t r = ridx[k + 1] - 1;
        if (ridx[k] == r) { run_line_off[r] = line_off[k]; run_chrom_len[r] = chrom_len[k]; }
        b.pos.push_back(pos[k]); b.baf.push_back(value[k]); b.run.push_back(run_base + r); b.key.push_back(text_base + line_off[k]);
    }
    b.max_key = std::max(b.max_key, text_base + bytes.size() - 1);
    for (uint32_t r = 0; r < R; r++) b.run_contig.push_back(b.id_of(sv((const char *)text + run_line_off[r], run_chrom_len[r])));   // one string per run
    g_runs += R;
    for (uint32_t off : defer_off) {
        const void *nl = memchr(text + off, '\n', bytes.size() - off);
        size_t end = nl ? (size_t)((const uint8_t *)nl - text) : bytes.size();
        if (end > off && text[end - 1] == '\r') end--;
        SnpLineRecord r;
        if (snp_record_of_line(sv((const char *)text + off, end - off), true, true, r)) b.host_record(r, text_base + off);
    }
    free(text);
}

struct Column { std::vector<uint32_t> pos; std::vector<double> baf; };

// csvgpu_snp_builder_finish: one stable order by the packed key, the columns per contig id
bool finish(const Builder &b, std::map<uint32_t, Column> &cols)
{
    const size_t n = b.pos.size();
    const int shift = snpbuild::bits_for(b.max_key);
    if (shift > 48) { fail("a key above 2^48", ""); return false; }
    std::vector<uint64_t> keys(n);
    for (size_t i = 0; i < n; i++) {
        const uint32_t id = snpbuild::contig_of(b.run[i], b.run_contig.data());
        if (id >= snpbuild::ID_LIMIT || b.key[i] >> shift) { fail("an id or a key outside the packing", ""); return false; }
        keys[i] = snpbuild::pack_key(id, b.key[i], shift);
        if (snpbuild::id_of(keys[i], shift) != id || (keys[i] & ((1ull << shift) - 1)) != b.key[i]) { fail("the packing loses bits", ""); return false; }
    }
    std::vector<uint32_t> order(n);
    std::iota(order.begin(), order.end(), 0u);
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return keys[x] < keys[y]; });
    for (size_t i = 0; i < n; i++) {
        if (i && keys[order[i]] == keys[order[i - 1]]) { fail("two records share a key", ""); return false; }
        Column &c = cols[snpbuild::id_of(keys[order[i]], shift)];
        c.pos.push_back(b.pos[order[i]]); c.baf.push_back(b.baf[order[i]]);
    }
    return true;
}

bool same(double a, double b) { return (std::isnan(a) && std::isnan(b)) || memcmp(&a, &b, 8) == 0; }

void check_text(const std::string &header, const std::vector<uint8_t> &bytes, const char *scratch, std::mt19937_64 &rng)
{
    // three batches cut at line ends, appended as 2, 0, 1 (or in another order of the six)
    size_t cut[4] = {0, bytes.size() / 3, 2 * bytes.size() / 3, bytes.size()};
    for (int i = 1; i < 3; i++) {
        const void *nl = cut[i] < bytes.size() ? memchr(bytes.data() + cut[i], '\n', bytes.size() - cut[i]) : nullptr;
        cut[i] = nl ? (size_t)((const uint8_t *)nl - bytes.data()) + 1 : bytes.size();
    }
    int perm[3] = {2, 0, 1};
    std::shuffle(perm, perm + 3, rng);
    Builder b;
    for (int i : perm) append(b, std::vector<uint8_t>(bytes.begin() + cut[i], bytes.begin() + cut[i + 1]), cut[i]);
    std::map<uint32_t, Column> cols;
    if (!finish(b, cols)) return;
    g_records += (long)b.pos.size();

    FILE *f = fopen(scratch, "wb");
    if (!f || fwrite(header.data(), 1, header.size(), f) != header.size() || (!bytes.empty() && fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size())) {
        fprintf(stderr, "cannot write %s\n", scratch);
        exit(2);
    }
    fclose(f);
    SNPFile host;
    std::string err;
    if (!host.load(scratch, 1, &err)) { fail("SNPFile::load", err); return; }
    if (host.records_kept() != b.pos.size()) fail("the record counts differ", std::to_string(host.records_kept()) + " on the host, " + std::to_string(b.pos.size()));
    size_t seen = 0;
    for (const auto &[name, id] : b.ids) {
        const SNPFileTable &t = host.table(name, "", "", 1);
        const Column &c = cols[id];
        g_contigs++;
        seen += t.pos.size();
        bool ok = t.pos == c.pos && t.baf.size() == c.baf.size();
        for (size_t i = 0; ok && i < c.baf.size(); i++) ok = same(t.baf[i], c.baf[i]);
        if (!ok) fail("a contig's columns differ from the host's table", name + ": " + std::to_string(t.pos.size()) + " on the host, " + std::to_string(c.pos.size()));
    }
    if (seen != host.records_kept()) fail("the host holds a contig the builder has not", "");
}

bool read_u32(FILE *f, uint32_t &v) { return fread(&v, 4, 1, f) == 1; }
bool read_bytes(FILE *f, std::string &s) { uint32_t n; if (!read_u32(f, n)) return false; s.resize(n); return n == 0 || fread(&s[0], 1, n, f) == n; }

// the run rule and the packing at their edges, against plain restatements
void check_rules()
{
    const char *t = "ab\tabc\tab\tb\ta\tab";                    // fields at 0, 3, 7, 10, 12, 14
    const uint32_t off[] = {0, 3, 7, 10, 12, 14}, len[] = {2, 3, 2, 1, 1, 2};
    const bool want[] = {true, true, true, true, true, true};
    for (uint32_t k = 0; k < 6; k++)
        if (snpbuild::starts_run((const uint8_t *)t, off, len, k) != want[k]) fail("starts_run", std::to_string(k));
    const uint32_t off2[] = {0, 7, 14, 3}, len2[] = {2, 2, 2, 2};   // ab, ab, ab, "ab" of abc: one run
    for (uint32_t k = 1; k < 4; k++)
        if (snpbuild::starts_run((const uint8_t *)t, off2, len2, k)) fail("starts_run on equal names", std::to_string(k));
    if (snpbuild::chrom_differs((const uint8_t *)t, 0, 0, 5, 0)) fail("two empty names differ", "");
    for (uint64_t v : {0ull, 1ull, 2ull, 3ull, 255ull, 256ull, (1ull << 47), (1ull << 48) - 1}) {
        const int bits = snpbuild::bits_for(v);
        if ((bits < 64 && (v >> bits)) || (bits && !(v >> (bits - 1)))) fail("bits_for", std::to_string(v));
        for (uint32_t id : {0u, 1u, 65535u}) {
            const uint64_t p = snpbuild::pack_key(id, v, bits);
            if (snpbuild::id_of(p, bits) != id || (bits < 64 && (p & ((1ull << bits) - 1)) != v)) fail("pack_key", std::to_string(v));
            if (id && snpbuild::pack_key(id - 1, (bits ? (1ull << bits) - 1 : 0), bits) >= snpbuild::pack_key(id, 0, bits)) fail("pack_key order", std::to_string(v));
        }
    }
    if (snpbuild::pack_key(65535, (1ull << 48) - 1, 48) != ~0ull) fail("the widest key", "");
    const uint32_t rc[] = {7, 9};
    if (snpbuild::contig_of(1, rc) != 9 || snpbuild::contig_of(snpbuild::HOST_TAG | 4, rc) != 4) fail("contig_of", "");
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc < 5) { fprintf(stderr, "usage: snp_build_core_check <corpus> <mutations per text> <seed> <scratch file>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    char magic[4];
    uint32_t n_texts = 0;
    std::string header;
    if (!f || fread(magic, 1, 4, f) != 4 || memcmp(magic, "SNPB", 4) != 0 || !read_bytes(f, header) || !read_u32(f, n_texts)) {
        fprintf(stderr, "cannot read the corpus %s\n", argv[1]);
        return 2;
    }
    std::vector<std::vector<uint8_t>> texts(n_texts);
    for (auto &t : texts) {
        std::string b;
        if (!read_bytes(f, b)) { fprintf(stderr, "the corpus ends inside a text\n"); return 2; }
        t.assign(b.begin(), b.end());
    }
    fclose(f);
    check_rules();
    const int n_mut = atoi(argv[2]);
    std::mt19937_64 rng(strtoull(argv[3], nullptr, 10));
    static const char kBytes[] = {'\t', '0', '1', '2', '3', '4', '5', '6', '7', '8', '9', ':', ',', ';', '.', 'e', '-', 'c', 'h', 'r', '\0'};
    for (const auto &t : texts) {
        check_text(header, t, argv[4], rng);
        for (int m = 0; m < n_mut && !t.empty(); m++) {
            std::vector<uint8_t> b = t;
            // a copy's share of changed bytes grows with its number: from one byte to one in fifty
            const size_t changes = 1 + (size_t)((double)b.size() / 50 * m / std::max(1, n_mut - 1));
            for (size_t k = 0; k < changes; k++) b[rng() % b.size()] = (uint8_t)kBytes[rng() % sizeof(kBytes)];
            check_text(header, b, argv[4], rng);
        }
    }
    remove(argv[4]);
    printf("snp_build_core_check: %u texts, %ld records, %ld runs, %ld host records, %ld declined batches, %ld contigs, %ld failures\n", n_texts, g_records, g_runs,
           g_host, g_declined, g_contigs, g_fail);
    return g_fail ? 1 : 0;
}
