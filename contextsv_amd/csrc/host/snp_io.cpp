#include "snp_io.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <future>
#include <limits>
#include <sstream>

#include "../../../include/csvgpu.h"
#include "log.h"

namespace {
constexpr double kMinPfb = 0.01, kMaxPfb = 0.99;             // cnv_caller.cpp:33-34
constexpr int32_t kIntMissing = std::numeric_limits<int32_t>::min();        // bcf_int32_missing
constexpr int32_t kIntVectorEnd = std::numeric_limits<int32_t>::min() + 1;  // bcf_int32_vector_end

using sv = std::string_view;

// tab-separated field k of a line, or false
struct Fields {
    sv f[10];
    sv samples;          // everything after FORMAT
    int n = 0;
};
bool split_fields(sv line, Fields &out)
{
    out.n = 0;
    size_t a = 0;
    while (out.n < 9) {
        const size_t t = line.find('\t', a);
        if (t == sv::npos) { out.f[out.n++] = line.substr(a); out.samples = sv(); return out.n >= 8; }
        out.f[out.n++] = line.substr(a, t - a);
        a = t + 1;
    }
    out.samples = line.substr(a);
    return true;
}

// bcf_is_snp: every allele (REF and ALTs) is one base other than '*', or the symbolic <X> / <*>
bool is_snp(sv ref, sv alt)
{
    auto one = [](sv a) { return (a.size() == 1 && a[0] != '*') || a == "<X>" || a == "<*>"; };
    if (!one(ref)) return false;
    if (alt == ".") return true;                          // no ALT allele: only REF is tested
    size_t a = 0;
    for (;;) {
        const size_t c = alt.find(',', a);
        if (!one(alt.substr(a, c == sv::npos ? sv::npos : c - a))) return false;
        if (c == sv::npos) return true;
        a = c + 1;
    }
}

// index of `key` among the ':'-separated FORMAT keys, or -1
int format_index(sv format, sv key)
{
    int i = 0;
    size_t a = 0;
    for (;;) {
        const size_t c = format.find(':', a);
        if (format.substr(a, c == sv::npos ? sv::npos : c - a) == key) return i;
        if (c == sv::npos) return -1;
        a = c + 1;
        i++;
    }
}

// field `idx` of one sample column ("" when the sample has fewer fields: trailing fields may be dropped)
sv sample_field(sv sample, int idx)
{
    size_t a = 0;
    for (int i = 0; i < idx; i++) {
        const size_t c = sample.find(':', a);
        if (c == sv::npos) return sv();
        a = c + 1;
    }
    const size_t c = sample.find(':', a);
    return sample.substr(a, c == sv::npos ? sv::npos : c - a);
}

// integer vector of one FORMAT field value: "." / "" -> one missing value
void parse_ints(sv v, std::vector<int32_t> &out)
{
    out.clear();
    if (v.empty() || v == ".") { out.push_back(kIntMissing); return; }
    size_t a = 0;
    for (;;) {
        const size_t c = v.find(',', a);
        sv t = v.substr(a, c == sv::npos ? sv::npos : c - a);
        if (t.empty() || t == ".") out.push_back(kIntMissing);
        else out.push_back((int32_t)strtol(std::string(t).c_str(), nullptr, 10));
        if (c == sv::npos) return;
        a = c + 1;
    }
}

// what bcf_get_format_int32 hands back for `key`: sample-major, every sample padded to the longest with vector-end marks
bool format_ints(sv format, sv samples, sv key, std::vector<int32_t> &flat)
{
    const int idx = format_index(format, key);
    if (idx < 0) return false;
    std::vector<std::vector<int32_t>> per;
    size_t a = 0;
    for (;;) {
        const size_t t = samples.find('\t', a);
        per.emplace_back();
        parse_ints(sample_field(samples.substr(a, t == sv::npos ? sv::npos : t - a), idx), per.back());
        if (t == sv::npos) break;
        a = t + 1;
    }
    size_t width = 0;
    for (const auto &p : per) width = std::max(width, p.size());
    flat.clear();
    for (const auto &p : per) {
        flat.insert(flat.end(), p.begin(), p.end());
        flat.insert(flat.end(), width - p.size(), kIntVectorEnd);
    }
    return true;
}

// "##FORMAT=<ID=DP,Number=1,Type=Integer,...>" -> (kind, id, type)
bool header_decl(sv line, sv kind, std::string &id, std::string &type)
{
    const std::string prefix = "##" + std::string(kind) + "=<";
    if (line.substr(0, prefix.size()) != prefix) return false;
    auto grab = [&](sv key) -> std::string {
        const std::string k = std::string(key) + "=";
        size_t p = line.find(k, prefix.size() - 1);
        while (p != sv::npos && line[p - 1] != '<' && line[p - 1] != ',') p = line.find(k, p + 1);
        if (p == sv::npos) return "";
        const size_t e = line.find_first_of(",>", p + k.size());
        return std::string(line.substr(p + k.size(), e == sv::npos ? sv::npos : e - p - k.size()));
    };
    id = grab("ID");
    type = grab("Type");
    return !id.empty();
}

bool file_exists(const std::string &p) { std::ifstream f(p); return (bool)f; }

// iterate the lines of a chunk
template <class F>
bool for_lines(sv chunk, F fn)
{
    size_t a = 0;
    while (a < chunk.size()) {
        size_t e = chunk.find('\n', a);
        if (e == sv::npos) e = chunk.size();
        sv line = chunk.substr(a, e - a);
        if (!line.empty() && line.back() == '\r') line.remove_suffix(1);
        if (!line.empty() && !fn(line)) return false;
        a = e + 1;
    }
    return true;
}
}  // namespace

// ---- TextFile -----------------------------------------------------------------------------------------------
bool TextFile::open(const std::string &path, std::string *err)
{
    if (!file.open(path, err)) return false;
    const uint8_t *p = file.data();
    is_bgzf = false;
    if (file.size() >= 2 && p[0] == 0x1f && p[1] == 0x8b) {
        bgzf::Block b;
        if (!bgzf::parse_block(p, file.size(), 0, b, err)) { if (err) *err = path + " is gzip but not BGZF (use bgzip): " + *err; return false; }
        is_bgzf = true;
    }
    return true;
}

bool TextFile::forEachChunk(int threads, const std::function<bool(std::string_view)> &on_lines, std::string *err, size_t window_blocks)
{
    if (!is_bgzf) {                                       // plain text: one chunk
        if (file.size()) on_lines(sv((const char *)file.data(), file.size()));
        return true;
    }
    struct Batch { std::vector<bgzf::Block> blocks; HugeVec<uint8_t> data; bool ok = true; std::string err; uint64_t next = 0; };
    const size_t kHead = 1 << 20, W = window_blocks ? window_blocks : 1024;
    auto load = [&](uint64_t coff, Batch &b) {
        b.blocks.clear(); b.ok = true;
        uint64_t total = 0;
        while (coff < file.size() && b.blocks.size() < W) {
            bgzf::Block blk;
            if (!bgzf::parse_block(file.data() + coff, file.size() - coff, coff, blk, &b.err)) { b.ok = false; return; }
            b.blocks.push_back(blk);
            total += blk.isize;
            coff += blk.csize;
        }
        b.next = coff;
        b.data.resize_uninit(kHead + total);
        if (!bgzf::inflate_range(file.data(), b.blocks, 0, b.blocks.size(), b.data.data() + kHead, threads, &b.err)) b.ok = false;
    };
    Batch batch[2];
    load(0, batch[0]);
    int cur = 0;
    std::string carry;                                    // the unterminated tail of the previous batch
    HugeVec<uint8_t> joined;
    for (;;) {
        Batch &b = batch[cur];
        if (!b.ok) { if (err) *err = b.err; return false; }
        if (b.blocks.empty()) break;
        std::future<void> ahead;
        const bool more = b.next < file.size();
        if (more) ahead = std::async(std::launch::async, load, b.next, std::ref(batch[cur ^ 1]));
        char *p = (char *)b.data.data() + kHead;
        size_t n = b.data.size() - kHead;
        if (!carry.empty()) {
            if (carry.size() <= kHead) { p -= carry.size(); memcpy(p, carry.data(), carry.size()); n += carry.size(); }
            else { joined.clear(); joined.append((const uint8_t *)carry.data(), carry.size()); joined.append((const uint8_t *)p, n); p = (char *)joined.data(); n = joined.size(); }
            carry.clear();
        }
        size_t whole = n;
        if (more) {                                       // keep the last partial line for the next batch
            while (whole > 0 && p[whole - 1] != '\n') whole--;
            carry.assign(p + whole, n - whole);
        }
        const bool go = whole == 0 || on_lines(sv(p, whole));
        if (more) ahead.get();
        if (!go || !more) break;
        cur ^= 1;
    }
    return true;
}

// ---- --pfb table ----------------------------------------------------------------------------------------------
bool AlleleFreqFiles::load(const std::string &table_path, std::string *err)
{
    if (table_path.empty()) return true;
    std::ifstream in(table_path);
    if (!in.is_open()) { if (err) *err = "Population allele frequency file does not exist: " + table_path; return false; }
    std::string line;
    while (std::getline(in, line)) {
        if (!line.empty() && line[0] == '#') continue;
        line = line.substr(0, 255);                       // the reference reads through a 256-byte fgets buffer (:248-250)
        std::vector<std::string> parts;
        std::istringstream ss(line);
        std::string tok;
        while (std::getline(ss, tok, '=')) parts.push_back(tok);
        if (parts.size() != 2) continue;
        const std::string vcf = parts[1].substr(0, parts[1].find_first_of("\r\n"));
        if (!file_exists(vcf)) { if (err) *err = "Error: Allele frequency file does not exist: " + vcf; return false; }
        paths[parts[0]] = vcf;
    }
    return true;
}

std::string AlleleFreqFiles::get(std::string chr) const
{
    if (chr.find("chr") != std::string::npos) chr = chr.substr(3, chr.size() - 3);     // wherever "chr" was found (:297-300)
    auto it = paths.find(chr);
    return it == paths.end() ? "" : it->second;
}

std::string gnomadContigName(const std::string &chr, const std::string &pfb_filepath)
{
    std::string g = chr;
    if (pfb_filepath.find("chr") == std::string::npos) {
        if (g.find("chr") != std::string::npos) g = g.substr(3);
    } else if (g.find("chr") == std::string::npos) {
        g = "chr" + chr;
    }
    return g;
}

// ---- one data line ----------------------------------------------------------------------------------------------
namespace {
// (dp, ad: the caller's scratch, so that a file's lines share two allocations)
inline bool snp_record_impl(sv line, bool dp_int, bool ad_int, std::vector<int32_t> &dp, std::vector<int32_t> &ad, SnpLineRecord &rec)
{
    Fields f;
    if (!split_fields(line, f) || f.n < 9) return false;                     // no FORMAT / sample columns: DP lookup fails (:696-701)
    if (!is_snp(f.f[3], f.f[4])) return false;                                // :679-683
    if (f.f[5] == ".") return false;                                          // QUAL missing (:686)
    const float qual = (float)strtod(std::string(f.f[5]).c_str(), nullptr);
    if (qual <= 30) return false;
    if (!dp_int || !format_ints(f.f[8], f.samples, "DP", dp) || dp[0] <= 10) return false;    // :693-701 (missing = INT32_MIN)
    if (f.f[6] != "." && f.f[6] != "PASS") {                                 // bcf_has_filter(.., "PASS") (:704-707)
        bool pass = false;
        size_t a = 0;
        for (;;) {
            const size_t c = f.f[6].find(';', a);
            if (f.f[6].substr(a, c == sv::npos ? sv::npos : c - a) == "PASS") pass = true;
            if (c == sv::npos) break;
            a = c + 1;
        }
        if (!pass) return false;
    }
    if (!ad_int || !format_ints(f.f[8], f.samples, "AD", ad) || ad.size() < 2) return false;  // :710-717
    rec.baf = (double)ad[1] / (double)(int32_t)((uint32_t)ad[0] + (uint32_t)ad[1]);           // :720
    rec.chrom = f.f[0];
    rec.pos = (uint32_t)strtol(std::string(f.f[1]).c_str(), nullptr, 10);
    return true;
}

inline AfLine af_record_impl(sv line, sv contig, sv needle, const std::vector<uint32_t> &sorted, uint32_t last_pos, uint32_t &pos, double &af)
{
    Fields f;
    if (!split_fields(line, f)) return AfLine::Skip;
    if (f.f[0] != contig) return AfLine::Skip;
    const uint32_t p = (uint32_t)strtol(std::string(f.f[1]).c_str(), nullptr, 10);
    if (p > last_pos) return AfLine::Stop;
    if (!std::binary_search(sorted.begin(), sorted.end(), p)) return AfLine::Skip;   // :782-786
    if (!is_snp(f.f[3], f.f[4])) return AfLine::Skip;                        // :775-779
    // INFO key at the start of the field or behind ';'
    sv info = f.f[7];
    size_t k = info.find(needle);
    while (k != sv::npos && k != 0 && info[k - 1] != ';') k = info.find(needle, k + 1);
    if (k == sv::npos) return AfLine::Skip;                                  // status < 0
    const size_t e = info.find_first_of(";,", k + needle.size());
    const sv val = info.substr(k + needle.size(), e == sv::npos ? sv::npos : e - k - needle.size());
    if (val.empty()) return AfLine::Skip;                                    // count == 0
    const double v = val == "." ? std::nan("") : (double)(float)strtod(std::string(val).c_str(), nullptr);
    if (v <= kMinPfb || v >= kMaxPfb) return AfLine::Skip;                   // :795-799 (NaN passes, as there)
    pos = p;
    af = v;
    return AfLine::Keep;
}
}  // namespace

bool snp_record_of_line(std::string_view line, bool dp_int, bool ad_int, SnpLineRecord &rec)
{
    static thread_local std::vector<int32_t> dp, ad;
    return snp_record_impl(line, dp_int, ad_int, dp, ad, rec);
}

AfLine af_record_of_line(std::string_view line, std::string_view contig, std::string_view needle, const std::vector<uint32_t> &sorted, uint32_t last_pos,
                         uint32_t &pos, double &af)
{
    return af_record_impl(line, contig, needle, sorted, last_pos, pos, af);
}

// ---- tables -----------------------------------------------------------------------------------------------------
void SNPFileTable::query(uint32_t start_pos, uint32_t end_pos, std::vector<uint32_t> &snp_pos, std::unordered_map<uint32_t, double> &snp_baf,
                         std::unordered_map<uint32_t, double> &snp_pfb) const
{
    // pos is ascending for an indexed file; tolerate local disorder by scanning from the first position >= start
    const size_t a = std::lower_bound(pos.begin(), pos.end(), start_pos) - pos.begin();
    uint32_t lo = UINT32_MAX, hi = 0;
    bool any = false;
    for (size_t i = a; i < pos.size() && pos[i] <= end_pos; i++) {
        snp_pos.push_back(pos[i]);
        snp_baf[pos[i]] = baf[i];
        lo = std::min(lo, pos[i]); hi = std::max(hi, pos[i]);
        any = true;
    }
    if (!any) return;                                     // :734-740
    const size_t g = std::lower_bound(af_pos.begin(), af_pos.end(), lo) - af_pos.begin();
    if (g < af_pos.size() && af_pos[g] <= hi) snp_pfb[af_pos[g]] = af[g];     // first acceptable record, then the reference breaks (:800-801)
}

// ---- a chunk's data lines on the device ---------------------------------------------------------------------------
namespace {
// the line that starts at chunk[off]
sv line_at(sv chunk, size_t off)
{
    size_t e = chunk.find('\n', off);
    if (e == sv::npos) e = chunk.size();
    sv line = chunk.substr(off, e - off);
    if (!line.empty() && line.back() == '\r') line.remove_suffix(1);
    return line;
}

// The header lines in front of a chunk's first data line go to on_header; -> the first data line's offset (chunk.size() if there is none)
template <class F>
size_t leading_header(sv chunk, F on_header)
{
    size_t a = 0;
    while (a < chunk.size()) {
        size_t e = chunk.find('\n', a);
        if (e == sv::npos) e = chunk.size();
        sv line = chunk.substr(a, e - a);
        if (!line.empty() && line.back() == '\r') line.remove_suffix(1);
        if (!line.empty()) {
            if (line[0] != '#') return a;
            on_header(line);
        }
        a = e + 1;
    }
    return chunk.size();
}

// One chunk of data lines through csvgpu_vcf_*_parse: a sizing call where the arrays are too small, then the kept records and the
// deferred lines' offsets in `o`. -> CSV_OK, 1 (declined: the caller parses the chunk), or a CSV_E* with *err set.
struct DeviceLines {
    std::vector<uint32_t> line_off, chrom_len, pos, defer_off;
    std::vector<double> value;
    csv_vcf_counts counts{};
    // room for `n` kept records before the first call (a guess from the chunk's size spares most chunks the sizing call)
    void expect(size_t n)
    {
        if (n > line_off.size()) { line_off.resize(n); chrom_len.resize(n); pos.resize(n); value.resize(n); }
        if (defer_off.size() < 4096) defer_off.resize(4096);
    }
    template <class Call>
    int run(csv_ctx *ctx, bool af, Call call, std::string *err)
    {
        for (int pass = 0; pass < 2; pass++) {
            csv_vcf_out o{};
            o.line_off = line_off.data(); o.chrom_len = af ? nullptr : chrom_len.data(); o.pos = pos.data(); o.value = value.data(); o.defer_off = defer_off.data();
            o.cap = line_off.size(); o.cap_defer = defer_off.size();
            const int rc = call(&o, &counts);
            if (rc != CSV_ECAPACITY || pass) {
                if (rc < 0 && err) *err = std::string("device VCF parser: ") + csvgpu_last_error(ctx);
                return rc;
            }
            if (counts.n_kept > line_off.size()) { const size_t n = counts.n_kept + counts.n_kept / 4; line_off.resize(n); chrom_len.resize(n); pos.resize(n); value.resize(n); }
            if (counts.n_deferred > defer_off.size()) defer_off.resize(counts.n_deferred + counts.n_deferred / 4);
        }
        return CSV_EHIP;
    }
};
}  // namespace

bool SNPFile::load(const std::string &snp_vcf, int threads, std::string *err, const SNPDeviceOptions *dev)
{
    if (snp_vcf.empty()) { if (err) *err = "ERROR: SNP file path is empty."; return false; }
    TextFile tf;
    if (!tf.open(snp_vcf, err)) return false;
    if (tf.compressed() && !file_exists(snp_vcf + ".tbi") && !file_exists(snp_vcf + ".csi")) {
        if (err) *err = "ERROR: Could not add SNP file to reader: " + snp_vcf + " (no .tbi / .csi index)";
        return false;
    }
    bool dp_int = false, ad_int = false;
    std::vector<int32_t> dp, ad;
    std::string last_chr;
    SNPFileTable *cur = nullptr;
    auto on_header = [&](sv line) {
        std::string id, type;
        if (header_decl(line, "FORMAT", id, type)) {
            if (id == "DP") dp_int = type == "Integer";
            if (id == "AD") ad_int = type == "Integer";
        }
    };
    auto keep = [&](sv chrom, uint32_t pos, double baf) {
        if (cur == nullptr || chrom != last_chr) {
            last_chr.assign(chrom);
            cur = &tables[last_chr];
        }
        cur->pos.push_back(pos);
        cur->baf.push_back(baf);
        n_kept++;
    };
    auto on_line = [&](sv line) {
        if (line[0] == '#') { on_header(line); return true; }
        SnpLineRecord rec;
        if (snp_record_impl(line, dp_int, ad_int, dp, ad, rec)) keep(rec.chrom, rec.pos, rec.baf);
        return true;
    };
    if (dev == nullptr || dev->ctx == nullptr) return tf.forEachChunk(threads, [&](sv chunk) { return for_lines(chunk, on_line); }, err);
    if (dev->tables_on_device) {
        std::string why;
        if (loadTables(snp_vcf, threads, &why, *dev)) return true;
        printError("WARNING: SNP tables are not built on the device (" + why + "): the records of " + snp_vcf + " are merged on the host");
    }

    DeviceLines d;
    bool failed = false;
    const bool ok = tf.forEachChunk(threads, [&](sv chunk) {
        const size_t a = leading_header(chunk, on_header);
        const sv rest = chunk.substr(a);
        if (rest.empty()) return true;
        if (rest.size() >= (1ull << 32)) return for_lines(rest, on_line);
        d.expect(rest.size() / 64 + 16);                  // (a sample's data line is rarely shorter)
        const int rc = d.run(dev->ctx, false, [&](const csv_vcf_out *o, csv_vcf_counts *c) {
            return csvgpu_vcf_snp_parse(dev->ctx, (const uint8_t *)rest.data(), rest.size(), dp_int, ad_int, o, c);
        }, err);
        if (rc < 0) { failed = true; return false; }
        if (rc == 1) { dev_stats.declined_batches++; return for_lines(rest, on_line); }       // (a header line behind data may change dp_int / ad_int)
        dev_stats.lines += d.counts.n_lines; dev_stats.kept += d.counts.n_kept; dev_stats.deferred += d.counts.n_deferred;
        // Kept records and deferred lines in file order. A run of records with one CHROM (length and bytes equal to the run's first: one
        // short memcmp per record) goes straight into the run's table; the name becomes a string, and the table is looked up, once per run.
        uint64_t k = 0, q = 0;
        uint32_t run_len = UINT32_MAX;
        const char *run_name = nullptr;
        SNPFileTable *run_table = nullptr;
        while (k < d.counts.n_kept || q < d.counts.n_deferred) {
            if (q >= d.counts.n_deferred || (k < d.counts.n_kept && d.line_off[k] < d.defer_off[q])) {
                const char *name = rest.data() + d.line_off[k];
                if (run_table == nullptr || d.chrom_len[k] != run_len || memcmp(name, run_name, run_len) != 0) {
                    run_len = d.chrom_len[k]; run_name = name;
                    keep(sv(run_name, run_len), d.pos[k], d.value[k]);
                    run_table = cur;
                } else {
                    run_table->pos.push_back(d.pos[k]);
                    run_table->baf.push_back(d.value[k]);
                    n_kept++;
                }
                k++;
            } else {
                SnpLineRecord rec;
                if (snp_record_of_line(line_at(rest, d.defer_off[q]), dp_int, ad_int, rec)) { keep(rec.chrom, rec.pos, rec.baf); run_table = nullptr; }   // (it may have changed the contig)
                q++;
            }
        }
        return true;
    }, err, dev->window_blocks);
    return ok && !failed;
}

// ---- the tables built on the device (SNPDeviceOptions::tables_on_device) ----------------------------------------------------------
// Replaces, per chunk, the parse call and the per-record loop above by one csvgpu_snp_builder_append: the kept records stay on the device,
// a run table comes back, and every run's name is looked up once. Deferred lines, declined batches and batches of 2^32 bytes or more go
// through snp_record_of_line and csvgpu_snp_builder_append_host with their offsets in the text as keys.
bool SNPFile::loadTables(const std::string &snp_vcf, int threads, std::string *err, const SNPDeviceOptions &dev)
{
    csv_ctx *ctx = dev.ctx;
    TextFile tf;
    if (!tf.open(snp_vcf, err)) return false;
    csv_snp_builder *b = csvgpu_snp_builder_create(ctx, 0);
    if (!b) { *err = csvgpu_last_error(ctx); return false; }
    bool dp_int = false, ad_int = false;
    auto on_header = [&](sv line) {
        std::string id, type;
        if (header_decl(line, "FORMAT", id, type)) {
            if (id == "DP") dp_int = type == "Integer";
            if (id == "AD") ad_int = type == "Integer";
        }
    };
    std::unordered_map<std::string, uint32_t> ids;
    std::vector<std::string> names;
    auto id_of = [&](sv name) {
        auto it = ids.find(std::string(name));
        if (it != ids.end()) return it->second;
        names.emplace_back(name);
        return ids.emplace(names.back(), (uint32_t)names.size() - 1).first->second;
    };
    std::vector<uint32_t> run_contig, run_first, run_line_off, run_chrom_len, defer_off(4096), h_id, h_pos;
    std::vector<uint64_t> h_key;
    std::vector<double> h_baf;
    SNPDeviceStats st;
    uint64_t base = 0;                                    // the chunk's offset in the text: the order keys' base
    bool failed = false;
    auto fail = [&](const std::string &what) { *err = what; failed = true; return false; };
    auto host_line = [&](sv line, uint64_t key) {
        SnpLineRecord rec;
        if (!snp_record_of_line(line, dp_int, ad_int, rec)) return;
        h_id.push_back(id_of(rec.chrom)); h_key.push_back(key); h_pos.push_back(rec.pos); h_baf.push_back(rec.baf);
    };
    auto flush_host = [&]() {
        if (h_id.empty()) return true;
        const int rc = csvgpu_snp_builder_append_host(ctx, b, h_id.size(), h_id.data(), h_key.data(), h_pos.data(), h_baf.data());
        st.appended_host += h_id.size();
        h_id.clear(); h_key.clear(); h_pos.clear(); h_baf.clear();
        return rc == CSV_OK;
    };
    const bool ok = tf.forEachChunk(threads, [&](sv chunk) {
        const uint64_t chunk_base = base;
        base += chunk.size();
        const size_t a = leading_header(chunk, on_header);
        const sv rest = chunk.substr(a);
        if (rest.empty()) return true;
        const uint64_t rest_base = chunk_base + a;
        // the whole batch through the host parser (a header line behind data may change dp_int / ad_int)
        auto host_batch = [&]() {
            for_lines(rest, [&](sv line) {
                if (line[0] == '#') on_header(line);
                else host_line(line, rest_base + (uint64_t)(line.data() - rest.data()));
                return true;
            });
            return flush_host() ? true : fail(csvgpu_last_error(ctx));
        };
        if (rest.size() >= (1ull << 32)) return host_batch();
        csv_snp_append_counts c{};
        int rc = CSV_OK;
        for (int pass = 0; pass < 2; pass++) {
            csv_snp_runs o{};
            o.run_first = run_first.data(); o.run_line_off = run_line_off.data(); o.run_chrom_len = run_chrom_len.data(); o.defer_off = defer_off.data();
            o.cap_runs = run_first.size(); o.cap_defer = defer_off.size();
            rc = csvgpu_snp_builder_append(ctx, b, (const uint8_t *)rest.data(), rest.size(), rest_base, dp_int, ad_int, &o, &c);
            if (rc != CSV_ECAPACITY) break;
            if (c.n_runs > run_first.size()) { const size_t n = c.n_runs + c.n_runs / 4 + 16; run_first.resize(n); run_line_off.resize(n); run_chrom_len.resize(n); }
            if (c.n_deferred > defer_off.size()) defer_off.resize(c.n_deferred + c.n_deferred / 4);
        }
        if (rc < 0) return fail(csvgpu_last_error(ctx));
        if (rc == 1) { st.declined_batches++; return host_batch(); }
        st.lines += c.n_lines; st.kept += c.n_kept; st.deferred += c.n_deferred; st.runs += c.n_runs;
        if (run_contig.size() != c.first_run) return fail("the builder's run count is not the caller's");
        for (uint64_t r = 0; r < c.n_runs; r++) run_contig.push_back(id_of(rest.substr(run_line_off[r], run_chrom_len[r])));      // one string per run
        for (uint64_t q = 0; q < c.n_deferred; q++) host_line(line_at(rest, defer_off[q]), rest_base + defer_off[q]);
        return flush_host() ? true : fail(csvgpu_last_error(ctx));
    }, err, dev.window_blocks ? dev.window_blocks : 1024);
    if (!ok || failed) { csvgpu_snp_builder_destroy(ctx, b); return false; }
    csv_snp_columns *cols = csvgpu_snp_builder_finish(ctx, b, run_contig.data(), run_contig.size());       // (consumes b)
    if (!cols) { *err = csvgpu_last_error(ctx); return false; }
    // every contig's columns ONCE to the host vectors: query, queryFlat, declined copy-number batches and csvhost_snp_table work unchanged
    uint64_t n_contigs = 0;
    csvgpu_snp_columns_describe(cols, 0, nullptr, nullptr, nullptr, &n_contigs);
    std::vector<uint32_t> cid(n_contigs);
    std::vector<uint64_t> count(n_contigs);
    std::vector<uint8_t> asc(n_contigs);
    bool good = csvgpu_snp_columns_describe(cols, n_contigs, cid.data(), count.data(), asc.data(), &n_contigs) == CSV_OK;
    std::unordered_map<std::string, SNPFileTable> built;
    std::unordered_map<std::string, std::pair<uint32_t, bool>> where;
    uint64_t total = 0;
    for (uint64_t k = 0; good && k < n_contigs; k++) {
        good = cid[k] < names.size();
        if (!good) break;
        SNPFileTable &t = built[names[cid[k]]];
        t.pos.resize(count[k]); t.baf.resize(count[k]);
        good = csvgpu_snp_columns_fetch(ctx, cols, cid[k], t.pos.data(), t.baf.data()) == CSV_OK;
        where[names[cid[k]]] = {cid[k], asc[k] != 0};
        total += count[k];
    }
    if (!good) { *err = std::string("the columns' fetch: ") + csvgpu_last_error(ctx); csvgpu_snp_columns_free(ctx, cols); return false; }
    tables = std::move(built);
    column_of = std::move(where);
    columns = cols; columns_ctx = ctx;
    n_kept = total;
    dev_stats.lines += st.lines; dev_stats.kept += st.kept; dev_stats.deferred += st.deferred; dev_stats.declined_batches += st.declined_batches;
    dev_stats.runs += st.runs; dev_stats.appended_host += st.appended_host;
    return true;
}

void SNPFile::dropColumns()
{
    if (columns) csvgpu_snp_columns_free(columns_ctx, columns);
    columns = nullptr; columns_ctx = nullptr;
    column_of.clear();
}

SNPFile::~SNPFile()
{
    for (auto &kv : tables)
        if (kv.second.resident) { csvgpu_snp_table_free(kv.second.resident_ctx, kv.second.resident); kv.second.resident = nullptr; }      // (dropResident)
    dropColumns();
}

const SNPFileTable &SNPFile::table(const std::string &chr, const std::string &pfb_vcf, const std::string &ethnicity, int threads, const SNPDeviceOptions *dev)
{
    auto it = tables.find(chr);
    if (it == tables.end()) return none;
    SNPFileTable &t = it->second;
    if (af_done[chr]) return t;
    af_done[chr] = true;
    // the contig's columns are resident and ascending: the population file is read against them, and the table is made from them
    int64_t column_id = -1;
    if (dev && dev->ctx && dev->tables_on_device && columns && dev->ctx == columns_ctx) {
        auto c = column_of.find(chr);
        if (c != column_of.end() && c->second.second) column_id = c->second.first;
    }
    attachAf(t, chr, pfb_vcf, ethnicity, threads, dev, column_id);
    if (column_id >= 0 && !t.resident) {
        // (a table the device refuses keeps the host arrays only: the host route serves the contig, with the same results)
        t.resident = csvgpu_snp_columns_table(columns_ctx, columns, (uint32_t)column_id, t.af_pos.data(), t.af.data(), t.af_pos.size());
        if (t.resident) { t.resident_ctx = columns_ctx; dev_stats.tables_resident++; }
        else printError(std::string("WARNING: no resident SNP table for ") + chr + ": " + csvgpu_last_error(columns_ctx));
    }
    return t;
}

void SNPFile::attachAf(SNPFileTable &t, const std::string &chr, const std::string &pfb_vcf, const std::string &ethnicity, int threads, const SNPDeviceOptions *dev,
                       int64_t column_id)
{
    if (pfb_vcf.empty() || !file_exists(pfb_vcf) || t.pos.empty()) return;        // use_pfb = false (:596-611)
    TextFile tf;
    std::string err;
    if (!tf.open(pfb_vcf, &err) || (tf.compressed() && !file_exists(pfb_vcf + ".tbi") && !file_exists(pfb_vcf + ".csi"))) {
        printError("ERROR: Could not add population allele frequency file to reader: " + pfb_vcf);
        return;
    }
    const std::string key = ethnicity.empty() ? std::string("AF") : "AF_" + ethnicity;       // :616-623
    const std::string contig = gnomadContigName(chr, pfb_vcf);
    std::vector<uint32_t> sorted = t.pos;
    std::sort(sorted.begin(), sorted.end());
    const uint32_t last_pos = sorted.back();
    bool key_is_float = false;
    const std::string needle = key + "=";
    auto on_header = [&](sv line) {
        std::string id, type;
        if (header_decl(line, "INFO", id, type) && id == key) key_is_float = type == "Float";
    };
    auto on_line = [&](sv line) {
        if (line[0] == '#') { on_header(line); return true; }
        if (!key_is_float) return false;                                     // bcf_get_info_float fails on every record (:789-793)
        uint32_t p = 0;
        double v = 0;
        const AfLine what = af_record_impl(line, contig, needle, sorted, last_pos, p, v);
        if (what == AfLine::Stop) return false;                              // sorted file: nothing further can match
        if (what == AfLine::Skip) return true;
        t.af_pos.push_back(p);
        t.af.push_back(v);
        return true;
    };
    if (dev == nullptr || dev->ctx == nullptr) {
        tf.forEachChunk(threads, [&](sv chunk) { return for_lines(chunk, on_line); }, &err);
        return;
    }
    // table() has no way to report a failure (an unreadable population file is logged and leaves the table without hits): a device call that
    // fails (CSV_E*: out of memory, a HIP error) is logged ONCE and the host parser reads that chunk and the rest of the file — the table is
    // complete either way. load() has the caller's `err` and fails instead.
    DeviceLines d;
    bool device_failed = false;
    tf.forEachChunk(threads, [&](sv chunk) {
        const size_t a = leading_header(chunk, on_header);
        const sv rest = chunk.substr(a);
        if (rest.empty()) return true;
        if (!key_is_float) return false;
        if (device_failed || rest.size() >= (1ull << 32)) return for_lines(rest, on_line);
        d.expect(std::min(rest.size() / 64, 2 * sorted.size()) + 16);
        const int rc = d.run(dev->ctx, true, [&](const csv_vcf_out *o, csv_vcf_counts *c) {
            // (resident columns: the contig's positions are on the device already, and ascending, so they are the sorted ones — none goes up)
            if (column_id >= 0)
                return csvgpu_snp_columns_af_parse(dev->ctx, columns, (uint32_t)column_id, (const uint8_t *)rest.data(), rest.size(), contig.data(),
                                                   (uint32_t)contig.size(), needle.data(), (uint32_t)needle.size(), o, c);
            return csvgpu_vcf_af_parse(dev->ctx, (const uint8_t *)rest.data(), rest.size(), contig.data(), (uint32_t)contig.size(), needle.data(),
                                       (uint32_t)needle.size(), sorted.data(), sorted.size(), o, c);
        }, &err);
        if (rc < 0) { printError("ERROR: " + err + " (the host parser reads the rest of " + pfb_vcf + ")"); device_failed = true; return for_lines(rest, on_line); }
        if (rc == 1) { dev_stats.declined_batches++; return for_lines(rest, on_line); }
        dev_stats.lines += d.counts.n_lines; dev_stats.kept += d.counts.n_kept; dev_stats.deferred += d.counts.n_deferred;
        // file order; the first STOP ends the file, whether the device found it (behind everything it reported) or a deferred line is one
        uint64_t k = 0, q = 0;
        while (k < d.counts.n_kept || q < d.counts.n_deferred) {
            if (q >= d.counts.n_deferred || (k < d.counts.n_kept && d.line_off[k] < d.defer_off[q])) {
                t.af_pos.push_back(d.pos[k]);
                t.af.push_back(d.value[k]);
                k++;
            } else {
                if (!on_line(line_at(rest, d.defer_off[q]))) return false;
                q++;
            }
        }
        return d.counts.stop_off == UINT64_MAX;
    }, &err, dev->window_blocks);
}
