#include "fasta_query.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstring>
#include <iostream>
#include <mutex>
#include <stdexcept>

#include "../../../include/csvgpu.h"
#include "../fasta_core.hpp"
#include "log.h"

namespace {
// read-only mapping of a whole file; empty files map to (nullptr, 0)
struct FileMap {
    const char *p = nullptr;
    size_t n = 0;
    explicit FileMap(const std::string &path)
    {
        int fd = ::open(path.c_str(), O_RDONLY);
        if (fd < 0) throw std::runtime_error("Could not open FASTA file " + path);
        struct stat st;
        if (fstat(fd, &st) != 0 || !S_ISREG(st.st_mode)) { ::close(fd); throw std::runtime_error("Could not open FASTA file " + path); }
        n = (size_t)st.st_size;
        if (n) {
            void *m = mmap(nullptr, n, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m == MAP_FAILED) { ::close(fd); throw std::runtime_error("Could not map FASTA file " + path); }
            (void)madvise(m, n, MADV_SEQUENTIAL);
            p = (const char *)m;
        }
        ::close(fd);
    }
    ~FileMap() { if (p) munmap((void *)p, n); }
    FileMap(const FileMap &) = delete;
    FileMap &operator=(const FileMap &) = delete;
};

constexpr uint64_t kDefaultWindow = (uint64_t)256 << 20;
}  // namespace

// The device backing: the genome lives on `ctx`'s device; every fetch goes through that context, one at a time.
struct ReferenceGenome::Device {
    csv_ctx *ctx = nullptr;
    csv_genome *g = nullptr;
    std::unordered_map<std::string, uint32_t> record;     // name -> its LAST record, as the host loader's map keeps the last one stored
    mutable std::mutex mu;
    mutable FastaDeviceStats stats;
    ~Device() { if (g) csvgpu_genome_free(ctx, g); }

    // items of records rec[i]; out_off as csvgpu_genome_fetch takes it; bytes: room for out_off[n]
    void fetch(const uint32_t *rec, const uint32_t *ps, const uint32_t *pe, const uint64_t *out_off, uint64_t n, bool mask, char *bytes) const
    {
        std::lock_guard<std::mutex> lock(mu);
        const int rc = csvgpu_genome_fetch(ctx, g, rec, ps, pe, out_off, n, mask ? 1 : 0, bytes);
        if (rc != CSV_OK) throw std::runtime_error(std::string("csvgpu_genome_fetch: ") + csvgpu_last_error(ctx));
        stats.fetch_calls++;
        stats.items_fetched += n;
    }
};

ReferenceGenome::ReferenceGenome() = default;
ReferenceGenome::~ReferenceGenome() = default;

FastaDeviceStats ReferenceGenome::deviceStats() const
{
    if (!dev) return load_stats;
    std::lock_guard<std::mutex> lock(dev->mu);
    return dev->stats;
}

const csv_genome *ReferenceGenome::deviceGenome(csv_ctx **ctx) const
{
    if (ctx) *ctx = dev ? dev->ctx : nullptr;
    return dev ? dev->g : nullptr;
}

int64_t ReferenceGenome::deviceRecord(const std::string &chr) const
{
    if (!dev) return -1;
    const auto it = dev->record.find(chr);
    return it == dev->record.end() ? -1 : (int64_t)it->second;
}

void ReferenceGenome::addContig(const std::string &name, std::string sequence)
{
    chromosomes.push_back(name);
    chr_to_length[name] = (uint32_t)sequence.length();
    chr_to_seq[name] = std::move(sequence);
    std::sort(chromosomes.begin(), chromosomes.end());
}

int ReferenceGenome::setFilepath(std::string path)
{
    if (path == "") {
        std::cout << "No FASTA filepath provided" << std::endl;
        return 1;
    }
    fasta_filepath = path;
    FileMap file(path);
    loadHost(file.p, file.n);
    return 0;
}

void ReferenceGenome::loadHost(const char *text, size_t n)
{
    // Line semantics of std::getline (:40): split on '\n' only, a final unterminated line counts, '\r' stays in the data.
    // The pending sequence is cleared only when a named contig is stored (:46-53), so residues in front of the first
    // header or under an empty-named header run into the next named contig, as they do in the reference.
    std::string current_chr, sequence;
    auto store = [&] {
        chromosomes.push_back(current_chr);
        chr_to_length[current_chr] = (uint32_t)sequence.length();
        chr_to_seq[current_chr] = std::move(sequence);
        sequence.clear();
    };
    const char *cur = text, *end = text + n;
    while (cur < end) {
        const char *nl = (const char *)memchr(cur, '\n', (size_t)(end - cur));
        const char *eol = nl ? nl : end;
        if (eol > cur && *cur == '>') {
            if (current_chr != "") store();
            const char *sp = (const char *)memchr(cur + 1, ' ', (size_t)(eol - cur - 1));   // description starts at the first blank (:58-62)
            current_chr.assign(cur + 1, sp ? sp : eol);
        } else {
            sequence.append(cur, eol);
        }
        cur = nl ? nl + 1 : end;
    }
    if (current_chr != "") store();
    std::sort(chromosomes.begin(), chromosomes.end());
}

int ReferenceGenome::setFilepath(std::string path, const FastaDeviceOptions &opt)
{
    if (!opt.ctx) return setFilepath(path);
    if (path == "") {
        std::cout << "No FASTA filepath provided" << std::endl;
        return 1;
    }
    fasta_filepath = path;
    FileMap file(path);
    // the mapped file up in windows; the reserve is the file's size, so the base array never grows
    const uint64_t window = std::min<uint64_t>(opt.window_bytes ? opt.window_bytes : kDefaultWindow, 0xffffffffull);
    std::unique_ptr<Device> d(new Device());
    d->ctx = opt.ctx;
    bool ok = false;
    csv_genome_counts c{};
    std::vector<uint64_t> name_off;
    std::vector<uint32_t> length;
    std::string names;
    if (csv_genome_builder *b = csvgpu_genome_builder_create(opt.ctx, file.n)) {
        ok = true;
        for (uint64_t off = 0; ok && off < file.n; off += window)
            ok = csvgpu_genome_builder_append(opt.ctx, b, (const uint8_t *)file.p + off, std::min<uint64_t>(window, file.n - off)) == CSV_OK;
        if (ok) { d->g = csvgpu_genome_builder_finish(opt.ctx, b); ok = d->g != nullptr; }      // (consumes the builder, also on failure)
        else csvgpu_genome_builder_destroy(opt.ctx, b);
    }
    if (ok) {                                             // names and lengths: the first call sizes the second
        const int rc = csvgpu_genome_describe(opt.ctx, d->g, 0, 0, nullptr, nullptr, nullptr, &c);
        ok = rc == CSV_OK || rc == CSV_ECAPACITY;
        if (ok) {
            name_off.resize(c.n_records + 1); length.resize(c.n_records + 1); names.resize(c.n_name_bytes + 1);
            ok = csvgpu_genome_describe(opt.ctx, d->g, c.n_records, c.n_name_bytes, name_off.data(), &names[0], length.data(), &c) == CSV_OK;
        }
    }
    if (!ok) {                                            // the whole file on the host, as if the option were off
        printError(std::string("Reference genome: the device loader refused (") + csvgpu_last_error(opt.ctx) + "); loading on the host");
        d.reset();
        loadHost(file.p, file.n);
        load_stats = FastaDeviceStats{};
        load_stats.fallback = 1;
        return 0;
    }
    for (uint64_t i = 0; i < c.n_records; i++) {
        const std::string name = names.substr((size_t)name_off[i], (size_t)(name_off[i + 1] - name_off[i]));
        chromosomes.push_back(name);
        chr_to_length[name] = length[i];
        d->record[name] = (uint32_t)i;
    }
    std::sort(chromosomes.begin(), chromosomes.end());
    d->stats.bytes_uploaded = c.n_text_bytes; d->stats.lines = c.n_lines; d->stats.records = c.n_records; d->stats.bases = c.total_bases;
    dev = std::move(d);
    return 0;
}

std::string_view ReferenceGenome::query(const std::string &chr, uint32_t pos_start, uint32_t pos_end) const
{
    if (dev) {
        const uint32_t rec = dev->record.at(chr);
        uint32_t first = 0;
        const uint64_t off[2] = {0, fastacore::cut_len(chr_to_length.at(chr), pos_start, pos_end, first)};
        static thread_local std::string bytes;            // what the returned view points into
        bytes.resize((size_t)off[1]);
        dev->fetch(&rec, &pos_start, &pos_end, off, 1, false, &bytes[0]);
        return bytes;
    }
    pos_start--;                                  // uint32 wrap for 0 is part of the contract (:91-92)
    pos_end--;
    const std::string &sequence = chr_to_seq.at(chr);
    if (pos_end >= sequence.length() || pos_start > pos_end) return {};
    return std::string_view(sequence).substr(pos_start, (size_t)(pos_end - pos_start) + 1);
}

bool ReferenceGenome::compare(const std::string &chr, uint32_t pos_start, uint32_t pos_end, const std::string &compare_seq, float match_threshold) const
{
    std::string_view sub;
    if (dev) {
        (void)dev->record.at(chr);                        // (an unknown contig: std::out_of_range, as the host backing's map)
        const uint32_t length = chr_to_length.at(chr);
        if ((uint32_t)(pos_end - 1) >= length || (uint32_t)(pos_start - 1) >= (uint32_t)(pos_end - 1)) return false;
        sub = query(chr, pos_start, pos_end);
    } else {
        pos_start--;
        pos_end--;
        const std::string &sequence = chr_to_seq.at(chr);
        if (pos_end >= sequence.length() || pos_start >= pos_end) return false;
        sub = std::string_view(sequence).substr(pos_start, (size_t)(pos_end - pos_start) + 1);
    }
    if (sub.length() != compare_seq.length()) {
        printError("ERROR: Sequence lengths do not match for comparison");
        return false;
    }
    size_t matches = 0;
    for (size_t i = 0; i < sub.length(); i++) matches += sub[i] == compare_seq[i];
    return (float)matches / (float)sub.length() >= match_threshold;
}

void ReferenceGenome::queryMany(const std::string &chr, const std::vector<Cut> &cuts, bool mask, std::vector<std::string> &out) const
{
    out.assign(cuts.size(), std::string());
    if (cuts.empty()) return;
    if (!dev) {
        for (size_t i = 0; i < cuts.size(); i++) {
            out[i] = query(chr, cuts[i].pos_start, cuts[i].pos_end);
            if (mask) for (char &base : out[i]) base = (char)fastacore::mask_base((uint8_t)base);
        }
        return;
    }
    const uint32_t rec = dev->record.at(chr), length = chr_to_length.at(chr);
    const size_t n = cuts.size();
    std::vector<uint32_t> r(n, rec), ps(n), pe(n);
    std::vector<uint64_t> off(n + 1, 0);
    for (size_t i = 0; i < n; i++) {
        uint32_t first = 0;
        ps[i] = cuts[i].pos_start; pe[i] = cuts[i].pos_end;
        off[i + 1] = off[i] + fastacore::cut_len(length, ps[i], pe[i], first);
    }
    std::string bytes((size_t)off[n], '\0');
    dev->fetch(r.data(), ps.data(), pe.data(), off.data(), n, mask, &bytes[0]);
    for (size_t i = 0; i < n; i++) out[i] = bytes.substr((size_t)off[i], (size_t)(off[i + 1] - off[i]));
}

std::string ReferenceGenome::getContigHeader() const
{
    std::vector<std::string> names;
    names.reserve(chr_to_length.size());
    for (const auto &kv : chr_to_length) names.push_back(kv.first);               // (the key set of chr_to_seq, also where no sequence is held)
    std::sort(names.begin(), names.end());
    std::string out;
    for (const std::string &name : names)
        out += "##contig=<ID=" + name + ",length=" + std::to_string(dev ? (size_t)chr_to_length.at(name) : chr_to_seq.at(name).length()) + ">\n";
    if (!out.empty()) out.pop_back();             // the reference pops unconditionally (UB on an empty genome, :159)
    return out;
}

uint32_t ReferenceGenome::getChromosomeLength(std::string chr) const
{
    auto it = chr_to_length.find(chr);
    if (it == chr_to_length.end()) {
        printError("Length for chromosome " + chr + " not found in reference genome");
        return 0;
    }
    return it->second;
}
