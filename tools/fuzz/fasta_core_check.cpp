// fasta_core_check.cpp — the rules of the device's FASTA loader and of its cuts (contextsv_amd/csrc/fasta_core.hpp) against
// ReferenceGenome::setFilepath and ::query (host/fasta_query.cpp), on the CPU under AddressSanitizer + UBSan. A program of its own:
// `make -C contextsv_amd/csrc fasta-check` links it with host/fasta_query.cpp; tests/test_fasta_core.py writes the corpus and runs it.
//   fasta_core_check <corpus> <mutations per text> <seed> <scratch file>
// corpus: "FAST", u32 texts, then per text: u32 len, bytes. Every text and every byte-mutated copy of it lies in a heap block of exactly
// its size. Checked per text:
//   - the core fed whole: the records' names, lengths and sequences against the loader's chromosome list, lengths and whole-contig queries
//     (the last record of a name is the one the loader keeps), and the contig header's unique sorted names;
//   - cuts at and around every edge, and random ones, through cut_len against ::query; mask_base against the writer's table;
//   - the core fed in two pieces cut at every offset, and in three pieces (every pair of offsets for a text of up to 320 bytes and for a
//     mutated copy of up to 48; 200 random pairs beyond that), equal to the core fed whole. Each of these twice: through the sequential
//     walk (fastacore::feed), and through the device's route — every line slot of a piece decided on its own as kernels/fasta.hip decides
//     it, the header slots as events into fastacore::apply_piece, the function the builder runs.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <string_view>
#include <vector>

#include "../../contextsv_amd/csrc/fasta_core.hpp"
#include "../../contextsv_amd/csrc/host/fasta_query.h"
#include "../../include/csvgpu.h"

// host/fasta_query.cpp's opt-in device backing calls these; this program never takes it
extern "C" {
csv_genome_builder *csvgpu_genome_builder_create(csv_ctx *, uint64_t) { abort(); }
int csvgpu_genome_builder_append(csv_ctx *, csv_genome_builder *, const uint8_t *, uint64_t) { abort(); }
csv_genome *csvgpu_genome_builder_finish(csv_ctx *, csv_genome_builder *) { abort(); }
void csvgpu_genome_builder_destroy(csv_ctx *, csv_genome_builder *) { abort(); }
void csvgpu_genome_free(csv_ctx *, csv_genome *) { abort(); }
int csvgpu_genome_describe(csv_ctx *, const csv_genome *, uint64_t, uint64_t, uint64_t *, char *, uint32_t *, csv_genome_counts *) { abort(); }
int csvgpu_genome_fetch(csv_ctx *, const csv_genome *, const uint32_t *, const uint32_t *, const uint32_t *, const uint64_t *, uint64_t, int, char *) { abort(); }
const char *csvgpu_last_error(const csv_ctx *) { abort(); }
}

void printError(const std::string &m) { (void)m; }     // (the mirror's logger is not linked; unknown contigs are asked for on purpose)
void printMessage(const std::string &m) { (void)m; }

using namespace fastacore;

namespace {

long g_fail = 0, g_texts = 0, g_records = 0, g_cuts = 0, g_builds = 0;

void fail(const char *what, size_t text_no, long detail)
{
    if (g_fail++ < 20) fprintf(stderr, "FAIL %s: text %zu (%ld)\n", what, text_no, detail);
}

struct Built {
    std::vector<Record> rec;
    std::string seq;                                      // the kept bytes that belong to a record
    bool operator==(const Built &o) const
    {
        if (rec.size() != o.rec.size() || seq != o.seq) return false;
        for (size_t i = 0; i < rec.size(); i++)
            if (rec[i].name != o.rec[i].name || rec[i].start != o.rec[i].start || rec[i].end != o.rec[i].end) return false;
        return true;
    }
};

// One piece as the device decides it (kernels/fasta.hip): cut into line slots at its line ends, every slot decided on its own with the
// core's line_kind / name_span — slot 0 goes on with the open line and takes its kind from the carry —, the header slots' events in order,
// the residue slots' bytes kept; then fastacore::apply_piece, the function the builder runs on the device's events.
void feed_by_events(Assembler &a, uint64_t &kept, const uint8_t *text, size_t len, std::string &seq)
{
    if (len == 0) return;                                 // (the entry points return before anything runs)
    std::vector<uint32_t> ev_kept, ev_off, ev_len;
    std::vector<uint8_t> ev_blank, names;
    uint32_t piece_kept = 0, tail_len = 0;
    uint8_t tail_kind = LINE_RESIDUES;
    size_t start = 0;
    for (size_t slot = 0;; slot++) {
        const uint8_t *nl = (const uint8_t *)memchr(text + start, '\n', len - start);
        const size_t end = nl ? (size_t)(nl - text) : len, n = end - start;
        const bool cont = slot == 0 && a.mid_line;
        const uint8_t kind = cont ? a.kind : line_kind(text + start, n);
        if (kind == LINE_HEADER) {
            const size_t from = cont ? 0 : 1;
            bool blank = false;
            const uint32_t k = name_span(text + start + from, (uint32_t)(n - from), blank);
            ev_kept.push_back(piece_kept); ev_off.push_back((uint32_t)names.size()); ev_len.push_back(k); ev_blank.push_back(blank);
            names.insert(names.end(), text + start + from, text + start + from + k);
        } else {
            seq.append((const char *)text + start, n);
            piece_kept += (uint32_t)n;
        }
        if (!nl) { tail_len = (uint32_t)n; tail_kind = kind; break; }
        start = end + 1;
        if (start == len) { tail_len = 0; tail_kind = LINE_RESIDUES; break; }      // (the empty slot behind a final line end)
    }
    PieceEvents e;
    e.n_hdr = (uint32_t)ev_kept.size(); e.kept = ev_kept.data(); e.name_off = ev_off.data(); e.name_len = ev_len.data(); e.blank = ev_blank.data();
    e.names = names.data(); e.tail_len = tail_len; e.tail_kind = tail_kind;
    apply_piece(a, kept, e);
    kept += piece_kept;
}

// the text in the given pieces, each in a heap block of exactly its size; by_events: through the device's per-slot decisions and apply_piece
Built build(const uint8_t *text, size_t len, const std::vector<size_t> &cuts, bool by_events = false)
{
    Assembler a;
    uint64_t kept = 0;
    std::string seq;
    size_t from = 0;
    for (size_t k = 0; k <= cuts.size(); k++) {
        const size_t to = k < cuts.size() ? cuts[k] : len;
        std::unique_ptr<uint8_t[]> piece(new uint8_t[to - from]);
        memcpy(piece.get(), text + from, to - from);
        if (by_events) feed_by_events(a, kept, piece.get(), to - from, seq);
        else feed(a, kept, piece.get(), to - from, [&](const uint8_t *p, uint64_t n) { seq.append((const char *)p, (size_t)n); });
        from = to;
    }
    const uint64_t total = a.finish(kept);
    seq.resize((size_t)total);
    g_builds++;
    return Built{a.rec, seq};
}

const char kAmbiguous[] = "RYKMSWBDHV";

void check_text(const std::vector<uint8_t> &t, size_t no, std::mt19937_64 &rng, const char *scratch, size_t all_pairs_up_to)
{
    std::unique_ptr<uint8_t[]> exact(new uint8_t[t.size()]);
    if (!t.empty()) memcpy(exact.get(), t.data(), t.size());
    const uint8_t *text = exact.get();
    const size_t len = t.size();
    const Built whole = build(text, len, {});
    g_texts++;
    g_records += (long)whole.rec.size();

    FILE *f = fopen(scratch, "wb");
    if (!f || (len && fwrite(text, 1, len, f) != len)) { fprintf(stderr, "cannot write %s\n", scratch); exit(2); }
    fclose(f);
    ReferenceGenome g;
    g.setFilepath(scratch);

    // names, lengths, sequences
    std::vector<std::string> names;
    std::map<std::string, size_t> last;
    for (size_t i = 0; i < whole.rec.size(); i++) { names.push_back(whole.rec[i].name); last[whole.rec[i].name] = i; }
    std::sort(names.begin(), names.end());
    if (names != g.getChromosomes()) fail("chromosome list", no, (long)names.size());
    std::string header;
    for (const auto &kv : last) {
        const Record &r = whole.rec[kv.second];
        header += "##contig=<ID=" + kv.first + ",length=" + std::to_string(r.end - r.start) + ">\n";
    }
    if (!header.empty()) header.pop_back();
    if (header != g.getContigHeader()) fail("contig header", no, 0);
    if (whole.rec.empty() ? !whole.seq.empty() : whole.rec.back().end != whole.seq.size()) fail("the last record ends the kept bytes", no, 0);
    for (const auto &kv : last) {
        const Record &r = whole.rec[kv.second];
        const uint32_t L = (uint32_t)(r.end - r.start);
        if (g.getChromosomeLength(kv.first) != L) { fail("length", no, (long)kv.second); continue; }
        // cuts: the edges, then random ones
        std::vector<std::pair<uint32_t, uint32_t>> cuts = {{0, 0}, {0, 5}, {0, L}, {1, 0}, {1, 1}, {1, L}, {1, L + 1}, {2, 1}, {2, L}, {L, L}, {L, L + 1}, {L + 1, L + 1},
                                                           {1, 0xffffffffu}, {0xffffffffu, 0xffffffffu}, {0xffffffffu, 1}, {L - 1, L}, {L / 2, L}};
        for (int k = 0; k < 12; k++) cuts.emplace_back((uint32_t)(rng() % (L + 3)), (uint32_t)(rng() % (L + 3)));
        for (const auto &c : cuts) {
            uint32_t first = 0;
            const uint32_t n = cut_len(L, c.first, c.second, first);
            const std::string_view want = g.query(kv.first, c.first, c.second);
            g_cuts++;
            if (n != want.size() || (n && ((uint64_t)first + n > L || memcmp(whole.seq.data() + r.start + first, want.data(), n) != 0))) fail("cut", no, (long)c.first);
        }
    }
    bool threw = false;
    try { (void)g.query("\x01no such contig", 1, 2); } catch (const std::out_of_range &) { threw = true; }
    if (!threw) fail("unknown contig", no, 0);

    // pieces: the sequential walk, and the device's per-slot decisions with apply_piece
    if (!(build(text, len, {}, true) == whole)) fail("whole, by events", no, 0);
    for (size_t a = 0; a <= len; a++) {
        if (!(build(text, len, {a}) == whole)) fail("two pieces", no, (long)a);
        if (!(build(text, len, {a}, true) == whole)) fail("two pieces, by events", no, (long)a);
    }
    if (len <= all_pairs_up_to) {
        for (size_t a = 0; a <= len; a++)
            for (size_t b = a; b <= len; b++) {
                if (!(build(text, len, {a, b}) == whole)) fail("three pieces", no, (long)(a * 1000 + b));
                if (!(build(text, len, {a, b}, true) == whole)) fail("three pieces, by events", no, (long)(a * 1000 + b));
            }
    } else {
        for (int k = 0; k < 200; k++) {
            size_t a = (size_t)(rng() % (len + 1)), b = (size_t)(rng() % (len + 1));
            if (a > b) std::swap(a, b);
            if (!(build(text, len, {a, b}) == whole)) fail("three pieces", no, (long)(a * 1000 + b));
            if (!(build(text, len, {a, b}, true) == whole)) fail("three pieces, by events", no, (long)(a * 1000 + b));
        }
    }
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 5) { fprintf(stderr, "usage: fasta_core_check <corpus> <mutations per text> <seed> <scratch file>\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    std::vector<uint8_t> blob;
    uint8_t buf[65536];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;) blob.insert(blob.end(), buf, buf + n);
    fclose(f);
    const int n_mut = atoi(argv[2]);
    std::mt19937_64 rng((uint64_t)atoll(argv[3]));
    size_t at = 8;
    uint32_t n_texts = 0;
    if (blob.size() < 8 || memcmp(blob.data(), "FAST", 4) != 0) { fprintf(stderr, "not a corpus\n"); return 2; }
    memcpy(&n_texts, blob.data() + 4, 4);

    // the masking rule over every byte value
    for (int c = 0; c < 256; c++) {
        bool amb = false;
        for (const char *p = kAmbiguous; *p; p++) amb |= c == *p || c == *p + ('a' - 'A');
        if (mask_base((uint8_t)c) != (amb ? 'N' : c)) fail("mask_base", 0, c);
    }

    const uint8_t special[] = {'\n', '>', ' ', '\r', 'A', 0, '\n', '>'};
    for (uint32_t i = 0; i < n_texts; i++) {
        uint32_t len = 0;
        if (at + 4 > blob.size()) { fprintf(stderr, "corpus cut short\n"); return 2; }
        memcpy(&len, blob.data() + at, 4);
        at += 4;
        if (at + len > blob.size()) { fprintf(stderr, "corpus cut short\n"); return 2; }
        const std::vector<uint8_t> text(blob.begin() + (long)at, blob.begin() + (long)(at + len));
        at += len;
        check_text(text, i, rng, argv[4], 320);          // the texts themselves: every pair of offsets up to 320 bytes (the 300-byte feature text)
        for (int m = 0; m < n_mut && len > 0; m++) {          // a few bytes replaced by the bytes the rules turn on; sometimes one dropped or doubled
            std::vector<uint8_t> mt = text;
            const int k = 1 + (int)(rng() % 4);
            for (int j = 0; j < k; j++) mt[(size_t)(rng() % mt.size())] = special[rng() % sizeof special];
            const uint64_t how = rng() % 4;
            if (how == 0) mt.erase(mt.begin() + (long)(rng() % mt.size()));
            else if (how == 1) { const size_t p = (size_t)(rng() % mt.size()); mt.insert(mt.begin() + (long)p, mt[p]); }
            check_text(mt, i, rng, argv[4], 48);
        }
    }
    printf("fasta_core_check: %ld texts, %ld records, %ld cuts, %ld builds, %ld failures\n", g_texts, g_records, g_cuts, g_builds, g_fail);
    return g_fail ? 1 : 0;
}
