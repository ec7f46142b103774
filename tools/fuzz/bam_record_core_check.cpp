// bam_record_core_check.cpp — contextsv_amd/csrc/bam_record_core.hpp (the per-record decisions of the device's BAM record unpacking) on
// the CPU, under AddressSanitizer + UBSan, against the host reader. A program of its own, no GPU: built by
// `make -C contextsv_amd/csrc unpack-check`, driven by tests/test_bam_record_core.py, which writes the streams of tests/bam_unpack_inputs.py
// to a file.
//   usage: bam_record_core_check CORPUS SCRATCH_DIR [MUTANTS_PER_STREAM]
//   corpus: "BRC1", u32 count, then per stream: u32 len, the bytes of a BAM record stream (what follows a BAM header)
// Every stream, and byte-mutated copies of it (most mutations land in a record's first 40 bytes: the lengths and counts), goes two ways:
//   core   in a heap block of exactly len bytes, so that the sanitizer sees any byte outside it: the chain walked from offset 0, then
//          fields() on every record placed on one of the three contigs, in order;
//   host   written behind a three-contig header as a BGZF file and read by BamReader::readAll (unchanged host parser) in one batch.
// They must agree on accept or refuse — with the host's message for the core's reason — and, when both accept, on every placed record's
// pos, flag, mapq, CIGAR words (CG tags restored), sequence bytes and name.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <string>
#include <vector>

#include "../../contextsv_amd/csrc/bam_record_core.hpp"
#include "../../contextsv_amd/csrc/host/bam_io.h"

namespace brc = bam_record_core;

static const int kRefs = 3;

struct HostIn {                          // the buffer, every access checked against [0, n)
    const uint8_t *p;
    uint32_t n;
    void need(uint32_t off, uint32_t k) const
    {
        if ((uint64_t)off + k > n) { fprintf(stderr, "FAIL: the core read [%u, %u) of a %u-byte buffer\n", off, off + k, n); abort(); }
    }
    uint32_t u8(uint32_t off) const { need(off, 1); return p[off]; }
    uint32_t u16(uint32_t off) const { need(off, 2); return (uint32_t)p[off] | ((uint32_t)p[off + 1] << 8); }
    uint32_t u32(uint32_t off) const { need(off, 4); return (uint32_t)p[off] | ((uint32_t)p[off + 1] << 8) | ((uint32_t)p[off + 2] << 16) | ((uint32_t)p[off + 3] << 24); }
};

struct Rec { int32_t tid, pos; uint32_t flag, mapq; std::vector<uint32_t> cigar; std::vector<uint8_t> seq; std::string name; };

struct Offsets { std::vector<uint32_t> v; void put(uint32_t, uint32_t o) { v.push_back(o); } };

static const char *message_of(uint32_t reason)
{
    switch (reason) {
        case brc::R_SHORT: return "BAM: record shorter than its fixed fields";
        case brc::R_LONG: return "BAM: implausible record length";
        case brc::R_NEG_LSEQ: return "BAM: negative sequence length";
        case brc::R_FIELDS: return "BAM: record fields exceed the record length";
    }
    return "?";
}

// "" and the placed records, or the host's message for the refusal
static std::string core_parse(const std::vector<uint8_t> &buf, std::vector<Rec> &out, long &n_hops)
{
    const uint32_t n = (uint32_t)buf.size();
    std::unique_ptr<uint8_t[]> exact(new uint8_t[n ? n : 1]);
    if (n) memcpy(exact.get(), buf.data(), n);
    const HostIn in{exact.get(), n};
    Offsets offs;
    const brc::Walk w = brc::walk(in, 0, n, offs);
    n_hops += w.n;
    if (w.n != offs.v.size()) { fprintf(stderr, "FAIL: the walk counted %u records and handed out %zu\n", w.n, offs.v.size()); abort(); }
    for (size_t i = 1; i < offs.v.size(); i++) if (offs.v[i] - offs.v[i - 1] < brc::MIN_HOP) { fprintf(stderr, "FAIL: a hop shorter than %u bytes\n", brc::MIN_HOP); abort(); }
    if (w.reason != brc::R_OK) return message_of(w.reason);
    for (uint32_t o : offs.v) {
        const int32_t tid = brc::rec_tid(in, o);
        if (tid < 0 || tid >= kRefs) continue;
        brc::Fields f;
        const uint32_t bs = in.u32(o);
        const uint32_t why = brc::fields(in, o, bs, f);
        if (why != brc::R_OK) return message_of(why);
        // what the core names lies inside its record
        const uint64_t end = (uint64_t)o + 4 + bs;
        if ((uint64_t)f.cig_src + 4ull * f.cig_n > end || (uint64_t)f.seq_src + f.seq_n > end || (uint64_t)f.name_src + f.name_n > end) { fprintf(stderr, "FAIL: a range outside its record at %u\n", o); abort(); }
        Rec r;
        r.tid = f.tid; r.pos = f.pos; r.flag = f.flag; r.mapq = f.mapq;
        for (uint32_t k = 0; k < f.cig_n; k++) r.cigar.push_back(in.u32(f.cig_src + 4 * k));
        for (uint32_t k = 0; k < f.seq_n; k++) r.seq.push_back((uint8_t)in.u8(f.seq_src + k));
        for (uint32_t k = 0; k < f.name_n; k++) r.name.push_back((char)in.u8(f.name_src + k));
        out.push_back(std::move(r));
    }
    if (w.o != n) return "BAM: truncated record at end of file";
    return "";
}

static std::string host_parse(const std::vector<uint8_t> &buf, const std::string &path, std::vector<Rec> &out)
{
    {
        bgzf::Writer wr;
        std::string err;
        if (!wr.open(path, 1, 1, &err)) { fprintf(stderr, "cannot write %s: %s\n", path.c_str(), err.c_str()); exit(2); }
        std::vector<uint8_t> h = {'B', 'A', 'M', 1, 0, 0, 0, 0, (uint8_t)kRefs, 0, 0, 0};
        for (int r = 0; r < kRefs; r++) {
            const uint8_t ref[] = {3, 0, 0, 0, 'c', (uint8_t)('0' + r), 0, 0, 0, 0, 0x40};      // l_name 3, "c<r>", l_ref 2^30
            h.insert(h.end(), ref, ref + sizeof ref);
        }
        wr.append(h.data(), h.size());
        if (!buf.empty()) wr.append(buf.data(), buf.size());
        if (!wr.close(&err)) { fprintf(stderr, "cannot write %s: %s\n", path.c_str(), err.c_str()); exit(2); }
    }
    BamReader rd;
    if (!rd.open(path)) { fprintf(stderr, "FAIL: the host reader cannot open its own file: %s\n", rd.error().c_str()); exit(1); }
    BamReadOptions opt;
    opt.want_seq = opt.want_qnames = true;
    opt.threads = 2;
    opt.window_blocks = 1u << 20;                            // one batch: the host's checks in one order over the whole stream
    const bool ok = rd.readAll(opt, [&](BamShard &&s) {
        for (size_t i = 0; i < s.pos.size(); i++) {
            Rec r;
            r.tid = s.tid; r.pos = s.pos[i]; r.flag = s.flag[i]; r.mapq = s.mapq[i];
            r.cigar.assign(s.cigar.data() + s.cigar_off[i], s.cigar.data() + s.cigar_off[i + 1]);
            r.seq.assign(s.seq.data() + s.seq_off[i], s.seq.data() + s.seq_off[i + 1]);
            r.name = s.qnames[i];
            out.push_back(std::move(r));
        }
    });
    return ok ? "" : rd.error();
}

static uint32_t g_rng = 2463534242u;
static uint32_t rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 17; g_rng ^= g_rng << 5; return g_rng; }

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s CORPUS SCRATCH_DIR [MUTANTS_PER_STREAM]\n", argv[0]); return 2; }
    const int n_mut = argc > 3 ? atoi(argv[3]) : 150;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    char magic[4];
    uint32_t count = 0;
    if (fread(magic, 1, 4, f) != 4 || memcmp(magic, "BRC1", 4) != 0 || fread(&count, 4, 1, f) != 1) { fprintf(stderr, "bad corpus header\n"); return 2; }
    const std::string path = std::string(argv[2]) + "/brc_check.bam";
    long n_buffers = 0, n_accepted = 0, n_refused = 0, n_records = 0, n_hops = 0;
    int fail = 0;
    for (uint32_t s = 0; s < count; s++) {
        uint32_t len = 0;
        if (fread(&len, 4, 1, f) != 1) { fprintf(stderr, "corpus truncated at stream %u\n", s); return 2; }
        std::vector<uint8_t> intact(len);
        if (len && fread(intact.data(), 1, len, f) != len) { fprintf(stderr, "corpus truncated in stream %u\n", s); return 2; }
        std::vector<uint32_t> starts;                        // of the intact stream's records (mutations aim at their headers)
        for (uint32_t o = 0; (uint64_t)o + 4 <= len;) {
            const uint32_t bs = (uint32_t)intact[o] | ((uint32_t)intact[o + 1] << 8) | ((uint32_t)intact[o + 2] << 16) | ((uint32_t)intact[o + 3] << 24);
            if (bs < 32 || (uint64_t)o + 4 + bs > len) break;
            starts.push_back(o);
            o += 4 + bs;
        }
        for (int m = 0; m <= n_mut; m++) {
            std::vector<uint8_t> buf = intact;
            if (m > 0 && len) {
                if (m % 10 == 0) buf.resize(rnd() % len);                            // a cut
                const int flips = 1 + (int)(rnd() % 3);
                for (int k = 0; k < flips && !buf.empty(); k++) {
                    uint32_t at = rnd() % (uint32_t)buf.size();
                    if (!starts.empty() && rnd() % 10 < 6) at = starts[rnd() % starts.size()] + rnd() % 40;
                    if (at >= buf.size()) continue;
                    const uint32_t how = rnd() % 5;
                    buf[at] = how == 0 ? 0 : how == 1 ? 0xff : how == 2 ? (uint8_t)(buf[at] + 1) : how == 3 ? (uint8_t)(buf[at] ^ 0x80) : (uint8_t)rnd();
                }
            }
            n_buffers++;
            std::vector<Rec> a, b;
            const std::string core = core_parse(buf, a, n_hops), host = host_parse(buf, path, b);
            if (core != host) { fprintf(stderr, "FAIL: stream %u mutant %d: core \"%s\", host \"%s\"\n", s, m, core.c_str(), host.c_str()); fail++; continue; }
            if (!core.empty()) { n_refused++; continue; }
            n_accepted++;
            if (m == 0 && a.empty() && len) { fprintf(stderr, "FAIL: stream %u holds no placed record\n", s); fail++; }
            if (a.size() != b.size()) { fprintf(stderr, "FAIL: stream %u mutant %d: %zu records against the host's %zu\n", s, m, a.size(), b.size()); fail++; continue; }
            for (size_t i = 0; i < a.size(); i++) {
                n_records++;
                if (a[i].tid != b[i].tid || a[i].pos != b[i].pos || a[i].flag != b[i].flag || a[i].mapq != b[i].mapq || a[i].cigar != b[i].cigar || a[i].seq != b[i].seq ||
                    a[i].name != b[i].name) { fprintf(stderr, "FAIL: stream %u mutant %d: record %zu differs from the host's\n", s, m, i); fail++; break; }
            }
        }
    }
    fclose(f);
    remove(path.c_str());
    printf("bam_record_core_check: %ld buffers, %ld accepted, %ld refused, %ld records, %ld hops, %d failures\n", n_buffers, n_accepted, n_refused, n_records, n_hops, fail);
    return fail ? 1 : 0;
}
