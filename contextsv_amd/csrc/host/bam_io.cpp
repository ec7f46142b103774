#include "bam_io.h"

#include <algorithm>
#include <cstring>
#include <future>
#include <map>
#include <thread>

namespace {
inline uint16_t le16(const uint8_t *p) { return (uint16_t)(p[0] | (p[1] << 8)); }
inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint64_t le64(const uint8_t *p) { return (uint64_t)le32(p) | ((uint64_t)le32(p + 4) << 32); }
inline void put16(std::vector<uint8_t> &v, uint16_t x) { v.push_back((uint8_t)x); v.push_back((uint8_t)(x >> 8)); }
inline void put32(std::vector<uint8_t> &v, uint32_t x) { for (int i = 0; i < 4; i++) v.push_back((uint8_t)(x >> (8 * i))); }
inline void put64(std::vector<uint8_t> &v, uint64_t x) { for (int i = 0; i < 8; i++) v.push_back((uint8_t)(x >> (8 * i))); }

constexpr uint32_t OP_S = 4, OP_N = 3;
constexpr int kPseudoBin = 37450;
constexpr int kLinearShift = 14;

// Locate the CG:B,I array among the auxiliary fields (bam_aux_get + the checks of htslib's bam_tag2cigar).
// Returns the element pointer and count, or nullptr.
const uint8_t *find_cg(const uint8_t *aux, const uint8_t *end, uint32_t *count)
{
    const uint8_t *p = aux;
    while (p + 3 <= end) {
        const bool is_cg = p[0] == 'C' && p[1] == 'G';
        const uint8_t type = p[2];
        p += 3;
        size_t len;
        switch (type) {
            case 'A': case 'c': case 'C': len = 1; break;
            case 's': case 'S': len = 2; break;
            case 'i': case 'I': case 'f': len = 4; break;
            case 'd': len = 8; break;
            case 'Z': case 'H': {
                const uint8_t *z = (const uint8_t *)memchr(p, 0, (size_t)(end - p));
                if (!z) return nullptr;
                len = (size_t)(z - p) + 1;
                break;
            }
            case 'B': {
                if (p + 5 > end) return nullptr;
                const uint8_t sub = p[0];
                const uint32_t n = le32(p + 1);
                size_t es;
                switch (sub) { case 'c': case 'C': es = 1; break; case 's': case 'S': es = 2; break; case 'i': case 'I': case 'f': es = 4; break; default: return nullptr; }
                if ((size_t)(end - p - 5) < (size_t)n * es) return nullptr;
                if (is_cg) {
                    if (sub != 'I' && sub != 'i') return nullptr;
                    *count = n;
                    return p + 5;
                }
                len = 5 + (size_t)n * es;
                break;
            }
            default: return nullptr;
        }
        if (is_cg) return nullptr;                     // a CG tag of another type is not a CIGAR
        if ((size_t)(end - p) < len) return nullptr;
        p += len;
    }
    return nullptr;
}
}  // namespace

int32_t bam_ref_len(const uint32_t *cigar, uint32_t n_cigar)
{
    // M, D, N, =, X consume the reference (bam_cigar_type bit 2: 0x3C1A7 >> (op << 1) & 2)
    int32_t l = 0;
    for (uint32_t i = 0; i < n_cigar; i++)
        if ((0x3C1A7u >> ((cigar[i] & 15) << 1)) & 2) l += (int32_t)(cigar[i] >> 4);
    return l;
}

int bam_reg2bin(int64_t beg, int64_t end)
{
    --end;
    if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

int BamHeader::tid(const std::string &name) const
{
    for (size_t i = 0; i < names.size(); i++) if (names[i] == name) return (int)i;
    return -1;
}

csv_reads BamShard::view() const
{
    csv_reads r{};
    r.n_reads = pos.size();
    r.n_cigar = cigar.size();
    r.pos = pos.data(); r.flag = flag.data(); r.mapq = mapq.data(); r.tid = nullptr;
    r.cigar_off = cigar_off.data(); r.cigar = cigar.data();
    return r;
}

void BamShard::clear()
{
    pos.clear(); flag.clear(); mapq.clear(); cigar.clear(); seq.clear(); qnames.clear();
    resident.reset(); resident_cigar = 0;
    cigar_off.assign(1, 0);
    seq_off.assign(1, 0);
}

// ---- BAI -----------------------------------------------------------------------------------------------
struct BamReader::Index {
    struct Ref {
        bool any = false; uint64_t min_beg = ~0ull, max_end = 0;
        std::vector<uint64_t> anchors;     // chunk begins and linear-index offsets, ascending: virtual offsets that CLAIM to be record starts (device_unpack's hints)
    };
    std::vector<Ref> refs;
};

BamReader::BamReader() = default;
BamReader::~BamReader() = default;

bool BamReader::open(const std::string &p)
{
    path = p;
    if (!file.open(p, &err)) return false;
    if (file.size() == 0) { err = "BAM: empty file " + p; return false; }
    // The header is read block by block (it is small); remember where the first record starts.
    std::vector<uint8_t> text;
    uint64_t coff = 0;
    std::vector<uint64_t> block_start;         // uncompressed offset -> block bookkeeping for the first-record voffset
    std::vector<uint64_t> block_coff;
    auto need = [&](size_t n) -> bool {
        while (text.size() < n) {
            if (coff >= file.size()) { err = "BAM: truncated header in " + p; return false; }
            bgzf::Block b;
            if (!bgzf::parse_block(file.data() + coff, file.size() - coff, coff, b, &err)) return false;
            block_start.push_back(text.size());
            block_coff.push_back(coff);
            const size_t at = text.size();
            text.resize(at + b.isize);
            if (!bgzf::inflate_block(file.data(), b, text.data() + at, &err)) return false;
            coff += b.csize;
        }
        return true;
    };
    if (!need(12)) return false;
    if (memcmp(text.data(), "BAM\1", 4) != 0) { err = "BAM: bad magic in " + p; return false; }
    const uint32_t l_text = le32(text.data() + 4);
    if (!need(12 + (size_t)l_text)) return false;
    hdr.text.assign((const char *)text.data() + 8, l_text);
    while (!hdr.text.empty() && hdr.text.back() == '\0') hdr.text.pop_back();
    size_t o = 8 + (size_t)l_text;
    const uint32_t n_ref = le32(text.data() + o);
    o += 4;
    for (uint32_t i = 0; i < n_ref; i++) {
        if (!need(o + 4)) return false;
        const uint32_t l_name = le32(text.data() + o);
        if (!need(o + 4 + (size_t)l_name + 4)) return false;
        std::string name((const char *)text.data() + o + 4, l_name ? l_name - 1 : 0);
        hdr.names.push_back(name);
        hdr.lens.push_back(le32(text.data() + o + 4 + l_name));
        o += 8 + (size_t)l_name;
    }
    // o = uncompressed offset of the first record
    size_t bi = block_start.size() - 1;
    while (bi > 0 && block_start[bi] > o) bi--;
    if (o == text.size()) first_record_voffset = bgzf::voffset(coff, 0);       // starts with the next block
    else first_record_voffset = bgzf::voffset(block_coff[bi], (uint32_t)(o - block_start[bi]));
    return true;
}

bool BamReader::loadIndex(const std::string &index_path)
{
    std::vector<std::string> candidates;
    if (!index_path.empty()) candidates.push_back(index_path);
    else {
        candidates.push_back(path + ".bai");
        if (path.size() > 4 && path.compare(path.size() - 4, 4, ".bam") == 0) candidates.push_back(path.substr(0, path.size() - 4) + ".bai");
    }
    bgzf::MappedFile f;
    bool ok = false;
    std::string e;
    for (const std::string &c : candidates) if (f.open(c, &e)) { ok = true; break; }
    if (!ok) { err = "BAM: could not load index for " + path; return false; }
    const uint8_t *p = f.data();
    const size_t n = f.size();
    if (n < 8 || memcmp(p, "BAI\1", 4) != 0) { err = "BAI: bad magic"; return false; }
    auto idx = std::make_unique<Index>();
    const uint32_t n_ref = le32(p + 4);
    size_t o = 8;
    if ((uint64_t)n_ref * 8 > n - 8) { err = "BAI: truncated"; return false; }      // (every reference has at least its two counts: found by tools/fuzz — a flipped count asked for 2^32 entries)
    idx->refs.resize(n_ref);
    for (uint32_t r = 0; r < n_ref; r++) {
        if (o + 4 > n) { err = "BAI: truncated"; return false; }
        const uint32_t n_bin = le32(p + o);
        o += 4;
        for (uint32_t b = 0; b < n_bin; b++) {
            if (o + 8 > n) { err = "BAI: truncated"; return false; }
            const uint32_t bin = le32(p + o), n_chunk = le32(p + o + 4);
            o += 8;
            if (o + 16ull * n_chunk > n) { err = "BAI: truncated"; return false; }
            if (bin != (uint32_t)kPseudoBin) {
                for (uint32_t c = 0; c < n_chunk; c++) {
                    const uint64_t beg = le64(p + o + 16ull * c), end = le64(p + o + 16ull * c + 8);
                    idx->refs[r].any = true;
                    idx->refs[r].min_beg = std::min(idx->refs[r].min_beg, beg);
                    idx->refs[r].max_end = std::max(idx->refs[r].max_end, end);
                    idx->refs[r].anchors.push_back(beg);
                }
            }
            o += 16ull * n_chunk;
        }
        if (o + 4 > n) { err = "BAI: truncated"; return false; }
        const uint32_t n_intv = le32(p + o);
        const size_t lin = o + 4;
        o += 4 + 8ull * n_intv;
        if (o > n) { err = "BAI: truncated"; return false; }
        // (the values size nothing and are believed nowhere: unpackBatch holds each against the batch's block table, the device against the record chain)
        std::vector<uint64_t> &a = idx->refs[r].anchors;
        for (uint32_t k = 0; k < n_intv; k++) a.push_back(le64(p + lin + 8ull * k));
        std::sort(a.begin(), a.end());
        a.erase(std::unique(a.begin(), a.end()), a.end());
    }
    index = std::move(idx);
    return true;
}

namespace {
// run fn(t) for t in [0, nt) on nt threads (the caller's included)
template <class F>
void parallel_chunks(int nt, F fn)
{
    if (nt <= 1) { fn(0); return; }
    std::vector<std::thread> pool;
    for (int t = 1; t < nt; t++) pool.emplace_back(fn, t);
    fn(0);
    for (auto &t : pool) t.join();
}
}  // namespace

// The device library's entry points where it is linked (the stand-alone check programs build without it: no device route there)
extern "C" {
__attribute__((weak)) int csvgpu_bam_unpack_dev(csv_ctx *ctx, const uint8_t *d_bytes, uint64_t len, const uint32_t *anchors, uint32_t n_anchors, int32_t tid, int64_t end,
                                                uint64_t cigar_base, uint64_t seq_base, uint64_t name_base, const csv_bam_out *d_out, csv_bam_counts *counts);
__attribute__((weak)) int csvgpu_bgzf_inflate_dev(csv_ctx *ctx, const uint8_t *d_comp, uint64_t comp_len, const csv_bgzf_block *blocks, uint32_t n_blocks, uint8_t *d_out,
                                                  uint64_t out_len, uint8_t *d_status);
__attribute__((weak)) void *csvgpu_dev_alloc(csv_ctx *ctx, size_t bytes);
__attribute__((weak)) void csvgpu_dev_free(csv_ctx *ctx, void *dev_ptr);
__attribute__((weak)) int csvgpu_upload(csv_ctx *ctx, void *dev_dst, const void *host_src, size_t bytes);
__attribute__((weak)) int csvgpu_download(csv_ctx *ctx, void *host_dst, const void *dev_src, size_t bytes);
__attribute__((weak)) const char *csvgpu_last_error(const csv_ctx *ctx);
__attribute__((weak)) csv_shard_builder *csvgpu_shard_builder_create(csv_ctx *ctx, uint32_t want, const csv_shard_sizes *reserve);
__attribute__((weak)) int csvgpu_shard_builder_append_bam(csv_ctx *ctx, csv_shard_builder *b, const uint8_t *d_bytes, uint64_t len, const uint32_t *anchors,
                                                          uint32_t n_anchors, int32_t tid, int64_t end, csv_bam_counts *counts);
__attribute__((weak)) int csvgpu_shard_builder_append_host(csv_ctx *ctx, csv_shard_builder *b, const csv_reads *batch, const uint64_t *seq_off, const uint8_t *seq,
                                                           const uint64_t *name_off, const uint8_t *name, const uint64_t *name_hash);
__attribute__((weak)) csv_shard *csvgpu_shard_builder_finish(csv_ctx *ctx, csv_shard_builder *b, uint32_t depth_len);
__attribute__((weak)) void csvgpu_shard_builder_destroy(csv_ctx *ctx, csv_shard_builder *b);
__attribute__((weak)) int csvgpu_shard_sizes(csv_ctx *ctx, const csv_shard *shard, csv_shard_sizes *out);
__attribute__((weak)) int csvgpu_shard_fetch_reads(csv_ctx *ctx, csv_shard *shard, int32_t *pos, uint16_t *flag, uint8_t *mapq, uint64_t *cigar_off, uint32_t *cigar);
__attribute__((weak)) int csvgpu_shard_fetch_names(csv_ctx *ctx, csv_shard *shard, uint64_t *name_off, uint8_t *name, uint64_t *name_hash);
__attribute__((weak)) void csvgpu_shard_free(csv_ctx *ctx, csv_shard *shard);
}

void BamShard::ResidentFree::operator()(csv_shard *s) const { if (s && ctx && csvgpu_shard_free) csvgpu_shard_free(ctx, s); }

// Device memory of one stream() with BamReadOptions::device_unpack: the batch's decoded bytes behind kDevHead bytes of room for the carried
// partial record, the compressed bytes + status bytes of the device inflate, and the unpacked arrays. Grown when needed, freed with the stream.
struct BamReader::DevBufs {
    csv_ctx *ctx = nullptr;
    struct Buf { uint8_t *p = nullptr; size_t cap = 0; } bytes, comp, out;
    ~DevBufs() { for (Buf *b : {&bytes, &comp, &out}) if (b->p && csvgpu_dev_free) csvgpu_dev_free(ctx, b->p); }
    bool ensure(Buf &b, size_t need, std::string &err)
    {
        if (need <= b.cap) return true;
        if (b.p) csvgpu_dev_free(ctx, b.p);
        b.cap = need + need / 4 + 4096;
        b.p = (uint8_t *)csvgpu_dev_alloc(ctx, b.cap);
        if (!b.p) { b.cap = 0; err = std::string("BAM: no device memory for the batch: ") + csvgpu_last_error(ctx); return false; }
        return true;
    }
};
static const size_t kDevHead = 1 << 20;

// Decompressed record stream from a virtual offset: batches of blocks are inflated by the pool while the previous batch is parsed.
bool BamReader::stream(uint64_t start_voffset, const BamReadOptions &opt, const std::function<size_t(const RecRef *, size_t)> &on_batch, const RawFn &on_raw)
{
    struct Batch {
        std::vector<bgzf::Block> blocks; HugeVec<uint8_t> data; size_t head = 0; bool ok = true; std::string err; uint64_t next_coff = 0;
        bool resident = false;       // the decoded bytes are in dev.bytes at kDevHead, not in `data` (device inflate straight into the unpack's buffer)
        size_t total = 0;
    };
    // device_unpack: a batch's bytes go to the reader's device buffer and the arrays come back from there. With the inflate on the same
    // context the members are inflated straight into that buffer (kernel to kernel): the bytes come down only when the device declines the batch.
    const bool dev_route = on_raw && opt.device_unpack && csvgpu_dev_alloc && csvgpu_upload && csvgpu_download;
    const bool chain = dev_route && opt.device_inflate == opt.device_unpack && csvgpu_bgzf_inflate_dev;
    DevBufs dev;
    dev.ctx = opt.device_unpack;
    // the batch's members inflated on the device into dev.bytes; what the device declines is decoded on the host (bgzf::inflate_block: the
    // fast decoder, then zlib, the CRC behind either — the host route's messages) and copied into place
    auto load_chain = [&](Batch &b, uint64_t total) -> bool {
        const size_t n = b.blocks.size();
        b.resident = true; b.total = (size_t)total;
        b.data.clear();
        if (n == 0) return true;
        const uint64_t base = b.blocks[0].coffset;
        std::vector<csv_bgzf_block> tab(n);
        uint64_t acc = 0;
        for (size_t i = 0; i < n; i++) {
            const bgzf::Block &k = b.blocks[i];
            if (k.coffset < base || k.csize < (uint32_t)k.data_off + 8) { b.err = "BGZF: block table out of order at offset " + std::to_string(k.coffset); return false; }
            tab[i] = csv_bgzf_block{k.coffset - base + k.data_off, acc, k.csize - k.data_off - 8, k.isize, le32(file.data() + k.coffset + k.csize - 8), 0};
            acc += k.isize;
        }
        const uint64_t span = b.blocks[n - 1].coffset + b.blocks[n - 1].csize - base;
        if (!dev.ensure(dev.bytes, kDevHead + (size_t)total + 8, b.err) || !dev.ensure(dev.comp, (size_t)span + 256 + n, b.err)) return false;
        uint8_t *const d_status = dev.comp.p + (((size_t)span + 255) & ~(size_t)255);
        int rc = csvgpu_upload(dev.ctx, dev.comp.p, file.data() + base, (size_t)span);
        if (rc == 0) rc = csvgpu_bgzf_inflate_dev(dev.ctx, dev.comp.p, span, tab.data(), (uint32_t)n, dev.bytes.p + kDevHead, std::max<uint64_t>(total, 1), d_status);
        if (rc < 0) { b.err = std::string("BGZF: device inflate failed: ") + csvgpu_last_error(dev.ctx); return false; }
        if (rc == 0) return true;
        std::vector<uint8_t> status(n), tmp(bgzf::kMaxBlock);
        if (csvgpu_download(dev.ctx, status.data(), d_status, n)) { b.err = std::string("BGZF: device inflate failed: ") + csvgpu_last_error(dev.ctx); return false; }
        for (size_t i = 0; i < n; i++) {
            if (!status[i]) continue;
            if (!bgzf::inflate_block(file.data(), b.blocks[i], tmp.data(), &b.err)) return false;
            if (csvgpu_upload(dev.ctx, dev.bytes.p + kDevHead + tab[i].out_off, tmp.data(), b.blocks[i].isize)) { b.err = std::string("BGZF: device inflate failed: ") + csvgpu_last_error(dev.ctx); return false; }
        }
        return true;
    };
    const uint32_t W = std::max<uint32_t>(opt.window_blocks, 1);
    const size_t kHead = 1 << 20;                        // room in front of each batch for the carried partial record (grown when needed)
    auto load = [&](uint64_t coff, Batch &b, size_t head) {
        b.blocks.clear();
        b.ok = true;
        uint64_t total = 0;
        while (coff < file.size() && b.blocks.size() < W) {
            bgzf::Block blk;
            if (!bgzf::parse_block(file.data() + coff, file.size() - coff, coff, blk, &b.err)) { b.ok = false; return; }
            b.blocks.push_back(blk);
            total += blk.isize;
            coff += blk.csize;
        }
        b.next_coff = coff;
        b.head = head;
        b.resident = false; b.total = (size_t)total;
        if (chain) { if (!load_chain(b, total)) b.ok = false; return; }
        b.data.resize_uninit(head + total);
        const bool ok = opt.device_inflate ? bgzf::inflate_range_device(opt.device_inflate, file.data(), b.blocks, 0, b.blocks.size(), b.data.data() + head, opt.threads, &b.err)
                                           : bgzf::inflate_range(file.data(), b.blocks, 0, b.blocks.size(), b.data.data() + head, opt.threads, &b.err);
        if (!ok) b.ok = false;
    };
    Batch batch[2];
    uint64_t coff = start_voffset >> 16;
    size_t skip = (size_t)(start_voffset & 0xffff);
    if (coff >= file.size()) return true;
    load(coff, batch[0], kHead);
    int cur = 0;
    std::vector<uint8_t> carry;
    HugeVec<uint8_t> joined;                             // only when a carried record is larger than the head room
    std::vector<RecRef> recs;
    for (;;) {
        Batch &b = batch[cur];
        if (!b.ok) { err = b.err; return false; }
        if (b.blocks.empty()) break;
        std::future<void> ahead;
        const bool more = b.next_coff < file.size();
        // (one context serves one thread at a time: with the unpack on the inflate's context the next batch is loaded behind this one's unpack)
        const bool beside = !(on_raw && opt.device_inflate && opt.device_inflate == opt.device_unpack);
        if (more) ahead = std::async(beside ? std::launch::async : std::launch::deferred, load, b.next_coff, std::ref(batch[cur ^ 1]), kHead);
        auto fail = [&](const std::string &m) { err = m; if (more) ahead.get(); return false; };
        // records of this batch = carried bytes + inflated bytes
        uint8_t *p = nullptr;
        size_t n = 0;
        const size_t skipped = skip, carried = carry.size();
        if (skip > b.total) return fail("BAM: virtual offset beyond its block");
        // the bytes of a resident batch brought to the host (the device declined the batch, or the carried record is larger than the room)
        auto materialize = [&]() -> bool {
            if (!b.resident) return true;
            b.data.resize_uninit(b.head + b.total);
            if (b.total && csvgpu_download(dev.ctx, b.data.data() + b.head, dev.bytes.p + kDevHead, b.total)) { err = std::string("BAM: device unpack failed: ") + csvgpu_last_error(dev.ctx); return false; }
            b.resident = false;
            unpack_stats.batches_downloaded++;
            return true;
        };
        auto assemble = [&] {                            // on the host: p[0, n)
            p = b.data.data() + b.head + skip;
            n = b.total - skip;
            skip = 0;
            if (!carry.empty()) {
                if (carry.size() <= (size_t)(p - b.data.data())) { p -= carry.size(); memcpy(p, carry.data(), carry.size()); n += carry.size(); }
                else {
                    joined.clear();
                    joined.append(carry.data(), carry.size());
                    joined.append(p, n);
                    p = joined.data(); n = joined.size();
                }
                carry.clear();
            }
        };
        if (dev_route) {
            // on the device: d[0, dn) = the carried bytes in the room in front + the batch's bytes from `skip` on
            const size_t dn = carried + b.total - skip;
            const bool fits = carried <= kDevHead;
            uint8_t *d = nullptr;
            bool up = fits;
            if (fits && !b.resident) up = dev.ensure(dev.bytes, kDevHead + b.total + 8, err) && csvgpu_upload(dev.ctx, dev.bytes.p + kDevHead, b.data.data() + b.head, b.total) == 0;
            if (fits && up && carried) up = csvgpu_upload(dev.ctx, dev.bytes.p + kDevHead + skip - carried, carry.data(), carried) == 0;
            if (fits && !up) { if (err.empty()) err = std::string("BAM: device unpack failed: ") + csvgpu_last_error(dev.ctx); if (more) ahead.get(); return false; }
            if (fits) d = dev.bytes.p + kDevHead + skip - carried;
            int took = 0;
            size_t consumed = 0;
            bool stop = false;
            if (!d) unpack_stats.batches_host++;             // (a carried record larger than the room: the host parser)
            if (d) took = on_raw(RawBatch{d, dn, carried, skipped, &b.blocks, &dev}, &consumed, &stop);
            if (took < 0) { if (more) ahead.get(); return false; }
            if (took > 0) {
                if (b.resident && dn) unpack_stats.batches_kept_on_device++;      // (an empty batch — the EOF marker alone — is nobody's)
                if (stop) { if (more && beside) ahead.get(); return err.empty(); }       // (a deferred load that nobody waits for never runs)
                skip = 0;
                carry.resize(dn - consumed);
                if (dn > consumed && csvgpu_download(dev.ctx, carry.data(), d + consumed, dn - consumed)) return fail(std::string("BAM: device unpack failed: ") + csvgpu_last_error(dev.ctx));
                if (!more) break;
                ahead.get();
                cur ^= 1;
                continue;
            }
            if (!materialize()) { if (more) ahead.get(); return false; }
        }
        assemble();
        recs.clear();
        size_t o = 0;
        while (o + 4 <= n) {
            const uint32_t bs = le32(p + o);
            if (bs < 32) return fail("BAM: record shorter than its fixed fields");
            if (bs > (1u << 30)) return fail("BAM: implausible record length");
            if (o + 4 + (size_t)bs > n) break;
            recs.push_back(RecRef{p + o + 4, bs});
            o += 4 + (size_t)bs;
        }
        const size_t took = on_batch(recs.data(), recs.size());
        if (took < recs.size() || !err.empty()) { if (more) ahead.get(); return err.empty(); }
        carry.assign(p + o, p + n);
        if (!more) break;
        ahead.get();
        cur ^= 1;
    }
    if (!carry.empty()) { err = "BAM: truncated record at end of file"; return false; }
    return true;
}

// Records -> arrays: a serial pass sizes every record (and resolves CG-tag CIGARs), then the copies run on the pool.
bool BamReader::append(const RecRef *recs, size_t n, const BamReadOptions &opt, BamShard &out)
{
    if (n == 0) return true;
    struct Src { const uint8_t *cig; uint32_t n_cig; };
    std::vector<Src> src(n);
    const size_t r0 = out.pos.size();
    out.cigar_off.resize(r0 + 1 + n);
    if (opt.want_seq) out.seq_off.resize(r0 + 1 + n);
    uint64_t cig_at = out.cigar.size(), seq_at = out.seq.size();
    for (size_t i = 0; i < n; i++) {
        const uint8_t *rec = recs[i].p;
        const uint32_t len = recs[i].len;
        const uint32_t l_name = rec[8], n_cigar = le16(rec + 12);
        const int32_t l_seq = (int32_t)le32(rec + 16);
        if (l_seq < 0) { err = "BAM: negative sequence length"; return false; }
        const size_t fixed = 32 + (size_t)l_name + 4ull * n_cigar + ((size_t)l_seq + 1) / 2 + (size_t)l_seq;
        if (fixed > len) { err = "BAM: record fields exceed the record length"; return false; }
        const uint8_t *cig = rec + 32 + l_name;
        src[i] = Src{cig, n_cigar};
        // long CIGAR in the CG tag behind a <l_seq>S<n>N placeholder (bam_tag2cigar)
        if (n_cigar > 0 && (int32_t)le32(rec) >= 0 && (int32_t)le32(rec + 4) >= 0) {
            const uint32_t c0 = le32(cig);
            if ((c0 & 15) == OP_S && (int32_t)(c0 >> 4) == l_seq) {
                uint32_t cnt = 0;
                const uint8_t *cg = find_cg(rec + fixed, rec + len, &cnt);
                if (cg && cnt >= n_cigar && cnt < (1u << 29)) src[i] = Src{cg, cnt};
            }
        }
        cig_at += src[i].n_cig;
        out.cigar_off[r0 + 1 + i] = cig_at;
        if (opt.want_seq) { seq_at += ((size_t)l_seq + 1) / 2; out.seq_off[r0 + 1 + i] = seq_at; }
    }
    out.pos.resize(r0 + n);
    out.flag.resize(r0 + n);
    out.mapq.resize(r0 + n);
    out.cigar.resize_uninit(cig_at);
    if (opt.want_seq) out.seq.resize_uninit(seq_at);
    if (opt.want_qnames) out.qnames.resize(r0 + n);
    const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(opt.threads, 1), n / 256 + 1));
    parallel_chunks(nt, [&](int t) {
        const size_t a = n * (size_t)t / (size_t)nt, b = n * ((size_t)t + 1) / (size_t)nt;
        for (size_t i = a; i < b; i++) {
            const uint8_t *rec = recs[i].p;
            const size_t r = r0 + i;
            out.pos[r] = (int32_t)le32(rec + 4);
            out.mapq[r] = rec[9];
            out.flag[r] = le16(rec + 14);
            if (src[i].n_cig) memcpy(out.cigar.data() + out.cigar_off[r], src[i].cig, 4ull * src[i].n_cig);   // BAM is little-endian, as is the target
            const uint32_t l_name = rec[8];
            if (opt.want_seq) {
                const uint8_t *seq = rec + 32 + l_name + 4ull * le16(rec + 12);
                const size_t nb = (size_t)(out.seq_off[r + 1] - out.seq_off[r]);
                if (nb) memcpy(out.seq.data() + out.seq_off[r], seq, nb);
            }
            if (opt.want_qnames) out.qnames[r].assign((const char *)rec + 32, l_name ? strnlen((const char *)rec + 32, l_name) : 0);
        }
    });
    return true;
}

// One batch's records unpacked on the device and appended to `out` (BamReadOptions::device_unpack). The bytes are in the reader's device
// buffer already. The anchor candidates that lie in this batch are mapped from virtual offset to buffer offset through its block table; a
// sizing call gives the exact counts (CSV_ECAPACITY, the library's convention; the bytes stay where they are, only the chain, filter and
// field kernels run twice), the second call writes device arrays of exactly those sizes, and they are copied into the shard's arrays.
int BamReader::unpackBatch(const RawBatch &b, int tid, int64_t end, const std::vector<uint64_t> &candidates, const BamReadOptions &opt, BamShard &out, size_t *consumed, bool *stop)
{
    if (!csvgpu_bam_unpack_dev || !csvgpu_last_error) { err = "BAM: no device to unpack on"; return -1; }
    if (b.n == 0) { *consumed = 0; *stop = false; return 1; }
    if (b.n >= (1ull << 32)) { unpack_stats.batches_host++; return 0; }   // beyond the device's 32-bit offsets: the host parser
    std::vector<uint32_t> anchors(1, 0);                                  // d[0] is a record start: the carry's, or the stream's first
    {
        // block i's bytes start at buffer offset carried + (bytes of the blocks before it) - skip
        const std::vector<bgzf::Block> &bl = *b.blocks;
        size_t i = 0;
        uint64_t before = 0;
        auto it = bl.empty() ? candidates.end() : std::lower_bound(candidates.begin(), candidates.end(), bgzf::voffset(bl[0].coffset, 0));
        for (; it != candidates.end(); ++it) {
            const uint64_t coff = *it >> 16, uoff = *it & 0xffff;
            while (i < bl.size() && bl[i].coffset < coff) { before += bl[i].isize; i++; }
            if (i == bl.size()) break;
            if (bl[i].coffset != coff || uoff >= bl[i].isize) continue;   // not a block of this file, or beyond its bytes: not a hint
            const uint64_t at = b.carried + before + uoff;
            if (at <= b.skip + anchors.back() || at - b.skip >= b.n) continue;
            anchors.push_back((uint32_t)(at - b.skip));
        }
    }
    DevBufs &dev = *b.dev;
    auto dev_fail = [&] { err = std::string("BAM: device unpack failed: ") + csvgpu_last_error(opt.device_unpack); return -1; };
    if (shard_builder) {
        // BamReadOptions::device_shard: the records go behind the builder's tail where they are; nothing comes down
        csv_bam_counts c{};
        const int rc = csvgpu_shard_builder_append_bam(opt.device_unpack, shard_builder, b.d, b.n, anchors.data(), (uint32_t)anchors.size(), tid, end, &c);
        if (rc == 1) { unpack_stats.batches_host++; return 0; }          // declined, nothing appended: the host parser reads this batch
        if (rc != CSV_OK) return dev_fail();
        unpack_stats.batches_device++;
        unpack_stats.anchors += anchors.size();
        unpack_stats.records += c.n_kept;
        *consumed = (size_t)c.consumed;
        *stop = c.stopped != 0;
        return 1;
    }
    const size_t r0 = out.pos.size();
    const uint64_t cig_at = out.cigar.size(), seq_at = out.seq.size();
    if (!dev.ensure(dev.out, 4096, err)) return -1;
    csv_bam_out o{};
    csv_bam_counts c{};
    // sizing call: capacities of zero (with no record kept the three offset arrays still take their first entry: 8 bytes of scratch each)
    o.pos = (int32_t *)dev.out.p; o.flag = (uint16_t *)dev.out.p; o.mapq = dev.out.p; o.cigar = (uint32_t *)dev.out.p;
    o.cigar_off = (uint64_t *)(dev.out.p + 256);
    if (opt.want_seq) { o.seq_off = (uint64_t *)(dev.out.p + 512); o.seq = dev.out.p; }
    if (opt.want_qnames) { o.name_off = (uint64_t *)(dev.out.p + 768); o.name = dev.out.p; }
    int rc = csvgpu_bam_unpack_dev(opt.device_unpack, b.d, b.n, anchors.data(), (uint32_t)anchors.size(), tid, end, cig_at, seq_at, 0, &o, &c);
    if (rc == 1) { unpack_stats.batches_host++; return 0; }              // declined: the host parser reads this batch and words the refusal
    if (rc != CSV_OK && rc != CSV_ECAPACITY) return dev_fail();
    if (rc == CSV_ECAPACITY) {
        const size_t k = (size_t)c.n_kept;
        const csv_bam_counts sized = c;
        size_t at = 0;
        auto slot = [&](size_t bytes) { const size_t a = at; at += (bytes + 255) & ~(size_t)255; return a; };
        const size_t a_pos = slot(k * 4), a_flag = slot(k * 2), a_mapq = slot(k), a_coff = slot((k + 1) * 8), a_cig = slot(c.n_cigar * 4 + 4);
        const size_t a_soff = slot((k + 1) * 8), a_seq = slot(c.n_seq + 4), a_noff = slot((k + 1) * 8), a_name = slot(c.n_name + 4);
        if (!dev.ensure(dev.out, at, err)) return -1;
        uint8_t *const q = dev.out.p;
        o.pos = (int32_t *)(q + a_pos); o.flag = (uint16_t *)(q + a_flag); o.mapq = q + a_mapq; o.cigar_off = (uint64_t *)(q + a_coff); o.cigar = (uint32_t *)(q + a_cig);
        o.cap_records = k; o.cap_cigar = c.n_cigar;
        if (opt.want_seq) { o.seq_off = (uint64_t *)(q + a_soff); o.seq = q + a_seq; o.cap_seq = c.n_seq; }
        if (opt.want_qnames) { o.name_off = (uint64_t *)(q + a_noff); o.name = q + a_name; o.cap_name = c.n_name; }
        rc = csvgpu_bam_unpack_dev(opt.device_unpack, b.d, b.n, anchors.data(), (uint32_t)anchors.size(), tid, end, cig_at, seq_at, 0, &o, &c);
        if (rc < 0) return dev_fail();
        if (rc != CSV_OK || c.n_kept != sized.n_kept || c.n_cigar != sized.n_cigar || c.n_seq != sized.n_seq || c.n_name != sized.n_name) {
            err = "BAM: device unpack failed: the second call disagrees with the first";
            return -1;
        }
        // the arrays come down into the shard where they stand
        csv_ctx *const x = opt.device_unpack;
        out.pos.resize(r0 + k); out.flag.resize(r0 + k); out.mapq.resize(r0 + k);
        out.cigar_off.resize(r0 + 1 + k);
        out.cigar.resize_uninit(cig_at + c.n_cigar);
        unpack_stats.cigar_words_downloaded += c.n_cigar;
        if (csvgpu_download(x, out.pos.data() + r0, o.pos, k * 4) || csvgpu_download(x, out.flag.data() + r0, o.flag, k * 2) || csvgpu_download(x, out.mapq.data() + r0, o.mapq, k) ||
            csvgpu_download(x, out.cigar_off.data() + r0, o.cigar_off, (k + 1) * 8) || (c.n_cigar && csvgpu_download(x, out.cigar.data() + cig_at, o.cigar, c.n_cigar * 4))) return dev_fail();
        if (opt.want_seq) {
            out.seq_off.resize(r0 + 1 + k);
            out.seq.resize_uninit(seq_at + c.n_seq);
            if (csvgpu_download(x, out.seq_off.data() + r0, o.seq_off, (k + 1) * 8) || (c.n_seq && csvgpu_download(x, out.seq.data() + seq_at, o.seq, c.n_seq))) return dev_fail();
        }
        if (opt.want_qnames) {
            std::vector<uint64_t> name_off(k + 1);
            std::vector<uint8_t> name((size_t)c.n_name + 1);
            if (csvgpu_download(x, name_off.data(), o.name_off, (k + 1) * 8) || (c.n_name && csvgpu_download(x, name.data(), o.name, c.n_name))) return dev_fail();
            out.qnames.resize(r0 + k);
            for (size_t i = 0; i < k; i++) out.qnames[r0 + i].assign((const char *)name.data() + name_off[i], (size_t)(name_off[i + 1] - name_off[i]));
        }
    }
    unpack_stats.batches_device++;
    unpack_stats.anchors += anchors.size();
    unpack_stats.records += c.n_kept;
    *consumed = (size_t)c.consumed;
    *stop = c.stopped != 0;
    return 1;
}

bool BamReader::readContig(const std::string &chr, const BamReadOptions &opt, BamShard &out)
{
    err.clear();
    const int tid = hdr.tid(chr);
    if (tid < 0) { err = "BAM: unknown contig " + chr; return false; }
    if (!index) { err = "BAM: no index loaded for " + path; return false; }
    out.clear();
    unpack_stats = UnpackStats();
    out.tid = tid; out.name = chr; out.target_len = hdr.lens[tid];
    if ((size_t)tid >= index->refs.size() || !index->refs[tid].any) return true;
    const Index::Ref &ref = index->refs[tid];
    // size the big arrays once: the contig's compressed span bounds its records (BGZF rarely expands; CIGAR words dominate)
    // (offsets come from the index file: a corrupt one must not size an allocation — found by tools/fuzz)
    if ((ref.max_end >> 16) < (ref.min_beg >> 16) || (ref.min_beg >> 16) > file.size()) { err = "BAI: chunk offsets outside " + path; return false; }
    const uint64_t span = std::min<uint64_t>((ref.max_end >> 16) - (ref.min_beg >> 16), file.size()) + bgzf::kMaxBlock;
    const int64_t end = hdr.lens[tid];
    // BamReadOptions::device_shard: the contig's records are appended on the device to a builder held for this call; whatever way out is
    // taken, the builder does not outlive it
    struct BuilderGuard {
        BamReader &r; csv_ctx *ctx;
        ~BuilderGuard() { if (r.shard_builder) { csvgpu_shard_builder_destroy(ctx, r.shard_builder); r.shard_builder = nullptr; } }
    } guard{*this, opt.device_unpack};
    if (opt.device_shard) {
        if (!opt.device_unpack || !csvgpu_shard_builder_create || !csvgpu_shard_builder_append_bam || !csvgpu_shard_builder_append_host || !csvgpu_shard_builder_finish ||
            !csvgpu_shard_builder_destroy || !csvgpu_shard_sizes || !csvgpu_shard_fetch_reads || !csvgpu_shard_fetch_names || !csvgpu_shard_free || !csvgpu_last_error) {
            err = "BAM: device_shard needs device_unpack (and the device library)";
            return false;
        }
        // The reserve from the compressed span, like the host arrays' — but device memory is committed when it is allocated (the host's reserve
        // is address space only) and a finished shard keeps its blocks: as many bytes of CIGAR words as the span has compressed bytes, an
        // eighth of that for sequences; whatever a contig holds beyond it comes by growth (at least 1.5x a step).
        const csv_shard_sizes reserve{span / 256, span / 4, opt.want_seq ? span / 8 : 0, opt.want_qnames ? span / 64 : 0};
        shard_builder = csvgpu_shard_builder_create(opt.device_unpack, (opt.want_seq ? CSV_SB_SEQ : 0) | (opt.want_qnames ? CSV_SB_NAMES | CSV_SB_NAME_HASH : 0), &reserve);
        if (!shard_builder) { err = std::string("BAM: no shard builder: ") + csvgpu_last_error(opt.device_unpack); return false; }
    } else {
        out.cigar.reserve((size_t)(span * 4 / 4));        // ~4x compression of CIGAR words is typical; growth is by mremap anyway
    }
    RawFn on_raw;
    if (opt.device_unpack) on_raw = [&](const RawBatch &b, size_t *consumed, bool *stop) { return unpackBatch(b, tid, end, ref.anchors, opt, out, consumed, stop); };
    // a batch the host parser read, on the device_shard route: its arrays go up behind the builder's tail
    auto append_to_builder = [&](const RecRef *recs, size_t n) -> bool {
        BamShard part;
        part.clear();
        if (!append(recs, n, opt, part)) return false;
        std::vector<uint64_t> name_off, name_hash;
        std::vector<uint8_t> name;
        if (opt.want_qnames) {
            name_off.assign(1, 0);
            for (const std::string &q : part.qnames) {
                name.insert(name.end(), q.begin(), q.end());
                name_off.push_back(name.size());
                name_hash.push_back((uint64_t)std::hash<std::string>{}(q));
            }
            name.push_back(0);                            // (never a null array)
            name_hash.push_back(0);
        }
        const csv_reads v = part.view();
        if (csvgpu_shard_builder_append_host(opt.device_unpack, shard_builder, &v, opt.want_seq ? part.seq_off.data() : nullptr, opt.want_seq ? part.seq.data() : nullptr,
                                             opt.want_qnames ? name_off.data() : nullptr, opt.want_qnames ? name.data() : nullptr,
                                             opt.want_qnames ? name_hash.data() : nullptr) != CSV_OK) {
            err = std::string("BAM: device unpack failed: ") + csvgpu_last_error(opt.device_unpack);
            return false;
        }
        if (n) unpack_stats.batches_appended_host++;
        return true;
    };
    const bool ok = stream(ref.min_beg, opt, [&](const RecRef *recs, size_t n) -> size_t {
        // the contig's records are one run in a sorted file: skip an earlier contig's tail, stop at a later one / unplaced / past the end
        size_t a = 0;
        while (a < n && (int32_t)le32(recs[a].p) >= 0 && (int32_t)le32(recs[a].p) < tid) a++;
        size_t b = a;
        while (b < n && (int32_t)le32(recs[b].p) == tid && (int32_t)le32(recs[b].p + 4) < end) b++;
        if (!(shard_builder ? append_to_builder(recs + a, b - a) : append(recs + a, b - a, opt, out))) return 0;
        return b == n ? n : b;                            // anything left over ends the iteration
    }, on_raw) && err.empty();
    if (!ok || !shard_builder) return ok;
    // the builder becomes the contig's shard; the small per-record arrays come down for the host-side passes
    csv_ctx *const x = opt.device_unpack;
    csv_shard_builder *const done = shard_builder;
    shard_builder = nullptr;                              // (finish consumes it, also on failure)
    out.resident = std::unique_ptr<csv_shard, BamShard::ResidentFree>(csvgpu_shard_builder_finish(x, done, (uint32_t)hdr.lens[tid] + 1), BamShard::ResidentFree(x));
    auto fail = [&] { err = std::string("BAM: device unpack failed: ") + csvgpu_last_error(x); out.resident.reset(); return false; };
    if (!out.resident) return fail();
    csv_shard_sizes z{};
    if (csvgpu_shard_sizes(x, out.resident.get(), &z)) return fail();
    out.pos.resize(z.n_reads); out.flag.resize(z.n_reads); out.mapq.resize(z.n_reads);
    out.resident_cigar = z.n_cigar;
    if (csvgpu_shard_fetch_reads(x, out.resident.get(), out.pos.data(), out.flag.data(), out.mapq.data(), nullptr, nullptr)) return fail();
    if (opt.want_qnames) {
        std::vector<uint64_t> name_off(z.n_reads + 1);
        std::vector<uint8_t> name(z.n_name + 1);
        if (csvgpu_shard_fetch_names(x, out.resident.get(), name_off.data(), name.data(), nullptr)) return fail();
        out.qnames.resize(z.n_reads);
        for (uint64_t i = 0; i < z.n_reads; i++) out.qnames[i].assign((const char *)name.data() + name_off[i], (size_t)(name_off[i + 1] - name_off[i]));
    }
    unpack_stats.shard_resident = 1;
    return true;
}

bool BamReader::readAll(const BamReadOptions &opt, const std::function<void(BamShard &&)> &sink, uint64_t *n_unplaced)
{
    err.clear();
    BamShard cur;
    cur.clear();
    uint64_t unplaced = 0;
    auto flush = [&] {
        if (cur.tid >= 0 && cur.n_reads()) sink(std::move(cur));
        cur = BamShard();
        cur.clear();
    };
    const bool ok = stream(first_record_voffset, opt, [&](const RecRef *recs, size_t n) -> size_t {
        size_t i = 0;
        while (i < n) {
            const int32_t rtid = (int32_t)le32(recs[i].p);
            size_t j = i + 1;
            while (j < n && (int32_t)le32(recs[j].p) == rtid) j++;
            if (rtid < 0 || (size_t)rtid >= hdr.names.size()) unplaced += j - i;
            else {
                if (rtid != cur.tid) {
                    flush();
                    cur.tid = rtid; cur.name = hdr.names[rtid]; cur.target_len = hdr.lens[rtid];
                }
                if (!append(recs + i, j - i, opt, cur)) return 0;
            }
            i = j;
        }
        return n;
    }) && err.empty();
    if (ok) flush();
    if (n_unplaced) *n_unplaced = unplaced;
    return ok;
}

// ---- writer ------------------------------------------------------------------------------------------------
BamWriter::BamWriter() = default;
BamWriter::~BamWriter() = default;

bool BamWriter::open(const std::string &p, const BamHeader &header, int level, int threads)
{
    path = p;
    hdr = header;
    if (!out.open(p, level, threads, &err)) return false;
    std::vector<uint8_t> h;
    h.insert(h.end(), {'B', 'A', 'M', 1});
    put32(h, (uint32_t)hdr.text.size());
    h.insert(h.end(), hdr.text.begin(), hdr.text.end());
    put32(h, (uint32_t)hdr.names.size());
    for (size_t i = 0; i < hdr.names.size(); i++) {
        put32(h, (uint32_t)hdr.names[i].size() + 1);
        h.insert(h.end(), hdr.names[i].begin(), hdr.names[i].end());
        h.push_back(0);
        put32(h, hdr.lens[i]);
    }
    out.append(h.data(), h.size());
    opened = true;
    return true;
}

void BamWriter::add(int32_t tid, int32_t pos, uint8_t mapq, uint16_t flag, const std::string &qname, const uint32_t *cigar, uint32_t n_cigar,
                    const uint8_t *seq4, int32_t l_seq, const uint8_t *qual)
{
    const int32_t end = bam_end_pos(pos, flag, cigar, n_cigar);
    const bool long_cigar = n_cigar > 65535;
    const uint32_t l_name = (uint32_t)qname.size() + 1;
    rec.clear();
    put32(rec, 0);                                   // block_size, patched below
    put32(rec, (uint32_t)tid);
    put32(rec, (uint32_t)pos);
    rec.push_back((uint8_t)l_name);
    rec.push_back(mapq);
    put16(rec, (uint16_t)bam_reg2bin(pos, end));
    put16(rec, (uint16_t)(long_cigar ? 2 : n_cigar));
    put16(rec, flag);
    put32(rec, (uint32_t)l_seq);
    put32(rec, (uint32_t)-1);                        // next_refID
    put32(rec, (uint32_t)-1);                        // next_pos
    put32(rec, 0);                                   // tlen
    rec.insert(rec.end(), qname.begin(), qname.end());
    rec.push_back(0);
    if (long_cigar) {
        put32(rec, ((uint32_t)l_seq << 4) | OP_S);
        put32(rec, ((uint32_t)bam_ref_len(cigar, n_cigar) << 4) | OP_N);
    } else {
        const size_t at = rec.size();
        rec.resize(at + 4ull * n_cigar);
        if (n_cigar) memcpy(rec.data() + at, cigar, 4ull * n_cigar);
    }
    if (l_seq > 0) {
        rec.insert(rec.end(), seq4, seq4 + ((size_t)l_seq + 1) / 2);
        if (qual) rec.insert(rec.end(), qual, qual + l_seq);
        else rec.insert(rec.end(), (size_t)l_seq, (uint8_t)0xff);
    }
    if (long_cigar) {
        rec.insert(rec.end(), {'C', 'G', 'B', 'I'});
        put32(rec, n_cigar);
        const size_t at = rec.size();
        rec.resize(at + 4ull * n_cigar);
        memcpy(rec.data() + at, cigar, 4ull * n_cigar);
    }
    const uint32_t bs = (uint32_t)rec.size() - 4;
    rec[0] = (uint8_t)bs; rec[1] = (uint8_t)(bs >> 8); rec[2] = (uint8_t)(bs >> 16); rec[3] = (uint8_t)(bs >> 24);
    IndexEntry e;
    e.tid = tid; e.beg = pos; e.end = end; e.flag = flag;
    out.where(e.blk0, e.uo0);
    out.append(rec.data(), rec.size());
    out.where(e.blk1, e.uo1);
    entries.push_back(e);
    n_records++;
}

bool BamWriter::close()
{
    if (!opened) return true;
    opened = false;
    if (!out.close(&err)) return false;
    return writeIndex();
}

bool BamWriter::writeIndex()
{
    struct Chunk { uint64_t beg, end; };
    struct Ref {
        std::map<uint32_t, std::vector<Chunk>> bins;
        std::vector<uint64_t> linear;
        uint64_t off_beg = ~0ull, off_end = 0, n_mapped = 0, n_unmapped = 0;
        uint32_t last_bin = ~0u;
    };
    std::vector<Ref> refs(hdr.names.size());
    uint64_t n_no_coor = 0;
    for (const IndexEntry &e : entries) {
        if (e.tid < 0 || (size_t)e.tid >= refs.size()) { n_no_coor++; continue; }
        Ref &r = refs[e.tid];
        const uint64_t v0 = bgzf::voffset(out.block_coffset(e.blk0), e.uo0), v1 = bgzf::voffset(out.block_coffset(e.blk1), e.uo1);
        const uint32_t bin = (uint32_t)bam_reg2bin(e.beg, e.end);
        std::vector<Chunk> &ch = r.bins[bin];
        if (r.last_bin == bin && !ch.empty()) ch.back().end = v1;      // a run of records in one bin is one chunk
        else ch.push_back(Chunk{v0, v1});
        r.last_bin = bin;
        const size_t w0 = (size_t)(std::max(e.beg, 0) >> kLinearShift), w1 = (size_t)(std::max(e.end - 1, 0) >> kLinearShift);
        if (r.linear.size() <= w1) r.linear.resize(w1 + 1, ~0ull);
        for (size_t w = w0; w <= w1; w++) if (r.linear[w] == ~0ull) r.linear[w] = v0;
        r.off_beg = std::min(r.off_beg, v0);
        r.off_end = std::max(r.off_end, v1);
        if (e.flag & 4) r.n_unmapped++; else r.n_mapped++;
    }
    std::vector<uint8_t> b;
    b.insert(b.end(), {'B', 'A', 'I', 1});
    put32(b, (uint32_t)refs.size());
    for (Ref &r : refs) {
        const bool any = !r.bins.empty();
        put32(b, (uint32_t)r.bins.size() + (any ? 1 : 0));
        for (const auto &kv : r.bins) {
            put32(b, kv.first);
            put32(b, (uint32_t)kv.second.size());
            for (const Chunk &c : kv.second) { put64(b, c.beg); put64(b, c.end); }
        }
        if (any) {                                       // metadata pseudo-bin (SAMv1 §5.2)
            put32(b, (uint32_t)kPseudoBin);
            put32(b, 2);
            put64(b, r.off_beg); put64(b, r.off_end);
            put64(b, r.n_mapped); put64(b, r.n_unmapped);
        }
        for (size_t w = r.linear.size(); w-- > 0;)       // windows nothing starts in take the next window's offset
            if (r.linear[w] == ~0ull) r.linear[w] = w + 1 < r.linear.size() ? r.linear[w + 1] : 0;
        put32(b, (uint32_t)r.linear.size());
        for (uint64_t v : r.linear) put64(b, v);
    }
    put64(b, n_no_coor);
    FILE *f = fopen((path + ".bai").c_str(), "wb");
    if (!f) { err = "cannot create " + path + ".bai"; return false; }
    const bool ok = fwrite(b.data(), 1, b.size(), f) == b.size();
    if (fclose(f) != 0 || !ok) { err = "short write on " + path + ".bai"; return false; }
    return true;
}
