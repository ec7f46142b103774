// bam.cpp — BAM / BAI reader and writer (bam_io), the BGZF inflate of a whole file
#include "abi.hpp"
#include "../bgzf.h"
#include "../hugevec.h"

// device >= 0: the reads that follow inflate the BGZF blocks on that device, on a context of the handle's own (BamReadOptions::device_inflate);
// -1: on the host again. 0, or -1 with the reason in csvhost_last_error.
// The handle has ONE context for both options: a second option must name the device of the first (refused otherwise, nothing changed).
static int bam_set_device(csvhost_bam *h, bool &on, int device_or_minus_1)
{
    try {
        const bool other = &on == &h->inflate_on ? h->unpack_on : h->inflate_on;
        if (device_or_minus_1 < 0) {
            on = false;
            if (!other && h->inflate_ctx) { h->drop_residents(); csvgpu_destroy(h->inflate_ctx); h->inflate_ctx = nullptr; h->ctx_device = -1; }
            return 0;
        }
        if (other && h->inflate_ctx && h->ctx_device != device_or_minus_1) {
            set_error("the BAM reader's context is on device " + std::to_string(h->ctx_device) + ": inflate and unpack share it, switch the other option off first");
            return -1;
        }
        if (h->inflate_ctx && h->ctx_device != device_or_minus_1) { h->drop_residents(); csvgpu_destroy(h->inflate_ctx); h->inflate_ctx = nullptr; h->ctx_device = -1; }
        if (!h->inflate_ctx) {
            h->inflate_ctx = csvgpu_create(device_or_minus_1, nullptr);
            if (!h->inflate_ctx) { on = false; set_error(std::string("no device context for the BAM reader: ") + csvgpu_last_error(nullptr)); return -1; }
            h->ctx_device = device_or_minus_1;
        }
        on = true;
        return 0;
    } catch (const std::exception &e) { set_error(e.what()); return -1; }
}

// the synthetic shard's records, coordinate-sorted (verified rather than assumed: the generator emits reads in position order per thread
// slice and merges them sorted), through add(i, cigar, n_cigar)
template <class Add> static void for_each_sorted(const SynthShard &sh, Add add)
{
    for (size_t i = 0; i < sh.pos.size(); i++) {
        if (i && sh.pos[i] < sh.pos[i - 1]) throw std::runtime_error("synthetic shard is not coordinate-sorted");
        add(i, sh.cigar.data() + sh.cigar_off[i], (uint32_t)(sh.cigar_off[i + 1] - sh.cigar_off[i]));
    }
}

extern "C" {

csvhost_bam *csvhost_bam_open(const char *path, int load_index)
{
    csvhost_bam *h = new csvhost_bam();
    if (!h->r.open(path) || (load_index && !h->r.loadIndex())) { set_error(h->r.error()); delete h; return nullptr; }
    for (const std::string &n : h->r.header().names) { if (!h->names.empty()) h->names += '\n'; h->names += n; }
    return h;
}
void csvhost_bam_close(csvhost_bam *h) { delete h; }
int csvhost_bam_n_ref(const csvhost_bam *h) { return (int)h->r.header().names.size(); }
const char *csvhost_bam_names(const csvhost_bam *h) { return h->names.c_str(); }
const char *csvhost_bam_text(const csvhost_bam *h) { return h->r.header().text.c_str(); }
uint32_t csvhost_bam_ref_len(const csvhost_bam *h, int tid) { return h->r.header().lens[(size_t)tid]; }

int csvhost_bam_set_device_inflate(csvhost_bam *h, int device_or_minus_1) { return bam_set_device(h, h->inflate_on, device_or_minus_1); }
// device >= 0: the readContig calls that follow unpack every batch's records on that device (BamReadOptions::device_unpack), on the handle's
// own context — the one the inflate uses when both are set; -1: the host parser again. readAll keeps the host parser either way.
int csvhost_bam_set_device_unpack(csvhost_bam *h, int device_or_minus_1) { return bam_set_device(h, h->unpack_on, device_or_minus_1); }
// on != 0: the readContig calls that follow, while the unpack is on the device, build the contig's resident shard there (BamReadOptions::device_shard)
void csvhost_bam_set_device_shard(csvhost_bam *h, int on) { h->shard_on = on != 0; }

// Every BGZF block of a file inflated in batches of window_blocks, on `threads` host threads (ctx null: bgzf::inflate_range) or on ctx's device
// (bgzf::inflate_range_device), into one buffer that is reused: what tools/bench_inflate.py times. *ms: the inflate alone (the block scan before it).
int csvhost_bgzf_inflate_file(const char *path, int threads, csv_ctx *ctx, uint32_t window_blocks, uint64_t *n_blocks, uint64_t *in_bytes, uint64_t *out_bytes, double *ms)
{
    GUARD({
        bgzf::MappedFile f;
        std::string e;
        if (!f.open(path, &e)) throw std::runtime_error(e);
        std::vector<bgzf::Block> blocks;
        if (!bgzf::scan_blocks(f.data(), f.size(), 0, blocks, &e)) throw std::runtime_error(e);
        const size_t W = std::max<uint32_t>(window_blocks, 1);
        uint64_t largest = 0, total = 0;
        for (size_t i = 0; i < blocks.size(); i += W) {
            uint64_t acc = 0;
            for (size_t k = i; k < std::min(blocks.size(), i + W); k++) acc += blocks[k].isize;
            largest = std::max(largest, acc); total += acc;
        }
        HugeVec<uint8_t> buf;
        buf.resize_uninit(largest + 1);
        memset(buf.data(), 0, largest + 1);                           // pages touched before the clock starts
        const auto t0 = std::chrono::steady_clock::now();
        for (size_t i = 0; i < blocks.size(); i += W) {
            const size_t last = std::min(blocks.size(), i + W);
            const bool ok = ctx ? bgzf::inflate_range_device(ctx, f.data(), blocks, i, last, buf.data(), threads, &e) : bgzf::inflate_range(f.data(), blocks, i, last, buf.data(), threads, &e);
            if (!ok) throw std::runtime_error(e);
        }
        *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        *n_blocks = blocks.size(); *in_bytes = f.size(); *out_bytes = total;
    })
}

// chr != nullptr: readContig (needs the index) -> one shard; chr == nullptr: readAll -> one shard per contig with records.
// Returns the number of shards now held by the handle (replacing the previous ones), or -1.
int csvhost_bam_read(csvhost_bam *h, const char *chr, int want_seq, int want_qnames, int threads, uint32_t window_blocks, uint64_t *n_unplaced)
{
    try {
        BamReadOptions opt;
        opt.want_seq = want_seq != 0; opt.want_qnames = want_qnames != 0; opt.threads = threads;
        if (window_blocks) opt.window_blocks = window_blocks;
        opt.device_inflate = h->inflate_on ? h->inflate_ctx : nullptr;
        opt.device_unpack = h->unpack_on && chr ? h->inflate_ctx : nullptr;
        opt.device_shard = h->shard_on && opt.device_unpack;
        h->shards.clear();
        bool ok;
        if (chr) { h->shards.emplace_back(); ok = h->r.readContig(chr, opt, h->shards.back()); }
        else ok = h->r.readAll(opt, [&](BamShard &&s) { h->shards.push_back(std::move(s)); }, n_unplaced);
        if (!ok) { set_error(h->r.error()); h->shards.clear(); return -1; }
        return (int)h->shards.size();
    } catch (const std::exception &e) { set_error(e.what()); return -1; }
}
// BamReader::UnpackStats of the last csvhost_bam_read with a contig name: batches the device unpacked, batches the host parser read, anchors
// given to the device, records the device wrote, batches whose decoded bytes never came to the host, batches brought down after all
// — and, for BamReadOptions::device_shard: whether the contig ended as a resident shard, batches appended to it from the host parser's arrays,
// CIGAR words that came down into the host shard
void csvhost_bam_unpack_stats(const csvhost_bam *h, uint64_t out[9])
{
    const BamReader::UnpackStats &u = h->r.unpackStats();
    out[0] = u.batches_device; out[1] = u.batches_host; out[2] = u.anchors; out[3] = u.records; out[4] = u.batches_kept_on_device; out[5] = u.batches_downloaded;
    out[6] = u.shard_resident; out[7] = u.batches_appended_host; out[8] = u.cigar_words_downloaded;
}
// The resident shard of shard i (BamReadOptions::device_shard), handed to the caller, who frees it with csvgpu_shard_free on a context of the
// same device; null when there is none (a contig without records, the option off, or taken before). *n_cigar: its CIGAR words.
csv_shard *csvhost_bam_shard_take_resident(csvhost_bam *h, int i, uint64_t *n_cigar)
{
    BamShard &s = h->shards[(size_t)i];
    if (n_cigar) *n_cigar = s.resident_cigar;
    return s.resident.release();
}
// view of shard i: arrays stay owned by the handle until the next read / close
void csvhost_bam_shard(const csvhost_bam *h, int i, csv_reads *reads, int32_t *tid, uint32_t *target_len, const uint64_t **seq_off, const uint8_t **seq)
{
    const BamShard &s = h->shards[(size_t)i];
    *reads = s.view();
    *tid = s.tid; *target_len = s.target_len;
    *seq_off = s.seq_off.data(); *seq = s.seq.data();
}
// query names of shard i, '\n'-joined; returns the text length (copying at most cap bytes)
int64_t csvhost_bam_shard_qnames(const csvhost_bam *h, int i, char *buf, uint64_t cap)
{
    std::string t;
    for (const std::string &q : h->shards[(size_t)i].qnames) { t += q; t += '\n'; }
    return (int64_t)copy_text(t, buf, cap);
}

// Write a coordinate-sorted BAM + BAI from arrays. qnames: '\n'-separated (one per record). seq_off / seq may be null (l_seq = 0);
// l_seq[i] gives the base count (the packed length alone cannot tell odd from even).
int csvhost_bam_write(const char *path, const char *text, int n_ref, const char *ref_names, const uint32_t *ref_lens, uint64_t n, const int32_t *tid,
                      const int32_t *pos, const uint16_t *flag, const uint8_t *mapq, const uint64_t *cigar_off, const uint32_t *cigar,
                      const char *qnames, const uint64_t *seq_off, const uint8_t *seq, const int32_t *l_seq, int level, int threads)
{
    GUARD({
        BamHeader hd;
        hd.text = text ? text : "";
        hd.names = split_lines(ref_names, n_ref);
        hd.lens.assign(ref_lens, ref_lens + n_ref);
        BamWriter w;
        if (!w.open(path, hd, level, threads)) throw std::runtime_error(w.error());
        const char *q = qnames;
        for (uint64_t i = 0; i < n; i++) {
            const char *e = strchr(q, '\n');
            std::string name(q, e ? (size_t)(e - q) : strlen(q));
            q = e ? e + 1 : q + strlen(q);
            const int32_t ls = (seq && l_seq) ? l_seq[i] : 0;
            w.add(tid[i], pos[i], mapq[i], flag[i], name, cigar + cigar_off[i], (uint32_t)(cigar_off[i + 1] - cigar_off[i]),
                  ls ? seq + seq_off[i] : nullptr, ls, nullptr);
        }
        if (!w.close()) throw std::runtime_error(w.error());
    })
}

// The synthetic shard as a coordinate-sorted BAM + BAI on one contig ("stage inputs ... as a real BGZF BAM + BAI").
// Query names are r<read id> (a primary and its supplementary record share one); sequences are written when the shard has them, else l_seq = 0 ("*").
int csvhost_synth_write_bam(const csvhost_synth *h, const char *path, const char *chr_name, int level, int threads, uint64_t *bam_bytes)
{
    GUARD({
        const SynthShard &sh = h->sh;
        BamHeader hd;
        hd.text = std::string("@HD\tVN:1.6\tSO:coordinate\n@SQ\tSN:") + chr_name + "\tLN:" + std::to_string(sh.depth_len - 1) + "\n";
        hd.names.push_back(chr_name);
        hd.lens.push_back(sh.depth_len - 1);
        BamWriter w;
        if (!w.open(path, hd, level, threads)) throw std::runtime_error(w.error());
        const bool have_seq = !sh.seq.empty() && sh.seq_off.size() == sh.pos.size() + 1;
        for_each_sorted(sh, [&](size_t i, const uint32_t *cg, uint32_t nc) {
            int32_t l_seq = 0;
            if (have_seq) for (uint32_t k = 0; k < nc; k++) if ((0x3C1A7u >> ((cg[k] & 15) << 1)) & 1) l_seq += (int32_t)(cg[k] >> 4);   // query-consuming ops
            w.add(0, sh.pos[i], sh.mapq[i], sh.flag[i], "r" + std::to_string(sh.qname_id[i]), cg, nc, have_seq ? sh.seq.data() + sh.seq_off[i] : nullptr, l_seq, nullptr);
        });
        if (!w.close()) throw std::runtime_error(w.error());
        if (bam_bytes) { bgzf::MappedFile f; std::string e; *bam_bytes = f.open(path, &e) ? f.size() : 0; }
    })
}

// Several synthetic shards into ONE coordinate-sorted BAM + BAI, one contig each, appended in tid order.
struct csvhost_bam_writer { BamWriter w; };
csvhost_bam_writer *csvhost_bam_writer_open(const char *path, int n_ref, const char *ref_names, const uint32_t *ref_lens, int level, int threads)
{
    try {
        BamHeader hd;
        hd.text = "@HD\tVN:1.6\tSO:coordinate\n";
        hd.names = split_lines(ref_names, n_ref);
        hd.lens.assign(ref_lens, ref_lens + n_ref);
        for (int i = 0; i < n_ref; i++) hd.text += "@SQ\tSN:" + hd.names[(size_t)i] + "\tLN:" + std::to_string(ref_lens[i]) + "\n";
        csvhost_bam_writer *h = new csvhost_bam_writer();
        if (!h->w.open(path, hd, level, threads)) { set_error(h->w.error()); delete h; return nullptr; }
        return h;
    } catch (const std::exception &e) { set_error(e.what()); return nullptr; }
}
int csvhost_bam_writer_append_synth(csvhost_bam_writer *h, const csvhost_synth *syn, int tid)
{
    GUARD({
        const SynthShard &sh = syn->sh;
        for_each_sorted(sh, [&](size_t i, const uint32_t *cg, uint32_t nc) {
            h->w.add(tid, sh.pos[i], sh.mapq[i], sh.flag[i], "r" + std::to_string(tid) + "_" + std::to_string(sh.qname_id[i]), cg, nc, nullptr, 0, nullptr);
        });
    })
}
int csvhost_bam_writer_close(csvhost_bam_writer *h)
{
    GUARD({
        const bool ok = h->w.close();
        const std::string e = h->w.error();
        delete h;
        if (!ok) throw std::runtime_error(e);
    })
}

}  // extern "C"
