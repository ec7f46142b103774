// synth.cpp — synthetic shards
#include "abi.hpp"

extern "C" {

// sv_per_bp <= 0: the default density (one truth SV per 120 kb)
csvhost_synth *csvhost_synth_generate2(uint64_t seed, uint32_t chr_len, double depth, int tech, int threads, int with_seq, double sv_per_bp)
{
    try {
        SynthParams p; p.seed = seed; p.chr_len = chr_len; p.depth = depth; p.tech = tech; p.threads = threads; p.with_seq = with_seq;
        if (sv_per_bp > 0) p.sv_per_bp = sv_per_bp;
        csvhost_synth *h = new csvhost_synth();
        synth_generate(p, h->sh);
        return h;
    } catch (const std::exception &e) { set_error(e.what()); return nullptr; }
}
csvhost_synth *csvhost_synth_generate(uint64_t seed, uint32_t chr_len, double depth, int tech, int threads, int with_seq)
{
    return csvhost_synth_generate2(seed, chr_len, depth, tech, threads, with_seq, 0.0);
}
void csvhost_synth_view(const csvhost_synth *h, csv_reads *out, uint32_t *depth_len, const uint64_t **seq_off, const uint8_t **seq)
{
    *out = h->sh.view(); *depth_len = h->sh.depth_len;
    if (seq_off) *seq_off = h->sh.seq_off.empty() ? nullptr : h->sh.seq_off.data();
    if (seq) *seq = h->sh.seq.empty() ? nullptr : h->sh.seq.data();
}
const uint32_t *csvhost_synth_qname_ids(const csvhost_synth *h) { return h->sh.qname_id.data(); }
void csvhost_synth_free(csvhost_synth *h) { delete h; }

}  // extern "C"
