// copynumber.cpp — the copy-number pass (CNVCaller mirror): SNP queries, predictions, the HMM file
#include "abi.hpp"
#include "../dbscan.h"

CHMM chmm_from_pod(const csv_hmm *h)
{
    CHMM c; c.N = 6; c.M = 6;
    c.A.assign(6, std::vector<double>(6)); c.B.assign(6, std::vector<double>(6, 0.0));
    c.pi.resize(6); c.B1_mean.resize(6); c.B1_sd.resize(6); c.B2_mean.resize(5); c.B2_sd.resize(5);
    for (int i = 0; i < 6; i++) { for (int j = 0; j < 6; j++) c.A[i][j] = h->A[i * 6 + j]; c.pi[i] = h->pi[i]; c.B1_mean[i] = h->B1_mean[i]; c.B1_sd[i] = h->B1_sd[i]; }
    for (int i = 0; i < 5; i++) { c.B2_mean[i] = h->B2_mean[i]; c.B2_sd[i] = h->B2_sd[i]; }
    c.B1_uf = h->B1_uf; c.B2_uf = h->B2_uf;
    return c;
}
SNPTable snp_table(const uint32_t *pos, const double *baf, const double *pfb, const uint8_t *has_pfb, uint64_t n)
{
    SNPTable t;
    t.pos.assign(pos, pos + n); t.baf.assign(baf, baf + n); t.pfb.assign(pfb, pfb + n); t.has_pfb.assign(has_pfb, has_pfb + n);
    return t;
}

static int cn_prediction(csv_ctx *ctx, csv_shard *shard, int split, csvhost_call *calls, uint64_t n, uint64_t cap, uint64_t *n_out, const csv_hmm *hmm,
                         double mean_cov, int sample_size, uint32_t min_cnv, const uint32_t *snp_pos, const double *snp_baf, const double *snp_pfb,
                         const uint8_t *snp_has_pfb, uint64_t n_snp, bool observations_on_device, csv_snp_table *table = nullptr)
{
    GUARD({
        csvhost::set_context(ctx);
        CNVCaller cnv(ctx); cnv.sample_size = sample_size; cnv.min_cnv_length = min_cnv; cnv.device_observations = observations_on_device;
        SNPTable t = snp_table(snp_pos, snp_baf, snp_pfb, snp_has_pfb, n_snp);
        t.resident = table;                                  // borrowed: the caller's table of the same records
        CHMM h = chmm_from_pod(hmm);
        std::vector<SVCall> v; v.reserve(n);
        for (uint64_t i = 0; i < n; i++) v.push_back(from_pod(calls[i]));
        if (split) cnv.runSplitReadCopyNumberPredictions("chr", v, h, mean_cov, shard, t);
        else cnv.runCIGARCopyNumberPrediction("chr", v, h, mean_cov, shard, t);
        *n_out = v.size();
        for (size_t i = 0; i < v.size() && i < cap; i++) {
            // alt_allele carries the id for untouched calls; calls whose ALT was rewritten report id -1 (and a symbol ALT)
            calls[i] = to_pod(v[i]);
        }
    })
}

static int query_snp_regions(csv_ctx *ctx, csv_shard *shard, uint64_t n_regions, const uint32_t *start, const uint32_t *end, double mean_cov, int sample_size,
                             const uint32_t *snp_pos, const double *snp_baf, const double *snp_pfb, const uint8_t *snp_has_pfb, uint64_t n_snp, int on_device,
                             csv_snp_table *table, uint64_t *obs_off, uint32_t *pos_out, double *baf_out, double *pfb_out, double *log2_out, uint8_t *is_snp_out,
                             uint64_t cap, uint64_t *n_out)
{
    GUARD({
        CNVCaller cnv(ctx); cnv.sample_size = sample_size; cnv.device_observations = on_device != 0;
        SNPTable t = snp_table(snp_pos, snp_baf, snp_pfb, snp_has_pfb, n_snp);
        t.resident = table;                                  // borrowed (or none)
        std::vector<std::pair<uint32_t, uint32_t>> regions;
        for (uint64_t i = 0; i < n_regions; i++) regions.emplace_back(start[i], end[i]);
        std::vector<SNPData> d;
        cnv.querySNPRegions(regions, shard, mean_cov, t, d);
        uint64_t total = 0;
        for (uint64_t i = 0; i < n_regions; i++) { obs_off[i] = total; total += d[i].pos.size(); }
        obs_off[n_regions] = total;
        *n_out = total;
        if (total <= cap)
            for (uint64_t i = 0; i < n_regions; i++)
                for (size_t k = 0; k < d[i].pos.size(); k++) {
                    const uint64_t at = obs_off[i] + k;
                    pos_out[at] = d[i].pos[k]; baf_out[at] = d[i].baf[k]; pfb_out[at] = d[i].pfb[k]; log2_out[at] = d[i].log2_cov[k]; is_snp_out[at] = d[i].is_snp[k];
                }
    })
}

extern "C" {

// querySNPRegion for one region: observation arrays in the reference's order. cap = capacity of the outputs.
int csvhost_query_snp_region(csv_ctx *ctx, csv_shard *shard, uint32_t start, uint32_t end, double mean_cov, int sample_size,
                             const uint32_t *snp_pos, const double *snp_baf, const double *snp_pfb, const uint8_t *snp_has_pfb, uint64_t n_snp,
                             uint32_t *pos_out, double *baf_out, double *pfb_out, double *log2_out, uint8_t *is_snp_out, uint64_t cap, uint64_t *n_out)
{
    GUARD({
        CNVCaller cnv(ctx); cnv.sample_size = sample_size;
        SNPTable t = snp_table(snp_pos, snp_baf, snp_pfb, snp_has_pfb, n_snp);
        std::vector<SNPData> d;
        cnv.querySNPRegions({{start, end}}, shard, mean_cov, t, d);
        *n_out = d[0].pos.size();
        for (size_t i = 0; i < d[0].pos.size() && i < cap; i++) {
            pos_out[i] = d[0].pos[i]; baf_out[i] = d[0].baf[i]; pfb_out[i] = d[0].pfb[i]; log2_out[i] = d[0].log2_cov[i]; is_snp_out[i] = d[0].is_snp[i];
        }
    })
}

// querySNPRegion for many regions of one shard in one batch: region i's observations at [obs_off[i], obs_off[i + 1]) of the five arrays
// (an invalid region, start > end, has none). on_device: CNVCaller::device_observations. *n_out = the observations in all; nothing is
// written to the arrays when it exceeds cap.
int csvhost_query_snp_regions(csv_ctx *ctx, csv_shard *shard, uint64_t n_regions, const uint32_t *start, const uint32_t *end, double mean_cov, int sample_size,
                              const uint32_t *snp_pos, const double *snp_baf, const double *snp_pfb, const uint8_t *snp_has_pfb, uint64_t n_snp, int on_device,
                              uint64_t *obs_off, uint32_t *pos_out, double *baf_out, double *pfb_out, double *log2_out, uint8_t *is_snp_out, uint64_t cap, uint64_t *n_out)
{
    return query_snp_regions(ctx, shard, n_regions, start, end, mean_cov, sample_size, snp_pos, snp_baf, snp_pfb, snp_has_pfb, n_snp, on_device, nullptr, obs_off,
                             pos_out, baf_out, pfb_out, log2_out, is_snp_out, cap, n_out);
}

// csvhost_cn_prediction with the observation vectors built on the device (observations_on_device != 0: CNVCaller::device_observations)
int csvhost_cn_prediction_device(csv_ctx *ctx, csv_shard *shard, int split, csvhost_call *calls, uint64_t n, uint64_t cap, uint64_t *n_out,
                                 const csv_hmm *hmm, double mean_cov, int sample_size, uint32_t min_cnv,
                                 const uint32_t *snp_pos, const double *snp_baf, const double *snp_pfb, const uint8_t *snp_has_pfb, uint64_t n_snp,
                                 int observations_on_device)
{
    return cn_prediction(ctx, shard, split, calls, n, cap, n_out, hmm, mean_cov, sample_size, min_cnv, snp_pos, snp_baf, snp_pfb, snp_has_pfb, n_snp,
                         observations_on_device != 0);
}

// runCIGARCopyNumberPrediction (split == 0, in place) or runSplitReadCopyNumberPredictions (split == 1, may grow the list)
int csvhost_cn_prediction(csv_ctx *ctx, csv_shard *shard, int split, csvhost_call *calls, uint64_t n, uint64_t cap, uint64_t *n_out,
                          const csv_hmm *hmm, double mean_cov, int sample_size, uint32_t min_cnv,
                          const uint32_t *snp_pos, const double *snp_baf, const double *snp_pfb, const uint8_t *snp_has_pfb, uint64_t n_snp)
{
    return cn_prediction(ctx, shard, split, calls, n, cap, n_out, hmm, mean_cov, sample_size, min_cnv, snp_pos, snp_baf, snp_pfb, snp_has_pfb, n_snp, false);
}

// csvhost_cn_prediction_device with the SNPs looked up in `table` on the device (a csv_snp_table of the same records, the caller's to free;
// NULL: as csvhost_cn_prediction_device). The arrays stay the route of a batch the device declines.
int csvhost_cn_prediction_table(csv_ctx *ctx, csv_shard *shard, int split, csvhost_call *calls, uint64_t n, uint64_t cap, uint64_t *n_out,
                                const csv_hmm *hmm, double mean_cov, int sample_size, uint32_t min_cnv,
                                const uint32_t *snp_pos, const double *snp_baf, const double *snp_pfb, const uint8_t *snp_has_pfb, uint64_t n_snp,
                                int observations_on_device, csv_snp_table *table)
{
    return cn_prediction(ctx, shard, split, calls, n, cap, n_out, hmm, mean_cov, sample_size, min_cnv, snp_pos, snp_baf, snp_pfb, snp_has_pfb, n_snp,
                         observations_on_device != 0, table);
}

// csvhost_query_snp_regions with the SNPs looked up in `table` on the device (NULL: as csvhost_query_snp_regions)
int csvhost_query_snp_regions_table(csv_ctx *ctx, csv_shard *shard, uint64_t n_regions, const uint32_t *start, const uint32_t *end, double mean_cov, int sample_size,
                                    const uint32_t *snp_pos, const double *snp_baf, const double *snp_pfb, const uint8_t *snp_has_pfb, uint64_t n_snp, int on_device,
                                    csv_snp_table *table, uint64_t *obs_off, uint32_t *pos_out, double *baf_out, double *pfb_out, double *log2_out,
                                    uint8_t *is_snp_out, uint64_t cap, uint64_t *n_out)
{
    return query_snp_regions(ctx, shard, n_regions, start, end, mean_cov, sample_size, snp_pos, snp_baf, snp_pfb, snp_has_pfb, n_snp, on_device, table, obs_off,
                             pos_out, baf_out, pfb_out, log2_out, is_snp_out, cap, n_out);
}

// The first capacity the next table call of the mirror starts from (0: none remembered); forget != 0 clears it afterwards (tests, measurements)
uint64_t csvhost_cn_table_capacity_hint(int forget)
{
    const uint64_t h = CNVCaller::tableCapacityHint();
    if (forget) CNVCaller::forgetTableCapacityHint();
    return h;
}

// ---- HMM file + Viterbi seam
int csvhost_read_chmm(const char *path, csv_hmm *out, int32_t *N)
{
    GUARD({
        CHMM h = ReadCHMM(path);
        *N = h.N;
        if (h.N == 6) {
            for (int i = 0; i < 6; i++) { for (int j = 0; j < 6; j++) out->A[i * 6 + j] = h.A[i][j]; out->pi[i] = h.pi[i]; out->B1_mean[i] = h.B1_mean[i]; out->B1_sd[i] = h.B1_sd[i]; }
            for (int i = 0; i < 5; i++) { out->B2_mean[i] = h.B2_mean[i]; out->B2_sd[i] = h.B2_sd[i]; }
            out->B1_uf = h.B1_uf; out->B2_uf = h.B2_uf;
        }
    })
}

}  // extern "C"
