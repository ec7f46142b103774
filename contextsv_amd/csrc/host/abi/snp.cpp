// snp.cpp — SNP / population-frequency VCF ingestion (snp_io)
#include "abi.hpp"
#include "../snp_io.h"

extern "C" {

struct csvhost_snp {
    SNPFile f;
    SNPDeviceOptions dev;                                // ctx null: the host parser
    const SNPDeviceOptions *device() const { return dev.ctx ? &dev : nullptr; }
};

csvhost_snp *csvhost_snp_open(const char *snp_vcf, int threads)
{
    csvhost_snp *h = new csvhost_snp();
    std::string e;
    if (!h->f.load(snp_vcf ? snp_vcf : "", threads, &e)) { set_error(e); delete h; return nullptr; }
    return h;
}
// The same with every chunk's data lines decided on the device (csvgpu_vcf_snp_parse on ctx; the population files of later queries through
// csvgpu_vcf_af_parse); window_blocks: BGZF members per batch, 0 = the default. The tables are those of csvhost_snp_open.
csvhost_snp *csvhost_snp_open_device(const char *snp_vcf, int threads, csv_ctx *ctx, uint32_t window_blocks)
{
    if (!ctx) { set_error("csvhost_snp_open_device: no context"); return nullptr; }
    csvhost_snp *h = new csvhost_snp();
    h->dev.ctx = ctx; h->dev.window_blocks = window_blocks;
    std::string e;
    if (!h->f.load(snp_vcf ? snp_vcf : "", threads, &e, h->device())) { set_error(e); delete h; return nullptr; }
    return h;
}
// The same with the tables built on the device (SNPDeviceOptions::tables_on_device: csvgpu_snp_builder_* per chunk, the contigs' columns
// fetched once, csvhost_snp_table / csvhost_snp_query making each ascending contig's resident table from the columns). ctx must outlive h.
csvhost_snp *csvhost_snp_open_device_tables(const char *snp_vcf, int threads, csv_ctx *ctx, uint32_t window_blocks)
{
    if (!ctx) { set_error("csvhost_snp_open_device_tables: no context"); return nullptr; }
    csvhost_snp *h = new csvhost_snp();
    h->dev.ctx = ctx; h->dev.window_blocks = window_blocks; h->dev.tables_on_device = true;
    std::string e;
    if (!h->f.load(snp_vcf ? snp_vcf : "", threads, &e, h->device())) { set_error(e); delete h; return nullptr; }
    return h;
}
void csvhost_snp_free(csvhost_snp *h) { delete h; }
// out[3]: CHROM runs the builder reported, records appended through the host, contigs whose resident table was made from the columns
void csvhost_snp_build_stats(const csvhost_snp *h, uint64_t *out)
{
    const SNPDeviceStats &s = h->f.device_stats();
    out[0] = s.runs; out[1] = s.appended_host; out[2] = s.tables_resident;
}
// out[4]: lines the device examined, records it kept, lines it deferred to the host parser, batches it declined
void csvhost_snp_device_stats(const csvhost_snp *h, uint64_t *out)
{
    const SNPDeviceStats &s = h->f.device_stats();
    out[0] = s.lines; out[1] = s.kept; out[2] = s.deferred; out[3] = s.declined_batches;
}
// A contig's whole table (population hits attached as by csvhost_snp_query): n[0] positions / BAFs, n[1] population records, all in file
// order. Arrays may be null or short: the counts are always filled in, the arrays only when both capacities suffice. Returns 0, or 1 when
// nothing was copied.
int csvhost_snp_table(csvhost_snp *h, const char *chr, const char *pfb_vcf, const char *ethnicity, int threads, uint32_t *pos, double *baf, uint64_t cap,
                      uint32_t *af_pos, double *af, uint64_t af_cap, uint64_t *n)
{
    const SNPFileTable &t = h->f.table(chr, pfb_vcf ? pfb_vcf : "", ethnicity ? ethnicity : "", threads, h->device());
    n[0] = t.pos.size(); n[1] = t.af_pos.size();
    if (n[0] > cap || n[1] > af_cap) return 1;
    for (size_t i = 0; i < t.pos.size(); i++) { pos[i] = t.pos[i]; baf[i] = t.baf[i]; }
    for (size_t i = 0; i < t.af_pos.size(); i++) { af_pos[i] = t.af_pos[i]; af[i] = t.af[i]; }
    return 0;
}
uint64_t csvhost_snp_kept(const csvhost_snp *h) { return h->f.records_kept(); }

// readSNPAlleleFrequencies for one region from the loaded tables. Returns the number of positions (file order), -1 when cap is too
// small. baf_out[i] = map value at pos_out[i]; at most one population frequency (has_pfb, pfb_pos, pfb_val).
int64_t csvhost_snp_query(csvhost_snp *h, const char *chr, const char *pfb_vcf, const char *ethnicity, uint32_t start_pos, uint32_t end_pos,
                          uint32_t *pos_out, double *baf_out, uint64_t cap, int *has_pfb, uint32_t *pfb_pos, double *pfb_val, int threads)
{
    const SNPFileTable &t = h->f.table(chr, pfb_vcf ? pfb_vcf : "", ethnicity ? ethnicity : "", threads, h->device());
    std::vector<uint32_t> pos;
    std::unordered_map<uint32_t, double> baf, pfb;
    t.query(start_pos, end_pos, pos, baf, pfb);
    *has_pfb = 0;
    if (pos.size() > cap) return -1;
    for (size_t i = 0; i < pos.size(); i++) { pos_out[i] = pos[i]; baf_out[i] = baf[pos[i]]; }
    if (!pfb.empty()) { *has_pfb = (int)pfb.size(); *pfb_pos = pfb.begin()->first; *pfb_val = pfb.begin()->second; }
    return (int64_t)pos.size();
}

// the --pfb table: path for `chr` copied to buf (empty when absent); -1 when the table cannot be loaded
int64_t csvhost_pfb_path(const char *table_path, const char *chr, char *buf, uint64_t cap)
{
    AlleleFreqFiles a;
    std::string e;
    if (!a.load(table_path, &e)) { set_error(e); return -1; }
    return (int64_t)copy_text(a.get(chr), buf, cap);
}
int64_t csvhost_gnomad_contig(const char *chr, const char *pfb_path, char *buf, uint64_t cap) { return (int64_t)copy_text(gnomadContigName(chr, pfb_path), buf, cap); }

}  // extern "C"
