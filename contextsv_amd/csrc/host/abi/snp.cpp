// snp.cpp — SNP / population-frequency VCF ingestion (snp_io)
#include "abi.hpp"
#include "../snp_io.h"

extern "C" {

struct csvhost_snp { SNPFile f; };

csvhost_snp *csvhost_snp_open(const char *snp_vcf, int threads)
{
    csvhost_snp *h = new csvhost_snp();
    std::string e;
    if (!h->f.load(snp_vcf ? snp_vcf : "", threads, &e)) { set_error(e); delete h; return nullptr; }
    return h;
}
void csvhost_snp_free(csvhost_snp *h) { delete h; }
uint64_t csvhost_snp_kept(const csvhost_snp *h) { return h->f.records_kept(); }

// readSNPAlleleFrequencies for one region from the loaded tables. Returns the number of positions (file order), -1 when cap is too
// small. baf_out[i] = map value at pos_out[i]; at most one population frequency (has_pfb, pfb_pos, pfb_val).
int64_t csvhost_snp_query(csvhost_snp *h, const char *chr, const char *pfb_vcf, const char *ethnicity, uint32_t start_pos, uint32_t end_pos,
                          uint32_t *pos_out, double *baf_out, uint64_t cap, int *has_pfb, uint32_t *pfb_pos, double *pfb_val, int threads)
{
    const SNPFileTable &t = h->f.table(chr, pfb_vcf ? pfb_vcf : "", ethnicity ? ethnicity : "", threads);
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
