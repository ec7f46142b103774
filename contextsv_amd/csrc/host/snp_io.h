// snp_io.h — SNP / population-frequency VCF ingestion without htslib (reference: CNVCaller::readSNPAlleleFrequencies,
// src/cnv_caller.cpp:558-809; the PFB path table of InputData, src/input_data.cpp:211-310).
// The reference opens, indexes and region-queries both VCFs once per SV. Here each file is streamed once (BGZF blocks
// inflated by a pool, or plain text), the records that pass the reference's filters are kept per contig in sorted arrays,
// and query() answers a region from those arrays with the reference's result, including its quirks:
//   * positions come back in file order, duplicates included; the BAF map keeps the last duplicate;
//   * at most ONE population frequency per region: the first gnomAD SNP record inside [min SNP, max SNP] whose position is a
//     kept SNP, that has the AF key, and whose value is not <= 0.01 or >= 0.99 (a "." value is NaN and passes that test).
#pragma once
#include <cstdint>
#include <functional>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

#include "bgzf.h"
#include "cnv_caller.h"
#include "hugevec.h"

// Lines of a text file that is BGZF-compressed (.vcf.gz) or plain, streamed in batches.
class TextFile {
public:
    bool open(const std::string &path, std::string *err);
    // on_lines(chunk): chunk holds whole lines ('\n'-terminated except possibly the last of the file); return false to stop early.
    // window_blocks: BGZF members inflated per batch (a test makes lines straddle batches with a small one)
    bool forEachChunk(int threads, const std::function<bool(std::string_view)> &on_lines, std::string *err, size_t window_blocks = 1024);
    bool compressed() const { return is_bgzf; }
private:
    bgzf::MappedFile file;
    bool is_bgzf = false;
};

// --pfb table: "<chr without the chr prefix>=<path>" lines (input_data.cpp:211-292)
class AlleleFreqFiles {
public:
    // false + err when the table or one of the listed files cannot be opened (the reference exits there)
    bool load(const std::string &table_path, std::string *err);
    std::string get(std::string chr) const;              // "" when the contig has no entry (input_data.cpp:294-310)
    bool empty() const { return paths.empty(); }
private:
    std::unordered_map<std::string, std::string> paths;
};

// Opt-in: the data lines of every chunk decided on the device (csvgpu_vcf_snp_parse / csvgpu_vcf_af_parse on `ctx`); the lines it defers and
// the batches it declines run through the two functions below, so the tables are the same byte for byte.
struct csv_ctx;
struct csv_snp_columns;
// A device call that fails outright (CSV_E*): load() fails with the message in `err`; table(), which has no error channel, logs it once and
// lets the host parser read the rest of that population file.
// tables_on_device (needs ctx): load() hands every chunk to a csv_snp_builder, which cuts the kept records by contig on the device, and fetches
// each contig's columns once; table() reads the population file against the resident positions and makes the contig's resident table from
// the columns. Any CSV_E* from the builder makes load() start over on the parse_on_device path, with nothing kept from the builder.
struct SNPDeviceOptions { csv_ctx *ctx = nullptr; size_t window_blocks = 0; bool tables_on_device = false; };   // window_blocks 0: forEachChunk's default
struct SNPDeviceStats {
    uint64_t lines = 0, kept = 0, deferred = 0, declined_batches = 0;
    uint64_t runs = 0;                 // CHROM runs the builder reported (one name string each)
    uint64_t appended_host = 0;        // records that went through csvgpu_snp_builder_append_host (deferred lines, declined or oversized batches)
    uint64_t tables_resident = 0;      // contigs whose resident table was made from the columns
};

// One data line's decision, as SNPFile::load and SNPFile::table take it (the device parser's deferred lines and the stand-alone check of
// vcf_record_core.hpp call the same two functions).
struct SnpLineRecord { std::string_view chrom; uint32_t pos = 0; double baf = 0; };
// false: the line is not kept. dp_int / ad_int: the header declared FORMAT/DP, FORMAT/AD as Integer.
bool snp_record_of_line(std::string_view line, bool dp_int, bool ad_int, SnpLineRecord &rec);
enum class AfLine { Skip, Keep, Stop };
// `sorted`: the contig's kept SNP positions, ascending, not empty; last_pos = sorted.back(); needle = "<key>="
AfLine af_record_of_line(std::string_view line, std::string_view contig, std::string_view needle, const std::vector<uint32_t> &sorted, uint32_t last_pos,
                         uint32_t &pos, double &af);

// One contig's SNPs and population-frequency hits.
struct SNPFileTable : SNPSource {
    std::vector<uint32_t> pos;            // file order (coordinate-sorted files: ascending; duplicates kept)
    std::vector<double> baf;
    std::vector<uint32_t> af_pos;         // gnomAD records that can become a region's hit, file order
    std::vector<double> af;
    void query(uint32_t start_pos, uint32_t end_pos, std::vector<uint32_t> &snp_pos, std::unordered_map<uint32_t, double> &snp_baf,
               std::unordered_map<uint32_t, double> &snp_pfb) const override;
    // Opt-in: the table on ctx's device (the first-hit kind) from the host arrays, as SNPTable::makeResident. SNPFile::table sets `resident`
    // itself, from the device columns, when the file was loaded with SNPDeviceOptions::tables_on_device (runBam: SVCaller::snp_tables_on_device).
    bool makeResident(csv_ctx *ctx);
    void dropResident();
    const csv_snp_table *residentTable() const override { return resident; }
    csv_snp_table *resident = nullptr;
    csv_ctx *resident_ctx = nullptr;
};

// The sample's SNP VCF parsed once for every contig; population frequencies attached per contig on request.
class SNPFile {
public:
    // Streams the file once and keeps, per contig, the records that pass the reference's filters (SNP alleles only, QUAL > 30,
    // FORMAT/DP > 10, FILTER PASS or ".", FORMAT/AD with two values; cnv_caller.cpp:679-727). Like the reference's synced reader
    // it wants an index next to a compressed file (.tbi or .csi): without one, false.
    bool load(const std::string &snp_vcf, int threads, std::string *err, const SNPDeviceOptions *dev = nullptr);
    // The contig's table with gnomAD hits from `pfb_vcf` ("" = none) under INFO key AF[_<ethnicity>]; built on first use.
    // chr naming against the gnomAD file follows the reference's path heuristic (cnv_caller.cpp:624-640).
    const SNPFileTable &table(const std::string &chr, const std::string &pfb_vcf, const std::string &ethnicity, int threads, const SNPDeviceOptions *dev = nullptr);
    uint64_t records_kept() const { return n_kept; }
    const SNPDeviceStats &device_stats() const { return dev_stats; }       // summed over load() and every table() that parsed on the device
    SNPFile() = default;
    SNPFile(const SNPFile &) = delete;
    SNPFile &operator=(const SNPFile &) = delete;
    ~SNPFile();                                                              // frees the resident tables table() made, and the columns
private:
    // load() through a csv_snp_builder; false (err set, nothing kept) when the builder refused anything
    bool loadTables(const std::string &snp_vcf, int threads, std::string *err, const SNPDeviceOptions &dev);
    void attachAf(SNPFileTable &t, const std::string &chr, const std::string &pfb_vcf, const std::string &ethnicity, int threads, const SNPDeviceOptions *dev,
                  int64_t column_id);
    void dropColumns();
    csv_snp_columns *columns = nullptr;                                      // tables_on_device: the contigs' columns, and whose they are
    csv_ctx *columns_ctx = nullptr;
    std::unordered_map<std::string, std::pair<uint32_t, bool>> column_of;    // contig -> (id in `columns`, ascending)
    std::unordered_map<std::string, SNPFileTable> tables;
    std::unordered_map<std::string, bool> af_done;
    SNPFileTable none;
    uint64_t n_kept = 0;
    SNPDeviceStats dev_stats;
};

// the gnomAD contig name for `chr` given the file path (cnv_caller.cpp:624-640)
std::string gnomadContigName(const std::string &chr, const std::string &pfb_filepath);
