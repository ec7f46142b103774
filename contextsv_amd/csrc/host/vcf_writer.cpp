#include "vcf_writer.h"

#include <algorithm>
#include <atomic>
#include <ctime>
#include <fstream>
#include <iostream>
#include <sstream>
#include <stdexcept>

#include "log.h"
#include "sv_types.h"

using namespace sv_types;

namespace {
constexpr int kVersionMajor = 1, kVersionMinor = 0, kVersionPatch = 0;   // include/version.h:5-7

// IUPAC ambiguity codes, either case, become N in REF (:1295-1305)
struct AmbiguityTable {
    bool amb[256] = {};
    AmbiguityTable()
    {
        for (const char *c = "RYKMSWBDHV"; *c; c++) {
            amb[(unsigned char)*c] = true;
            amb[(unsigned char)(*c + ('a' - 'A'))] = true;
        }
    }
};
const AmbiguityTable kAmb;

// one output line, split around the two places the depth value goes
struct Record {
    std::string head;     // CHROM .. ";HMM=<x>;SUPPORT="
    std::string tail;     // ";CLUSTER=.." .. "\tGT:DP\t<GT>:"
    uint32_t pos;         // POS after the preceding-base shift: where SUPPORT / DP is read
};

const char *const kHeaderLines[] = {
    "##INFO=<ID=END,Number=1,Type=Integer,Description=\"End position of the variant described in this record\">",
    "##INFO=<ID=SVTYPE,Number=1,Type=String,Description=\"Type of structural variant\">",
    "##INFO=<ID=SVLEN,Number=1,Type=Integer,Description=\"Difference in length between REF and ALT alleles\">",
    "##INFO=<ID=SVMETHOD,Number=1,Type=String,Description=\"Method used to call the structural variant\">",
    "##INFO=<ID=ALN,Number=1,Type=String,Description=\"Feature used to identify the structural variant\">",
    "##INFO=<ID=HMM,Number=1,Type=Float,Description=\"HMM likelihood\">",
    "##INFO=<ID=LOH,Number=0,Type=Flag,Description=\"Site shows loss of heterozygosity\">",
    "##INFO=<ID=SUPPORT,Number=1,Type=Integer,Description=\"Number of reads supporting the variant\">",
    "##INFO=<ID=CLUSTER,Number=1,Type=Integer,Description=\"Cluster size\">",
    "##INFO=<ID=CN,Number=1,Type=Integer,Description=\"Copy number state\">",
    "##INFO=<ID=ALNOFFSET,Number=1,Type=Integer,Description=\"Read vs. reference alignment offset\">",
    "##FILTER=<ID=PASS,Description=\"All filters passed\">",
    "##FILTER=<ID=LowQual,Description=\"Low quality\">",
    "##FILTER=<ID=AssemblyGap,Description=\"Assembly gap\">",
    "##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">",
    "##FORMAT=<ID=DP,Number=1,Type=Integer,Description=\"Read depth at the variant site (sum of start and end positions)\">",
};
}  // namespace

namespace {
std::atomic<uint64_t> g_vcf_device_batches{0}, g_vcf_host_batches{0}, g_vcf_declined{0};

// status bits of csvgpu_vcf_format's line_status (csrc/vcf_format_core.hpp)
enum : uint8_t { ST_DISPOSITION = 3, ST_SKIP_UNCLASSIFIED = 1, ST_SKIP_FIRST_POSITION = 2, ST_EMPTY_REF = 4, ST_DEPTH_OUT_OF_RANGE = 16 };

// The record lines of all contigs from ONE csvgpu_vcf_format call, written to `out` with the host loop's messages replayed from the status
// bytes. false: nothing was written and the caller runs the host loop (the genome or the depth maps are not on the device, the device
// declined the batch, or the call failed).
bool formatOnDevice(std::ostream &out, const std::vector<std::pair<std::string, const std::vector<SVCall> *>> &contigs, const VCFOptions &opt,
                    const std::unordered_map<std::string, std::vector<std::pair<uint32_t, uint32_t>>> &gaps, const ReferenceGenome &ref_genome,
                    const DepthSource &depth, const std::string &sv_method, VCFCounts &counts)
{
    const ShardDepthSource *shards = dynamic_cast<const ShardDepthSource *>(&depth);
    const csv_genome *genome = ref_genome.deviceGenome();
    csv_ctx *ctx = opt.ctx ? opt.ctx : (shards ? shards->ctx : nullptr);
    if (!shards || !genome || !ctx) { g_vcf_host_batches++; return false; }

    const size_t n_contigs = contigs.size();
    std::vector<csv_vcf_contig> tab(n_contigs);
    std::vector<uint64_t> call_off(n_contigs + 1, 0);
    std::vector<std::vector<uint32_t>> gap_start(n_contigs), gap_end(n_contigs);
    std::vector<csv_vcf_call> calls;
    std::vector<uint64_t> alt_off(1, 0);
    std::string alts;
    uint64_t bound = 0;                                   // of the text: the cuts' lengths are the contigs' lengths at most
    for (size_t t = 0; t < n_contigs; t++) {
        const std::string &chr = contigs[t].first;
        csv_vcf_contig &c = tab[t];
        c.name = chr.data(); c.name_len = (uint32_t)chr.size();
        c.genome_record = ref_genome.deviceRecord(chr);
        const auto sh = shards->shards.find(chr);
        c.shard = sh == shards->shards.end() ? nullptr : sh->second;
        const auto gap_it = gaps.find(chr);
        if (gap_it != gaps.end())
            for (const auto &row : gap_it->second) { gap_start[t].push_back(row.first); gap_end[t].push_back(row.second); }
        c.gap_start = gap_start[t].data(); c.gap_end = gap_end[t].data(); c.n_gaps = (uint32_t)gap_start[t].size();
        const uint64_t contig_len = c.genome_record < 0 ? 0 : ref_genome.getChromosomeLength(chr);
        for (const SVCall &sv : *contigs[t].second) {
            csv_vcf_call p;
            p.start = sv.start; p.end = sv.end; p.sv_type = (int32_t)sv.sv_type; p.cluster_size = sv.cluster_size; p.hmm_likelihood = sv.hmm_likelihood; p.id = -1;
            p.aln_flags = (uint32_t)sv.aln_type.to_ulong(); p.genotype = (int32_t)sv.genotype; p.cn_state = sv.cn_state; p.aln_offset = sv.aln_offset;
            calls.push_back(p);
            alts += sv.alt_allele;
            alt_off.push_back(alts.size());
            uint64_t ref = 1;                             // a DEL's cut [preceding, end], the contig's length at most
            if (sv.sv_type == SVType::DEL) {
                const uint64_t preceding = sv.start >= 2 && sv.start < 0x80000000u ? sv.start - 1 : 1;
                ref = sv.end >= preceding ? std::min<uint64_t>(contig_len, sv.end - preceding + 1) : 1;
            }
            bound += chr.size() + ref + sv.alt_allele.size() + sv_method.size() + 400;
        }
        call_off[t + 1] = calls.size();
    }
    std::vector<uint8_t> status(calls.size() + 1);
    std::string text((size_t)bound, '\0');
    csv_vcf_format_counts fc{};
    int rc = csvgpu_vcf_format(ctx, genome, tab.data(), (uint32_t)n_contigs, call_off.data(), calls.data(), alt_off.data(), alts.data(), sv_method.data(),
                               (uint32_t)sv_method.size(), text.size(), &text[0], status.data(), &fc);
    if (rc == CSV_ECAPACITY) {                            // (the bound holds; handled all the same)
        text.assign((size_t)fc.text_bytes, '\0');
        rc = csvgpu_vcf_format(ctx, genome, tab.data(), (uint32_t)n_contigs, call_off.data(), calls.data(), alt_off.data(), alts.data(), sv_method.data(),
                               (uint32_t)sv_method.size(), text.size(), &text[0], status.data(), &fc);
    }
    if (rc != CSV_OK) {
        g_vcf_host_batches++;
        if (rc == 1) g_vcf_declined++;
        return false;
    }
    g_vcf_device_batches++;
    // the host loop's messages, contig by contig: the REF warnings in record order, then the depth warnings (the gather follows the records)
    for (size_t t = 0; t < n_contigs; t++) {
        const std::string &chr = contigs[t].first;
        printMessage("Saving SV calls for " + chr + "...");
        const std::vector<SVCall> &v = *contigs[t].second;
        for (size_t i = 0; i < v.size(); i++) {
            const uint8_t st = status[(size_t)call_off[t] + i];
            const SVCall &sv = v[i];
            if ((st & ST_DISPOSITION) == ST_SKIP_FIRST_POSITION)
                std::cerr << "Error: Insertion at the first position " << chr << ":" << sv.start << "-" << sv.end << std::endl;
            else if ((st & ST_EMPTY_REF) && sv.sv_type == SVType::DEL)
                std::cerr << "Warning: Reference allele is empty for deletion at " << chr << ":" << sv.start << "-" << sv.end << std::endl;
            else if (st & ST_EMPTY_REF)
                std::cerr << "Warning: Reference allele is empty for insertion at " << chr << ":" << sv.start - 1 << "-" << sv.end << std::endl;
        }
        for (size_t i = 0; i < v.size(); i++) {
            if (!(status[(size_t)call_off[t] + i] & ST_DEPTH_OUT_OF_RANGE)) continue;
            const SVCall &sv = v[i];
            const uint32_t pos = sv.sv_type == SVType::DEL ? (uint32_t)std::max(1, (int)sv.start - 1) : sv.sv_type == SVType::INS ? sv.start - 1 : sv.start;
            printError("Warning: Read depth for position " + std::to_string(pos) + " is out of range of the depth map");
        }
    }
    out.write(text.data(), (std::streamsize)fc.text_bytes);
    counts.total = (int)fc.total; counts.unclassified = (int)fc.unclassified; counts.assembly_gap_filtered = (int)fc.gap_filtered;
    return true;
}
}  // namespace

void vcfRouteStats(uint64_t *out, bool reset)
{
    out[0] = g_vcf_device_batches.load(); out[1] = g_vcf_host_batches.load(); out[2] = g_vcf_declined.load();
    if (reset) { g_vcf_device_batches = 0; g_vcf_host_batches = 0; g_vcf_declined = 0; }
}

std::string svMethodString()
{
    return "ContextSV v" + std::to_string(kVersionMajor) + "." + std::to_string(kVersionMinor) + "." + std::to_string(kVersionPatch);
}

void HostDepthSource::depthAt(const std::string &chr, const std::vector<uint32_t> &pos, std::vector<int32_t> &out) const
{
    const std::vector<uint32_t> &d = map.at(chr);
    out.resize(pos.size());
    for (size_t i = 0; i < pos.size(); i++) out[i] = pos[i] < d.size() ? (int32_t)d[pos[i]] : -1;
}

void ShardDepthSource::depthAt(const std::string &chr, const std::vector<uint32_t> &pos, std::vector<int32_t> &out) const
{
    csv_shard *sh = shards.at(chr);
    out.resize(pos.size());
    if (pos.empty()) return;
    if (csvgpu_depth_lookup_resident(ctx, sh, pos.data(), pos.size(), out.data()) != CSV_OK)
        throw std::runtime_error(std::string("depth lookup: ") + csvgpu_last_error(ctx));
}

bool loadAssemblyGaps(const std::string &path, std::unordered_map<std::string, std::vector<std::pair<uint32_t, uint32_t>>> &gaps)
{
    std::ifstream in(path);
    if (!in.is_open()) return false;
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream iss(line);
        std::string chr;
        uint32_t start, end;
        if (!(iss >> chr >> start >> end)) {
            printError("Failed to parse assembly gap file line: " + line);
            continue;
        }
        gaps[chr].emplace_back(start, end);
    }
    return true;
}

VCFCounts writeVCF(std::ostream &out, const std::vector<std::pair<std::string, const std::vector<SVCall> *>> &contigs, const VCFOptions &opt,
                   const std::unordered_map<std::string, std::vector<std::pair<uint32_t, uint32_t>>> &gaps, const ReferenceGenome &ref_genome,
                   const DepthSource &depth)
{
    VCFCounts counts;
    const std::string sv_method = svMethodString();

    std::string date = opt.file_date;
    if (date.empty()) {
        char buf[80];
        time_t raw;
        time(&raw);
        strftime(buf, sizeof buf, "%Y%m%d", localtime(&raw));
        date = buf;
    }
    std::string text;
    text += "##fileformat=VCFv4.2\n";
    text += "##fileDate=" + date + "\n";
    text += "##source=" + sv_method + "\n";
    text += "##reference=" + ref_genome.getFilepath() + "\n";
    text += ref_genome.getContigHeader() + "\n";
    for (const char *line : kHeaderLines) { text += line; text += '\n'; }
    text += "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tSAMPLE\n";
    out << text;

    if (opt.format_on_device && formatOnDevice(out, contigs, opt, gaps, ref_genome, depth, sv_method, counts)) {
        out.flush();
        return counts;
    }

    std::vector<Record> recs;
    std::vector<uint32_t> positions;
    std::vector<int32_t> depths;
    std::vector<ReferenceGenome::Cut> cuts;
    std::vector<std::string> refs;
    for (const auto &entry : contigs) {
        const std::string &chr = entry.first;
        printMessage("Saving SV calls for " + chr + "...");
        recs.clear();
        positions.clear();
        const auto gap_it = gaps.find(chr);
        // The contig's REF lookups in one call (one fetch where the genome lives on the device): the cuts of the calls that will ask for one,
        // by the gating of the loop below, in its order. Unmasked: ALT takes its first base from REF before REF is masked.
        cuts.clear();
        for (const SVCall &sv : *entry.second) {
            if (sv.sv_type == SVType::UNKNOWN || sv.sv_type == SVType::NEUTRAL) continue;
            if (sv.sv_type == SVType::DEL) cuts.push_back({(uint32_t)std::max(1, (int)sv.start - 1), sv.end});
            else if (sv.sv_type == SVType::INS && (int)sv.start > 1) cuts.push_back({sv.start - 1, sv.start - 1});
        }
        ref_genome.queryMany(chr, cuts, false, refs);
        size_t next_ref = 0;
        for (const SVCall &sv : *entry.second) {
            uint32_t start = sv.start, end = sv.end;
            int sv_length = (int)(end - start + 1);
            std::string ref_allele = ".", alt_allele = sv.alt_allele;
            const std::string genotype = getGenotypeString(sv.genotype);
            const std::string aln = getSVAlignmentTypeString(sv.aln_type);
            const char *filter = "PASS";
            const char *loh = getSVTypeFromCNState(sv.cn_state) == SVType::LOH ? ";LOH" : "";   // throws for states outside 0..6, as the table lookup does (:1199)

            if (sv.sv_type == SVType::UNKNOWN || sv.sv_type == SVType::NEUTRAL) { counts.unclassified++; continue; }
            counts.total++;

            // more than 20 % of the call inside one assembly gap (BED rows are 0-based; :1212-1239)
            if (gap_it != gaps.end()) {
                for (const auto &gap : gap_it->second) {
                    const uint32_t ov_start = std::max(start, gap.first + 1), ov_end = std::min(end, gap.second + 1);
                    if (ov_start <= ov_end && (double)(ov_end - ov_start + 1) / (double)sv_length > 0.2) {
                        filter = "AssemblyGap";
                        counts.assembly_gap_filtered++;
                        break;
                    }
                }
            }

            if (sv.sv_type == SVType::DEL) {
                // REF = preceding base + deleted bases, ALT = preceding base, POS on the preceding base (:1242-1260)
                const uint32_t preceding = (uint32_t)std::max(1, (int)start - 1);
                ref_allele = refs[next_ref++];
                if (ref_allele != "") {
                    alt_allele = ref_allele.substr(0, 1);
                } else {
                    ref_allele = "N";
                    alt_allele = "<DEL>";
                    std::cerr << "Warning: Reference allele is empty for deletion at " << chr << ":" << start << "-" << end << std::endl;
                }
                sv_length = -sv_length;
                start = preceding;
            } else if (sv.sv_type == SVType::INS) {
                // POS and END on the preceding base, its letter in front of a sequence ALT (:1265-1287)
                if ((int)start > 1) {
                    start -= 1;
                    ref_allele = refs[next_ref++];
                    if (ref_allele != "") {
                        if (alt_allele != "<INS>") alt_allele.insert(0, ref_allele);
                    } else {
                        ref_allele = "N";
                        alt_allele = "<INS>";
                        std::cerr << "Warning: Reference allele is empty for insertion at " << chr << ":" << start << "-" << end << std::endl;
                    }
                } else {
                    std::cerr << "Error: Insertion at the first position " << chr << ":" << start << "-" << end << std::endl;
                    continue;
                }
                end = start;
            } else {
                ref_allele = "N";                 // DUP / INV / BND convention (:1289-1291)
            }
            for (char &base : ref_allele) if (kAmb.amb[(unsigned char)base]) base = 'N';

            Record r;
            r.pos = start;
            r.head.reserve(ref_allele.size() + alt_allele.size() + 192);
            r.head += chr; r.head += '\t'; r.head += std::to_string(start); r.head += "\t.\t"; r.head += ref_allele; r.head += '\t';
            r.head += alt_allele; r.head += "\t.\t"; r.head += filter;
            r.head += "\tEND=" + std::to_string(end) + ";SVTYPE=" + getSVTypeString(sv.sv_type) + ";SVLEN=" + std::to_string(sv_length) +
                      ";SVMETHOD=" + sv_method + ";ALN=" + aln + ";HMM=" + std::to_string(sv.hmm_likelihood) + ";SUPPORT=";
            r.tail = ";CLUSTER=" + std::to_string(sv.cluster_size) + ";ALNOFFSET=" + std::to_string(sv.aln_offset) + ";CN=" +
                     std::to_string(sv.cn_state) + loh + "\tGT:DP\t" + genotype + ":";
            positions.push_back(r.pos);
            recs.push_back(std::move(r));
        }
        if (recs.empty()) continue;

        depth.depthAt(chr, positions, depths);    // one gather per contig
        text.clear();
        for (size_t i = 0; i < recs.size(); i++) {
            int read_depth = depths[i];
            if (read_depth < 0) {                 // getReadDepth's out_of_range branch (:1337-1341)
                printError("Warning: Read depth for position " + std::to_string(recs[i].pos) + " is out of range of the depth map");
                read_depth = 0;
            }
            const std::string d = std::to_string(read_depth);
            text += recs[i].head; text += d; text += recs[i].tail; text += d; text += '\n';
        }
        out << text;
    }
    out.flush();
    return counts;
}

bool saveToVCF(const std::unordered_map<std::string, std::vector<SVCall>> &sv_calls, const VCFOptions &opt, const ReferenceGenome &ref_genome,
               const DepthSource &depth, VCFCounts *counts_out)
{
    std::unordered_map<std::string, std::vector<std::pair<uint32_t, uint32_t>>> gaps;
    if (!opt.assembly_gaps.empty()) {
        printMessage("Loading assembly gap file: " + opt.assembly_gaps);
        if (!loadAssemblyGaps(opt.assembly_gaps, gaps)) {
            printError("Failed to open assembly gap file: " + opt.assembly_gaps);
            return false;
        }
        printMessage("Loaded " + std::to_string(gaps.size()) + " assembly gaps.");
    }
    const std::string path = opt.output_dir + "/output.vcf";
    printMessage("Writing VCF file to " + path);
    std::ofstream vcf(path);
    if (!vcf.is_open()) {
        printError("Failed to open VCF file for writing.");
        return false;
    }
    std::vector<std::pair<std::string, const std::vector<SVCall> *>> order;
    order.reserve(sv_calls.size());
    for (const auto &entry : sv_calls) order.emplace_back(entry.first, &entry.second);
    const VCFCounts c = writeVCF(vcf, order, opt, gaps, ref_genome, depth);
    vcf.close();
    printMessage("Finished writing VCF file. Total records: " + std::to_string(c.total));
    if (c.unclassified > 0) printMessage("Total unclassified SVs: " + std::to_string(c.unclassified));
    printMessage("Total filtered assembly gaps: " + std::to_string(c.assembly_gap_filtered));
    if (counts_out) *counts_out = c;
    return true;
}
