// fasta_query.h — reference-genome lookup with the reference's interface (include/fasta_query.h:16-44,
// src/fasta_query.cpp:18-185): whole FASTA in memory, 1-based inclusive queries returning views.
// The file is read in one block and split in place instead of getline + string append per line.
// Opt-in device backing (setFilepath with FastaDeviceOptions): the mapped file goes up in windows through csvgpu_genome_builder_*, no host
// sequence exists, and the queries are csvgpu_genome_fetch calls on the genome's own context. Same results either way.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

struct csv_ctx;
struct csv_genome;

struct FastaDeviceOptions {
    csv_ctx *ctx = nullptr;           // the context the genome is built on and fetched through
    uint64_t window_bytes = 0;        // bytes of the file per append; 0: 256 MiB
};
struct FastaDeviceStats {
    uint64_t bytes_uploaded = 0, lines = 0, records = 0, bases = 0;   // what the builder took and made
    uint64_t fetch_calls = 0, items_fetched = 0;                       // csvgpu_genome_fetch calls and their items
    uint64_t fallback = 0;                                             // 1: the builder refused and the host loader read the whole file
};

class ReferenceGenome {
public:
    ReferenceGenome();
    ~ReferenceGenome();
    ReferenceGenome(const ReferenceGenome &) = delete;
    ReferenceGenome &operator=(const ReferenceGenome &) = delete;

    // 0 on success, 1 for an empty path; a file that cannot be opened is fatal in the reference (exit(1), :31-35):
    // here it throws std::runtime_error so that a library caller decides.
    int setFilepath(std::string fasta_filepath);
    // The same with the sequences on the device. A builder refusal (a contig of 2^32 bytes or more, CSV_ENOMEM, any failure of an append)
    // falls back to the host loader for the whole file; deviceStats().fallback says so.
    int setFilepath(std::string fasta_filepath, const FastaDeviceOptions &opt);
    std::string getFilepath() const { return fasta_filepath; }

    // [pos_start, pos_end], 1-based inclusive; empty view when pos_end is past the contig or pos_start > pos_end (:88-102).
    // Unknown contig: std::out_of_range, as unordered_map::at. With a device backing: one fetch, and the view stays valid until the
    // calling thread's next query.
    std::string_view query(const std::string &chr, uint32_t pos_start, uint32_t pos_end) const;

    // fraction of equal characters against compare_seq >= match_threshold (:105-136)
    bool compare(const std::string &chr, uint32_t pos_start, uint32_t pos_end, const std::string &compare_seq, float match_threshold) const;

    // Many cuts of one contig: out[i] = query(chr, cuts[i]), ambiguity codes of either case as N when mask. Device backing: ONE fetch. Host
    // backing: a loop over query. No cut: nothing is looked up (and an unknown contig is not an error).
    struct Cut { uint32_t pos_start, pos_end; };
    void queryMany(const std::string &chr, const std::vector<Cut> &cuts, bool mask, std::vector<std::string> &out) const;

    // "##contig=<ID=…,length=…>" lines, contigs in std::sort order, no trailing newline (:139-162)
    std::string getContigHeader() const;
    std::vector<std::string> getChromosomes() const { return chromosomes; }   // sorted; duplicates kept (:50, :73, :78)
    uint32_t getChromosomeLength(std::string chr) const;                       // 0 + printError when unknown (:169-180)

    // in-memory construction for tests / synthetic runs: same post-conditions as setFilepath
    void addContig(const std::string &name, std::string sequence);

    bool onDevice() const { return dev != nullptr; }
    // The device genome and the context it was built on (both null with a host backing), and a name's record in it: the LAST record of a
    // duplicated name, as the loader's map decides; -1 when the genome has none. For csvgpu_vcf_format (host/vcf_writer.cpp).
    const csv_genome *deviceGenome(csv_ctx **ctx = nullptr) const;
    int64_t deviceRecord(const std::string &chr) const;
    FastaDeviceStats deviceStats() const;

private:
    void loadHost(const char *text, size_t n);            // the host loader over the mapped file
    struct Device;                                        // the genome's handle, its context, the name -> record table, the counters
    std::string fasta_filepath;
    std::vector<std::string> chromosomes;
    std::unordered_map<std::string, std::string> chr_to_seq;          // empty with a device backing
    std::unordered_map<std::string, uint32_t> chr_to_length;
    std::unique_ptr<Device> dev;
    FastaDeviceStats load_stats;                          // fallback only: what a load without a device genome leaves
};
