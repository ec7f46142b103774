// split_caller.h — host mirror of SVCaller::findSplitSVSignatures (src/sv_caller.cpp:68-504): split-alignment evidence ->
// SPLITDIST1 insertion / unknown candidates and SPLIT (or inversion) dummy calls for the copy-number pass.
//
// What moved to the GPU: the per-record CIGAR walk of the reference's third BAM pass (getAlignmentReadPositions +
// bam_endpos, :152, :162) — the scan kernel already produced ref_end / q_start / q_end for every record — and the six
// DBSCAN1D(100, 5) fits per overlap group (:270-372), which are collected for ALL groups of a chromosome and solved by
// one batched launch for the whole genome (DBSCAN1D::fitBatch -> csvgpu_dbscan_1d). What stays here: the order-defining
// steps (SURVEY §7 hard part 2) — the iteration order of the reference's qname-keyed unordered_map, replayed exactly by
// umap_order.h instead of building 6e5 string-keyed nodes per chromosome; the (unbalanced) interval tree that order builds; the
// overlap groups, medians and votes — one host thread per contig, contigs being independent. The tree and the groups can also come from
// the device for a whole batch of contigs (SplitGroupSource below: csvgpu_split_groups, the same lists member for member); off unless
// SplitParams::device_groups is set.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "sv_object.h"

// One alignment record as the split pass sees it (file order).
struct SplitRecord {
    int32_t  tid;
    int32_t  pos;        // 0-based
    uint16_t flag;
    uint8_t  mapq;
    int32_t  ref_end;    // bam_endpos           } from the scan kernel
    int32_t  q_start;    // query_start          } (csv_chr_result.ref_end / q_start / q_end
    int32_t  q_end;      // query_end            }  or csvgpu_aln_intervals)
};

// Where the scan kernel's per-record intervals come from when they are not handed over as whole arrays: only the records that take
// part in a group (primaries with a supplementary record, and those records) are ever asked for — a few per cent of a contig — and
// for all contigs in one request.
struct IntervalSource {
    virtual ~IntervalSource() = default;
    // contig which[k] (index into the `contigs` vector): records rec[rec_off[k] .. rec_off[k+1]) (ascending, distinct) -> their
    // ref_end / q_start / q_end at the same positions of the three outputs
    virtual void gather(const std::vector<size_t> &which, const std::vector<uint32_t> &rec, const std::vector<uint64_t> &rec_off,
                        int32_t *ref_end, int32_t *q_start, int32_t *q_end) const = 0;
};

// The surviving primaries of several contigs, each in the iteration order of the reference's per-chromosome qname map, computed
// somewhere else than on this host thread (the device: csvgpu_split_order behind ShardOrderSource in sv_caller.cpp).
struct SplitOrderSource {
    virtual ~SplitOrderSource() = default;
    // which[k] indexes the `contigs` vector of findSplitSVSignatures; recs[k] = record indices of contig which[k]'s primaries whose name
    // hash is in supp_hash (sorted, distinct), in iteration order. Only asked for contigs with SplitContig::unique_names.
    virtual void survivors(const std::vector<size_t> &which, int min_mapq, const std::vector<uint64_t> &supp_hash, std::vector<std::vector<uint32_t>> &recs) const = 0;
    // Optional head start: called with the same `which` before the supplementary records have been collected, so that whatever does not
    // depend on them (on the device: the nodes and all but the last epochs of every map, csvgpu_split_order_begin) runs meanwhile.
    // `complete`: `which` holds every contig of the run that has records — every supplementary record of the run is one of theirs, so the
    // source may take the supplementary hashes from its own copy of the records (csvgpu_split_order_begin_self: nothing then waits for
    // the collection) and ignore the ones survivors() is given.
    virtual void begin(const std::vector<size_t> &which, int min_mapq, bool complete) const { (void)which; (void)min_mapq; (void)complete; }
};

// The overlap groups of several contigs (the interval tree and the greedy seeding of sv_caller.cpp:215-238, :948-980), computed somewhere else
// than on the host threads (the device: csvgpu_split_groups behind ShardGroupSource in sv_caller.cpp).
struct SplitGroupSource {
    virtual ~SplitGroupSource() = default;
    // segment k = members [seg_off[k], seg_off[k+1]) of one contig in the iteration order of its qname map, each the closed interval
    // [start, end] (pos + 1, bam_endpos). -> the groups with more than one member: segment k's are [seg_group_off[k], seg_group_off[k+1]) in seed
    // order, group g's members are members[group_off[g] .. group_off[g+1]): indices WITHIN the segment, in findOverlaps' traversal order.
    // One call per batch of contigs; asked from the thread that runs finishEarly / finishFor / finish.
    virtual void groups(const std::vector<int32_t> &start, const std::vector<int32_t> &end, const std::vector<uint64_t> &seg_off,
                        std::vector<uint64_t> &seg_group_off, std::vector<uint64_t> &group_off, std::vector<uint32_t> &members) const = 0;
};

// What the reference derives from every overlap group before it makes calls (sv_caller.cpp:248-416: strand vote, six point sets, six DBSCAN1D fits,
// largest clusters, medians), computed somewhere else than on the host threads (the device: csvgpu_split_fits / csvgpu_split_groups_fits behind
// ShardFitSource in sv_caller.cpp). The tables are csv_split_tables' arrays for a batch of contigs, the record is csv_split_fit.
struct SplitFitTables {
    std::vector<int32_t> start, end, q_start, q_end;      // [members]: pos + 1, bam_endpos, query_start, query_end; map iteration order per segment
    std::vector<uint8_t> reverse;                         // [members]: 1 = FLAG 0x10
    std::vector<uint64_t> supp_off;                       // [members + 1]
    std::vector<int32_t> supp_start, supp_end, supp_q_start, supp_q_end;
    std::vector<uint8_t> supp_flags;                      // bit 0 reverse strand, bit 1 on another tid than the primary
};
struct SplitFit {
    int32_t  median[6];               // sets in the order of Group::sets (split_caller.cpp); sorted largest cluster [size / 2], 0 when there is none
    uint32_t size[6];                 // points in the largest cluster
    uint32_t n_members, n_opposite;   // the strand vote's two counts (:248-265)
    uint32_t reserved[2];
};
struct SplitFitSource {
    virtual ~SplitFitSource() = default;
    // segment k = members [seg_off[k], seg_off[k+1]). groups given (seg_group_off / group_off / members as SplitGroupSource::groups returns them):
    // their fits; groups == nullptr: the source computes the groups itself (the same ones) and returns their seg_group_off. fits[g] per group.
    struct Groups { const std::vector<uint64_t> *seg_group_off, *group_off; const std::vector<uint32_t> *members; };
    virtual void fits(const SplitFitTables &tables, const std::vector<uint64_t> &seg_off, const Groups *groups, double eps, int min_pts,
                      std::vector<uint64_t> &seg_group_off, std::vector<SplitFit> &fits) const = 0;
};

// The same evidence from record REFERENCES: for contigs whose records lie in resident shards (those served by an IntervalSource) nothing of the tables
// has to be gathered, built or uploaded — the device builds them from the shards (csvgpu_split_resident_fits behind ShardTableSource in sv_caller.cpp).
// csv_split_refs' arrays for a batch of contigs.
struct SplitRefTables {
    std::vector<uint32_t> member_rec;                     // [members]: the primary's record index in its contig, map iteration order per segment
    std::vector<uint64_t> supp_off;                       // [members + 1]
    std::vector<uint32_t> supp_rec;                       // [entries]: record index in ITS contig (read by the device only when supp_where == 0)
    std::vector<uint8_t> supp_where;                      // [entries]: 0 = on the member's contig, else 2 | reverse strand
    std::vector<int32_t> supp_tid;                        // [entries]: the entry's tid (for tests and tools; no source reads it)
};
struct SplitTableSource {
    virtual ~SplitTableSource() = default;
    // segment k = members [seg_off[k], seg_off[k+1]) of contig which[k] (index into the `contigs` vector). -> the groups' seg_group_off and fits[g] per group,
    // as SplitFitSource::fits returns them without given groups. One call per batch; asked from the thread that runs finishEarly / finishFor / finish.
    virtual void fits(const std::vector<size_t> &which, const SplitRefTables &refs, const std::vector<uint64_t> &seg_off, double eps, int min_pts,
                      std::vector<uint64_t> &seg_group_off, std::vector<SplitFit> &fits) const = 0;
};

struct SplitParams {
    int min_mapq = 20;        // sv_caller.h:72
    double eps = 100;         // DBSCAN1D(100, 5) at sv_caller.cpp:270
    int min_pts = 5;
    int min_length = 2000;    // :243
    int max_length = 1000000; // :244
    const IntervalSource *intervals = nullptr;        // for contigs given without ref_end / q_start / q_end arrays
    const SplitOrderSource *device_order = nullptr;   // where contigs with unique_names get their iteration order from (nullptr: replayed on the host)
    const SplitGroupSource *device_groups = nullptr;  // where the overlap groups come from (nullptr: the host's interval tree, one contig per host thread)
    const SplitFitSource *device_fits = nullptr;      // where the groups' point sets, fits, largest clusters and medians come from (nullptr: setsOf + one DBSCAN1D batch + the host's
                                                      // reductions); with device_groups also set the source computes the groups too and they never reach the host
    const SplitTableSource *device_tables = nullptr;  // contigs WITHOUT ref_end / q_start / q_end arrays (those `intervals` serves): tables, groups and fits from this source, given only
                                                      // record references — no interval gather, no members, no flattening for them; contigs with arrays keep the routes above
    int threads = 0;          // host threads over contigs (0: one per contig, at most the hardware's); the result does not depend on it
};

// The records of one contig (one tid), struct of arrays, file order — what a decoded shard holds on the host plus the scan
// kernel's intervals. Query names are needed for two things only: their std::hash<std::string> value (qhash: it fixes where the
// reference's unordered_map puts a read, see umap_order.h) and equality. Equality comes from the names themselves (name_bytes /
// name_off) or from run-wide dictionary ids (name_id: equal id <=> equal name) — at least one of the two must be given.
struct SplitContig {
    int32_t tid = 0;
    uint64_t n = 0;
    const int32_t *pos = nullptr;
    const uint16_t *flag = nullptr;
    const uint8_t *mapq = nullptr;
    const int32_t *ref_end = nullptr, *q_start = nullptr, *q_end = nullptr;   // whole arrays, or null: SplitParams::intervals is asked for the few records that matter
    const uint64_t *qhash = nullptr;
    const uint64_t *name_id = nullptr;
    const char *name_bytes = nullptr;
    const uint64_t *name_off = nullptr;      // [n + 1]
    bool unique_names = false;               // established when the contig was staged: no two non-supplementary records share a name hash
    const uint64_t *file_idx = nullptr;      // optional: position of each record in the file (default: contigs in the order given, records in array order)
};

// Fills sv_calls[target_names[tid]] for every contig that has primary alignments, like the reference. Contigs must be given in
// file order (or carry file_idx): a read's supplementary records are visited in file order.
void findSplitSVSignatures(const std::vector<SplitContig> &contigs, const std::vector<std::string> &target_names, const SplitParams &params,
                           std::unordered_map<std::string, std::vector<SVCall>> &sv_calls);

// The same in two halves: prepare() needs no alignment intervals (primaries / supplementaries, the map's iteration order, survivors) and may
// run while the scan kernel's outputs are still being produced; finish() does the rest. `contigs` and `target_names` must outlive the object.
class SplitPass {
public:
    SplitPass(const std::vector<SplitContig> &contigs, const std::vector<std::string> &target_names, const SplitParams &params);
    ~SplitPass();
    void prepare();
    void finish(std::unordered_map<std::string, std::vector<SVCall>> &sv_calls);
    // between the two: contigs (indices into the constructor's list) whose alignment intervals exist already — their interval gather and
    // overlap groups now instead of inside finish(); any subset, any number of times, after prepare()
    void finishEarly(const std::vector<size_t> &contig_ids);
    // finish() for a subset of the contigs (those of it not done yet): a contig's calls depend on nothing outside the contig, so any
    // partition of the contigs over calls gives the calls one finish() gives; finish() afterwards does what is left
    void finishFor(const std::vector<size_t> &contig_ids, std::unordered_map<std::string, std::vector<SVCall>> &sv_calls);
    // after prepare(): the record references of these contigs' members and supplementary entries (what SplitParams::device_tables is given), segment k =
    // contig contig_ids[k]
    void references(const std::vector<size_t> &contig_ids, SplitRefTables &refs, std::vector<uint64_t> &seg_off);
private:
    struct Impl;
    std::unique_ptr<Impl> p;
    bool prepared = false;
};

// Same, from records in file order (any mix of tids) and their names as strings.
void findSplitSVSignatures(const std::vector<SplitRecord> &records, const std::vector<std::string> &qnames,
                           const std::vector<std::string> &target_names, const SplitParams &params,
                           std::unordered_map<std::string, std::vector<SVCall>> &sv_calls);

// The references prepare() computes, from records in file order and their names: segment t = the members of tid t (t < n_targets), record indices counted
// within the tid's records in file order (a contig uploaded as its own shard). Needs no alignment intervals and no device.
void splitReferences(const std::vector<SplitRecord> &records, const std::vector<std::string> &qnames, size_t n_targets, const SplitParams &params,
                     SplitRefTables &refs, std::vector<uint64_t> &seg_off);

// The overlap groups of csvgpu_split_groups computed by the host's interval tree (the path SplitParams::device_groups == nullptr takes), same
// outputs: seg_group_off [n_seg + 1], group_off [groups + 1], members. Throws std::invalid_argument on end < start or descending offsets.
void splitGroupsHost(const int32_t *start, const int32_t *end, const uint64_t *seg_off, uint64_t n_seg, std::vector<uint64_t> &seg_group_off,
                     std::vector<uint64_t> &group_off, std::vector<uint32_t> &members);

// The records of csvgpu_split_fits by the route SplitParams::device_fits == nullptr takes — the six point sets of every group built on this thread, ONE
// DBSCAN1D batch for all of them (csvgpu_dbscan_1d on the host mirror's context), largest clusters and medians on this thread: what tools/bench_split_fits.py
// measures the device entry points against. Throws std::invalid_argument on tables that do not fit.
void splitFitsHost(const SplitFitTables &tables, const std::vector<uint64_t> &seg_off, const std::vector<uint64_t> &seg_group_off,
                   const std::vector<uint64_t> &group_off, const std::vector<uint32_t> &members, double eps, int min_pts, std::vector<SplitFit> &fits);
