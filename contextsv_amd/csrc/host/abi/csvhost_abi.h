/* csvhost_abi.h — the plain structs that cross the host mirror's C ABI (libcontextsv_host.so). C-compatible, declarations only;
 * contextsv_amd/host.py keeps a ctypes twin of each (tests/test_run_options.py holds the two together). */
#ifndef CSVHOST_ABI_H
#define CSVHOST_ABI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* POD view of an SVCall for tests (alt allele / flags travel separately) */
struct csvhost_call {
    uint32_t start, end;
    int32_t  sv_type;
    int32_t  cluster_size;
    double   hmm_likelihood;
    int64_t  id;            /* caller's tag, carried through merges in aln_offset-independent form */
    uint32_t aln_flags;     /* SVEvidenceFlags bits */
    int32_t  genotype, cn_state, aln_offset;
};

struct csvhost_chr_stats {
    uint64_t n_signatures, n_del, n_ins, depth_sum;
    uint32_t depth_nonzero; int32_t min_pts;
    double mean_cov, ms_device, ms_host_merge;
    uint64_t n_calls;
};

struct csvhost_stage_times {
    double ms_cigar, ms_cigar_cn, ms_split_fetch, ms_split, ms_split_cn, ms_merge_split, ms_merge_final, ms_vcf, ms_total, ms_split_prepare;
    uint64_t n_reads, n_signatures, n_cigar_calls, n_cigar_cn_regions, n_split_calls, n_final_calls;
};

struct csvhost_bam_stats { uint64_t n_contigs, n_reads, n_cigar, bam_bytes; double ms_decode, ms_total;
                           uint64_t unpack_batches_device, unpack_batches_host, unpack_anchors, unpack_batches_kept_on_device;
                           uint64_t contigs_resident, unpack_batches_appended_host; };

/* What a caller may set of a run (csvhost_run, csvhost_genome_run, csvhost_run_bam): one field per RunParams / RunSchedule field of
 * sv_caller.h, same name, same sense; flags are 0 / 1. csvhost_run_options_init fills `size` and RunParams' own defaults; an entry point
 * reads the fields its run reads and refuses a struct whose `size` is not its own. */
struct csvhost_run_options {
    uint32_t size;                      /* sizeof(csvhost_run_options) */
    double dbscan_epsilon;
    double dbscan_min_pts_pct;
    int32_t sample_size;
    int32_t min_cnv_length;
    int32_t host_threads;
    int32_t cigar_cn;
    int32_t split_svs;
    int32_t merge_split_svs;
    int32_t merge_final_svs;
    int32_t split_order_on_device;
    int32_t overlap_split_prepare;
    int32_t split_groups_on_device;
    int32_t split_fits_on_device;
    int32_t split_tables_on_device;
    int32_t cn_observations_on_device;
    int32_t inflate_on_device;
    int32_t inflate_device;
    int32_t unpack_on_device;
    int32_t shard_on_device;
    int32_t save_cnv;
    int32_t early_batches;              /* RunSchedule::EarlyBatches: 0 timed, 1 none, 2 all at once, 3 every three */
    int32_t split_beside_pass;
    int32_t split_order_self;
    int32_t prepare_delay_ms;
};

void csvhost_run_options_init(struct csvhost_run_options *opt);

#ifdef __cplusplus
}
#endif
#endif
