"""ctypes bindings of the C-ABI in include/csvgpu.h (plumbing only — no compute happens in Python).

The product path fails loudly when the HIP library is missing or no GPU is usable: there is no
CPU fallback behind these bindings (the oracle under oracle/ is test infrastructure and is never
imported from this package).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# CSVGPU_LIB: another build of the same library (tests: lib/libcsvgpu_testhooks.so, which also exports the allocation-failure hook)
LIB_PATH = os.environ.get("CSVGPU_LIB") or os.path.join(_HERE, "lib", "libcsvgpu.so")
ABI_VERSION = 4          # include/csvgpu.h CSVGPU_ABI_VERSION

CSV_OK, CSV_EINVAL, CSV_ENODEV, CSV_ENOMEM, CSV_EHIP, CSV_ECAPACITY = 0, -1, -2, -3, -4, -5
STATUS_NAMES = {0: "CSV_OK", -1: "CSV_EINVAL", -2: "CSV_ENODEV", -3: "CSV_ENOMEM", -4: "CSV_EHIP", -5: "CSV_ECAPACITY"}

K_CIGAR_SCAN, K_DEPTH, K_SORT, K_DBSCAN, K_DBSCAN1D, K_WINDOW, K_VITERBI, K_MISC, K_SPLIT_ORDER, K_SPLIT_GROUPS, K_SPLIT_FITS, K_COUNT = range(12)
KERNEL_NAMES = ["cigar_scan", "depth", "sort", "dbscan", "dbscan1d", "window", "viterbi", "misc", "split_order", "split_groups", "split_fits"]

SIG_DTYPE = np.dtype([("start", "<u4"), ("end", "<u4"), ("read", "<u4"), ("qpos_kind", "<u4")])
KIND_INS, KIND_DEL, KIND_CLIP = 0, 1, 2
# csv_split_fit: one overlap group's evidence (csvgpu_split_fits), 64 bytes
SPLIT_FIT_DTYPE = np.dtype([("median", "<i4", (6,)), ("size", "<u4", (6,)), ("n_members", "<u4"), ("n_opposite", "<u4"), ("reserved", "<u4", (2,))])


class CsvError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {msg}")
        self.status = status


class csv_reads(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_cigar", C.c_uint64), ("pos", C.c_void_p), ("flag", C.c_void_p),
                ("mapq", C.c_void_p), ("tid", C.c_void_p), ("cigar_off", C.c_void_p), ("cigar", C.c_void_p)]


class csv_hmm(C.Structure):
    _fields_ = [("A", C.c_double * 36), ("pi", C.c_double * 6), ("B1_mean", C.c_double * 6), ("B1_sd", C.c_double * 6),
                ("B1_uf", C.c_double), ("B2_mean", C.c_double * 5), ("B2_sd", C.c_double * 5), ("B2_uf", C.c_double)]


class csv_chr_result(C.Structure):
    _fields_ = [("n_sig", C.c_uint64), ("n_del", C.c_uint64), ("n_ins", C.c_uint64), ("depth_sum", C.c_uint64),
                ("depth_nonzero", C.c_uint32), ("min_pts", C.c_int32), ("mean_cov", C.c_double),
                ("sig_del", C.c_void_p), ("sig_ins", C.c_void_p), ("label_del", C.c_void_p), ("label_ins", C.c_void_p),
                ("depth", C.c_void_p), ("ref_end", C.c_void_p), ("q_start", C.c_void_p), ("q_end", C.c_void_p)]


class csv_tuning(C.Structure):
    _fields_ = [("scan_form", C.c_int32), ("split_tail", C.c_int32), ("sort_three_launch", C.c_int32), ("dbscan_all_pairs", C.c_int32),
                ("split_chain_only", C.c_int32)]


class csv_merge_counts(C.Structure):
    _fields_ = [("n_rep", C.c_uint64 * 2), ("n_declined", C.c_uint64 * 2)]


class csv_merge_rep(C.Structure):
    _fields_ = [("sig", C.c_uint32 * 4), ("label", C.c_int32), ("cluster_size", C.c_uint32), ("status", C.c_uint32), ("reserved", C.c_uint32)]


# csv_merge_rep as a numpy record: the chosen signature's four words, then the bucket's
MERGE_REP_DTYPE = np.dtype([("start", "<u4"), ("end", "<u4"), ("read", "<u4"), ("qpos_kind", "<u4"), ("label", "<i4"), ("cluster_size", "<u4"),
                            ("status", "<u4"), ("reserved", "<u4")])
REP_CHOSEN, REP_PASS_THROUGH, REP_DECLINED = 0, 1, 2
SORT_SLOT_LDS_CAP = 4096      # contextsv_amd/csrc/sort_select_core.hpp LDS_CAP: the largest range a workgroup replays in LDS
SORT_SLOT_NONE = 0xFFFFFFFF


class csv_split_tables(C.Structure):
    _fields_ = [("n_members", C.c_uint64), ("n_supp", C.c_uint64), ("start", C.c_void_p), ("end", C.c_void_p), ("q_start", C.c_void_p),
                ("q_end", C.c_void_p), ("reverse", C.c_void_p), ("supp_off", C.c_void_p), ("supp_start", C.c_void_p), ("supp_end", C.c_void_p),
                ("supp_q_start", C.c_void_p), ("supp_q_end", C.c_void_p), ("supp_flags", C.c_void_p)]


class csv_split_refs(C.Structure):
    _fields_ = [("n_members", C.c_uint64), ("n_supp", C.c_uint64), ("member_rec", C.c_void_p), ("supp_off", C.c_void_p), ("supp_rec", C.c_void_p),
                ("supp_where", C.c_void_p)]


class csv_bgzf_block(C.Structure):
    _fields_ = [("in_off", C.c_uint64), ("out_off", C.c_uint64), ("in_len", C.c_uint32), ("out_len", C.c_uint32), ("crc32", C.c_uint32),
                ("reserved", C.c_uint32)]


# the same 32 bytes as a numpy record
BGZF_BLOCK_DTYPE = np.dtype([("in_off", "<u8"), ("out_off", "<u8"), ("in_len", "<u4"), ("out_len", "<u4"), ("crc32", "<u4"), ("reserved", "<u4")])


class csv_bam_out(C.Structure):
    _fields_ = [("pos", C.c_void_p), ("flag", C.c_void_p), ("mapq", C.c_void_p), ("cigar_off", C.c_void_p), ("cigar", C.c_void_p), ("seq_off", C.c_void_p),
                ("seq", C.c_void_p), ("name_off", C.c_void_p), ("name", C.c_void_p), ("name_hash", C.c_void_p), ("cap_records", C.c_uint64),
                ("cap_cigar", C.c_uint64), ("cap_seq", C.c_uint64), ("cap_name", C.c_uint64)]


class csv_bam_counts(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("kept_first", C.c_uint64), ("n_kept", C.c_uint64), ("n_cigar", C.c_uint64), ("n_seq", C.c_uint64),
                ("n_name", C.c_uint64), ("consumed", C.c_uint64), ("status", C.c_uint64), ("stopped", C.c_uint32), ("reserved", C.c_uint32)]


class csv_vcf_out(C.Structure):
    _fields_ = [("line_off", C.c_void_p), ("chrom_len", C.c_void_p), ("pos", C.c_void_p), ("value", C.c_void_p), ("defer_off", C.c_void_p),
                ("cap", C.c_uint64), ("cap_defer", C.c_uint64)]


class csv_vcf_counts(C.Structure):
    _fields_ = [("n_lines", C.c_uint64), ("n_kept", C.c_uint64), ("n_deferred", C.c_uint64), ("stop_off", C.c_uint64), ("status", C.c_uint64)]


class csv_snp_runs(C.Structure):
    _fields_ = [("run_first", C.c_void_p), ("run_line_off", C.c_void_p), ("run_chrom_len", C.c_void_p), ("defer_off", C.c_void_p),
                ("cap_runs", C.c_uint64), ("cap_defer", C.c_uint64)]


class csv_snp_append_counts(C.Structure):
    _fields_ = [("n_lines", C.c_uint64), ("n_kept", C.c_uint64), ("n_deferred", C.c_uint64), ("n_runs", C.c_uint64), ("first_run", C.c_uint64),
                ("status", C.c_uint64)]


VCF_TILE_BYTES = 4096    # include/csvgpu.h CSV_VCF_TILE_BYTES
VCF_HEADER_LINE = 1      # csv_vcf_counts::status reason
VCF_NO_STOP = (1 << 64) - 1


class csv_shard_sizes(C.Structure):
    _fields_ = [("n_reads", C.c_uint64), ("n_cigar", C.c_uint64), ("n_seq", C.c_uint64), ("n_name", C.c_uint64)]


# csv_vcf_call: csvhost_call's layout (host.CALL_DTYPE is the same dtype)
VCF_CALL_DTYPE = np.dtype([("start", "<u4"), ("end", "<u4"), ("sv_type", "<i4"), ("cluster_size", "<i4"), ("hmm_likelihood", "<f8"),
                           ("id", "<i8"), ("aln_flags", "<u4"), ("genotype", "<i4"), ("cn_state", "<i4"), ("aln_offset", "<i4")])
# the status byte of a call (csrc/vcf_format_core.hpp): disposition in the low two bits, flags above; why a batch is declined
VCF_WRITTEN, VCF_SKIP_UNCLASSIFIED, VCF_SKIP_FIRST_POSITION, VCF_DISPOSITION, VCF_EMPTY_REF, VCF_GAP_FILTERED, VCF_DEPTH_OUT_OF_RANGE = 0, 1, 2, 3, 4, 8, 16
VCF_WHY_LIKELIHOOD, VCF_WHY_DEL_LENGTH, VCF_WHY_ENUM, VCF_WHY_NO_RECORD, VCF_WHY_DEL_START, VCF_WHY_TEXT_BYTES = 1, 2, 3, 4, 5, 6


class csv_vcf_contig(C.Structure):
    _fields_ = [("name", C.c_void_p), ("name_len", C.c_uint32), ("genome_record", C.c_int64), ("shard", C.c_void_p),
                ("gap_start", C.c_void_p), ("gap_end", C.c_void_p), ("n_gaps", C.c_uint32)]


class csv_vcf_format_counts(C.Structure):
    _fields_ = [("text_bytes", C.c_uint64), ("n_lines", C.c_uint64), ("total", C.c_uint32), ("unclassified", C.c_uint32),
                ("gap_filtered", C.c_uint32), ("declined_why", C.c_uint32)]


class csv_genome_counts(C.Structure):
    _fields_ = [("n_records", C.c_uint64), ("n_name_bytes", C.c_uint64), ("total_bases", C.c_uint64), ("n_text_bytes", C.c_uint64), ("n_lines", C.c_uint64)]


# csv_shard_builder's `want` bits
SB_SEQ, SB_NAMES, SB_NAME_HASH = 1, 2, 4

# csv_bam_counts::status: (offset << 8) | reason
BAM_SHORT, BAM_LONG, BAM_NEG_LSEQ, BAM_FIELDS, BAM_ANCHOR = 1, 2, 3, 4, 5
BAM_REASONS = {1: "record shorter than its fixed fields", 2: "implausible record length", 3: "negative sequence length",
               4: "record fields exceed the record length", 5: "anchor missed"}


class csv_cn_regions(C.Structure):
    _fields_ = [("n_shards", C.c_int32), ("shards", C.c_void_p), ("mean_cov", C.c_void_p), ("reg_off", C.c_void_p), ("region_start", C.c_void_p),
                ("region_end", C.c_void_p), ("sample_size", C.c_void_p), ("snp_off", C.c_void_p), ("snp_pos", C.c_void_p), ("snp_baf", C.c_void_p),
                ("snp_pfb", C.c_void_p)]


class csv_cn_table_regions(C.Structure):
    _fields_ = [("n_shards", C.c_int32), ("shards", C.c_void_p), ("tables", C.c_void_p), ("mean_cov", C.c_void_p), ("reg_off", C.c_void_p),
                ("region_start", C.c_void_p), ("region_end", C.c_void_p), ("sample_size", C.c_void_p)]


# every symbol include/csvgpu.h declares: name -> (restype, argtypes)
_P = C.c_void_p
ABI = {
    "csvgpu_create": (_P, [C.c_int, _P]),
    "csvgpu_create_background": (_P, [C.c_int]),
    "csvgpu_destroy": (None, [_P]),
    "csvgpu_abi_version": (C.c_int, []),
    "csvgpu_last_error": (C.c_char_p, [_P]),
    "csvgpu_synchronize": (C.c_int, [_P]),
    "csvgpu_timing_enable": (C.c_int, [_P, C.c_int]),
    "csvgpu_timing_reset": (C.c_int, [_P]),
    "csvgpu_timing_get": (C.c_int, [_P, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "csvgpu_set_tuning": (C.c_int, [_P, C.POINTER(csv_tuning)]),
    "csvgpu_set_cigar_packing": (C.c_int, [_P, C.c_int]),
    "csvgpu_cigar_scan": (C.c_int, [_P, C.POINTER(csv_reads), C.c_uint32, C.c_uint32, C.c_uint8, _P, C.POINTER(C.c_uint64)]),
    "csvgpu_aln_intervals": (C.c_int, [_P, C.POINTER(csv_reads), _P, _P, _P]),
    "csvgpu_depth": (C.c_int, [_P, C.POINTER(csv_reads), C.c_uint32, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]),
    "csvgpu_dbscan_iv": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_double, C.c_int32, _P]),
    "csvgpu_dbscan_iv_batch": (C.c_int, [_P, _P, _P, _P, C.c_uint64, C.c_double, C.c_int32, _P]),
    "csvgpu_dbscan_1d": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_double, C.c_int32, _P]),
    "csvgpu_window_log2": (C.c_int, [_P, _P, C.c_uint32, _P, _P, _P, _P, C.c_uint64, C.c_double, _P, _P, _P]),
    "csvgpu_viterbi": (C.c_int, [_P, C.POINTER(csv_hmm), _P, _P, _P, _P, C.c_uint64, _P, _P]),
    "csvgpu_shard_upload": (_P, [_P, C.POINTER(csv_reads), C.c_uint32]),
    "csvgpu_shard_wrap_dev": (_P, [_P, C.POINTER(csv_reads), C.c_uint32]),
    "csvgpu_shard_free": (None, [_P, _P]),
    "csvgpu_chr_pipeline_dev": (C.c_int, [_P, _P, C.c_uint32, C.c_uint8, C.c_double, C.c_double, C.POINTER(csv_chr_result)]),
    "csvgpu_chr_pipeline_fetch": (C.c_int, [_P, _P, C.c_uint32, C.c_uint8, C.c_double, C.c_double, C.POINTER(csv_chr_result), _P, _P, C.c_uint64]),
    "csvgpu_sort_slot": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.c_uint32, _P, _P]),
    "csvgpu_merge_select": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint64, C.c_uint32, _P, C.c_uint64, C.POINTER(csv_merge_counts)]),
    "csvgpu_chr_merge_select": (C.c_int, [_P, _P, C.POINTER(csv_chr_result), C.c_uint32, _P, C.c_uint64, C.POINTER(csv_merge_counts)]),
    "csvgpu_chr_job_cluster_select": (C.c_int, [_P, _P, C.c_double, C.c_uint32, _P, C.c_uint64, _P]),
    "csvgpu_chr_job_begin": (_P, [_P, _P, C.c_uint32, C.c_uint8, C.c_double]),
    "csvgpu_chr_job_cluster": (C.c_int, [_P, _P, C.c_double, _P, _P, C.c_uint64]),
    "csvgpu_chr_job_end": (C.c_int, [_P, _P, C.POINTER(csv_chr_result)]),
    "csvgpu_chr_job_abort": (C.c_int, [_P, _P]),
    "csvgpu_gate_create": (_P, []),
    "csvgpu_gate_open": (C.c_int, [_P, C.c_int]),
    "csvgpu_gate_destroy": (None, [_P]),
    "csvgpu_set_gate": (C.c_int, [_P, _P]),
    "csvgpu_host_alloc": (_P, [_P, C.c_size_t]),
    "csvgpu_host_free": (None, [_P, _P]),
    "csvgpu_aln_intervals_resident": (C.c_int, [_P, _P, _P, _P, _P]),
    "csvgpu_aln_intervals_gather_resident": (C.c_int, [_P, _P, _P, C.c_uint64, _P, _P, _P]),
    "csvgpu_aln_intervals_gather_batch": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P]),
    "csvgpu_shard_set_qname_hash": (C.c_int, [_P, _P, _P]),
    "csvgpu_split_order": (C.c_int, [_P, C.c_int, _P, C.c_uint8, _P, C.c_uint64, _P, C.c_uint64, _P]),
    "csvgpu_split_order_begin": (C.c_int, [_P, C.c_int, _P, C.c_uint8]),
    "csvgpu_split_order_begin_self": (C.c_int, [_P, C.c_int, _P, C.c_uint8]),
    "csvgpu_split_order_finish": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint64, _P]),
    "csvgpu_split_groups": (C.c_int, [_P, _P, _P, _P, C.c_uint64, _P, _P, _P, C.POINTER(C.c_uint64)]),
    "csvgpu_split_fits": (C.c_int, [_P, C.POINTER(csv_split_tables), _P, C.c_uint64, _P, _P, _P, C.c_double, C.c_int32, _P]),
    "csvgpu_split_groups_fits": (C.c_int, [_P, C.POINTER(csv_split_tables), _P, C.c_uint64, C.c_double, C.c_int32, _P, _P, C.POINTER(C.c_uint64)]),
    "csvgpu_split_tables_resident": (C.c_int, [_P, C.c_uint64, _P, C.POINTER(csv_split_refs), _P, C.POINTER(csv_split_tables)]),
    "csvgpu_split_resident_fits": (C.c_int, [_P, C.c_uint64, _P, C.POINTER(csv_split_refs), _P, C.c_double, C.c_int32, _P, _P, C.POINTER(C.c_uint64)]),
    "csvgpu_cn_observations_resident_many": (C.c_int, [_P, C.POINTER(csv_cn_regions), _P, _P, _P, _P, _P, _P, C.POINTER(C.c_uint64)]),
    "csvgpu_cn_decode_resident_many": (C.c_int, [_P, C.POINTER(csv_cn_regions), C.POINTER(csv_hmm), _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_uint64)]),
    "csvgpu_snp_table_create": (_P, [_P, _P, _P, _P, _P, C.c_uint64]),
    "csvgpu_snp_table_create_hits": (_P, [_P, _P, _P, _P, _P, C.c_uint64, C.c_uint64]),
    "csvgpu_snp_table_create_dev": (_P, [_P, _P, _P, _P, _P, C.c_uint64]),
    "csvgpu_snp_table_create_hits_dev": (_P, [_P, _P, _P, _P, _P, C.c_uint64, C.c_uint64]),
    "csvgpu_snp_table_free": (None, [_P, _P]),
    "csvgpu_snp_table_size": (C.c_uint64, [_P]),
    "csvgpu_snp_table_query": (C.c_int, [_P, _P, _P, _P, C.c_uint64, _P, _P, _P, _P, C.POINTER(C.c_uint64)]),
    "csvgpu_cn_observations_tables_many": (C.c_int, [_P, C.POINTER(csv_cn_table_regions), _P, _P, _P, _P, _P, _P, C.POINTER(C.c_uint64)]),
    "csvgpu_cn_decode_tables_many": (C.c_int, [_P, C.POINTER(csv_cn_table_regions), C.POINTER(csv_hmm), _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(C.c_uint64)]),
    "csvgpu_bgzf_inflate": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P, C.c_uint64, _P]),
    "csvgpu_bgzf_inflate_dev": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, _P, C.c_uint64, _P]),
    "csvgpu_bam_unpack": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, C.c_int32, C.c_int64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(csv_bam_out),
                                    C.POINTER(csv_bam_counts)]),
    "csvgpu_bam_unpack_dev": (C.c_int, [_P, _P, C.c_uint64, _P, C.c_uint32, C.c_int32, C.c_int64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(csv_bam_out),
                                        C.POINTER(csv_bam_counts)]),
    "csvgpu_vcf_snp_parse": (C.c_int, [_P, _P, C.c_uint64, C.c_int, C.c_int, C.POINTER(csv_vcf_out), C.POINTER(csv_vcf_counts)]),
    "csvgpu_vcf_snp_parse_dev": (C.c_int, [_P, _P, C.c_uint64, C.c_int, C.c_int, C.POINTER(csv_vcf_out), C.POINTER(csv_vcf_counts)]),
    "csvgpu_vcf_af_parse": (C.c_int, [_P, _P, C.c_uint64, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, _P, C.c_uint64, C.POINTER(csv_vcf_out),
                                      C.POINTER(csv_vcf_counts)]),
    "csvgpu_vcf_af_parse_dev": (C.c_int, [_P, _P, C.c_uint64, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, _P, C.c_uint64, C.POINTER(csv_vcf_out),
                                          C.POINTER(csv_vcf_counts)]),
    "csvgpu_shard_builder_create": (_P, [_P, C.c_uint32, C.POINTER(csv_shard_sizes)]),
    "csvgpu_shard_builder_append_bam": (C.c_int, [_P, _P, _P, C.c_uint64, _P, C.c_uint32, C.c_int32, C.c_int64, C.POINTER(csv_bam_counts)]),
    "csvgpu_shard_builder_append_host": (C.c_int, [_P, _P, C.POINTER(csv_reads), _P, _P, _P, _P, _P]),
    "csvgpu_shard_builder_sizes": (C.c_int, [_P, _P, C.POINTER(csv_shard_sizes)]),
    "csvgpu_shard_builder_finish": (_P, [_P, _P, C.c_uint32]),
    "csvgpu_shard_builder_destroy": (None, [_P, _P]),
    "csvgpu_shard_sizes": (C.c_int, [_P, _P, C.POINTER(csv_shard_sizes)]),
    "csvgpu_shard_cigar_bytes": (C.c_uint64, [_P]),
    "csvgpu_shard_fetch_reads": (C.c_int, [_P, _P, _P, _P, _P, _P, _P]),
    "csvgpu_shard_fetch_names": (C.c_int, [_P, _P, _P, _P, _P]),
    "csvgpu_shard_drop_sequences": (C.c_int, [_P, _P]),
    "csvgpu_alt_bases_resident": (C.c_int, [_P, _P, _P, _P, _P, C.c_uint64, _P]),
    "csvgpu_genome_builder_create": (_P, [_P, C.c_uint64]),
    "csvgpu_genome_builder_append": (C.c_int, [_P, _P, _P, C.c_uint64]),
    "csvgpu_genome_builder_append_dev": (C.c_int, [_P, _P, _P, C.c_uint64]),
    "csvgpu_genome_builder_finish": (_P, [_P, _P]),
    "csvgpu_genome_builder_destroy": (None, [_P, _P]),
    "csvgpu_genome_free": (None, [_P, _P]),
    "csvgpu_genome_describe": (C.c_int, [_P, _P, C.c_uint64, C.c_uint64, _P, _P, _P, C.POINTER(csv_genome_counts)]),
    "csvgpu_genome_fetch": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint64, C.c_int, _P]),
    "csvgpu_vcf_format": (C.c_int, [_P, _P, _P, C.c_uint32, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint64, _P, _P, C.POINTER(csv_vcf_format_counts)]),
    "csvgpu_vcf_format_dev": (C.c_int, [_P, _P, _P, C.c_uint32, _P, _P, _P, _P, _P, C.c_uint32, C.c_uint64, _P, _P, C.POINTER(csv_vcf_format_counts)]),
    "csvgpu_snp_builder_create": (_P, [_P, C.c_uint64]),
    "csvgpu_snp_builder_append": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(csv_snp_runs), C.POINTER(csv_snp_append_counts)]),
    "csvgpu_snp_builder_append_dev": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(csv_snp_runs), C.POINTER(csv_snp_append_counts)]),
    "csvgpu_snp_builder_append_host": (C.c_int, [_P, _P, C.c_uint64, _P, _P, _P, _P]),
    "csvgpu_snp_builder_finish": (_P, [_P, _P, _P, C.c_uint64]),
    "csvgpu_snp_builder_destroy": (None, [_P, _P]),
    "csvgpu_snp_columns_describe": (C.c_int, [_P, C.c_uint64, _P, _P, _P, C.POINTER(C.c_uint64)]),
    "csvgpu_snp_columns_fetch": (C.c_int, [_P, _P, C.c_uint32, _P, _P]),
    "csvgpu_snp_columns_af_parse": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint64, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(csv_vcf_out),
                                              C.POINTER(csv_vcf_counts)]),
    "csvgpu_snp_columns_af_parse_dev": (C.c_int, [_P, _P, C.c_uint32, _P, C.c_uint64, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.POINTER(csv_vcf_out),
                                                  C.POINTER(csv_vcf_counts)]),
    "csvgpu_snp_columns_table": (_P, [_P, _P, C.c_uint32, _P, _P, C.c_uint64]),
    "csvgpu_snp_columns_free": (None, [_P, _P]),
    "csvgpu_window_log2_resident": (C.c_int, [_P, _P, _P, _P, _P, _P, C.c_uint64, C.c_double, _P, _P, _P]),
    "csvgpu_window_log2_resident_many": (C.c_int, [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "csvgpu_chr_fetch": (C.c_int, [_P, _P, C.POINTER(csv_chr_result), _P, _P]),
    "csvgpu_depth_lookup_resident": (C.c_int, [_P, _P, _P, C.c_uint64, _P]),
    "csvgpu_download": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "csvgpu_dev_alloc": (_P, [_P, C.c_size_t]),
    "csvgpu_dev_free": (None, [_P, _P]),
    "csvgpu_upload": (C.c_int, [_P, _P, _P, C.c_size_t]),
    "csvgpu_dbscan_iv_dev": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_double, C.c_int32, _P]),
    "csvgpu_dbscan_1d_dev": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint64, C.c_uint32, C.c_double, C.c_int32, _P]),
    "csvgpu_window_log2_dev": (C.c_int, [_P, _P, C.c_uint32, _P, _P, _P, _P, C.c_uint64, C.c_uint64, C.c_double, _P, _P, _P]),
    "csvgpu_viterbi_dev": (C.c_int, [_P, C.POINTER(csv_hmm), _P, _P, _P, _P, C.c_uint64, C.c_uint64, _P, _P]),
}

# the CSV_TEST_HOOKS block of include/csvgpu.h beside csvgpu_test_fail_next_alloc: registered only where the loaded build exports them
TEST_HOOKS = {
    "csvgpu_test_radix_sort": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_int32, C.c_int32, _P, _P, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]),
    "csvgpu_test_radix_sort_devn": (C.c_int, [_P, _P, _P, C.c_uint64, C.c_uint64, C.c_int32, _P, _P, C.POINTER(C.c_uint32), C.POINTER(C.c_int32)]),
    "csvgpu_test_exclusive_sum": (C.c_int, [_P, _P, C.c_uint64]),
    "csvgpu_test_prefix_max": (C.c_int, [_P, _P, C.c_uint64, _P]),
}

_lib = None


def load() -> C.CDLL:
    """Load libcsvgpu.so (built in-tree by __graft_entry__.build()). Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"HIP extension not built: {LIB_PATH} is missing — run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the product path)")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in ABI.items():
        fn = getattr(lib, name)          # AttributeError here = ABI mismatch, which must be loud
        fn.restype = res
        fn.argtypes = args
    got = lib.csvgpu_abi_version()
    if got != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} has ABI version {got}, this package expects {ABI_VERSION}: rebuild (__graft_entry__.build())")
    if hasattr(lib, "csvgpu_test_fail_next_alloc"):          # only in the test build (libcsvgpu_testhooks.so via CSVGPU_LIB)
        lib.csvgpu_test_fail_next_alloc.restype = None
        lib.csvgpu_test_fail_next_alloc.argtypes = [C.c_int]
    for name, (res, args) in TEST_HOOKS.items():             # the same build's hooks on the device primitives (tests/sort_primitives_check.py)
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
    _lib = lib
    return lib


def ptr(a):
    """Host pointer of a C-contiguous numpy array (or None)."""
    if a is None:
        return None
    assert a.flags["C_CONTIGUOUS"]
    return a.ctypes.data


def make_hmm(A, pi, B1_mean, B1_sd, B1_uf, B2_mean, B2_sd, B2_uf) -> csv_hmm:
    h = csv_hmm()
    h.A[:] = list(np.asarray(A, dtype=np.float64).reshape(36))
    h.pi[:] = list(np.asarray(pi, dtype=np.float64))
    h.B1_mean[:] = list(np.asarray(B1_mean, dtype=np.float64))
    h.B1_sd[:] = list(np.asarray(B1_sd, dtype=np.float64))
    h.B1_uf = float(B1_uf)
    h.B2_mean[:] = list(np.asarray(B2_mean, dtype=np.float64))
    h.B2_sd[:] = list(np.asarray(B2_sd, dtype=np.float64))
    h.B2_uf = float(B2_uf)
    return h
