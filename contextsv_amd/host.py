"""ctypes bindings of the C++ host mirror (csrc/host/ -> lib/libcontextsv_host.so): mergeSVs and friends,
the per-chromosome SVCaller path, the HMM file parser and the synthetic shard generator. Plumbing only."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from .context import Context, Reads, Shard

# CONTEXTSV_HOST_LIB: another build of the host mirror (tests: the AddressSanitizer build, csrc/_obj/libcontextsv_host_asan.so)
HOST_LIB_PATH = os.environ.get("CONTEXTSV_HOST_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libcontextsv_host.so")

# the structs below are the twins of csrc/host/abi/csvhost_abi.h (tests/test_run_options.py holds the two together)
CALL_DTYPE = np.dtype([("start", "<u4"), ("end", "<u4"), ("sv_type", "<i4"), ("cluster_size", "<i4"), ("hmm_likelihood", "<f8"),
                       ("id", "<i8"), ("aln_flags", "<u4"), ("genotype", "<i4"), ("cn_state", "<i4"), ("aln_offset", "<i4")])


class run_options(C.Structure):
    """csvhost_run_options: what a caller may set of a run, one field per RunParams / RunSchedule field (same name, same sense)."""
    _fields_ = [("size", C.c_uint32), ("dbscan_epsilon", C.c_double), ("dbscan_min_pts_pct", C.c_double)] + \
               [(k, C.c_int32) for k in ("sample_size", "min_cnv_length", "host_threads", "cigar_cn", "split_svs", "merge_split_svs", "merge_final_svs",
                                         "split_order_on_device", "overlap_split_prepare", "split_groups_on_device", "split_fits_on_device",
                                         "split_tables_on_device", "cn_observations_on_device", "inflate_on_device", "inflate_device", "unpack_on_device",
                                         "shard_on_device", "save_cnv", "early_batches", "split_beside_pass", "split_order_self", "prepare_delay_ms")]


class chr_stats(C.Structure):
    _fields_ = [("n_signatures", C.c_uint64), ("n_del", C.c_uint64), ("n_ins", C.c_uint64), ("depth_sum", C.c_uint64),
                ("depth_nonzero", C.c_uint32), ("min_pts", C.c_int32), ("mean_cov", C.c_double), ("ms_device", C.c_double),
                ("ms_host_merge", C.c_double), ("n_calls", C.c_uint64)]


class bam_stats(C.Structure):
    _fields_ = [("n_contigs", C.c_uint64), ("n_reads", C.c_uint64), ("n_cigar", C.c_uint64), ("bam_bytes", C.c_uint64),
                ("ms_decode", C.c_double), ("ms_total", C.c_double), ("unpack_batches_device", C.c_uint64), ("unpack_batches_host", C.c_uint64),
                ("unpack_anchors", C.c_uint64), ("unpack_batches_kept_on_device", C.c_uint64), ("contigs_resident", C.c_uint64),
                ("unpack_batches_appended_host", C.c_uint64)]


class stage_times(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("ms_cigar", "ms_cigar_cn", "ms_split_fetch", "ms_split", "ms_split_cn", "ms_merge_split", "ms_merge_final",
                                          "ms_vcf", "ms_total", "ms_split_prepare")] + \
               [(k, C.c_uint64) for k in ("n_reads", "n_signatures", "n_cigar_calls", "n_cigar_cn_regions", "n_split_calls", "n_final_calls")]


_P = C.c_void_p
_hlib = None


def load() -> C.CDLL:
    global _hlib
    if _hlib is not None:
        return _hlib
    _lib.load()          # libcsvgpu.so first (the host mirror links against it)
    if not os.path.exists(HOST_LIB_PATH):
        raise RuntimeError(f"host mirror not built: {HOST_LIB_PATH} is missing — run __graft_entry__.build()")
    lib = C.CDLL(HOST_LIB_PATH)
    lib.csvhost_last_error.restype = C.c_char_p
    lib.csvhost_set_context.argtypes = [_P]
    lib.csvhost_set_quiet.argtypes = [C.c_int]
    lib.csvhost_merge_svs.argtypes = [_P, C.c_uint64, C.c_double, C.c_int32, C.c_int, _P, C.POINTER(C.c_uint64)]
    lib.csvhost_merge_type_with_labels.argtypes = [_P, _P, C.c_uint64, C.c_int, _P, C.POINTER(C.c_uint64)]
    lib.csvhost_merge_duplicates.argtypes = [_P, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.csvhost_add_sv_calls.argtypes = [_P, C.c_uint64, _P, C.POINTER(C.c_uint64)]
    lib.csvhost_synth_generate.restype = _P
    lib.csvhost_synth_generate.argtypes = [C.c_uint64, C.c_uint32, C.c_double, C.c_int, C.c_int, C.c_int]
    lib.csvhost_synth_view.argtypes = [_P, C.POINTER(_lib.csv_reads), C.POINTER(C.c_uint32), C.POINTER(_P), C.POINTER(_P)]
    lib.csvhost_synth_free.argtypes = [_P]
    lib.csvhost_process_resident_chromosome.argtypes = [_P, _P, _P, _P, C.c_double, C.c_double, _P, _P, C.c_uint64, C.POINTER(chr_stats)]
    lib.csvhost_process_resident_pipelined.argtypes = [_P, _P, C.c_uint64, _P, _P, C.c_double, C.c_double, _P, _P, C.c_uint64,
                                                       C.POINTER(chr_stats), C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.csvhost_query_snp_region.argtypes = [_P, _P, C.c_uint32, C.c_uint32, C.c_double, C.c_int, _P, _P, _P, _P, C.c_uint64,
                                             _P, _P, _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.csvhost_cn_prediction.argtypes = [_P, _P, C.c_int, _P, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(_lib.csv_hmm),
                                          C.c_double, C.c_int, C.c_uint32, _P, _P, _P, _P, C.c_uint64]
    lib.csvhost_query_snp_regions.argtypes = [_P, _P, C.c_uint64, _P, _P, C.c_double, C.c_int, _P, _P, _P, _P, C.c_uint64, C.c_int,
                                              _P, _P, _P, _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.csvhost_cn_prediction_device.argtypes = [_P, _P, C.c_int, _P, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(_lib.csv_hmm),
                                                 C.c_double, C.c_int, C.c_uint32, _P, _P, _P, _P, C.c_uint64, C.c_int]
    lib.csvhost_cn_prediction_table.argtypes = [_P, _P, C.c_int, _P, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(_lib.csv_hmm),
                                                C.c_double, C.c_int, C.c_uint32, _P, _P, _P, _P, C.c_uint64, C.c_int, _P]
    lib.csvhost_query_snp_regions_table.argtypes = [_P, _P, C.c_uint64, _P, _P, C.c_double, C.c_int, _P, _P, _P, _P, C.c_uint64, C.c_int, _P,
                                                    _P, _P, _P, _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.csvhost_genome_snp_tables_resident.argtypes = [_P, C.c_int]
    lib.csvhost_genome_merge_on_device.argtypes = [_P, C.c_int, C.c_uint32]
    lib.csvhost_set_merge_on_device.restype = None
    lib.csvhost_set_merge_on_device.argtypes = [C.c_int, C.c_uint32]
    lib.csvhost_merge_route_stats.restype = None
    lib.csvhost_merge_route_stats.argtypes = [_P, C.c_int]
    lib.csvhost_cn_table_capacity_hint.restype = C.c_uint64
    lib.csvhost_cn_table_capacity_hint.argtypes = [C.c_int]
    lib.csvhost_split_signatures.argtypes = [_P, C.c_uint64, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.csvhost_split_signatures_opts.argtypes = [_P, C.c_uint64, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.csvhost_split_signatures_dev.argtypes = [_P, C.c_uint64, _P, _P, _P, _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.csvhost_split_fits_host.argtypes = [_P, C.POINTER(_lib.csv_split_tables), _P, C.c_uint64, _P, _P, _P, C.c_double, C.c_int, _P]
    lib.csvhost_split_refs.argtypes = [C.c_uint64, _P, _P, _P, _P, _P, C.c_int, C.c_int, _P, _P, _P, _P, _P, _P, C.c_uint64, _P]
    lib.csvhost_split_groups_host.argtypes = [_P, _P, _P, C.c_uint64, _P, _P, _P, C.POINTER(C.c_uint64)]
    lib.csvhost_run_options_init.restype = None
    lib.csvhost_run_options_init.argtypes = [C.POINTER(run_options)]
    lib.csvhost_run.argtypes = [_P, C.c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, C.POINTER(_lib.csv_hmm), C.POINTER(run_options),
                                _P, _P, C.c_uint64, C.POINTER(C.c_uint64), _P, C.c_char_p, C.c_char_p, C.c_char_p, _P, C.c_uint64, _P]
    lib.csvhost_read_chmm.argtypes = [C.c_char_p, C.POINTER(_lib.csv_hmm), C.POINTER(C.c_int32)]
    lib.csvhost_sort_select_check.argtypes = [_P, C.c_uint64, C.c_uint64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.csvhost_partition_check.argtypes = [_P, C.c_uint64, C.POINTER(C.c_int)]
    lib.csvhost_sort_select_rounds.restype = C.c_int64
    lib.csvhost_sort_select_rounds.argtypes = [_P, C.c_uint64, C.c_uint64]
    lib.csvhost_fasta_open.restype = _P
    lib.csvhost_fasta_open.argtypes = [C.c_char_p]
    lib.csvhost_fasta_open_device.restype = _P
    lib.csvhost_fasta_open_device.argtypes = [C.c_char_p, _P, C.c_uint64]
    lib.csvhost_fasta_device_stats.restype = None
    lib.csvhost_fasta_device_stats.argtypes = [_P, _P]
    lib.csvhost_fasta_free.argtypes = [_P]
    lib.csvhost_fasta_query.restype = C.c_int64
    lib.csvhost_fasta_query.argtypes = [_P, C.c_char_p, C.c_uint32, C.c_uint32, _P, C.c_uint64]
    lib.csvhost_fasta_compare.argtypes = [_P, C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_float]
    lib.csvhost_fasta_length.restype = C.c_uint32
    lib.csvhost_fasta_length.argtypes = [_P, C.c_char_p]
    lib.csvhost_fasta_contig_header.restype = C.c_int64
    lib.csvhost_fasta_contig_header.argtypes = [_P, _P, C.c_uint64]
    lib.csvhost_fasta_chromosomes.restype = C.c_int64
    lib.csvhost_fasta_chromosomes.argtypes = [_P, _P, C.c_uint64]
    lib.csvhost_save_vcf.argtypes = [_P, C.c_char_p, _P, C.c_char_p, C.c_char_p, C.c_int, _P, _P, _P, _P, _P, _P, _P, C.c_int, _P]
    lib.csvhost_save_vcf_device.argtypes = lib.csvhost_save_vcf.argtypes + [C.c_int]
    lib.csvhost_vcf_route_stats.restype = None
    lib.csvhost_vcf_route_stats.argtypes = [_P, C.c_int]
    lib.csvhost_set_vcf_on_device.restype = None
    lib.csvhost_set_vcf_on_device.argtypes = [C.c_int]
    lib.csvhost_bam_open.restype = _P
    lib.csvhost_bam_open.argtypes = [C.c_char_p, C.c_int]
    lib.csvhost_bam_close.argtypes = [_P]
    lib.csvhost_bam_n_ref.argtypes = [_P]
    lib.csvhost_bam_names.restype = C.c_char_p
    lib.csvhost_bam_names.argtypes = [_P]
    lib.csvhost_bam_text.restype = C.c_char_p
    lib.csvhost_bam_text.argtypes = [_P]
    lib.csvhost_bam_ref_len.restype = C.c_uint32
    lib.csvhost_bam_ref_len.argtypes = [_P, C.c_int]
    lib.csvhost_bam_read.argtypes = [_P, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_uint64)]
    lib.csvhost_bam_set_device_inflate.argtypes = [_P, C.c_int]
    lib.csvhost_bam_set_device_unpack.argtypes = [_P, C.c_int]
    lib.csvhost_bam_unpack_stats.restype = None
    lib.csvhost_bam_unpack_stats.argtypes = [_P, C.POINTER(C.c_uint64 * 9)]
    lib.csvhost_bam_set_device_shard.restype = None
    lib.csvhost_bam_set_device_shard.argtypes = [_P, C.c_int]
    lib.csvhost_bam_shard_take_resident.restype = _P
    lib.csvhost_bam_shard_take_resident.argtypes = [_P, C.c_int, C.POINTER(C.c_uint64)]
    lib.csvhost_bgzf_inflate_file.argtypes = [C.c_char_p, C.c_int, _P, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    lib.csvhost_bam_shard.argtypes = [_P, C.c_int, C.POINTER(_lib.csv_reads), C.POINTER(C.c_int32), C.POINTER(C.c_uint32), C.POINTER(_P), C.POINTER(_P)]
    lib.csvhost_bam_shard_qnames.restype = C.c_int64
    lib.csvhost_bam_shard_qnames.argtypes = [_P, C.c_int, _P, C.c_uint64]
    lib.csvhost_bam_write.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, _P, C.c_uint64, _P, _P, _P, _P, _P, _P, C.c_char_p, _P, _P, _P,
                                      C.c_int, C.c_int]
    lib.csvhost_synth_write_bam.argtypes = [_P, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_uint64)]
    lib.csvhost_run_bam.argtypes = [_P, C.c_char_p, C.c_char_p, C.c_int, C.POINTER(_lib.csv_hmm), C.POINTER(run_options),
                                    _P, C.c_char_p, C.c_char_p, C.c_char_p, _P, _P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(bam_stats),
                                    C.c_char_p, C.c_char_p, C.c_char_p]
    lib.csvhost_snp_open.restype = _P
    lib.csvhost_snp_open.argtypes = [C.c_char_p, C.c_int]
    lib.csvhost_snp_free.argtypes = [_P]
    lib.csvhost_snp_open_device.restype = _P
    lib.csvhost_snp_open_device.argtypes = [C.c_char_p, C.c_int, _P, C.c_uint32]
    lib.csvhost_snp_open_device_tables.restype = _P
    lib.csvhost_snp_open_device_tables.argtypes = [C.c_char_p, C.c_int, _P, C.c_uint32]
    lib.csvhost_snp_build_stats.restype = None
    lib.csvhost_snp_build_stats.argtypes = [_P, _P]
    lib.csvhost_set_snp_on_device.restype = None
    lib.csvhost_set_snp_on_device.argtypes = [C.c_int, C.c_int]
    lib.csvhost_cn_route_stats.restype = None
    lib.csvhost_cn_route_stats.argtypes = [_P, C.c_int]
    lib.csvhost_snp_device_stats.restype = None
    lib.csvhost_snp_device_stats.argtypes = [_P, _P]
    lib.csvhost_snp_table.restype = C.c_int
    lib.csvhost_snp_table.argtypes = [_P, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, _P, _P, C.c_uint64, _P, _P, C.c_uint64, _P]
    lib.csvhost_snp_kept.restype = C.c_uint64
    lib.csvhost_snp_kept.argtypes = [_P]
    lib.csvhost_snp_query.restype = C.c_int64
    lib.csvhost_snp_query.argtypes = [_P, C.c_char_p, C.c_char_p, C.c_char_p, C.c_uint32, C.c_uint32, _P, _P, C.c_uint64, C.POINTER(C.c_int),
                                      C.POINTER(C.c_uint32), C.POINTER(C.c_double), C.c_int]
    lib.csvhost_pfb_path.restype = C.c_int64
    lib.csvhost_pfb_path.argtypes = [C.c_char_p, C.c_char_p, _P, C.c_uint64]
    lib.csvhost_gnomad_contig.restype = C.c_int64
    lib.csvhost_gnomad_contig.argtypes = [C.c_char_p, C.c_char_p, _P, C.c_uint64]
    lib.csvhost_process_resident_lanes.argtypes = [C.c_int, _P, _P, _P, C.c_double, C.c_double, _P, C.c_uint64, C.POINTER(chr_stats),
                                                   C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
    lib.csvhost_bam_writer_open.restype = _P
    lib.csvhost_bam_writer_open.argtypes = [C.c_char_p, C.c_int, C.c_char_p, _P, C.c_int, C.c_int]
    lib.csvhost_bam_writer_append_synth.argtypes = [_P, _P, C.c_int]
    lib.csvhost_bam_writer_close.argtypes = [_P]
    lib.csvhost_umap_order_check.argtypes = [C.c_char_p, C.c_uint64, _P, _P, _P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                             C.POINTER(C.c_uint64)]
    lib.csvhost_synth_qname_ids.restype = _P
    lib.csvhost_synth_qname_ids.argtypes = [_P]
    lib.csvhost_genome_create.restype = _P
    lib.csvhost_genome_free.argtypes = [_P]
    lib.csvhost_genome_add.argtypes = [_P, _P, C.c_char_p, C.c_int32, C.POINTER(_lib.csv_reads), C.c_uint32, _P, C.c_int, _P, _P, _P, _P, C.c_uint64]
    lib.csvhost_synth_generate2.restype = _P
    lib.csvhost_synth_generate2.argtypes = [C.c_uint64, C.c_uint32, C.c_double, C.c_int, C.c_int, C.c_int, C.c_double]
    lib.csvhost_genome_add_synth.argtypes = [_P, _P, C.c_char_p, C.c_int32, _P, C.c_uint64, C.c_int]
    lib.csvhost_genome_n_contigs.restype = C.c_uint64
    lib.csvhost_genome_n_contigs.argtypes = [_P]
    lib.csvhost_genome_contig_info.argtypes = [_P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(_P)]
    lib.csvhost_genome_run.argtypes = [_P, _P, C.c_int, _P, C.POINTER(_lib.csv_hmm), C.POINTER(run_options), _P, _P,
                                       C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(stage_times), _P]
    lib.csvhost_sig_alts.argtypes = [_P, C.c_uint64, _P, _P, _P, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.csvhost_process_resident_chromosome_alts.argtypes = [_P, _P, _P, _P, C.c_double, C.c_double, _P, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.csvhost_process_resident_chromosome_alts_resident.argtypes = [_P, _P, C.c_double, C.c_double, _P, C.c_uint64, C.POINTER(C.c_uint64)]
    lib.csvhost_par_selftest.argtypes = [C.c_int, C.c_int]
    lib.csvhost_string_hashes.argtypes = [C.c_char_p, C.c_uint64, _P]
    lib.csvhost_assign_shards.argtypes = [_P, C.c_uint64, C.c_int, _P]
    lib.csvhost_set_quiet(1)
    _hlib = lib
    return lib


def _check(rc):
    if rc != 0:
        raise RuntimeError((load().csvhost_last_error() or b"host error").decode())


def set_context(ctx: Context):
    load().csvhost_set_context(ctx.h)


def make_calls(start, end, sv_type, cluster_size=None, hmm_likelihood=None) -> np.ndarray:
    n = len(start)
    c = np.zeros(n, CALL_DTYPE)
    c["start"], c["end"], c["sv_type"] = start, end, sv_type
    c["cluster_size"] = 0 if cluster_size is None else cluster_size
    c["hmm_likelihood"] = 0.0 if hmm_likelihood is None else hmm_likelihood
    c["id"] = np.arange(n)
    c["genotype"] = 3
    return c


def merge_svs(calls: np.ndarray, eps: float, min_pts: int, keep_noise: bool) -> np.ndarray:
    """mergeSVs (host mirror; DBSCAN labels from the GPU). Needs set_context()."""
    calls = np.ascontiguousarray(calls, CALL_DTYPE)
    out = np.zeros(max(len(calls), 1), CALL_DTYPE)
    n = C.c_uint64(0)
    _check(load().csvhost_merge_svs(calls.ctypes.data, len(calls), eps, min_pts, int(keep_noise), out.ctypes.data, C.byref(n)))
    return out[: n.value].copy()


def merge_type_with_labels(calls: np.ndarray, labels: np.ndarray, keep_noise: bool) -> np.ndarray:
    calls = np.ascontiguousarray(calls, CALL_DTYPE)
    labels = np.ascontiguousarray(labels, np.int32)
    out = np.zeros(max(len(calls), 1), CALL_DTYPE)
    n = C.c_uint64(0)
    _check(load().csvhost_merge_type_with_labels(calls.ctypes.data, labels.ctypes.data, len(calls), int(keep_noise), out.ctypes.data, C.byref(n)))
    return out[: n.value].copy()


def merge_duplicates(calls: np.ndarray) -> np.ndarray:
    calls = np.ascontiguousarray(calls, CALL_DTYPE).copy()
    n = C.c_uint64(0)
    _check(load().csvhost_merge_duplicates(calls.ctypes.data, len(calls), C.byref(n)))
    return calls[: n.value].copy()


def add_sv_calls_order(calls: np.ndarray) -> np.ndarray:
    calls = np.ascontiguousarray(calls, CALL_DTYPE)
    ids = np.zeros(max(len(calls), 1), np.int64)
    n = C.c_uint64(0)
    _check(load().csvhost_add_sv_calls(calls.ctypes.data, len(calls), ids.ctypes.data, C.byref(n)))
    return ids[: n.value].copy()


class SynthShard:
    """A generated shard living in the host library's memory; `reads` are zero-copy numpy views."""

    def __init__(self, seed: int, chr_len: int, depth: float, tech: int = 0, threads: int = 8, with_seq: bool = False, sv_per_bp: float = 0.0):
        lib = load()
        self.h = lib.csvhost_synth_generate2(seed, chr_len, depth, tech, threads, int(with_seq), sv_per_bp)
        if not self.h:
            raise RuntimeError((lib.csvhost_last_error() or b"").decode())
        r = _lib.csv_reads()
        dl = C.c_uint32(0)
        so, sq = _P(), _P()
        lib.csvhost_synth_view(self.h, C.byref(r), C.byref(dl), C.byref(so), C.byref(sq))
        n, m = r.n_reads, r.n_cigar

        def view(p, count, dtype):
            if not p or count == 0:
                return np.zeros(0, dtype)
            buf = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(p)
            return np.frombuffer(buf, dtype=dtype)

        self.depth_len = dl.value
        self.reads = Reads.__new__(Reads)
        self.reads.pos = view(r.pos, n, np.int32)
        self.reads.flag = view(r.flag, n, np.uint16)
        self.reads.mapq = view(r.mapq, n, np.uint8)
        self.reads.tid = view(r.tid, n, np.int32)
        self.reads.cigar_off = view(r.cigar_off, n + 1, np.uint64)
        self.reads.cigar = view(r.cigar, m, np.uint32)
        self.seq_off_ptr, self.seq_ptr = so.value, sq.value
        self.qname_id = view(lib.csvhost_synth_qname_ids(self.h), n, np.uint32)

    def write_bam(self, path: str, chr_name: str = "chr22", level: int = 1, threads: int = 8) -> int:
        """The shard as a coordinate-sorted BAM + BAI on one contig; returns the BAM's size in bytes."""
        nbytes = C.c_uint64(0)
        _check(load().csvhost_synth_write_bam(self.h, os.fsencode(path), chr_name.encode(), level, threads, C.byref(nbytes)))
        return nbytes.value

    def free(self):
        if self.h:
            self.reads = None
            load().csvhost_synth_free(self.h)
            self.h = None


_EARLY_BATCHES = {"timed": 0, "none": 1, "all": 2, "every3": 3}          # RunSchedule::EarlyBatches
# keywords of Genome.run / run / run_bam whose run_options field has another name (the others are called what their field is called)
_OPTION_OF = {"eps": "dbscan_epsilon", "min_pts_pct": "dbscan_min_pts_pct", "min_cnv": "min_cnv_length", "overlap_split": "overlap_split_prepare"}
_OPTION_TYPES = dict(run_options._fields_[1:])


def _run_options(**keywords) -> run_options:
    """The library's defaults (csvhost_run_options_init: RunParams' own) with the fields set that the keywords name."""
    o = run_options()
    load().csvhost_run_options_init(C.byref(o))
    for key, value in keywords.items():
        if key == "early_batches":
            if value not in _EARLY_BATCHES:
                raise ValueError(f"early_batches must be one of {sorted(_EARLY_BATCHES)}, not {value!r}")
            o.early_batches = _EARLY_BATCHES[value]
        elif key == "merges":
            o.merge_split_svs = o.merge_final_svs = int(bool(value))
        elif key == "host_split_order":
            o.split_order_on_device = int(not value)
        else:
            field = _OPTION_OF.get(key, key)
            if field not in _OPTION_TYPES:
                raise TypeError(f"{key!r} is no run option")
            if field == "prepare_delay_ms" and not 0 <= int(value) < 1 << 31:
                raise ValueError(f"prepare_delay_ms must be in [0, {(1 << 31) - 1}], not {value!r}")
            setattr(o, field, value if _OPTION_TYPES[field] is C.c_double else int(value))
    if o.shard_on_device:
        o.unpack_on_device = 1
    return o


class Genome:
    """A staged genome: contigs resident in HBM + the small host arrays of the host-side passes; run() = SVCaller::runResident
    (one step of the whole-genome benchmark). Contigs are added through a Context (they may use different contexts of one GPU)."""

    def __init__(self):
        self.h = load().csvhost_genome_create()
        self.names = []

    def add(self, ctx: Context, name: str, global_tid: int, reads: Reads, depth_len: int, qname_id=None, snps=None, name_style: int = 0):
        rs = reads.c_struct()
        q = np.ascontiguousarray(qname_id, np.uint32) if qname_id is not None else None
        sp = np.ascontiguousarray(snps["pos"], np.uint32) if snps is not None else np.zeros(0, np.uint32)
        sb = np.ascontiguousarray(snps["baf"], np.float64) if snps is not None else np.zeros(0, np.float64)
        sf = np.ascontiguousarray(snps["pfb"], np.float64) if snps is not None and "pfb" in snps else None
        sh = np.ascontiguousarray(snps["has_pfb"], np.uint8) if snps is not None and "has_pfb" in snps else None
        _check(load().csvhost_genome_add(self.h, ctx.h, name.encode(), global_tid, C.byref(rs), depth_len, q.ctypes.data if q is not None else None,
                                         name_style, sp.ctypes.data, sb.ctypes.data, sf.ctypes.data if sf is not None else None,
                                         sh.ctypes.data if sh is not None else None, len(sp)))
        self.names.append(name)

    def add_synth(self, ctx: Context, name: str, global_tid: int, syn: "SynthShard", snp_seed: int = 0, with_snps: bool = True):
        _check(load().csvhost_genome_add_synth(self.h, ctx.h, name.encode(), global_tid, syn.h, snp_seed, int(with_snps)))
        self.names.append(name)

    def __len__(self):
        return int(load().csvhost_genome_n_contigs(self.h))

    def contig_info(self, i: int) -> dict:
        nr, nc, dl, gt, sh = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_int32(0), _P()
        load().csvhost_genome_contig_info(self.h, i, C.byref(nr), C.byref(nc), C.byref(dl), C.byref(gt), C.byref(sh))
        return {"n_reads": nr.value, "n_cigar": nc.value, "depth_len": dl.value, "global_tid": gt.value, "shard": sh.value}

    def run(self, ctx: Context, hmm, lanes=None, eps=0.1, min_pts_pct=0.1, sample_size=20, min_cnv=2000, split_svs=True, cigar_cn=True, merges=True,
            host_threads=0, capacity: int = 1 << 20, host_split_order: bool = False, overlap_split: bool = True, copy: bool = True,
            early_batches: str = "timed", split_beside_pass: bool = True, split_order_self: bool = True, prepare_delay_ms: int = 0,
            split_groups_on_device: bool = False, split_fits_on_device: bool = False, split_tables_on_device: bool = False,
            cn_observations_on_device: bool = False):
        """-> (calls[CALL_DTYPE], global tid per call, stage_times, per-contig chr_stats list). copy=False: the two arrays are views of buffers
        the genome owns (two sets, used alternately) and stay valid until the run after the next one. early_batches ("timed" | "none" | "all" |
        "every3"), split_beside_pass, split_order_self and prepare_delay_ms are RunParams::schedule: no result depends on them, they force
        the branches that timing otherwise decides. split_groups_on_device: the split-read pass's overlap groups from csvgpu_split_groups (one
        call per batch of contigs) instead of the host's interval tree; the calls are the same. split_fits_on_device: what the pass derives from
        every group (point sets, DBSCAN1D fits, largest clusters, medians, strand vote) from csvgpu_split_fits — with split_groups_on_device from
        csvgpu_split_groups_fits, the groups then staying on the device — instead of the host's sets and one DBSCAN1D batch; the calls are the same.
        split_tables_on_device: the members' and supplementary records' tables built on the device from the resident shards and fed straight into
        that chain (csvgpu_split_resident_fits): no interval gather, no members on the host, no upload; groups and fits then come from the device
        whatever the two other switches say; the calls are the same. cn_observations_on_device: the observation vectors of both copy-number
        passes built on the device from the window kernel's output and decoded there (csvgpu_cn_decode_resident_many) instead of windows back,
        the vectors assembled on the host pool and sent up again; the calls are the same."""
        opt = _run_options(eps=eps, min_pts_pct=min_pts_pct, sample_size=sample_size, min_cnv=min_cnv, split_svs=split_svs, cigar_cn=cigar_cn, merges=merges,
                           host_threads=host_threads, host_split_order=host_split_order, overlap_split=overlap_split, early_batches=early_batches,
                           split_beside_pass=split_beside_pass, split_order_self=split_order_self, prepare_delay_ms=prepare_delay_ms,
                           split_groups_on_device=split_groups_on_device, split_fits_on_device=split_fits_on_device,
                           split_tables_on_device=split_tables_on_device, cn_observations_on_device=cn_observations_on_device)
        n = len(self)
        if getattr(self, "_cap", 0) < capacity:              # result buffers live with the genome (tens of megabytes of page faults per call otherwise)
            self._bufs = [(np.empty(capacity, CALL_DTYPE), np.empty(capacity, np.int32)) for _ in range(2)]
            self._cap, self._flip = capacity, 0
        self._flip ^= 1
        out, tid = self._bufs[self._flip]
        k = C.c_uint64(0)
        st = stage_times()
        cs = (chr_stats * max(n, 1))()
        lanes = lanes or []
        lp = (C.c_void_p * max(len(lanes), 1))(*[c.h for c in lanes])
        _check(load().csvhost_genome_run(self.h, ctx.h, len(lanes), lp, C.byref(hmm), C.byref(opt), out.ctypes.data, tid.ctypes.data, capacity, C.byref(k), C.byref(st), cs))
        if k.value > capacity:
            raise RuntimeError("Genome.run: capacity too small")
        if copy:
            return out[: k.value].copy(), tid[: k.value].copy(), st, list(cs)[:n]
        return out[: k.value], tid[: k.value], st, list(cs)[:n]

    def snp_tables_resident(self, on: bool = True) -> int:
        """Opt-in: every staged contig's SNP table resident on its context's device (csvgpu_snp_table_create); run() then looks the SNPs of
        the copy-number passes up there instead of querying them on the host — same calls. on=False frees the tables (free() does too).
        -> the number of resident tables (a contig whose table the device refuses stays on the host route)."""
        return int(load().csvhost_genome_snp_tables_resident(self.h, int(bool(on))))

    def merge_on_device(self, on: bool = True, max_partitions: int = 0):
        """Opt-in: run() has the CIGAR merge's representatives chosen on the device (csvgpu_chr_job_cluster_select): only their records come
        back instead of every signature and label. Same calls and statistics; a contig with a bucket the device declines (max_partitions bounds
        the partitions per bucket, 0 = the library's own limit) takes the host route — merge_route_stats() says how many did."""
        _check(load().csvhost_genome_merge_on_device(self.h, int(bool(on)), int(max_partitions)))

    def free(self):
        if self.h:
            load().csvhost_genome_free(self.h)
            self.h = None


def assign_shards(weights, world: int) -> list:
    """SVCaller::assignShards (the C++ mirror of parallel.assign_shards): the shard indices of every rank, ascending."""
    w = np.ascontiguousarray(weights, np.float64)
    r = np.zeros(max(len(w), 1), np.int32)
    _check(load().csvhost_assign_shards(w.ctypes.data, len(w), world, r.ctypes.data))
    return [[int(i) for i in np.nonzero(r[: len(w)] == k)[0]] for k in range(world)]


def string_hashes(names) -> np.ndarray:
    """libstdc++ std::hash<std::string> of every name (uint64)."""
    out = np.zeros(max(len(names), 1), np.uint64)
    _check(load().csvhost_string_hashes("\n".join(names).encode(), len(names), out.ctypes.data))
    return out[: len(names)]


def umap_order_check(keys, erase_mask=None):
    """(order of a real std::unordered_map<std::string,int>, order from the replay in umap_order.h, bucket counts) — CPU only."""
    n = len(keys)
    blob = "\n".join(keys).encode()
    a, b = np.zeros(max(n, 1), np.int64), np.zeros(max(n, 1), np.int64)
    na, nb, ba, bb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    em = np.ascontiguousarray(erase_mask, np.uint8) if erase_mask is not None else None
    _check(load().csvhost_umap_order_check(blob, n, em.ctypes.data if em is not None else None, a.ctypes.data, b.ctypes.data, C.byref(na), C.byref(nb),
                                           C.byref(ba), C.byref(bb)))
    return a[: na.value].copy(), b[: nb.value].copy(), (ba.value, bb.value)


def sig_alts(sig: np.ndarray, seq_off=None, seq=None):
    """ALT string of every signature (SVCaller::toSVCall; host only). seq_off: uint64[n_reads + 1] byte offsets, seq: uint8 4-bit packed."""
    sig = np.ascontiguousarray(sig, _lib.SIG_DTYPE)
    so = np.ascontiguousarray(seq_off, np.uint64) if seq_off is not None else None
    sq = np.ascontiguousarray(seq, np.uint8) if seq is not None else None
    cap = 64 * len(sig) + 16
    buf = C.create_string_buffer(cap)
    ln = C.c_uint64(0)
    _check(load().csvhost_sig_alts(sig.ctypes.data, len(sig), so.ctypes.data if so is not None else None, sq.ctypes.data if sq is not None else None,
                                   buf, cap, C.byref(ln)))
    return buf.raw[: ln.value].decode().split("\n")[:-1]


def merge_ordered(sig: np.ndarray, labels: np.ndarray, n_del: int, reps: int = 1):
    """SVCaller::mergeOrdered alone (no device): ordered signatures + labels -> (merged calls, mean ms of one of `reps` repetitions)."""
    sig = np.ascontiguousarray(sig, _lib.SIG_DTYPE)
    labels = np.ascontiguousarray(labels, np.int32)
    cap = len(sig) // 2 + 4
    out = np.zeros(cap, CALL_DTYPE)
    n, ms = C.c_uint64(0), C.c_double(0)
    lib = load()
    lib.csvhost_merge_ordered.argtypes = [_P, _P, C.c_uint64, C.c_uint64, C.c_int, _P, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_double)]
    _check(lib.csvhost_merge_ordered(sig.ctypes.data, labels.ctypes.data, n_del, len(sig) - n_del, reps, out.ctypes.data, cap, C.byref(n), C.byref(ms)))
    return out[: min(n.value, cap)].copy(), ms.value


def merge_route_stats(reset: bool = False) -> dict:
    """Which route the contigs of this process took since the last reset (SVCaller::mergeRouteStats): device = the representatives came from
    the device; host_declined / host_overflow = fetched and merged on the host because a bucket was declined / the records overflowed twice;
    buckets_declined = buckets the device declined in all."""
    out = np.zeros(4, np.uint64)
    load().csvhost_merge_route_stats(out.ctypes.data, int(bool(reset)))
    return dict(device=int(out[0]), host_declined=int(out[1]), host_overflow=int(out[2]), buckets_declined=int(out[3]))


class _merge_switch:
    """SVCaller::merge_on_device for the callers behind the process_resident_* functions, for the length of one call"""
    def __init__(self, on, max_partitions):
        self.on, self.mp = bool(on), int(max_partitions)

    def __enter__(self):
        if self.on:
            load().csvhost_set_merge_on_device(1, self.mp)

    def __exit__(self, *a):
        if self.on:
            load().csvhost_set_merge_on_device(0, 0)


def process_resident_chromosome_alts(ctx: Context, shard: Shard, eps: float, min_pts_pct: float, seq_off=None, seq=None, resident_seq: bool = False,
                                     merge_on_device: bool = False, merge_max_partitions: int = 0):
    """processChromosome on a resident shard -> [(start, end, ALT)] of the merged calls. resident_seq: the 50-base ALT strings are cut on the
    device from the sequences the shard itself holds (a shard built with _lib.SB_SEQ) instead of from seq_off / seq."""
    so = np.ascontiguousarray(seq_off, np.uint64) if seq_off is not None else None
    sq = np.ascontiguousarray(seq, np.uint8) if seq is not None else None
    cap = 1 << 22
    buf = C.create_string_buffer(cap)
    ln = C.c_uint64(0)
    if resident_seq and (so is not None or sq is not None):
        raise ValueError("process_resident_chromosome_alts: resident_seq takes the shard's own sequences, not seq_off / seq")
    with _merge_switch(merge_on_device, merge_max_partitions):
        if resident_seq:
            _check(load().csvhost_process_resident_chromosome_alts_resident(ctx.h, shard.h, eps, min_pts_pct, buf, cap, C.byref(ln)))
        else:
            _check(load().csvhost_process_resident_chromosome_alts(ctx.h, shard.h, so.ctypes.data if so is not None else None,
                                                                   sq.ctypes.data if sq is not None else None, eps, min_pts_pct, buf, cap, C.byref(ln)))
    out = []
    for line in buf.raw[: ln.value].decode().split("\n")[:-1]:
        a, b, alt = line.split("\t")
        out.append((int(a), int(b), alt))
    return out


def process_resident_chromosome(ctx: Context, shard: Shard, eps: float, min_pts_pct: float, seq_off_ptr=None, seq_ptr=None, capacity: int = 1 << 20,
                                merge_on_device: bool = False, merge_max_partitions: int = 0):
    """SVCaller::processChromosome mirror on a resident shard -> (merged calls, alt tags, stats)."""
    out = np.zeros(capacity, CALL_DTYPE)
    tag = np.zeros(capacity, np.uint8)
    st = chr_stats()
    with _merge_switch(merge_on_device, merge_max_partitions):
        _check(load().csvhost_process_resident_chromosome(ctx.h, shard.h, seq_off_ptr, seq_ptr, eps, min_pts_pct, out.ctypes.data, tag.ctypes.data,
                                                          capacity, C.byref(st)))
    n = min(st.n_calls, capacity)
    return out[:n].copy(), tag[:n].copy(), st


def process_resident_pipelined(ctx: Context, shard: Shard, n_steps: int, eps: float, min_pts_pct: float, seq_off_ptr=None, seq_ptr=None,
                               capacity: int = 1 << 20, merge_on_device: bool = False, merge_max_partitions: int = 0):
    """n_steps pipelined passes over one resident shard (device chain of step i+1 overlaps the host merge of step i).
    -> (merged calls of the last step, alt tags, stats averaged over steps, wall ms, total merged calls)."""
    out = np.zeros(capacity, CALL_DTYPE)
    tag = np.zeros(capacity, np.uint8)
    st = chr_stats()
    ms, tot = C.c_double(0), C.c_uint64(0)
    with _merge_switch(merge_on_device, merge_max_partitions):
        _check(load().csvhost_process_resident_pipelined(ctx.h, shard.h, n_steps, seq_off_ptr, seq_ptr, eps, min_pts_pct, out.ctypes.data,
                                                         tag.ctypes.data, capacity, C.byref(st), C.byref(ms), C.byref(tot)))
    n = min(st.n_calls, capacity)
    return out[:n].copy(), tag[:n].copy(), st, ms.value, tot.value


def process_resident_lanes(ctxs, shards, steps, eps: float, min_pts_pct: float, capacity: int = 1 << 20, merge_on_device: bool = False,
                           merge_max_partitions: int = 0):
    """Several contexts of one GPU, lane l doing steps[l] pipelined passes over shards[l] at the same time (attach one Gate to all
    contexts first). -> (lane 0's last merged calls, stats averaged over all steps, wall ms, total merged calls)."""
    n = len(ctxs)
    cp = (C.c_void_p * n)(*[c.h for c in ctxs])
    sp = (C.c_void_p * n)(*[s.h for s in shards])
    st_n = np.asarray(steps, np.uint64)
    out = np.zeros(capacity, CALL_DTYPE)
    st = chr_stats()
    ms, tot = C.c_double(0), C.c_uint64(0)
    with _merge_switch(merge_on_device, merge_max_partitions):
        _check(load().csvhost_process_resident_lanes(n, cp, sp, st_n.ctypes.data, eps, min_pts_pct, out.ctypes.data, capacity, C.byref(st), C.byref(ms),
                                                     C.byref(tot)))
    return out[: min(st.n_calls, capacity)].copy(), st, ms.value, tot.value


def _snp_arrays(snps):
    pos = np.ascontiguousarray(snps["pos"], np.uint32)
    baf = np.ascontiguousarray(snps["baf"], np.float64)
    pfb = np.ascontiguousarray(snps["pfb"], np.float64)
    has = np.ascontiguousarray(snps["has_pfb"], np.uint8)
    return pos, baf, pfb, has


def query_snp_region(ctx: Context, shard: Shard, start: int, end: int, mean_cov: float, sample_size: int, snps: dict, cap: int = 1 << 16):
    """CNVCaller::querySNPRegion mirror on the shard's resident depth map -> dict of observation arrays."""
    pos, baf, pfb, has = _snp_arrays(snps)
    o_pos = np.zeros(cap, np.uint32); o_baf = np.zeros(cap); o_pfb = np.zeros(cap); o_l2 = np.zeros(cap); o_is = np.zeros(cap, np.uint8)
    n = C.c_uint64(0)
    _check(load().csvhost_query_snp_region(ctx.h, shard.h, start, end, mean_cov, sample_size, pos.ctypes.data, baf.ctypes.data, pfb.ctypes.data,
                                           has.ctypes.data, len(pos), o_pos.ctypes.data, o_baf.ctypes.data, o_pfb.ctypes.data, o_l2.ctypes.data,
                                           o_is.ctypes.data, cap, C.byref(n)))
    k = n.value
    return {"pos": o_pos[:k], "baf": o_baf[:k], "pfb": o_pfb[:k], "log2_cov": o_l2[:k], "is_snp": o_is[:k].astype(bool)}


def cn_table_capacity_hint(forget: bool = False) -> int:
    """The capacity the mirror's next resident-SNP-table call starts from (the largest bound a table call has asked for; 0: none yet).
    forget=True clears it afterwards: the next call then finds its capacity with one CSV_ECAPACITY round."""
    return int(load().csvhost_cn_table_capacity_hint(int(bool(forget))))


def query_snp_regions(ctx: Context, shard: Shard, starts, ends, mean_cov: float, sample_size: int, snps: dict, on_device: bool = False,
                      cap: int | None = None, snp_table=None) -> dict:
    """CNVCaller::querySNPRegions mirror: many regions of one shard in one batch -> dict(obs_off, pos, baf, pfb, log2_cov, is_snp), region i
    at [obs_off[i], obs_off[i + 1]). on_device: the observation vectors from csvgpu_cn_observations_resident_many instead of the window
    launch and the host's assembly (same arrays; a batch outside that call's domain takes the host route). snp_table: a Context.snp_table of
    the same records — the SNPs are then looked up on the device (csvgpu_cn_observations_tables_many), whatever on_device says."""
    pos, baf, pfb, has = _snp_arrays(snps)
    st, en = np.ascontiguousarray(starts, np.uint32), np.ascontiguousarray(ends, np.uint32)
    if len(st) != len(en):
        raise ValueError("query_snp_regions: starts and ends differ in length")
    if cap is None:
        cap = int(len(st)) * max(int(sample_size), 1) + 4 * int(len(pos)) * max(len(st), 1) + 16
        cap = min(cap, 1 << 26)
    off = np.zeros(len(st) + 1, np.uint64)
    o_pos = np.zeros(cap, np.uint32); o_baf = np.zeros(cap); o_pfb = np.zeros(cap); o_l2 = np.zeros(cap); o_is = np.zeros(cap, np.uint8)
    n = C.c_uint64(0)
    head = (ctx.h, shard.h, len(st), st.ctypes.data, en.ctypes.data, mean_cov, sample_size, pos.ctypes.data, baf.ctypes.data, pfb.ctypes.data, has.ctypes.data,
            len(pos), int(bool(on_device)))
    tail = (off.ctypes.data, o_pos.ctypes.data, o_baf.ctypes.data, o_pfb.ctypes.data, o_l2.ctypes.data, o_is.ctypes.data, cap, C.byref(n))
    if snp_table is not None:
        _check(load().csvhost_query_snp_regions_table(*head, snp_table.h, *tail))
    else:
        _check(load().csvhost_query_snp_regions(*head, *tail))
    k = n.value
    if k > cap:
        return query_snp_regions(ctx, shard, starts, ends, mean_cov, sample_size, snps, on_device, cap=int(k), snp_table=snp_table)
    return {"obs_off": off, "pos": o_pos[:k].copy(), "baf": o_baf[:k].copy(), "pfb": o_pfb[:k].copy(), "log2_cov": o_l2[:k].copy(), "is_snp": o_is[:k].astype(bool)}


def cn_prediction(ctx: Context, shard: Shard, calls: np.ndarray, hmm, mean_cov: float, snps: dict, split: bool, sample_size: int = 20,
                  min_cnv: int = 2000, observations_on_device: bool = False, snp_table=None) -> np.ndarray:
    """runCIGARCopyNumberPrediction (split=False) / runSplitReadCopyNumberPredictions (split=True) mirror. observations_on_device:
    CNVCaller::device_observations (the observation vectors built and decoded on the device; same calls). snp_table: a Context.snp_table
    of the same records — the SNPs are then looked up on the device (csvgpu_cn_decode_tables_many); a batch it declines takes the route the
    other options select."""
    pos, baf, pfb, has = _snp_arrays(snps)
    cap = 2 * len(calls) + 16
    buf = np.zeros(cap, CALL_DTYPE)
    buf[: len(calls)] = np.ascontiguousarray(calls, CALL_DTYPE)
    n = C.c_uint64(0)
    args = (ctx.h, shard.h, int(split), buf.ctypes.data, len(calls), cap, C.byref(n), C.byref(hmm), mean_cov, sample_size, min_cnv, pos.ctypes.data,
            baf.ctypes.data, pfb.ctypes.data, has.ctypes.data, len(pos), int(bool(observations_on_device)))
    if snp_table is not None:
        _check(load().csvhost_cn_prediction_table(*args, snp_table.h))
    else:
        _check(load().csvhost_cn_prediction_device(*args))
    return buf[: n.value].copy()


SPLIT_CALL_DTYPE = np.dtype([("start", "<u4"), ("end", "<u4"), ("sv_type", "<i4"), ("cluster_size", "<i4"), ("aln_offset", "<i4"),
                             ("aln_flags", "<u4"), ("tid", "<i4")])


def split_signatures(ctx: Context, tid, pos, flag, mapq, ref_end, q_start, q_end, qname_id, n_targets: int, min_mapq: int = 20,
                     device_groups: bool = False, device_fits: bool = False) -> np.ndarray:
    """findSplitSVSignatures mirror (qname of record i = "r<qname_id[i]>") -> calls sorted by contig id. device_groups: the overlap groups
    from csvgpu_split_groups on `ctx` instead of the host's interval tree (same calls). device_fits: the groups' point sets, DBSCAN1D fits,
    largest clusters and medians from csvgpu_split_fits (with device_groups: groups and fits from csvgpu_split_groups_fits) instead of the
    host's sets and one csvgpu_dbscan_1d batch (same calls)."""
    a = [np.ascontiguousarray(x, dt) for x, dt in ((tid, np.int32), (pos, np.int32), (flag, np.uint16), (mapq, np.uint8), (ref_end, np.int32),
                                                    (q_start, np.int32), (q_end, np.int32), (qname_id, np.uint32))]
    n = len(a[0])
    cap = 4 * n + 16
    out = np.zeros(cap, SPLIT_CALL_DTYPE)
    k = C.c_uint64(0)
    _check(load().csvhost_split_signatures_dev(ctx.h, n, *[x.ctypes.data for x in a], n_targets, min_mapq, int(bool(device_groups)), int(bool(device_fits)),
                                               out.ctypes.data, cap, C.byref(k)))
    return out[: k.value].copy()


def split_refs(tid, pos, flag, mapq, qname_id, n_targets: int, min_mapq: int = 20):
    """The record references SplitPass::prepare() computes (qname of record i = "r<qname_id[i]>"; records in file order, any mix of tids): which
    primaries have a supplementary record, in the iteration order of their contig's qname map, and those records in file order. Needs no
    alignment intervals and no GPU. -> (SplitRefs, seg_off, supp_tid): segment t = tid t; record indices count within the tid's records (contig t
    uploaded as its own shard); supp_tid[z] is the tid of entry z, whose supp_rec counts within that tid."""
    from .context import SplitRefs
    a = [np.ascontiguousarray(x, dt) for x, dt in ((tid, np.int32), (pos, np.int32), (flag, np.uint16), (mapq, np.uint8), (qname_id, np.uint32))]
    n = len(a[0])
    seg_off, member_rec, supp_off = np.zeros(n_targets + 1, np.uint64), np.zeros(max(n, 1), np.uint32), np.zeros(n + 1, np.uint64)
    cap = max(n, 1)
    for _ in range(2):
        supp_rec, supp_where, supp_tid = np.zeros(cap, np.uint32), np.zeros(cap, np.uint8), np.zeros(cap, np.int32)
        k = np.zeros(2, np.uint64)
        rc = load().csvhost_split_refs(n, *[x.ctypes.data for x in a], n_targets, min_mapq, seg_off.ctypes.data, member_rec.ctypes.data, supp_off.ctypes.data,
                                       supp_rec.ctypes.data, supp_where.ctypes.data, supp_tid.ctypes.data, cap, k.ctypes.data)
        if rc != _lib.CSV_ECAPACITY:
            break
        cap = int(k[1])
    if rc == _lib.CSV_EINVAL:
        raise ValueError((load().csvhost_last_error() or b"").decode())
    _check(rc)
    nm, ns = int(k[0]), int(k[1])
    return SplitRefs(member_rec[:nm].copy(), supp_off[: nm + 1].copy(), supp_rec[:ns].copy(), supp_where[:ns].copy()), seg_off, supp_tid[:ns].copy()


def split_fits_host(ctx: Context, tables, seg_off, groups, eps: float = 100.0, min_pts: int = 5):
    """The records of Context.split_fits(tables, seg_off, groups) by the host route the split-read pass takes without device_fits: point sets,
    largest clusters and medians on this thread, one csvgpu_dbscan_1d batch on `ctx` -> fits[SPLIT_FIT_DTYPE]."""
    seg_off = np.ascontiguousarray(seg_off, np.uint64)
    sgo, go, mem = (np.ascontiguousarray(groups[0], np.uint64), np.ascontiguousarray(groups[1], np.uint64), np.ascontiguousarray(groups[2], np.uint32))
    n_seg = len(seg_off) - 1
    if len(sgo) != n_seg + 1 or len(go) < int(sgo[n_seg]) + 1 or len(mem) < int(go[int(sgo[n_seg])]):
        raise ValueError("split_fits_host: the group tables do not fit the segments")
    out = np.zeros(max(int(sgo[n_seg]), 1), _lib.SPLIT_FIT_DTYPE)
    t = tables.c_struct()
    rc = load().csvhost_split_fits_host(ctx.h, C.byref(t), seg_off.ctypes.data, n_seg, sgo.ctypes.data, go.ctypes.data, mem.ctypes.data, eps, min_pts, out.ctypes.data)
    if rc == _lib.CSV_EINVAL:
        raise ValueError((load().csvhost_last_error() or b"").decode())
    _check(rc)
    return out[: int(sgo[n_seg])]


def split_groups_host(start, end, seg_off):
    """The outputs of Context.split_groups computed by the host mirror's interval tree (sv_caller.cpp:215-238, :948-980 as host/split_caller.cpp
    restates them) -> (seg_group_off, group_off, members). Needs no GPU. ValueError on end < start or descending offsets."""
    start = np.ascontiguousarray(start, np.int32)
    end = np.ascontiguousarray(end, np.int32)
    seg_off = np.ascontiguousarray(seg_off, np.uint64)
    n_seg = len(seg_off) - 1
    if n_seg < 0 or len(start) != len(end) or int(seg_off[-1]) != len(start) or int(seg_off[0]) != 0:
        raise ValueError("split_groups_host: seg_off must run from 0 to the number of members")
    sgo = np.zeros(n_seg + 1, np.uint64)
    go = np.zeros(len(start) + 1, np.uint64)
    cap = max(1024, 2 * len(start))
    for _ in range(2):
        mem = np.zeros(max(cap, 1), np.uint32)
        n = C.c_uint64(cap)
        rc = load().csvhost_split_groups_host(start.ctypes.data, end.ctypes.data, seg_off.ctypes.data, n_seg, sgo.ctypes.data, go.ctypes.data,
                                              mem.ctypes.data, C.byref(n))
        if rc != _lib.CSV_ECAPACITY:
            break
        cap = int(n.value)
    if rc == _lib.CSV_EINVAL:
        raise ValueError((load().csvhost_last_error() or b"").decode())
    _check(rc)
    return sgo, go[: int(sgo[n_seg]) + 1].copy(), mem[: int(n.value)].copy()


def run(ctx: Context, contigs: list, hmm, eps=0.1, min_pts_pct=0.1, sample_size=20, min_cnv=2000, genome=None, vcf_dir=None,
        gap_path=None, file_date=None, want_alts=False, save_cnv=False):
    """SVCaller::run mirror. contigs: list of dicts {reads: Reads, depth_len, qname_id: uint32[n], snps: dict}; contig t is named
    "contig<t>". With genome (ReferenceGenome) and vcf_dir the run ends by writing <vcf_dir>/output.vcf.
    -> (merged calls, contig id per call[, ALT strings])."""
    opt = _run_options(eps=eps, min_pts_pct=min_pts_pct, sample_size=sample_size, min_cnv=min_cnv, save_cnv=save_cnv)
    read_off =np.zeros(len(contigs) + 1, np.uint64)
    read_off[1:] = np.cumsum([c["reads"].n_reads for c in contigs])
    cig_base = np.concatenate([[0], np.cumsum([c["reads"].n_cigar for c in contigs])]).astype(np.uint64)
    pos = np.ascontiguousarray(np.concatenate([c["reads"].pos for c in contigs]), np.int32)
    flag = np.ascontiguousarray(np.concatenate([c["reads"].flag for c in contigs]), np.uint16)
    mapq = np.ascontiguousarray(np.concatenate([c["reads"].mapq for c in contigs]), np.uint8)
    cigar = np.ascontiguousarray(np.concatenate([c["reads"].cigar for c in contigs]), np.uint32)
    coff = np.ascontiguousarray(np.concatenate([c["reads"].cigar_off[:-1] + cig_base[i] for i, c in enumerate(contigs)] + [cig_base[-1:]]), np.uint64)
    qid = np.ascontiguousarray(np.concatenate([c["qname_id"] for c in contigs]), np.uint32)
    dl = np.asarray([c["depth_len"] for c in contigs], np.uint32)
    snp_off = np.zeros(len(contigs) + 1, np.uint64)
    snp_off[1:] = np.cumsum([len(c["snps"]["pos"]) for c in contigs])
    sp = np.ascontiguousarray(np.concatenate([c["snps"]["pos"] for c in contigs]), np.uint32)
    sb = np.ascontiguousarray(np.concatenate([c["snps"]["baf"] for c in contigs]), np.float64)
    sf = np.ascontiguousarray(np.concatenate([c["snps"]["pfb"] for c in contigs]), np.float64)
    sh = np.ascontiguousarray(np.concatenate([c["snps"]["has_pfb"] for c in contigs]), np.uint8)
    cap = len(cigar) + 1024
    out = np.zeros(cap, CALL_DTYPE)
    tid = np.zeros(cap, np.int32)
    n = C.c_uint64(0)
    alt_cap = 64 * cap if want_alts else 0
    alt_buf = np.zeros(max(alt_cap, 1), np.uint8)
    alt_off = np.zeros(cap + 1, np.uint64)
    _check(load().csvhost_run(ctx.h, len(contigs), read_off.ctypes.data, dl.ctypes.data, pos.ctypes.data, flag.ctypes.data, mapq.ctypes.data,
                              coff.ctypes.data, cigar.ctypes.data, qid.ctypes.data, snp_off.ctypes.data, sp.ctypes.data, sb.ctypes.data,
                              sf.ctypes.data, sh.ctypes.data, C.byref(hmm), C.byref(opt), out.ctypes.data, tid.ctypes.data, cap, C.byref(n),
                              genome.h if genome is not None and vcf_dir else None, os.fsencode(vcf_dir) if vcf_dir else None,
                              os.fsencode(gap_path) if gap_path else None, file_date.encode() if file_date else None,
                              alt_buf.ctypes.data if want_alts else None, alt_cap, alt_off.ctypes.data if want_alts else None))
    if want_alts:
        raw = alt_buf.tobytes()
        alts = [raw[int(alt_off[i]):int(alt_off[i + 1])] for i in range(n.value)]
        return out[: n.value].copy(), tid[: n.value].copy(), alts
    return out[: n.value].copy(), tid[: n.value].copy()


def sort_select_check(keys: np.ndarray, nth: int):
    """(id std::sort leaves at slot nth, id std_sort_select returns) for a descending sort by key."""
    keys = np.ascontiguousarray(keys, np.uint32)
    a, b = C.c_int64(-1), C.c_int64(-1)
    _check(load().csvhost_sort_select_check(keys.ctypes.data, len(keys), nth, C.byref(a), C.byref(b)))
    return a.value, b.value


def sort_select_rounds(keys: np.ndarray, nth: int) -> int:
    """How many partitions libstdc++'s std::sort (descending by key) runs on the ranges that hold slot nth, or -1 where its depth limit runs
    out first (it heap-sorts there). Context.sort_slot declines the segments whose count exceeds its bound, and those of -1 always."""
    keys = np.ascontiguousarray(keys, np.uint32)
    r = load().csvhost_sort_select_rounds(keys.ctypes.data, len(keys), nth)
    if r < -1:
        raise RuntimeError("csvhost_sort_select_rounds failed")
    return int(r)


def partition_check(keys: np.ndarray) -> bool:
    """One partition step of sort_select.h: True when the block-wise form leaves the cut and the arrangement of the library's loop."""
    keys = np.ascontiguousarray(keys, np.uint32)
    d = C.c_int(1)
    _check(load().csvhost_partition_check(keys.ctypes.data, len(keys), C.byref(d)))
    return d.value == 0


def read_chmm(path: str):
    h = _lib.csv_hmm()
    n = C.c_int32(0)
    _check(load().csvhost_read_chmm(path.encode(), C.byref(h), C.byref(n)))
    return h, n.value


class ReferenceGenome:
    """ReferenceGenome of the host mirror (src/fasta_query.cpp): whole FASTA in memory, 1-based inclusive queries."""

    def __init__(self, path: str, load_on_device: bool = False, ctx: Context | None = None, window_bytes: int = 0):
        """load_on_device (opt-in): the sequences are built and kept on `ctx`'s device (Context.genome_builder's entry points; the file goes
        up in windows of window_bytes, 0: 256 MiB), no host copy exists, and query / compare / save_vcf fetch what they need. Every result is
        the host backing's. A file the device builder refuses is loaded on the host, whole: device_stats['fallback']."""
        self.path, self.ctx, self.h = path, None, None
        if load_on_device:
            if ctx is None:
                raise ValueError("ReferenceGenome: load_on_device needs a context")
            self.ctx = ctx                               # kept alive as long as the genome may fetch through it
            self.h = load().csvhost_fasta_open_device(os.fsencode(path), ctx.h, int(window_bytes))
        else:
            self.h = load().csvhost_fasta_open(os.fsencode(path))
        if not self.h:
            raise RuntimeError((load().csvhost_last_error() or b"cannot open FASTA").decode())

    @property
    def device_stats(self) -> dict:
        """Whether the sequences live on the device, what the builder took (bytes uploaded, line ends, records, bases), the fetches so far
        (calls, items), and whether the host loader had to read the file instead (fallback)."""
        out = np.zeros(8, np.uint64)
        load().csvhost_fasta_device_stats(self.h, out.ctypes.data)
        return dict(zip(("on_device", "bytes_uploaded", "lines", "records", "bases", "fetch_calls", "items_fetched", "fallback"), (int(x) for x in out)))

    def close(self):
        if self.h:
            load().csvhost_fasta_free(self.h)
        self.h = None

    def __del__(self):
        self.close()

    def _text(self, fn) -> bytes:
        n = fn(self.h, None, 0)
        buf = C.create_string_buffer(max(int(n), 1))
        fn(self.h, buf, n)
        return buf.raw[:n]

    def query(self, chr: str, pos_start: int, pos_end: int) -> bytes:
        """Raises KeyError for an unknown contig (std::out_of_range in the C++ interface)."""
        lib = load()
        n = lib.csvhost_fasta_query(self.h, chr.encode(), pos_start, pos_end, None, 0)
        if n < 0:
            raise KeyError(chr)
        buf = C.create_string_buffer(max(int(n), 1))
        lib.csvhost_fasta_query(self.h, chr.encode(), pos_start, pos_end, buf, n)
        return buf.raw[:n]

    def compare(self, chr: str, pos_start: int, pos_end: int, seq: bytes, threshold: float) -> bool:
        rc = load().csvhost_fasta_compare(self.h, chr.encode(), pos_start, pos_end, seq, threshold)
        if rc < 0:
            raise KeyError(chr)
        return bool(rc)

    def getChromosomeLength(self, chr: str) -> int:
        return int(load().csvhost_fasta_length(self.h, chr.encode()))

    def getContigHeader(self) -> bytes:
        return self._text(load().csvhost_fasta_contig_header)

    def getChromosomes(self):
        t = self._text(load().csvhost_fasta_chromosomes)
        return t.split(b"\n") if t else []


def save_vcf(out_dir: str, genome: ReferenceGenome, contigs, gap_path: str | None = None, file_date: str | None = None,
             ctx: Context | None = None, map_order: bool = False, format_on_device: bool = False):
    """saveToVCF (host mirror) -> <out_dir>/output.vcf. `contigs` = [(name, calls[CALL_DTYPE], alts[list of bytes], depth)] where depth is a
    resident Shard (SUPPORT/DP gathered on the device; needs ctx), a uint32 numpy array, or None. Returns (total, unclassified, gap_filtered).
    format_on_device (opt-in): with a genome opened with load_on_device and depth from shards, the record lines of all contigs come from ONE
    csvgpu_vcf_format call on ctx (Context.vcf_format's entry point); otherwise, and for a batch the device declines, the host loop writes
    them. The file is the same either way; vcf_route_stats() says which route ran."""
    lib = load()
    n = len(contigs)
    names = (C.c_char_p * n)(*[c[0].encode() for c in contigs])
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(c[1]) for c in contigs])
    calls = np.ascontiguousarray(np.concatenate([np.asarray(c[1], CALL_DTYPE) for c in contigs]) if n else np.zeros(0, CALL_DTYPE))
    alt_list = [a for c in contigs for a in c[2]]
    assert len(alt_list) == len(calls)
    alts = (C.c_char_p * max(len(alt_list), 1))(*alt_list)
    use_shards = n > 0 and all(hasattr(c[3], "h") or c[3] is None for c in contigs) and any(c[3] is not None for c in contigs)
    keep = []
    if use_shards:
        shards = (C.c_void_p * n)(*[(c[3].h if c[3] is not None else None) for c in contigs])
        depth_p, len_p, shard_p = None, None, shards
    else:
        arrs = [(np.ascontiguousarray(c[3], np.uint32) if c[3] is not None else None) for c in contigs]
        keep.append(arrs)
        dptr = (C.c_void_p * max(n, 1))(*[(a.ctypes.data if a is not None else None) for a in arrs])
        dlen = np.array([(len(a) if a is not None else 0) for a in arrs] + [0], np.uint64)
        depth_p, len_p, shard_p = dptr, dlen.ctypes.data, None
    counts = np.zeros(3, np.int32)
    args = (ctx.h if ctx is not None else None, os.fsencode(out_dir), genome.h, os.fsencode(gap_path) if gap_path else None,
            file_date.encode() if file_date else None, n, names, off.ctypes.data, calls.ctypes.data, alts, shard_p, depth_p, len_p, int(map_order), counts.ctypes.data)
    _check(lib.csvhost_save_vcf_device(*args, 1) if format_on_device else lib.csvhost_save_vcf(*args))
    return tuple(int(x) for x in counts)


def vcf_route_stats(reset: bool = False) -> dict:
    """Which route the VCF writer's batches took so far in this process with format_on_device / vcf_on_device set: 'device' (formatted by
    csvgpu_vcf_format), 'host' (the host loop), and of the latter 'declined' (the device refused a value of the batch)."""
    out = np.zeros(3, np.uint64)
    load().csvhost_vcf_route_stats(out.ctypes.data, int(bool(reset)))
    return dict(device=int(out[0]), host=int(out[1]), declined=int(out[2]))


def _np_from(ptr_, count, dtype):
    if not ptr_ or count == 0:
        return np.zeros(0, dtype)
    buf = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr_)
    return np.frombuffer(buf, dtype).copy()


class BamFile:
    """BamReader of the host mirror (BGZF/BAM/BAI without htslib). Shards come back as dicts of numpy arrays
    {tid, name, target_len, reads: Reads, seq_off, seq, qnames}."""

    def __init__(self, path: str, load_index: bool = True):
        self._inflate_device = -1
        self._unpack_device = -1
        self._shard_ctx = {}                  # device -> Context the shards of read_contig(shard_on_device=True) are handed out on
        self.h = load().csvhost_bam_open(os.fsencode(path), int(load_index))
        if not self.h:
            raise RuntimeError((load().csvhost_last_error() or b"cannot open BAM").decode())
        lib = load()
        n = lib.csvhost_bam_n_ref(self.h)
        names = lib.csvhost_bam_names(self.h).decode()
        self.names = names.split("\n") if n else []
        self.lens = [int(lib.csvhost_bam_ref_len(self.h, i)) for i in range(n)]
        self.text = lib.csvhost_bam_text(self.h).decode()

    def close(self):
        if self.h:
            load().csvhost_bam_close(self.h)
        self.h = None
        for c in getattr(self, "_shard_ctx", {}).values():      # (shards handed out on them must have been freed by now)
            c.close()
        self._shard_ctx = {}

    def __del__(self):
        self.close()

    def _shard(self, i, want_seq, want_qnames, resident=False):
        lib = load()
        rs, tid, tl, so, sq = _lib.csv_reads(), C.c_int32(0), C.c_uint32(0), C.c_void_p(), C.c_void_p()
        lib.csvhost_bam_shard(self.h, i, C.byref(rs), C.byref(tid), C.byref(tl), C.byref(so), C.byref(sq))
        n, m = rs.n_reads, rs.n_cigar
        addr = lambda p: C.cast(p, C.c_void_p).value
        reads = Reads.__new__(Reads)
        reads.pos, reads.flag, reads.mapq, reads.tid = _np_from(addr(rs.pos), n, np.int32), _np_from(addr(rs.flag), n, np.uint16), _np_from(addr(rs.mapq), n, np.uint8), None
        if resident:                          # (the CIGAR arrays are in the resident shard: the host's are empty)
            reads.cigar_off, reads.cigar = np.zeros(1, np.uint64), np.zeros(0, np.uint32)
        else:
            reads.cigar_off, reads.cigar = _np_from(addr(rs.cigar_off), n + 1, np.uint64), _np_from(addr(rs.cigar), m, np.uint32)
        out = {"tid": tid.value, "name": self.names[tid.value], "target_len": tl.value, "reads": reads}
        if want_seq:
            out["seq_off"] = _np_from(so.value, n + 1, np.uint64)
            out["seq"] = _np_from(sq.value, int(out["seq_off"][-1]), np.uint8)
        if want_qnames:
            ln = lib.csvhost_bam_shard_qnames(self.h, i, None, 0)
            buf = C.create_string_buffer(max(int(ln), 1))
            lib.csvhost_bam_shard_qnames(self.h, i, buf, ln)
            out["qnames"] = buf.raw[:ln].decode(errors="replace").split("\n")[:-1]
        return out

    def _inflate_on(self, on, device):
        """where the next read inflates the BGZF blocks: on `device` (a context of the reader's own; what the device declines is decoded on
        the host, every block CRC-checked either way) or on the host's threads"""
        want = int(device) if on else -1
        if want != self._inflate_device:
            if load().csvhost_bam_set_device_inflate(self.h, want) != 0:
                raise RuntimeError((load().csvhost_last_error() or b"no device context for the BAM reader").decode())
            self._inflate_device = want

    def _unpack_on(self, on, device):
        """where the next read_contig unpacks the records of its batches: on `device` (csvgpu_bam_unpack on the reader's own context, the
        inflate's when both are on; a batch the device declines is parsed on the host) or by the host parser"""
        want = int(device) if on else -1
        if want != self._unpack_device:
            if load().csvhost_bam_set_device_unpack(self.h, want) != 0:
                raise RuntimeError((load().csvhost_last_error() or b"no device context for the BAM reader").decode())
            self._unpack_device = want

    def unpack_stats(self) -> dict:
        """what unpack_on_device did in the last read_contig: batches the device unpacked / the host parser read (declined, or not given),
        anchors handed to the device, records it wrote, batches whose decoded bytes never came to the host, batches brought down after all"""
        v = (C.c_uint64 * 9)()
        load().csvhost_bam_unpack_stats(self.h, C.byref(v))
        return dict(zip(("batches_device", "batches_host", "anchors", "records", "batches_kept_on_device", "batches_downloaded", "shard_resident",
                         "batches_appended_host", "cigar_words_downloaded"), (int(x) for x in v)))

    def read_contig(self, chr: str, want_seq=False, want_qnames=False, threads=8, window_blocks=0, inflate_on_device=False, device=0, unpack_on_device=False,
                    shard_on_device=False, ctx: "Context | None" = None):
        """shard_on_device (implies unpack_on_device): the contig's records are appended on the device into a resident shard, batch by batch
        (csvgpu_shard_builder_*), instead of coming down: the dict then holds that `shard` (a Shard on `ctx`, or on a context this BamFile
        keeps for the purpose; the caller frees it) beside the small arrays — reads.pos / flag / mapq and the query names; reads.cigar_off,
        reads.cigar and seq stay empty, the sequences are inside the shard (Context.alt_bases). `shard` is None for a contig without records."""
        unpack_on_device = unpack_on_device or shard_on_device
        self._inflate_on(inflate_on_device, device)
        self._unpack_on(unpack_on_device, device)
        load().csvhost_bam_set_device_shard(self.h, int(bool(shard_on_device)))
        k = load().csvhost_bam_read(self.h, chr.encode(), int(want_seq), int(want_qnames), threads, window_blocks, None)
        if k < 0:
            raise RuntimeError((load().csvhost_last_error() or b"BAM read failed").decode())
        if not shard_on_device:
            return self._shard(0, want_seq, want_qnames)
        m = C.c_uint64(0)
        handle = load().csvhost_bam_shard_take_resident(self.h, 0, C.byref(m))
        if not handle:
            return dict(self._shard(0, want_seq, want_qnames), shard=None)
        out = self._shard(0, False, want_qnames, resident=True)
        if ctx is None:
            ctx = self._shard_ctx.get(device)
            if ctx is None:
                ctx = self._shard_ctx[device] = Context(device)
        out["shard"] = Shard(ctx, handle, out["reads"].n_reads, out["target_len"] + 1)
        return out

    def read_all(self, want_seq=False, want_qnames=False, threads=8, window_blocks=0, inflate_on_device=False, device=0):
        self._inflate_on(inflate_on_device, device)
        un = C.c_uint64(0)
        k = load().csvhost_bam_read(self.h, None, int(want_seq), int(want_qnames), threads, window_blocks, C.byref(un))
        if k < 0:
            raise RuntimeError((load().csvhost_last_error() or b"BAM read failed").decode())
        return [self._shard(i, want_seq, want_qnames) for i in range(k)], un.value


def bgzf_inflate_file(path: str, threads: int = 16, ctx: "Context | None" = None, window_blocks: int = 2048) -> dict:
    """Every BGZF block of a file inflated in batches, on the host's threads (ctx None) or on ctx's device (what the device declines on the
    host) -> dict(n_blocks, in_bytes, out_bytes, ms): the inflate alone, for tools/bench_inflate.py."""
    nb, ib, ob, ms = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0), C.c_double(0)
    _check(load().csvhost_bgzf_inflate_file(os.fsencode(path), threads, ctx.h if ctx is not None else None, window_blocks, C.byref(nb), C.byref(ib), C.byref(ob), C.byref(ms)))
    return {"n_blocks": nb.value, "in_bytes": ib.value, "out_bytes": ob.value, "ms": ms.value}


def write_bam(path: str, ref_names, ref_lens, tid, reads: Reads, qnames, seq_off=None, seq=None, l_seq=None, text="", level=1, threads=4):
    """BamWriter of the host mirror: coordinate-sorted records -> <path> + <path>.bai."""
    n = reads.n_reads
    tid = np.ascontiguousarray(tid, np.int32)
    lens = np.ascontiguousarray(ref_lens, np.uint32)
    pos, flag, mapq = (np.ascontiguousarray(a, t) for a, t in ((reads.pos, np.int32), (reads.flag, np.uint16), (reads.mapq, np.uint8)))
    coff, cig = np.ascontiguousarray(reads.cigar_off, np.uint64), np.ascontiguousarray(reads.cigar, np.uint32)
    assert len(qnames) == n
    so = np.ascontiguousarray(seq_off, np.uint64) if seq_off is not None else None
    sq = np.ascontiguousarray(seq, np.uint8) if seq is not None else None
    ls = np.ascontiguousarray(l_seq, np.int32) if l_seq is not None else None
    p = lambda a: a.ctypes.data if a is not None else None
    _check(load().csvhost_bam_write(os.fsencode(path), text.encode(), len(ref_names), "\n".join(ref_names).encode(), p(lens), n, p(tid), p(pos), p(flag),
                                    p(mapq), p(coff), p(cig), "\n".join(qnames).encode(), p(so), p(sq), p(ls), level, threads))


def run_bam(ctx: Context, bam_path: str, hmm, chromosomes=None, threads=8, eps=0.1, min_pts_pct=0.1, sample_size=20, min_cnv=2000, split_svs=True, cigar_cn=True, save_cnv=False,
            genome: ReferenceGenome | None = None, vcf_dir=None, gap_path=None, file_date=None, capacity: int = 1 << 20,
            snp_vcf=None, pfb_table=None, ethnicity="", inflate_on_device: bool = False, split_groups_on_device: bool = False, split_fits_on_device: bool = False,
            split_tables_on_device: bool = False, cn_observations_on_device: bool = False, unpack_on_device: bool = False, shard_on_device: bool = False,
            snp_parse_on_device: bool = False, snp_tables_on_device: bool = False, vcf_on_device: bool = False):
    """SVCaller::runBam: the whole run fed from a coordinate-sorted, indexed BAM. -> (calls, contig index per call, stats dict).
    vcf_on_device: SVCaller::vcf_format_on_device — with a genome opened with load_on_device, the record lines of <vcf_dir>/output.vcf come
    from one csvgpu_vcf_format call (vcf_route_stats() counts it); the same file. A process-wide switch like the two below.
    snp_parse_on_device / snp_tables_on_device: SVCaller's fields of those names (the SNP VCF parsed on ctx's device, on a context of the
    run's own; with the second the contigs' SNP tables are built and stay there, and the copy-number pass looks its SNPs up on the device:
    cn_route_stats() counts it). Process-wide switches, set for the length of this call and restored. Neither changes the calls.
    shard_on_device (implies unpack_on_device): every contig's resident shard is built on the device from the unpacked batches and handed to
    the run — no host arrays, no upload; the 50-base ALT strings are cut from the shard's own sequences on the device.
    unpack_on_device: the records of every batch are unpacked on ctx's device (csvgpu_bam_unpack, on the reader's own context) instead of
    by the host parser; a batch the device declines is parsed on the host.
    inflate_on_device: the BAM's BGZF blocks are inflated on ctx's device (csvgpu_bgzf_inflate, on a context of the reader's own) instead of
    on the host's threads; the other switches as in run(). None of them changes the calls."""
    opt = _run_options(eps=eps, min_pts_pct=min_pts_pct, sample_size=sample_size, min_cnv=min_cnv, split_svs=split_svs, cigar_cn=cigar_cn, save_cnv=save_cnv,
                       inflate_on_device=inflate_on_device, inflate_device=getattr(ctx, "device", 0), split_groups_on_device=split_groups_on_device,
                       split_fits_on_device=split_fits_on_device, split_tables_on_device=split_tables_on_device,
                       cn_observations_on_device=cn_observations_on_device, unpack_on_device=unpack_on_device, shard_on_device=shard_on_device)
    out = np.zeros(capacity, CALL_DTYPE)
    tid = np.zeros(capacity, np.int32)
    n = C.c_uint64(0)
    st = bam_stats()
    load().csvhost_set_snp_on_device(int(bool(snp_parse_on_device)), int(bool(snp_tables_on_device)))
    load().csvhost_set_vcf_on_device(int(bool(vcf_on_device)))
    try:
        _check(load().csvhost_run_bam(ctx.h, os.fsencode(bam_path), "\n".join(chromosomes).encode() if chromosomes else None, threads, C.byref(hmm),
                                      C.byref(opt), genome.h if genome is not None and vcf_dir else None,
                                      os.fsencode(vcf_dir) if vcf_dir else None, os.fsencode(gap_path) if gap_path else None,
                                      file_date.encode() if file_date else None, out.ctypes.data, tid.ctypes.data, capacity, C.byref(n), C.byref(st),
                                      os.fsencode(snp_vcf) if snp_vcf else None, os.fsencode(pfb_table) if pfb_table else None, ethnicity.encode()))
    finally:
        load().csvhost_set_snp_on_device(0, 0)
        load().csvhost_set_vcf_on_device(0)
    if n.value > capacity:
        raise RuntimeError("run_bam: capacity too small")
    return out[: n.value].copy(), tid[: n.value].copy(), {f: getattr(st, f) for f, _ in bam_stats._fields_}


def cn_route_stats(reset: bool = False) -> dict:
    """Which route the copy-number pass's decode calls took so far in this process: 'tables' (every contig's SNPs looked up in resident
    tables on the device) or 'queries' (the host's SNP queries)."""
    out = np.zeros(2, np.uint64)
    load().csvhost_cn_route_stats(out.ctypes.data, int(bool(reset)))
    return dict(tables=int(out[0]), queries=int(out[1]))


class SNPFile:
    """The sample's SNP VCF (.vcf or bgzipped + indexed .vcf.gz) parsed once with the reference's filters; query() gives what
    readSNPAlleleFrequencies returns for a region: (positions in file order, BAF at those positions, (pfb_pos, pfb) or None)."""

    def __init__(self, snp_vcf: str, threads: int = 4, parse_on_device: bool = False, ctx: Context | None = None, window_blocks: int = 0,
                 tables_on_device: bool = False):
        """parse_on_device (opt-in): the data lines of the file, and of the population files of later queries, are decided on `ctx`'s device
        (Context.vcf_snp_parse / vcf_af_parse); the tables are the same. window_blocks: BGZF members per batch (0: the default).
        tables_on_device (opt-in, needs ctx): the kept records are cut by contig on the device too (Context.snp_builder) and each contig's
        columns come down once; table() / query() read the population file against the resident positions and leave every ascending
        contig's first-hit table resident on the device. The tables are the same; build_stats says what the device did."""
        self.h, self.ctx = None, None
        if tables_on_device:
            if ctx is None:
                raise ValueError("SNPFile: tables_on_device needs a context")
            self.ctx = ctx
            self.h = load().csvhost_snp_open_device_tables(os.fsencode(snp_vcf), threads, ctx.h, window_blocks)
        elif parse_on_device:
            if ctx is None:
                raise ValueError("SNPFile: parse_on_device needs a context")
            self.ctx = ctx                               # kept alive as long as the file may parse on it
            self.h = load().csvhost_snp_open_device(os.fsencode(snp_vcf), threads, ctx.h, window_blocks)
        else:
            self.h = load().csvhost_snp_open(os.fsencode(snp_vcf), threads)
        if not self.h:
            raise RuntimeError((load().csvhost_last_error() or b"cannot load SNP VCF").decode())

    def close(self):
        if self.h:
            load().csvhost_snp_free(self.h)
        self.h = None

    def __del__(self):
        self.close()

    @property
    def records_kept(self) -> int:
        return int(load().csvhost_snp_kept(self.h))

    @property
    def device_stats(self) -> dict:
        """What the device parser did so far: lines it examined, records it kept, lines it deferred to the host parser, batches it declined."""
        out = np.zeros(4, np.uint64)
        load().csvhost_snp_device_stats(self.h, out.ctypes.data)
        return dict(zip(("lines", "kept", "deferred", "declined_batches"), (int(x) for x in out)))

    @property
    def build_stats(self) -> dict:
        """tables_on_device: CHROM runs the builder reported, records appended through the host (deferred lines, declined batches), contigs
        whose resident table was made from the device columns so far."""
        out = np.zeros(3, np.uint64)
        load().csvhost_snp_build_stats(self.h, out.ctypes.data)
        return dict(zip(("runs", "appended_host", "tables_resident"), (int(x) for x in out)))

    def table(self, chr: str, pfb_vcf: str | None = None, ethnicity: str = "", threads: int = 4):
        """The contig's whole tables, file order: (pos, baf, af_pos, af) — the kept SNP records and the population records that can become
        a region's hit (built from pfb_vcf on the contig's first use, as in query())."""
        n = np.zeros(2, np.uint64)
        args = (self.h, chr.encode(), os.fsencode(pfb_vcf) if pfb_vcf else None, ethnicity.encode(), threads)
        load().csvhost_snp_table(*args, None, None, 0, None, None, 0, n.ctypes.data)
        pos, baf = np.zeros(int(n[0]), np.uint32), np.zeros(int(n[0]), np.float64)
        af_pos, af = np.zeros(int(n[1]), np.uint32), np.zeros(int(n[1]), np.float64)
        if load().csvhost_snp_table(*args, pos.ctypes.data, baf.ctypes.data, len(pos), af_pos.ctypes.data, af.ctypes.data, len(af), n.ctypes.data) != 0:
            raise RuntimeError("SNP table: the counts changed between two calls")
        return pos, baf, af_pos, af

    def query(self, chr: str, start: int, end: int, pfb_vcf: str | None = None, ethnicity: str = "", threads: int = 4, cap: int = 1 << 20):
        pos, baf = np.zeros(cap, np.uint32), np.zeros(cap, np.float64)
        has, pp, pv = C.c_int(0), C.c_uint32(0), C.c_double(0)
        n = load().csvhost_snp_query(self.h, chr.encode(), os.fsencode(pfb_vcf) if pfb_vcf else None, ethnicity.encode(), start, end,
                                     pos.ctypes.data, baf.ctypes.data, cap, C.byref(has), C.byref(pp), C.byref(pv), threads)
        if n < 0:
            raise RuntimeError("SNP query: capacity too small")
        return pos[:n].copy(), baf[:n].copy(), ((pp.value, pv.value) if has.value else None)


def pfb_path(table_path: str, chr: str) -> str:
    """InputData::getAlleleFreqFilepath over a --pfb table file."""
    buf = C.create_string_buffer(4096)
    n = load().csvhost_pfb_path(os.fsencode(table_path), chr.encode(), buf, 4096)
    if n < 0:
        raise RuntimeError((load().csvhost_last_error() or b"").decode())
    return buf.raw[:n].decode()


def gnomad_contig(chr: str, pfb_path_: str) -> str:
    buf = C.create_string_buffer(4096)
    n = load().csvhost_gnomad_contig(chr.encode(), pfb_path_.encode(), buf, 4096)
    return buf.raw[:n].decode()


class SynthBamWriter:
    """Several SynthShards into one coordinate-sorted BAM + BAI, one contig each (append in contig order)."""

    def __init__(self, path: str, ref_names, ref_lens, level: int = 1, threads: int = 8):
        lens = np.ascontiguousarray(ref_lens, np.uint32)
        self.h = load().csvhost_bam_writer_open(os.fsencode(path), len(ref_names), "\n".join(ref_names).encode(), lens.ctypes.data, level, threads)
        if not self.h:
            raise RuntimeError((load().csvhost_last_error() or b"cannot create BAM").decode())

    def append(self, syn: SynthShard, tid: int):
        _check(load().csvhost_bam_writer_append_synth(self.h, syn.h, tid))

    def close(self):
        if self.h:
            h, self.h = self.h, None
            _check(load().csvhost_bam_writer_close(h))
