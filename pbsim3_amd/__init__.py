"""pbsim3_amd -- Python (ctypes) binding of the C ABI in include/pbsim3_amd.h.

The product is the HIP library pbsim3_amd/lib/libpbsim3_amd.so; this module
only loads it and mirrors its entry points (same names, same SUCCEEDED(1) /
FAILED(0) convention as the reference, pbsim.cpp:16-17).  There is no Python
or CPU implementation of the path behind it: if the library is missing, or no
gfx950 device is usable, the calls raise.
"""
import ctypes as C
import os
from typing import NamedTuple

from . import build as _build

STRATEGY_WGS, STRATEGY_TRANS, STRATEGY_TEMPL = 1, 2, 3
METHOD_QS, METHOD_ERR, METHOD_SAMPLE = 1, 2, 3


class Params(C.Structure):
    _fields_ = [
        ("strategy", C.c_int32), ("method", C.c_int32), ("seed", C.c_uint32), ("pass_num", C.c_int32),
        ("depth", C.c_double), ("accuracy_mean", C.c_double), ("len_mean", C.c_double), ("len_sd", C.c_double),
        ("hp_del_bias", C.c_double), ("len_min", C.c_int64), ("len_max", C.c_int64),
        ("sub_ratio", C.c_int64), ("ins_ratio", C.c_int64), ("del_ratio", C.c_int64),
        ("id_prefix", C.c_char * 64),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("res_num", C.c_int64), ("res_pass_num", C.c_int64), ("res_len_total", C.c_int64),
        ("res_len_min", C.c_int64), ("res_len_max", C.c_int64),
        ("res_sub_num", C.c_int64), ("res_ins_num", C.c_int64), ("res_del_num", C.c_int64),
        ("res_depth", C.c_double), ("res_len_mean", C.c_double), ("res_len_sd", C.c_double),
        ("res_accuracy_mean", C.c_double), ("res_accuracy_sd", C.c_double),
        ("res_sub_rate", C.c_double), ("res_ins_rate", C.c_double), ("res_del_rate", C.c_double),
    ]


class BatchInfo(C.Structure):
    _fields_ = [
        ("first_read", C.c_int64), ("n_reads", C.c_int64), ("n_final", C.c_int64),
        ("quota_reached", C.c_int32), ("need_truncated_read", C.c_int32),
        ("len_total_after", C.c_int64), ("bases", C.c_int64),
        ("read_text_bytes", C.c_int64), ("maf_text_bytes", C.c_int64),
        ("ref_bases", C.c_int64), ("maf_columns", C.c_int64),
    ]


class SampleStats(C.Structure):
    """pbsim_sample_stats: what print_sample_stats prints about a --sample FASTQ and its filtered profile"""
    _fields_ = [("num", C.c_int64), ("len_min", C.c_int64), ("len_max", C.c_int64), ("len_total", C.c_int64),
                ("num_filtered", C.c_int64), ("len_min_filtered", C.c_int64), ("len_max_filtered", C.c_int64),
                ("len_total_filtered", C.c_int64), ("len_mean_filtered", C.c_double), ("len_sd_filtered", C.c_double),
                ("accuracy_mean_filtered", C.c_double), ("accuracy_sd_filtered", C.c_double)]


SINK_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_char), C.c_int64)


class Sink(C.Structure):
    _fields_ = [("user", C.c_void_p), ("on_read_text", SINK_CB), ("on_maf_text", SINK_CB)]


class ReadArrays(C.Structure):
    """pbsim_read_arrays: device pointers, one per array (ref_pos may be NULL)"""
    _fields_ = [("seq", C.c_void_p), ("qual", C.c_void_p), ("ref_pos", C.c_void_p), ("offsets", C.c_void_p),
                ("read_number", C.c_void_p), ("pass_index", C.c_void_p), ("unit", C.c_void_p), ("strand", C.c_void_p),
                ("ref_start", C.c_void_p), ("ref_span", C.c_void_p), ("n_sub", C.c_void_p), ("n_ins", C.c_void_p),
                ("n_del", C.c_void_p)]


ARRAY_ALLOC_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.POINTER(ReadArrays))
ARRAY_BATCH_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(BatchInfo))


class ArraySink(C.Structure):
    _fields_ = [("user", C.c_void_p), ("alloc", ARRAY_ALLOC_CB), ("on_batch", ARRAY_BATCH_CB)]


# (name, dtype, per task / per base) of the arrays of a ReadBatch, in pbsim_read_arrays order
ARRAY_FIELDS = [("seq", "uint8", "base"), ("qual", "uint8", "base"), ("ref_pos", "int32", "base"),
                ("offsets", "int64", "offset"), ("read_number", "int64", "task"), ("pass_index", "int32", "task"),
                ("unit", "int32", "task"), ("strand", "uint8", "task"), ("ref_start", "int64", "task"),
                ("ref_span", "int32", "task"), ("n_sub", "int32", "task"), ("n_ins", "int32", "task"),
                ("n_del", "int32", "task")]


class ReadBatch(NamedTuple):
    """Reads of one batch (or of a whole run) as torch tensors on the context's device; include/pbsim3_amd.h
    pbsim_read_arrays has the contract.  Task t = read r, pass h at t = r * pass_num + h; its bases are
    seq[offsets[t]:offsets[t + 1]].  ref_pos is None when simulated with labels=False.  first_read: the number of the
    batch's first read."""
    seq: object
    qual: object
    ref_pos: object
    offsets: object
    read_number: object
    pass_index: object
    unit: object
    strand: object
    ref_start: object
    ref_span: object
    n_sub: object
    n_ins: object
    n_del: object
    first_read: int


OP_SUM, OP_MIN, OP_MAX = 0, 1, 2
GATHER_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64))
REDUCE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_int64), C.c_int64, C.c_int32)
BCAST_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32)
ABORT_CB = C.CFUNCTYPE(C.c_int, C.c_void_p)


class Comm(C.Structure):
    """pbsim_comm: blocking collectives over the ranks of a job (one context per GPU)."""
    _fields_ = [("user", C.c_void_p), ("rank", C.c_int32), ("world", C.c_int32),
                ("all_gather_i64", GATHER_CB), ("all_reduce_i64", REDUCE_CB), ("broadcast", BCAST_CB),
                ("abort", ABORT_CB)]


REC_TEXT_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.POINTER(C.c_char), C.c_int64, C.c_int64)
REC_DONE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.POINTER(Stats), C.c_int64, C.c_int64)


class RecordSink(C.Structure):
    _fields_ = [("user", C.c_void_p), ("on_read_text", REC_TEXT_CB), ("on_maf_text", REC_TEXT_CB),
                ("on_record_done", REC_DONE_CB)]


SORTED_BAM_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64)
SORTED_INDEX_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)


class SortedBamSink(C.Structure):
    _fields_ = [("user", C.c_void_p), ("on_bam", SORTED_BAM_CB), ("on_index", SORTED_INDEX_CB)]


class EvalTruth(C.Structure):
    _fields_ = [("bytes", C.c_char_p), ("n", C.c_int64), ("ref_name", C.c_char_p)]


class EvalOpts(C.Structure):
    _fields_ = [("overlap_permille", C.c_int32), ("hash_bits", C.c_int32)]


EVAL_VERDICTS_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)


class EvalSink(C.Structure):
    _fields_ = [("user", C.c_void_p), ("on_verdicts", EVAL_VERDICTS_CB)]


EVAL_COUNTS = ["truth_records", "query_records", "primary", "secondary", "supplementary", "unknown", "duplicate", "unmapped",
               "scored", "correct", "wrong", "missing"]


class DepthOpts(C.Structure):
    _fields_ = [("exclude_flags", C.c_int32), ("min_mapq", C.c_int32), ("count_deletions", C.c_int32), ("format", C.c_int32),
                ("window", C.c_int64), ("piece_bytes", C.c_int64)]


DEPTH_TEXT_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64)
DEPTH_REFS_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64))
DEPTH_ARRAY_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64)


class DepthSink(C.Structure):
    _fields_ = [("user", C.c_void_p), ("on_text", DEPTH_TEXT_CB), ("on_refs", DEPTH_REFS_CB), ("on_depth", DEPTH_ARRAY_CB)]


DEPTH_COUNTS = ["records", "counted", "skipped_flag", "skipped_unplaced", "skipped_mapq", "clipped"]
DEPTH_FORMATS = {"bedgraph": 0, "window": 1}


class StatsFile(C.Structure):
    _fields_ = [("bam", C.c_void_p), ("n", C.c_int64)]


class StatsOpts(C.Structure):
    _fields_ = [("exclude_flags", C.c_int32), ("min_mapq", C.c_int32), ("piece_bytes", C.c_int64)]


STATS_TEXT_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64)


class StatsSink(C.Structure):
    _fields_ = [("user", C.c_void_p), ("on_text", STATS_TEXT_CB)]


STATS_COUNTS = ["records", "skipped_flag", "unaligned", "skipped_mapq", "aligned", "no_seq", "no_qual", "no_nm", "nm_bad", "scored"]
STATS_LEN_ROW = ["n", "bases", "min", "max", "mean_milli", "sd", "median"] + ["N%d" % x for x in range(10, 100, 10)]
STATS_TOTALS = ["cols", "sub", "ins", "del", "ins_events", "del_events", "soft", "hard", "identity_sum", "acc_sum", "acc_reads", "q_sum"]


class ErrorsRef(C.Structure):
    _fields_ = [("name", C.c_char_p), ("lines", C.c_void_p), ("bytes", C.c_int64)]


class ErrorsFile(C.Structure):
    _fields_ = [("bam", C.c_void_p), ("n", C.c_int64), ("ref_name", C.c_char_p)]


class ErrorsOpts(C.Structure):
    _fields_ = [("exclude_flags", C.c_int32), ("min_mapq", C.c_int32), ("piece_bytes", C.c_int64)]


ERRORS_TEXT_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64)


class ErrorsSink(C.Structure):
    _fields_ = [("user", C.c_void_p), ("on_text", ERRORS_TEXT_CB)]


ERRORS_COUNTS = ["records", "skipped_flag", "unaligned", "skipped_mapq", "skipped_ref", "aligned", "no_seq", "misfit", "scored", "no_nm",
                 "nm_unchecked", "nm_agree", "nm_differ", "with_qual"]
ERRORS_TOTALS = ["cols", "match", "sub", "ambiguous", "ins", "del", "ins_events", "del_events", "soft", "hard", "identity_sum"]
# the arrays of pbsim_errors_result behind counts and totals, in the struct's order (qcal: [128][3] laid flat)
ERRORS_ARRAYS = [("pair", 25), ("hp_cols", 12), ("hp_sub", 12), ("hp_del", 12), ("ins_len", 64), ("del_len", 64), ("ins_base", 5),
                 ("del_base", 5), ("qcal", 384), ("hist_identity", 1001)]
ERRORS_FIT = ["fit_ok", "fit_bias_milli", "fit_suggest_milli"]


class ErrorsResult(C.Structure):
    _fields_ = [("counts", C.c_int64 * 14), ("totals", C.c_int64 * 11)] + [(name, C.c_int64 * n) for name, n in ERRORS_ARRAYS] + \
               [(name, C.c_int64) for name in ERRORS_FIT]


class PileupOpts(C.Structure):
    _fields_ = [("exclude_flags", C.c_int32), ("min_mapq", C.c_int32), ("min_baseq", C.c_int32), ("format", C.c_int32),
                ("min_depth", C.c_int64), ("piece_bytes", C.c_int64)]


PILEUP_TEXT_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64)
PILEUP_CELLS_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64)


class PileupSink(C.Structure):
    _fields_ = [("user", C.c_void_p), ("on_text", PILEUP_TEXT_CB), ("on_cells", PILEUP_CELLS_CB)]


PILEUP_COUNTS = ["records", "skipped_flag", "unaligned", "skipped_mapq", "skipped_ref", "aligned", "no_seq", "misfit", "scored"]
PILEUP_SITES = ["sites", "ref_n", "low", "called", "concordant", "sub_site", "del_site", "ins_site", "discordant"]
PILEUP_CELLS = ["A", "C", "G", "T", "other", "del", "ins", "masked"]
PILEUP_HP = ["hp_called", "hp_sub", "hp_del", "hp_ins"]
PILEUP_FORMATS = {"sites": 0, "all": 1}


class PileupResult(C.Structure):
    _fields_ = [("counts", C.c_int64 * 9), ("sites", C.c_int64 * 9), ("cell_sums", C.c_int64 * 8), ("ins_unanchored", C.c_int64),
                ("max_depth", C.c_int64)] + [(name, C.c_int64 * 12) for name in PILEUP_HP]


class ConsensusOpts(C.Structure):
    _fields_ = [("exclude_flags", C.c_int32), ("min_mapq", C.c_int32), ("min_baseq", C.c_int32), ("fill", C.c_int32), ("min_depth", C.c_int64),
                ("max_ins", C.c_int32), ("line_width", C.c_int32), ("piece_bytes", C.c_int64)]


CONSENSUS_TEXT_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64)
CONSENSUS_RECORD_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_int64, C.c_int64)


class ConsensusSink(C.Structure):
    _fields_ = [("user", C.c_void_p), ("on_text", CONSENSUS_TEXT_CB), ("on_record", CONSENSUS_RECORD_CB)]


CONSENSUS_BASES = ["out", "kept", "sub", "ins", "fill", "del"]
CONSENSUS_FILL = {"n": 0, "ref": 1}


class ConsensusResult(C.Structure):
    _fields_ = [("counts", C.c_int64 * 9), ("sites", C.c_int64 * 9), ("ins_unanchored", C.c_int64), ("max_depth", C.c_int64),
                ("bases", C.c_int64 * 6), ("ins_sites", C.c_int64), ("ins_longest", C.c_int64), ("ins_capped", C.c_int64),
                ("ins_len", C.c_int64 * 64), ("text_bytes", C.c_int64)]


class CallOpts(C.Structure):
    _fields_ = [("exclude_flags", C.c_int32), ("min_mapq", C.c_int32), ("min_baseq", C.c_int32), ("max_ins", C.c_int32), ("min_depth", C.c_int64),
                ("piece_bytes", C.c_int64)]


CALL_TEXT_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64)
CALL_RECORD_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_int64, C.c_int64)


class CallSink(C.Structure):
    _fields_ = [("user", C.c_void_p), ("on_text", CALL_TEXT_CB), ("on_record", CALL_RECORD_CB)]


CALL_TYPES = ["snv", "ins", "del", "complex"]


class CallResult(C.Structure):
    _fields_ = [("counts", C.c_int64 * 9), ("sites", C.c_int64 * 9), ("ins_unanchored", C.c_int64), ("max_depth", C.c_int64),
                ("variants", C.c_int64), ("types", C.c_int64 * 4), ("ref_bases", C.c_int64), ("alt_bases", C.c_int64), ("longest_ref", C.c_int64),
                ("longest_alt", C.c_int64), ("unplaced_records", C.c_int64), ("unplaced_sites", C.c_int64), ("header_bytes", C.c_int64),
                ("text_bytes", C.c_int64)]



class MutateOpts(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("snv_ppm", C.c_int32), ("ins_ppm", C.c_int32), ("del_ppm", C.c_int32), ("ext_ppm", C.c_int32),
                ("max_indel", C.c_int32), ("line_width", C.c_int32), ("piece_bytes", C.c_int64)]


MUTATE_TEXT_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64)
MUTATE_RECORD_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64)
MUTATE_ORIGIN_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64)


class MutateSink(C.Structure):
    _fields_ = [("user", C.c_void_p), ("on_fasta", MUTATE_TEXT_CB), ("on_vcf", MUTATE_TEXT_CB), ("on_record", MUTATE_RECORD_CB),
                ("on_origin", MUTATE_ORIGIN_CB)]


MUTATE_TYPES = ["snv", "ins", "del"]


class MutateResult(C.Structure):
    _fields_ = [("records", C.c_int64), ("bases_in", C.c_int64), ("eligible", C.c_int64), ("bases_out", C.c_int64), ("drawn", C.c_int64 * 3),
                ("void_del", C.c_int64), ("dropped", C.c_int64), ("merged", C.c_int64), ("substituted", C.c_int64), ("inserted", C.c_int64),
                ("deleted", C.c_int64), ("variants", C.c_int64), ("types", C.c_int64 * 3), ("ref_bases", C.c_int64), ("alt_bases", C.c_int64),
                ("longest_ref", C.c_int64), ("longest_alt", C.c_int64), ("header_bytes", C.c_int64), ("vcf_bytes", C.c_int64),
                ("fasta_bytes", C.c_int64)]


class CompareOpts(C.Structure):
    _fields_ = [("lines", C.c_int32), ("min_ms", C.c_int32), ("piece_bytes", C.c_int64)]


COMPARE_TEXT_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64)


class CompareSink(C.Structure):
    _fields_ = [("user", C.c_void_p), ("on_text", COMPARE_TEXT_CB)]


COMPARE_LINES = {"discordant": 0, "all": 1}


class CompareResult(C.Structure):
    _fields_ = [("files", C.c_int64 * 11 * 2), ("types", C.c_int64 * 6 * 4), ("lengths", C.c_int64 * 4 * 5 * 2), ("ms", C.c_int64 * 2 * 64),
                ("text_bytes", C.c_int64)]

class ApplyOpts(C.Structure):
    _fields_ = [("haplotype", C.c_int32), ("sample", C.c_int32), ("lines", C.c_int32), ("line_width", C.c_int32), ("piece_bytes", C.c_int64)]


APPLY_TEXT_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64)
APPLY_RECORD_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64)
APPLY_ORIGIN_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_void_p, C.c_int64)


class ApplySink(C.Structure):
    _fields_ = [("user", C.c_void_p), ("on_fasta", APPLY_TEXT_CB), ("on_text", APPLY_TEXT_CB), ("on_record", APPLY_RECORD_CB),
                ("on_origin", APPLY_ORIGIN_CB)]


APPLY_LINES = {"discordant": 0, "all": 1}
APPLY_TYPES = ["snv", "ins", "del", "complex"]
APPLY_SCALARS = ["lines", "malformed", "unknown_contig", "no_call", "ref_allele", "unsupported", "ref_mismatch", "filtered", "no_change", "overlap",
                 "applied", "bases_in", "bases_out", "inserted", "deleted", "substituted", "longest_cluster", "fasta_bytes", "text_bytes"]


class ApplyResult(C.Structure):
    _fields_ = [("lines", C.c_int64), ("malformed", C.c_int64), ("unknown_contig", C.c_int64), ("no_call", C.c_int64), ("ref_allele", C.c_int64),
                ("unsupported", C.c_int64), ("ref_mismatch", C.c_int64), ("filtered", C.c_int64), ("no_change", C.c_int64), ("overlap", C.c_int64),
                ("applied", C.c_int64), ("types", C.c_int64 * 4), ("bases_in", C.c_int64), ("bases_out", C.c_int64), ("inserted", C.c_int64),
                ("deleted", C.c_int64), ("substituted", C.c_int64), ("longest_cluster", C.c_int64), ("fasta_bytes", C.c_int64),
                ("text_bytes", C.c_int64)]

class LiftOrigin(C.Structure):
    _fields_ = [("origin", C.c_void_p), ("n", C.c_int64)]


LIFT_BAM_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64)


class LiftSink(C.Structure):
    _fields_ = [("user", C.c_void_p), ("on_bam", LIFT_BAM_CB)]


LIFT_COUNTS = ["records", "unaligned", "unsupported", "unplaced", "lifted", "moved", "no_seq", "long_cigar_in", "long_cigar_out"]
LIFT_TOTALS = ["cols_in", "cols_out", "m", "ins", "del", "soft", "sub", "gap_del", "bases_to_ins", "dels_vanished", "bytes_in", "bytes_out"]


class LiftResult(C.Structure):
    _fields_ = [("counts", C.c_int64 * 9), ("totals", C.c_int64 * 12)]


# every symbol include/pbsim3_amd.h declares: (name, restype, argtypes)
API = [
    ("pbsim_job_add_record", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("pbsim_job_add_record_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("pbsim_job_add_record_lines", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    ("pbsim_job_add_record_comm", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(Comm), C.c_int32]),
    ("pbsim_job_records", C.c_int64, [C.c_void_p]),
    ("pbsim_job_begin", C.c_int, [C.c_void_p, C.c_int64]),
    ("pbsim_job_clear", C.c_int, [C.c_void_p]),
    ("pbsim_job_run", C.c_int, [C.c_void_p, C.POINTER(Comm), C.POINTER(RecordSink)]),
    ("pbsim_job_sam_header", C.c_int64, [C.c_void_p, C.c_int64, C.c_char_p, C.c_int64]),
    ("pbsim_job_bam_header", C.c_int64, [C.c_void_p, C.c_int64, C.c_char_p, C.c_int64]),
    ("pbsim_job_counters", C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    ("pbsim_job_progress", C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    ("pbsim_job_set_interleave", C.c_int, [C.c_void_p, C.c_int]),
    ("pbsim_job_expect", C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    ("pbsim_job_feed_abort", C.c_int, [C.c_void_p, C.c_char_p]),
    ("pbsim_scratch_state", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("pbsim_batch_fetch_lengths", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pbsim_job_breakdown", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("pbsim_bind_host_to_device", C.c_int, [C.c_int, C.c_char_p, C.c_int64]),
    ("pbsim_rccl_unique_id", C.c_int64, [C.c_void_p, C.c_int64]),
    ("pbsim_rccl_comm_create", C.POINTER(Comm), [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32]),
    ("pbsim_rccl_comm_create_file", C.POINTER(Comm), [C.c_char_p, C.c_int32, C.c_int32, C.c_int32]),
    ("pbsim_rccl_comm_info", C.c_int, [C.POINTER(Comm), C.POINTER(C.c_int64)]),
    ("pbsim_rccl_comm_destroy", None, [C.POINTER(Comm)]),
    ("pbsim_stats_keep_values", C.c_int, [C.c_void_p, C.c_int]),
    ("pbsim_stats_merge", C.c_int, [C.c_void_p, C.POINTER(Comm)]),
    ("pbsim_stats_add_tasks", C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    ("pbsim_format_stats", C.c_int64, [C.POINTER(Params), C.POINTER(Stats), C.c_int64, C.c_char_p, C.c_int64]),
    ("pbsim_cli_main", C.c_int, [C.c_int, C.POINTER(C.c_char_p), C.POINTER(Comm), C.c_int]),
    ("pbsim_params_default", None, [C.POINTER(Params)]),
    ("pbsim_create", C.c_void_p, [C.POINTER(Params), C.c_int]),
    ("pbsim_destroy", None, [C.c_void_p]),
    ("pbsim_last_error", C.c_char_p, []),
    ("pbsim_version", C.c_char_p, []),
    ("pbsim_load_errhmm", C.c_int, [C.c_void_p, C.c_char_p]),
    ("pbsim_load_qshmm", C.c_int, [C.c_void_p, C.c_char_p]),
    ("pbsim_set_reference", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    ("pbsim_set_reference_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int64]),
    ("pbsim_add_hp_census", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("pbsim_finish_hp_census", C.c_int, [C.c_void_p]),
    ("pbsim_set_transcripts", C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_char_p), C.POINTER(C.c_int64),
                                        C.POINTER(C.c_int64), C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    ("pbsim_set_templates", C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_char_p), C.POINTER(C.c_void_p),
                                      C.POINTER(C.c_int64)]),
    ("pbsim_simulate_templ", C.c_int, [C.c_void_p, C.POINTER(Sink)]),
    ("pbsim_prefetch_reference", C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    ("pbsim_prefetch_reference_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    ("pbsim_simulate_units_range", C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.POINTER(Sink)]),
    ("pbsim_unit_reads", C.c_int64, [C.c_void_p]),
    ("pbsim_load_transcript_file", C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]),
    ("pbsim_load_template_file", C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]),
    ("pbsim_simulate_wgs", C.c_int, [C.c_void_p, C.POINTER(Sink)]),
    ("pbsim_simulate_trans", C.c_int, [C.c_void_p, C.POINTER(Sink)]),
    ("pbsim_simulate_arrays", C.c_int, [C.c_void_p, C.POINTER(ArraySink)]),
    ("pbsim_get_stats", C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    ("pbsim_sam_header", C.c_int64, [C.c_void_p, C.c_char_p, C.c_int64]),
    ("pbsim_set_bam_output", C.c_int, [C.c_void_p, C.c_int]),
    ("pbsim_bam_header", C.c_int64, [C.c_void_p, C.c_char_p, C.c_int64]),
    ("pbsim_set_truth_bam", C.c_int, [C.c_void_p, C.c_int]),
    ("pbsim_truth_bam_header", C.c_int64, [C.c_void_p, C.c_char_p, C.c_int64]),
    ("pbsim_job_truth_bam_header", C.c_int64, [C.c_void_p, C.c_int64, C.c_char_p, C.c_int64]),
    ("pbsim_set_sample_profile", C.c_int, [C.c_void_p, C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    ("pbsim_simulate_sample", C.c_int, [C.c_void_p, C.POINTER(Sink)]),
    ("pbsim_sample_profile_from_bytes", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.POINTER(SampleStats)]),
    ("pbsim_sample_profile_from_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.POINTER(SampleStats)]),
    ("pbsim_load_sample_fastq", C.c_int, [C.c_void_p, C.c_char_p, C.c_double, C.c_double, C.POINTER(SampleStats)]),
    ("pbsim_load_sample", C.c_int, [C.c_void_p, C.c_char_p, C.c_double, C.c_double, C.POINTER(SampleStats)]),
    ("pbsim_sample_profile_from_bam_bytes", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.POINTER(SampleStats)]),
    ("pbsim_sample_profile_from_bam_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_double, C.c_double, C.POINTER(SampleStats)]),
    ("pbsim_sample_profile_text", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    ("pbsim_set_sample_chunk_bytes", C.c_int, [C.c_void_p, C.c_int64]),
    ("pbsim_simulate_sample_comm", C.c_int, [C.c_void_p, C.POINTER(Comm), C.POINTER(RecordSink)]),
    ("pbsim_set_deflate", C.c_int, [C.c_void_p, C.c_int]),
    ("pbsim_deflate_bound", C.c_int64, [C.c_int64]),
    ("pbsim_batch_fetch_deflated", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                             C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("pbsim_deflate_buffer", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    ("pbsim_inflate_bound", C.c_int64, [C.c_void_p, C.c_int64]),
    ("pbsim_inflate_buffer", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]),
    ("pbsim_truth_bam_sort", C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(SortedBamSink), C.POINTER(C.c_int64)]),
    ("pbsim_truth_bam_eval", C.c_int, [C.c_void_p, C.POINTER(EvalTruth), C.c_int, C.c_char_p, C.c_int64, C.POINTER(EvalOpts),
                                       C.POINTER(EvalSink), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("pbsim_eval_report", C.c_int64, [C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_char_p, C.c_int64]),
    ("pbsim_bam_depth", C.c_int, [C.c_void_p, C.c_char_p, C.c_int64, C.POINTER(DepthOpts), C.POINTER(DepthSink), C.POINTER(C.c_int64),
                                  C.POINTER(C.c_int64)]),
    ("pbsim_depth_report", C.c_int64, [C.POINTER(C.c_int64), C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                       C.c_char_p, C.c_int64]),
    ("pbsim_bam_stats", C.c_int, [C.c_void_p, C.POINTER(StatsFile), C.c_int, C.POINTER(StatsOpts), C.POINTER(StatsSink)] + [C.POINTER(C.c_int64)] * 6),
    ("pbsim_stats_report", C.c_int64, [C.POINTER(C.c_int64)] * 6 + [C.c_char_p, C.c_int64]),
    ("pbsim_bam_errors", C.c_int, [C.c_void_p, C.POINTER(ErrorsRef), C.c_int, C.POINTER(ErrorsFile), C.c_int, C.POINTER(ErrorsOpts),
                                   C.POINTER(ErrorsSink), C.POINTER(ErrorsResult)]),
    ("pbsim_errors_report", C.c_int64, [C.POINTER(ErrorsResult), C.c_char_p, C.c_int64]),
    ("pbsim_bam_pileup", C.c_int, [C.c_void_p, C.POINTER(ErrorsRef), C.c_int, C.POINTER(ErrorsFile), C.c_int, C.POINTER(PileupOpts),
                                   C.POINTER(PileupSink), C.POINTER(PileupResult)]),
    ("pbsim_pileup_report", C.c_int64, [C.POINTER(PileupResult), C.c_char_p, C.c_int64]),
    ("pbsim_bam_consensus", C.c_int, [C.c_void_p, C.POINTER(ErrorsRef), C.c_int, C.POINTER(ErrorsFile), C.c_int, C.POINTER(ConsensusOpts),
                                      C.POINTER(ConsensusSink), C.POINTER(ConsensusResult)]),
    ("pbsim_consensus_report", C.c_int64, [C.POINTER(ConsensusResult), C.c_char_p, C.c_int64]),
    ("pbsim_bam_call", C.c_int, [C.c_void_p, C.POINTER(ErrorsRef), C.c_int, C.POINTER(ErrorsFile), C.c_int, C.POINTER(CallOpts), C.POINTER(CallSink),
                                 C.POINTER(CallResult)]),
    ("pbsim_call_report", C.c_int64, [C.POINTER(CallResult), C.c_char_p, C.c_int64]),
    ("pbsim_genome_mutate", C.c_int, [C.c_void_p, C.POINTER(ErrorsRef), C.c_int, C.POINTER(MutateOpts), C.POINTER(MutateSink),
                                      C.POINTER(MutateResult)]),
    ("pbsim_mutate_report", C.c_int64, [C.POINTER(MutateResult), C.c_char_p, C.c_int64]),
    ("pbsim_vcf_compare", C.c_int, [C.c_void_p, C.POINTER(ErrorsRef), C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_int64, C.c_char_p, C.c_int64,
                                    C.POINTER(CompareOpts), C.POINTER(CompareSink), C.POINTER(CompareResult)]),
    ("pbsim_compare_report", C.c_int64, [C.POINTER(CompareResult), C.c_char_p, C.c_int64]),
    ("pbsim_vcf_apply", C.c_int, [C.c_void_p, C.POINTER(ErrorsRef), C.c_int, C.POINTER(C.c_char_p), C.c_char_p, C.c_int64, C.POINTER(ApplyOpts),
                                  C.POINTER(ApplySink), C.POINTER(ApplyResult)]),
    ("pbsim_apply_report", C.c_int64, [C.POINTER(ApplyResult), C.c_char_p, C.c_int64]),
    ("pbsim_apply_sample", C.c_int32, [C.c_char_p, C.c_int64, C.c_char_p]),
    ("pbsim_bam_lift", C.c_int, [C.c_void_p, C.POINTER(ErrorsRef), C.c_int, C.POINTER(LiftOrigin), C.POINTER(ErrorsFile), C.POINTER(LiftSink),
                                 C.POINTER(LiftResult)]),
    ("pbsim_lift_report", C.c_int64, [C.POINTER(LiftResult), C.c_char_p, C.c_int64]),
    ("pbsim_batch_walk", C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.POINTER(C.c_int64)]),
    ("pbsim_slot_count", C.c_int, []),
    ("pbsim_select_slot", C.c_int, [C.c_void_p, C.c_int]),
    ("pbsim_batch_walk_begin", C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int64]),
    ("pbsim_batch_walk_end", C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    ("pbsim_batch_finalize", C.c_int, [C.c_void_p, C.c_int64, C.POINTER(BatchInfo)]),
    ("pbsim_batch_fetch", C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    ("pbsim_batch_account", C.c_int, [C.c_void_p]),
    ("pbsim_reset_stats", C.c_int, [C.c_void_p]),
    ("pbsim_unit_quota", C.c_int64, [C.c_void_p]),
    ("pbsim_batch_capacity", C.c_int64, [C.c_void_p]),
    ("pbsim_set_scratch_bytes", C.c_int, [C.c_void_p, C.c_int64]),
    ("pbsim_release_pools", C.c_int, [C.c_void_p]),
    ("pbsim_prof_reset", C.c_int, [C.c_void_p]),
    ("pbsim_prof_get", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    ("pbsim_prof_walk_busy", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("pbsim_prof_tail", C.c_int, [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    ("pbsim_prof_secondary", C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    ("pbsim_prof_wave_launches", C.c_int64, [C.c_void_p]),
    ("pbsim_stream", C.c_void_p, [C.c_void_p]),
    ("pbsim_device_synchronize", C.c_int, [C.c_void_p]),
    ("pbsim_philox4x32_10", None, [C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    ("pbsim_dump_table", C.c_int64, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64]),
]

_lib = None


def lib_path():
    return _build.LIB


def _torch_runtime_first():
    """PyTorch-ROCm wheels bundle their own libhsa-runtime64 / libamdhip64; this library links the system copies.  The two
    coexist in one process only when torch's are mapped first, so if torch is installed but not imported yet, map its two
    runtime libraries now (no `import torch`): a later `import torch` in the same process then still finds its device.
    PBSIM_TORCH_COMPAT=0 skips this."""
    import sys
    if "torch" in sys.modules or os.environ.get("PBSIM_TORCH_COMPAT", "1") == "0":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if not spec or not spec.origin:
            return
        libdir = os.path.join(os.path.dirname(spec.origin), "lib")
        for name in ("libhsa-runtime64.so", "libamdhip64.so"):
            path = os.path.join(libdir, name)
            if os.path.exists(path):
                C.CDLL(path, mode=C.RTLD_GLOBAL)
    except Exception:       # best effort: the product itself does not depend on it
        pass


def load(build_if_missing=True):
    """Loads libpbsim3_amd.so (building it in-tree with hipcc when absent)."""
    global _lib
    if _lib is not None:
        return _lib
    _torch_runtime_first()
    if not os.path.exists(_build.LIB):
        if not build_if_missing:
            raise RuntimeError("libpbsim3_amd.so is not built (python -m pbsim3_amd.build)")
        _build.build()
    lib = C.CDLL(_build.LIB)
    for name, res, args in API:
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def eval_report(counts, hist) -> bytes:
    """The report text of Context.eval_bam's counts (the dict, or the twelve values in order) and hist ([256][2]):
    pbsim_eval_report, no device needed."""
    vals = [counts[k] for k in EVAL_COUNTS] if isinstance(counts, dict) else list(counts)
    c = (C.c_int64 * 12)(*[int(v) for v in vals])
    h = (C.c_int64 * 512)(*[int(v) for row in hist for v in row])
    n = load().pbsim_eval_report(c, h, None, 0)
    if n < 0:
        raise PbsimError("pbsim_eval_report: bad argument")
    buf = C.create_string_buffer(max(n, 1))
    load().pbsim_eval_report(c, h, buf, n)
    return buf.raw[:n]


def depth_report(counts, refs, hist) -> bytes:
    """The report text of Context.bam_depth's counts (the dict, or the six values in order), refs (a list of (name, l_ref,
    covered, sum, max)) and hist (256 values): pbsim_depth_report, no device needed."""
    vals = [counts[k] for k in DEPTH_COUNTS] if isinstance(counts, dict) else list(counts)
    refs = list(refs)
    c = (C.c_int64 * 6)(*[int(v) for v in vals])
    h = (C.c_int64 * 256)(*[int(v) for v in hist])
    names = (C.c_char_p * max(len(refs), 1))(*[r[0].encode() if isinstance(r[0], str) else bytes(r[0]) for r in refs])
    rows = (C.c_int64 * max(4 * len(refs), 1))(*[int(v) for r in refs for v in r[1:5]])
    n = load().pbsim_depth_report(c, len(refs), names, rows, h, None, 0)
    if n < 0:
        raise PbsimError("pbsim_depth_report: bad argument")
    buf = C.create_string_buffer(max(n, 1))
    load().pbsim_depth_report(c, len(refs), names, rows, h, buf, n)
    return buf.raw[:n]


def stats_report(counts, len_row, totals, hist_q, hist_identity, hist_qacc) -> bytes:
    """The report text of Context.bam_stats's counts, len_row and totals (the dicts, or the values in order) and its three
    histograms (128, 1001 and 1001 values): pbsim_stats_report, no device needed."""
    def vals(x, names):
        return [int(x[k]) for k in names] if isinstance(x, dict) else [int(v) for v in x]
    parts = [vals(counts, STATS_COUNTS), vals(len_row, STATS_LEN_ROW), vals(totals, STATS_TOTALS), [int(v) for v in hist_q],
             [int(v) for v in hist_identity], [int(v) for v in hist_qacc]]
    if [len(p) for p in parts] != [10, 16, 12, 128, 1001, 1001]:
        raise ValueError("stats_report: 10 counts, 16 length values, 12 totals and histograms of 128, 1001 and 1001 bins")
    arrs = [(C.c_int64 * len(p))(*p) for p in parts]
    n = load().pbsim_stats_report(*arrs, None, 0)
    if n < 0:
        raise PbsimError("pbsim_stats_report: bad argument")
    buf = C.create_string_buffer(max(n, 1))
    load().pbsim_stats_report(*arrs, buf, n)
    return buf.raw[:n]


def _errors_dict(res) -> dict:
    """an ErrorsResult as a dict: counts and totals as dicts by name, the arrays as lists, the fit's three values"""
    out = dict(counts=dict(zip(ERRORS_COUNTS, (int(v) for v in res.counts))), totals=dict(zip(ERRORS_TOTALS, (int(v) for v in res.totals))))
    for name, _ in ERRORS_ARRAYS:
        out[name] = [int(v) for v in getattr(res, name)]
    for name in ERRORS_FIT:
        out[name] = int(getattr(res, name))
    return out


def errors_report(result) -> bytes:
    """The report text of Context.bam_errors's result (the dict; counts and totals as dicts by name or as the values in order; the
    fit's values are not read): pbsim_errors_report, no device needed."""
    def vals(x, names):
        return [int(x[k]) for k in names] if isinstance(x, dict) else [int(v) for v in x]
    parts = [("counts", vals(result["counts"], ERRORS_COUNTS)), ("totals", vals(result["totals"], ERRORS_TOTALS))] + \
            [(name, [int(v) for v in result[name]]) for name, _ in ERRORS_ARRAYS]
    res = ErrorsResult()
    for name, v in parts:
        if len(v) != len(getattr(res, name)):
            raise ValueError("errors_report: %s has %d values, not %d" % (name, len(v), len(getattr(res, name))))
        setattr(res, name, type(getattr(res, name))(*v))
    n = load().pbsim_errors_report(C.byref(res), None, 0)
    if n < 0:
        raise PbsimError("pbsim_errors_report: bad argument")
    buf = C.create_string_buffer(max(n, 1))
    load().pbsim_errors_report(C.byref(res), buf, n)
    return buf.raw[:n]


def _pileup_dict(res) -> dict:
    """a PileupResult as a dict: counts and sites as dicts by name, cell_sums as a dict by cell, the four arrays as lists"""
    out = dict(counts=dict(zip(PILEUP_COUNTS, (int(v) for v in res.counts))), sites=dict(zip(PILEUP_SITES, (int(v) for v in res.sites))),
               cell_sums=dict(zip(PILEUP_CELLS, (int(v) for v in res.cell_sums))), ins_unanchored=int(res.ins_unanchored),
               max_depth=int(res.max_depth))
    for name in PILEUP_HP:
        out[name] = [int(v) for v in getattr(res, name)]
    return out


def pileup_report(result) -> bytes:
    """The report text of Context.bam_pileup's result (the dict; counts, sites and cell_sums as dicts by name or as the values in
    order): pbsim_pileup_report, no device needed."""
    def vals(x, names):
        return [int(x[k]) for k in names] if isinstance(x, dict) else [int(v) for v in x]
    parts = [("counts", vals(result["counts"], PILEUP_COUNTS)), ("sites", vals(result["sites"], PILEUP_SITES)),
             ("cell_sums", vals(result["cell_sums"], PILEUP_CELLS))] + [(name, [int(v) for v in result[name]]) for name in PILEUP_HP]
    res = PileupResult()
    for name, v in parts:
        if len(v) != len(getattr(res, name)):
            raise ValueError("pileup_report: %s has %d values, not %d" % (name, len(v), len(getattr(res, name))))
        setattr(res, name, type(getattr(res, name))(*v))
    res.ins_unanchored, res.max_depth = int(result["ins_unanchored"]), int(result["max_depth"])
    n = load().pbsim_pileup_report(C.byref(res), None, 0)
    if n < 0:
        raise PbsimError("pbsim_pileup_report: bad argument")
    buf = C.create_string_buffer(max(n, 1))
    load().pbsim_pileup_report(C.byref(res), buf, n)
    return buf.raw[:n]


CONSENSUS_SCALARS = ["ins_unanchored", "max_depth", "ins_sites", "ins_longest", "ins_capped", "text_bytes"]


def _consensus_dict(res) -> dict:
    """a ConsensusResult as a dict: counts, sites and bases as dicts by name, ins_len as a list, the rest as numbers"""
    out = dict(counts=dict(zip(PILEUP_COUNTS, (int(v) for v in res.counts))), sites=dict(zip(PILEUP_SITES, (int(v) for v in res.sites))),
               bases=dict(zip(CONSENSUS_BASES, (int(v) for v in res.bases))), ins_len=[int(v) for v in res.ins_len])
    for name in CONSENSUS_SCALARS:
        out[name] = int(getattr(res, name))
    return out


def consensus_report(result) -> bytes:
    """The report text of Context.bam_consensus's result (the dict; counts, sites and bases as dicts by name or as the values in
    order): pbsim_consensus_report, no device needed."""
    def vals(x, names):
        return [int(x[k]) for k in names] if isinstance(x, dict) else [int(v) for v in x]
    parts = [("counts", vals(result["counts"], PILEUP_COUNTS)), ("sites", vals(result["sites"], PILEUP_SITES)),
             ("bases", vals(result["bases"], CONSENSUS_BASES)), ("ins_len", [int(v) for v in result["ins_len"]])]
    res = ConsensusResult()
    for name, v in parts:
        if len(v) != len(getattr(res, name)):
            raise ValueError("consensus_report: %s has %d values, not %d" % (name, len(v), len(getattr(res, name))))
        setattr(res, name, type(getattr(res, name))(*v))
    for name in CONSENSUS_SCALARS:
        setattr(res, name, int(result.get(name, 0)))
    n = load().pbsim_consensus_report(C.byref(res), None, 0)
    if n < 0:
        raise PbsimError("pbsim_consensus_report: bad argument")
    buf = C.create_string_buffer(max(n, 1))
    load().pbsim_consensus_report(C.byref(res), buf, n)
    return buf.raw[:n]


CALL_SCALARS = ["ins_unanchored", "max_depth", "variants", "ref_bases", "alt_bases", "longest_ref", "longest_alt", "unplaced_records", "unplaced_sites",
                "header_bytes", "text_bytes"]


def _call_dict(res) -> dict:
    """a CallResult as a dict: counts, sites and types as dicts by name, the rest as numbers"""
    out = dict(counts=dict(zip(PILEUP_COUNTS, (int(v) for v in res.counts))), sites=dict(zip(PILEUP_SITES, (int(v) for v in res.sites))),
               types=dict(zip(CALL_TYPES, (int(v) for v in res.types))))
    for name in CALL_SCALARS:
        out[name] = int(getattr(res, name))
    return out


def call_report(result) -> bytes:
    """The report text of Context.bam_call's result (the dict; counts, sites and types as dicts by name or as the values in order):
    pbsim_call_report, no device needed."""
    def vals(x, names):
        return [int(x[k]) for k in names] if isinstance(x, dict) else [int(v) for v in x]
    parts = [("counts", vals(result["counts"], PILEUP_COUNTS)), ("sites", vals(result["sites"], PILEUP_SITES)), ("types", vals(result["types"], CALL_TYPES))]
    res = CallResult()
    for name, v in parts:
        if len(v) != len(getattr(res, name)):
            raise ValueError("call_report: %s has %d values, not %d" % (name, len(v), len(getattr(res, name))))
        setattr(res, name, type(getattr(res, name))(*v))
    for name in CALL_SCALARS:
        setattr(res, name, int(result.get(name, 0)))
    n = load().pbsim_call_report(C.byref(res), None, 0)
    if n < 0:
        raise PbsimError("pbsim_call_report: bad argument")
    buf = C.create_string_buffer(max(n, 1))
    load().pbsim_call_report(C.byref(res), buf, n)
    return buf.raw[:n]


MUTATE_SCALARS = ["records", "bases_in", "eligible", "bases_out", "void_del", "dropped", "merged", "substituted", "inserted", "deleted", "variants",
                  "ref_bases", "alt_bases", "longest_ref", "longest_alt", "header_bytes", "vcf_bytes", "fasta_bytes"]


def _mutate_dict(res) -> dict:
    """a MutateResult as a dict: drawn and types as dicts by name, the rest as numbers"""
    out = dict(drawn=dict(zip(MUTATE_TYPES, (int(v) for v in res.drawn))), types=dict(zip(MUTATE_TYPES, (int(v) for v in res.types))))
    for name in MUTATE_SCALARS:
        out[name] = int(getattr(res, name))
    return out


def mutate_report(result) -> bytes:
    """The report text of Context.mutate_genome's result (the dict; drawn and types as dicts by name or as the values in order):
    pbsim_mutate_report, no device needed."""
    def vals(x, names):
        return [int(x[k]) for k in names] if isinstance(x, dict) else [int(v) for v in x]
    res = MutateResult()
    for name in ("drawn", "types"):
        v = vals(result[name], MUTATE_TYPES)
        if len(v) != len(getattr(res, name)):
            raise ValueError("mutate_report: %s has %d values, not %d" % (name, len(v), len(getattr(res, name))))
        setattr(res, name, type(getattr(res, name))(*v))
    for name in MUTATE_SCALARS:
        setattr(res, name, int(result.get(name, 0)))
    n = load().pbsim_mutate_report(C.byref(res), None, 0)
    if n < 0:
        raise PbsimError("pbsim_mutate_report: bad argument")
    buf = C.create_string_buffer(max(n, 1))
    load().pbsim_mutate_report(C.byref(res), buf, n)
    return buf.raw[:n]


COMPARE_SHAPES = dict(files=(2, 11), types=(4, 6), lengths=(2, 5, 4), ms=(64, 2))


def _nested(x):
    """a ctypes array of arrays as lists of ints"""
    return [_nested(v) for v in x] if hasattr(x, "__len__") else int(x)


def _compare_dict(res) -> dict:
    """a CompareResult as a dict: files [truth, calls][11], types [snv, ins, del, complex][6], lengths [ins, del][bin][4], ms [64][2] as
    nested lists in the header's order, text_bytes as a number"""
    out = {name: _nested(getattr(res, name)) for name in COMPARE_SHAPES}
    out["text_bytes"] = int(res.text_bytes)
    return out


def compare_report(result) -> bytes:
    """The report text of Context.compare_vcf's result (the dict of nested lists): pbsim_compare_report, no device needed."""
    import numpy as np
    res = CompareResult()
    for name, shape in COMPARE_SHAPES.items():
        v = np.asarray(result.get(name, np.zeros(shape, np.int64)), dtype=np.int64)
        if v.shape != shape:
            raise ValueError("compare_report: %s has the shape %s, not %s" % (name, v.shape, shape))
        C.memmove(C.addressof(getattr(res, name)), np.ascontiguousarray(v).ctypes.data, v.nbytes)
    res.text_bytes = int(result.get("text_bytes", 0))
    n = load().pbsim_compare_report(C.byref(res), None, 0)
    if n < 0:
        raise PbsimError("pbsim_compare_report: bad argument")
    buf = C.create_string_buffer(max(n, 1))
    load().pbsim_compare_report(C.byref(res), buf, n)
    return buf.raw[:n]


def _apply_dict(res) -> dict:
    """an ApplyResult as a dict: types as a dict by name, the rest as numbers"""
    out = dict(types=dict(zip(APPLY_TYPES, (int(v) for v in res.types))))
    for name in APPLY_SCALARS:
        out[name] = int(getattr(res, name))
    return out


def apply_report(result) -> bytes:
    """The report text of Context.apply_vcf's result (the dict; types as a dict by name or as the values in order):
    pbsim_apply_report, no device needed."""
    res = ApplyResult()
    v = result.get("types", [0] * 4)
    v = [int(v[k]) for k in APPLY_TYPES] if isinstance(v, dict) else [int(x) for x in v]
    if len(v) != len(res.types):
        raise ValueError("apply_report: types has %d values, not %d" % (len(v), len(res.types)))
    res.types = type(res.types)(*v)
    for name in APPLY_SCALARS:
        setattr(res, name, int(result.get(name, 0)))
    n = load().pbsim_apply_report(C.byref(res), None, 0)
    if n < 0:
        raise PbsimError("pbsim_apply_report: bad argument")
    buf = C.create_string_buffer(max(n, 1))
    load().pbsim_apply_report(C.byref(res), buf, n)
    return buf.raw[:n]


def apply_sample(vcf, name) -> int:
    """The 0-based sample column `name` has in the #CHROM line of the VCF text (pbsim_apply_sample, no device needed); -1: none."""
    vcf = bytes(vcf)
    return int(load().pbsim_apply_sample(vcf, len(vcf), name.encode() if isinstance(name, str) else bytes(name)))


def _lift_dict(res) -> dict:
    """a LiftResult as a dict by name: the counts, then the totals"""
    out = dict(zip(LIFT_COUNTS, (int(v) for v in res.counts)))
    out.update(zip(LIFT_TOTALS, (int(v) for v in res.totals)))
    return out


def lift_report(result) -> bytes:
    """The report text of Context.lift_bam's result (the dict): pbsim_lift_report, no device needed."""
    res = LiftResult()
    res.counts = type(res.counts)(*[int(result.get(k, 0)) for k in LIFT_COUNTS])
    res.totals = type(res.totals)(*[int(result.get(k, 0)) for k in LIFT_TOTALS])
    n = load().pbsim_lift_report(C.byref(res), None, 0)
    if n < 0:
        raise PbsimError("pbsim_lift_report: bad argument")
    buf = C.create_string_buffer(max(n, 1))
    load().pbsim_lift_report(C.byref(res), buf, n)
    return buf.raw[:n]


def inflate_bound(data: bytes) -> int:
    """Inflated size of BGZF `data` from its member headers (no device needed), or -1 when it is not BGZF."""
    return load().pbsim_inflate_bound(data, len(data))


class PbsimError(RuntimeError):
    pass


def _check(ok):
    if not ok:
        raise PbsimError(load().pbsim_last_error().decode(errors="replace"))


def default_params(**kw):
    p = Params()
    load().pbsim_params_default(C.byref(p))
    for k, v in kw.items():
        if k == "id_prefix":
            v = v.encode() if isinstance(v, str) else v
        setattr(p, k, v)
    return p


# empty BGZF block: the end-of-file marker of a BAM file (SAMv1 4.1.2), also a valid empty gzip member
BGZF_EOF = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])


def make_comm(rank, world, all_gather, all_reduce, broadcast=None, abort=None):
    """pbsim_comm from Python callables (numpy int64 arrays in and out; the statistics merge moves millions of values):
         all_gather(array[n]) -> array[world, n] (rank-major), all_reduce(array[n], op) -> array[n],
         broadcast(ptr:int, nbytes:int, root:int, on_device:bool) -> None (optional, C1).
    The returned Comm keeps the ctypes trampolines alive (comm._keep)."""
    def _g(user, send, n, recv):
        try:
            import numpy as np
            if n == 0:
                return 1
            a = np.ctypeslib.as_array(send, shape=(n,))
            out = np.ctypeslib.as_array(recv, shape=(world * n,))
            out[:] = np.asarray(all_gather(a), dtype=np.int64).reshape(-1)   # rank-major
            return 1
        except Exception:
            import traceback
            traceback.print_exc()
            return 0

    def _r(user, buf, n, op):
        try:
            import numpy as np
            a = np.ctypeslib.as_array(buf, shape=(n,)) if n else None
            if n:
                a[:] = all_reduce(a, op)
            return 1
        except Exception:
            import traceback
            traceback.print_exc()
            return 0

    def _b(user, ptr, nbytes, root, on_device):
        try:
            broadcast(ptr, nbytes, root, bool(on_device))
            return 1
        except Exception:
            import traceback
            traceback.print_exc()
            return 0

    def _a(user):
        try:
            abort()
            return 1
        except Exception:
            import traceback
            traceback.print_exc()
            return 0

    cbs = (GATHER_CB(_g), REDUCE_CB(_r), BCAST_CB(_b) if broadcast else BCAST_CB(), ABORT_CB(_a) if abort else ABORT_CB())
    comm = Comm(None, rank, world, *cbs)
    comm._keep = cbs
    return comm


def torch_comm(dist, device):
    """pbsim_comm over torch.distributed (backend nccl = RCCL on the GPUs, gloo on the CPU): the job's integer collectives
    (C3 all_gather, C2 all_reduce).  `device`: the torch device the collectives run on (this rank's GPU for nccl, cpu for
    gloo).  No broadcast callback: a caller that holds the records as torch tensors broadcasts them itself (C1,
    dist.broadcast) and hands every rank its copy (pbsim_job_add_record_device); pbsim_cli_main has every rank read the
    <prefix>_NNNN.ref files instead."""
    import numpy as np
    import torch
    rank, world = dist.get_rank(), dist.get_world_size()

    def all_gather(arr):
        t = torch.from_numpy(np.ascontiguousarray(arr)).to(device)
        out = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(out, t)
        return torch.stack(out).cpu().numpy()

    def all_reduce(arr, op):
        t = torch.from_numpy(np.ascontiguousarray(arr)).to(device)
        dist.all_reduce(t, op={OP_SUM: dist.ReduceOp.SUM, OP_MIN: dist.ReduceOp.MIN, OP_MAX: dist.ReduceOp.MAX}[op])
        return t.cpu().numpy()

    def abort():
        # one process per rank (torchrun): the other ranks wait in a collective this rank will never enter.  Ending this
        # process is what tears the group down -- the launcher then ends the others (include/pbsim3_amd.h, pbsim_comm.abort).
        import sys
        sys.stderr.write("pbsim3_amd: rank %d failed inside the job (%s): leaving the process group\n"
                         % (rank, load().pbsim_last_error().decode(errors="replace")))
        sys.stderr.flush()
        os._exit(1)

    return make_comm(rank, world, all_gather, all_reduce, None, abort)


RCCL_ID_BYTES = 128


class RcclComm:
    """pbsim_comm over RCCL for ONE PROCESS PER GPU (pbsim_rccl_comm_create = ncclCommInitRank): the communicator bench.py
    --gpus N and run_multi use by default.  `exchange(id_or_None) -> id`: the launcher's side channel -- rank 0 passes the id it
    made and every rank gets it back (torch's store: RcclComm.from_torch; a rendezvous file: RcclComm.from_file).
    .ref is what pbsim_job_run / pbsim_cli_main take (C.byref of the library's own struct); .comm the struct itself."""

    def __init__(self, ptr):
        if not ptr:
            raise PbsimError(load().pbsim_last_error().decode(errors="replace"))
        self.ptr = ptr
        self.comm = ptr.contents
        self.ref = ptr

    @classmethod
    def create(cls, rank, world, device, exchange):
        lib = load()
        ident = None
        if rank == 0:
            buf = C.create_string_buffer(RCCL_ID_BYTES)
            if lib.pbsim_rccl_unique_id(buf, RCCL_ID_BYTES) != RCCL_ID_BYTES:
                # the others wait in `exchange`: tell them (an empty id) before raising
                exchange(b"")
                raise PbsimError(lib.pbsim_last_error().decode(errors="replace"))
            ident = buf.raw
        ident = exchange(ident)
        if len(ident) != RCCL_ID_BYTES:
            raise PbsimError("rank 0 could not make an RCCL id")
        return cls(lib.pbsim_rccl_comm_create(ident, len(ident), rank, world, device))

    @classmethod
    def from_torch(cls, dist, device, key="pbsim_rccl_id"):
        """the id through torch.distributed's key-value store (TCP, the rendezvous torchrun already made)"""
        return cls.create(dist.get_rank(), dist.get_world_size(), device, store_exchange(dist, key))

    @classmethod
    def from_file(cls, path, rank, world, device):
        return cls(load().pbsim_rccl_comm_create_file(os.fsencode(path), rank, world, device))

    def info(self):
        out = (C.c_int64 * 4)()
        _check(load().pbsim_rccl_comm_info(self.ptr, out))
        return {"ranks_seen": out[0], "rank": out[1], "device": out[2], "collectives": out[3]}

    def close(self):
        if self.ptr:
            load().pbsim_rccl_comm_destroy(self.ptr)
            self.ptr = self.ref = None


_store_round = [0]


def store_exchange(dist, key="pbsim_rccl_id"):
    """exchange(id_or_None) -> id over torch.distributed's key-value store: rank 0 sets the bytes under a key of this call's
    own (a process that makes several communicators gets several keys -- every rank counts the calls alike), the others block
    in get() until it is there.  Device-free: works under any backend (tests/test_multi_gloo.py)."""
    rank = dist.get_rank()
    store = dist.distributed_c10d._get_default_store()
    _store_round[0] += 1
    k = "%s/%d" % (key, _store_round[0])

    def exchange(ident):
        if rank == 0:
            store.set(k, ident)
            return ident
        return bytes(store.get(k))
    return exchange


def comm_latency(comm_ref, n_words=8, iters=1000, warm=50):
    """microseconds per all_gather_i64 / all_reduce_i64 of `n_words` through the function pointers of a pbsim_comm exactly as
    job.cpp calls them (blocking, one after the other); comm_ref: C.byref(Comm) or a POINTER(Comm).  Collective: every rank
    of the communicator calls it with the same arguments."""
    import time
    cm = comm_ref.contents if hasattr(comm_ref, "contents") else comm_ref._obj
    send = (C.c_int64 * n_words)(*range(n_words))
    recv = (C.c_int64 * (n_words * cm.world))()
    res = {"world": cm.world, "words": n_words, "iters": iters}
    for name, call in (("all_gather_us", lambda: cm.all_gather_i64(cm.user, send, n_words, recv)),
                       ("all_reduce_us", lambda: cm.all_reduce_i64(cm.user, send, n_words, OP_MAX))):
        for _ in range(warm):
            if not call():
                raise PbsimError("comm_latency: the collective failed")
        t0 = time.perf_counter()
        for _ in range(iters):
            call()
        res[name] = (time.perf_counter() - t0) / iters * 1e6
    return res


def bind_host_to_device(device):
    """Binds the calling thread (and the threads and pinned allocations it creates from now on) to the CPUs and the memory of
    the NUMA node `device`'s PCIe slot hangs off; call before the first HIP call of the process.  Returns a description of what
    was done ("" when there is nothing to bind to).  PBSIM_NUMA_BIND=0 turns it off."""
    buf = C.create_string_buffer(512)
    load().pbsim_bind_host_to_device(device, buf, 512)
    return buf.value.decode(errors="replace")


def cli_main(argv, comm=None, device=-1):
    """pbsim_cli_main: the whole command line for this rank (argv without the program name)."""
    args = [b"pbsim"] + [os.fsencode(a) for a in argv]
    arr = (C.c_char_p * (len(args) + 1))(*args, None)
    ref = None if comm is None else (C.byref(comm) if isinstance(comm, Comm) else comm)   # a Comm, or a POINTER(Comm) (RcclComm.ref)
    return load().pbsim_cli_main(len(args), arr, ref, device)


class Context:
    """One GPU context (pbsim_ctx).  device=-1 gives a tables-only context that
    can build and dump host tables but refuses every compute call."""

    def __init__(self, params, device=0):
        self.lib = load()
        self.params = params
        self.device = device
        self.h = self.lib.pbsim_create(C.byref(params), device)
        if not self.h:
            raise PbsimError(self.lib.pbsim_last_error().decode(errors="replace"))

    def close(self):
        if self.h:
            self.lib.pbsim_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def load_errhmm(self, path):
        _check(self.lib.pbsim_load_errhmm(self.h, os.fsencode(path)))

    def load_qshmm(self, path):
        _check(self.lib.pbsim_load_qshmm(self.h, os.fsencode(path)))

    def set_reference(self, seq: bytes, record_index: int):
        buf = C.create_string_buffer(seq, len(seq))
        _check(self.lib.pbsim_set_reference(self.h, C.cast(buf, C.c_void_p), len(seq), record_index))

    def set_reference_device(self, ptr: int, length: int, record_index: int):
        _check(self.lib.pbsim_set_reference_device(self.h, C.c_void_p(ptr), length, record_index))

    def prefetch_reference_device(self, ptr: int, length: int):
        """upload + prepare the NEXT record beside the current simulation; set_reference_device(ptr, length, ...) adopts it"""
        _check(self.lib.pbsim_prefetch_reference_device(self.h, C.c_void_p(ptr), length))

    def add_hp_census(self, seq: bytes):
        buf = C.create_string_buffer(seq, len(seq))
        _check(self.lib.pbsim_add_hp_census(self.h, C.cast(buf, C.c_void_p), len(seq)))

    def finish_hp_census(self):
        _check(self.lib.pbsim_finish_hp_census(self.h))

    def simulate_wgs(self, collect=True):
        """Runs the quota loop of the current record; returns (read_text, maf_text)."""
        reads, mafs = [], []

        def on_read(user, text, n):
            reads.append(C.string_at(text, n))
            return 1

        def on_maf(user, text, n):
            mafs.append(C.string_at(text, n))
            return 1

        sink = Sink(None, SINK_CB(on_read), SINK_CB(on_maf))
        _check(self.lib.pbsim_simulate_wgs(self.h, C.byref(sink) if collect else None))
        return b"".join(reads), b"".join(mafs)

    def simulate_arrays(self, on_batch=None, labels=True):
        """Simulates the current unit (wgs: the record set by set_reference*; trans/templ: all loaded units) into torch
        tensors on this context's device instead of text.  With on_batch, calls on_batch(ReadBatch) once per batch in
        read order (returning False aborts: PbsimError) and returns None; without, returns one ReadBatch of all batches.
        labels=False leaves ref_pos out (None): 2 instead of 6 bytes per base."""
        import collections

        import torch
        dev = torch.device("cuda", self.device)
        pending, batches, error = collections.deque(), [], []

        def alloc(user, tasks, bases, out):
            try:
                # the caching allocator may hand out memory that torch's own stream still uses: let that finish before
                # this context's stream writes into it
                torch.cuda.current_stream(dev).synchronize()
                t = {}
                for name, dtype, per in ARRAY_FIELDS:
                    if name == "ref_pos" and not labels:
                        t[name] = None
                        continue
                    n = bases if per == "base" else tasks + 1 if per == "offset" else tasks
                    t[name] = torch.empty(n, dtype=getattr(torch, dtype), device=dev)
                    setattr(out.contents, name, t[name].data_ptr() or None)
                pending.append(t)
                return 1
            except BaseException as e:     # (an exception must not cross the C frames)
                error.append(e)
                return 0

        def done(user, info):
            try:
                b = ReadBatch(first_read=info.contents.first_read, **pending.popleft())
                if on_batch is None:
                    batches.append(b)
                    return 1
                return 0 if on_batch(b) is False else 1
            except BaseException as e:
                error.append(e)
                return 0

        sink = ArraySink(None, ARRAY_ALLOC_CB(alloc), ARRAY_BATCH_CB(done))
        ok = self.lib.pbsim_simulate_arrays(self.h, C.byref(sink))
        if error:
            raise error[0]
        _check(ok)
        if on_batch is not None:
            return None
        if not batches:
            empty = {name: torch.zeros(1 if per == "offset" else 0, dtype=getattr(torch, dtype), device=dev)
                     for name, dtype, per in ARRAY_FIELDS}
            if not labels:
                empty["ref_pos"] = None
            return ReadBatch(first_read=1, **empty)
        cat = {}
        for name, _, per in ARRAY_FIELDS:
            if name == "ref_pos" and not labels:
                cat[name] = None
            elif per == "offset":
                base, parts = 0, []
                for b in batches:
                    parts.append(b.offsets[:-1] + base)
                    base += int(b.offsets[-1])
                parts.append(torch.tensor([base], dtype=torch.int64, device=dev))
                cat[name] = torch.cat(parts)
            else:
                cat[name] = torch.cat([getattr(b, name) for b in batches])
        return ReadBatch(first_read=batches[0].first_read, **cat)

    def sam_header(self):
        n = self.lib.pbsim_sam_header(self.h, None, 0)
        buf = C.create_string_buffer(n + 1)
        self.lib.pbsim_sam_header(self.h, buf, n + 1)
        return buf.raw[:n]

    def set_sample_profile(self, quals):
        """quals: list[bytes], the filtered quality strings in file order (pbsim3_amd.args.read_sample_fastq)"""
        n = len(quals)
        keep = [C.create_string_buffer(q, len(q)) for q in quals]
        ptrs = (C.c_void_p * n)(*[C.cast(b, C.c_void_p).value for b in keep])
        lens = (C.c_int64 * n)(*[len(q) for q in quals])
        _check(self.lib.pbsim_set_sample_profile(self.h, n, ptrs, lens))

    def load_sample_fastq(self, path, acc_min=0.75, acc_max=1.0):
        """The profile of the --sample FASTQ `path` (plain, BGZF or other gzip), parsed and filtered on the GPU: lengths within
        the params' len_min / len_max, accuracies within [acc_min, acc_max].  Returns its SampleStats."""
        st = SampleStats()
        _check(self.lib.pbsim_load_sample_fastq(self.h, os.fsencode(path), acc_min, acc_max, C.byref(st)))
        return st

    def sample_profile_from_fastq(self, data, acc_min=0.75, acc_max=1.0):
        """The same from FASTQ bytes: `bytes`, or a contiguous uint8 torch tensor on the context's device."""
        st = SampleStats()
        if isinstance(data, (bytes, bytearray, memoryview)):
            data = bytes(data)
            _check(self.lib.pbsim_sample_profile_from_bytes(self.h, data, len(data), acc_min, acc_max, C.byref(st)))
            return st
        import torch
        if not (isinstance(data, torch.Tensor) and data.dtype == torch.uint8 and data.is_cuda and data.is_contiguous()):
            raise TypeError("sample_profile_from_fastq: bytes or a contiguous uint8 tensor on the context's device")
        if data.device.index != self.device:
            raise ValueError("sample_profile_from_fastq: the tensor is on another device than the context")
        torch.cuda.current_stream(data.device).synchronize()   # the bytes are complete when the library reads them
        _check(self.lib.pbsim_sample_profile_from_device(self.h, C.c_void_p(data.data_ptr()), data.numel(), acc_min, acc_max,
                                                         C.byref(st)))
        return st

    def load_sample(self, path, acc_min=0.75, acc_max=1.0):
        """The profile of the --sample file `path`, FASTQ or BAM (unaligned or aligned), recognised by content behind any gzip
        layer.  A BAM gives the profile of the FASTQ `samtools fastq` would write from it: secondary and supplementary
        records skipped, reverse-strand records in the read's own orientation.  Returns its SampleStats."""
        st = SampleStats()
        _check(self.lib.pbsim_load_sample(self.h, os.fsencode(path), acc_min, acc_max, C.byref(st)))
        return st

    def sample_profile_from_bam(self, data, acc_min=0.75, acc_max=1.0):
        """The same from inflated BAM bytes: `bytes`, or a contiguous uint8 torch tensor on the context's device."""
        st = SampleStats()
        if isinstance(data, (bytes, bytearray, memoryview)):
            data = bytes(data)
            _check(self.lib.pbsim_sample_profile_from_bam_bytes(self.h, data, len(data), acc_min, acc_max, C.byref(st)))
            return st
        import torch
        if not (isinstance(data, torch.Tensor) and data.dtype == torch.uint8 and data.is_cuda and data.is_contiguous()):
            raise TypeError("sample_profile_from_bam: bytes or a contiguous uint8 tensor on the context's device")
        if data.device.index != self.device:
            raise ValueError("sample_profile_from_bam: the tensor is on another device than the context")
        torch.cuda.current_stream(data.device).synchronize()   # the bytes are complete when the library reads them
        _check(self.lib.pbsim_sample_profile_from_bam_device(self.h, C.c_void_p(data.data_ptr()), data.numel(), acc_min, acc_max,
                                                             C.byref(st)))
        return st

    def sample_profile(self):
        """The filtered quality strings the context holds, in file order (the lines of sample_profile_<ID>.fastq)."""
        n = C.c_int64(0)
        _check(self.lib.pbsim_sample_profile_text(self.h, None, 0, C.byref(n)))
        buf = C.create_string_buffer(max(n.value, 1))
        _check(self.lib.pbsim_sample_profile_text(self.h, buf, n.value, C.byref(n)))
        return buf.raw[:n.value].split(b"\n")[:-1]

    def set_sample_chunk_bytes(self, n):
        """FASTQ (or inflated BAM) bytes per window of the GPU profile builder (0: the default); the profile does not depend on it."""
        _check(self.lib.pbsim_set_sample_chunk_bytes(self.h, n))

    def simulate_sample(self, collect=True):
        return self._simulate(self.lib.pbsim_simulate_sample, collect)

    def _simulate(self, fn, collect):
        reads, mafs = [], []

        def on_read(user, text, n):
            reads.append(C.string_at(text, n))
            return 1

        def on_maf(user, text, n):
            mafs.append(C.string_at(text, n))
            return 1

        sink = Sink(None, SINK_CB(on_read), SINK_CB(on_maf))
        _check(fn(self.h, C.byref(sink) if collect else None))
        return b"".join(reads), b"".join(mafs)

    def set_deflate(self, mask=3):
        """bit 0: read sink, bit 1: MAF sink receive gzip members compressed on the GPU"""
        _check(self.lib.pbsim_set_deflate(self.h, 3 if mask is True else int(mask)))

    def deflate_buffer(self, data: bytes) -> bytes:
        """gzip members (BGZF-framed) of `data`, compressed by the GPU kernels."""
        cap = self.lib.pbsim_deflate_bound(len(data)) + 64
        dst = C.create_string_buffer(cap)
        n = C.c_int64(0)
        src = C.create_string_buffer(data, len(data)) if data else None
        _check(self.lib.pbsim_deflate_buffer(self.h, src, len(data), dst, cap, C.byref(n)))
        return dst.raw[:n.value]

    def inflate_buffer(self, data: bytes) -> bytes:
        """The bytes of BGZF `data` (gzip members with the 'BC' field), inflated by the GPU kernels."""
        cap = inflate_bound(data)
        if cap < 0:
            _check(self.lib.pbsim_inflate_buffer(self.h, data, len(data), None, 0, C.byref(C.c_int64(0))))
        dst = C.create_string_buffer(max(cap, 1))
        n = C.c_int64(0)
        _check(self.lib.pbsim_inflate_buffer(self.h, data, len(data), dst, cap, C.byref(n)))
        return dst.raw[:n.value]

    def sort_truth_bam(self, data, on_index=None):
        """A finished truth BAM (the bytes of a --truth-format bam file) -> (the coordinate-sorted BAM, its .csi index,
        (records, references with records, inflated record bytes, index bins)): pbsim_truth_bam_sort.  `on_index`
        (optional) is called when the index arrives -- after the last piece of the BAM, and never when the call fails."""
        parts, index, at = [], [], [0]

        def on_bam(user, ptr, n, offset):
            if offset != at[0]:      # (the pieces come in offset order)
                return 0
            parts.append(C.string_at(ptr, n))
            at[0] += n
            return 1

        def on_idx(user, ptr, n):
            index.append(C.string_at(ptr, n))
            if on_index:
                on_index(index[-1])
            return 1
        sink = SortedBamSink(None, SORTED_BAM_CB(on_bam), SORTED_INDEX_CB(on_idx))
        stats = (C.c_int64 * 4)()
        _check(self.lib.pbsim_truth_bam_sort(self.h, bytes(data), len(data), C.byref(sink), stats))
        return b"".join(parts), b"".join(index), tuple(stats)

    def eval_bam(self, truth, query, ref_names=None, overlap=0.1, verdicts=False, hash_bits=0):
        """A mapper's BAM scored against the truth (pbsim_truth_bam_eval; the rule: include/pbsim3_amd.h).  truth: the bytes
        of one truth BAM or a list of them; query: the bytes of the mapper's BAM; ref_names: per truth file None or the name
        (str / bytes) its only reference has in the query; overlap: the least intersection / union of a correct mapping,
        in (0, 1]; hash_bits: see the header (tests only).  Returns (counts, hist, report) -- a dict, a numpy [256, 2] array of
        (scored, wrong) by MAPQ, the report text -- and with `verdicts` a fourth item: one uint8 per truth record, 0 missing,
        1 unmapped, 2 wrong, 3 correct."""
        import numpy as np
        files = [truth] if isinstance(truth, (bytes, bytearray, memoryview)) else list(truth)
        names = list(ref_names) if ref_names is not None else [None] * len(files)
        if len(names) != len(files):
            raise ValueError("ref_names: one entry per truth file (%d given for %d files)" % (len(names), len(files)))
        if not 0 < overlap <= 1:
            raise ValueError("overlap must be in (0, 1]")
        keep = [bytes(f) for f in files]
        arr = (EvalTruth * max(len(keep), 1))()
        for k, (f, nm) in enumerate(zip(keep, names)):
            arr[k] = EvalTruth(f, len(f), None if nm is None else (nm.encode() if isinstance(nm, str) else bytes(nm)))
        opts = EvalOpts(max(1, int(round(overlap * 1000))), int(hash_bits))
        got = []

        def on_verdicts(user, ptr, n):
            got.append(np.frombuffer(C.string_at(ptr, n), dtype=np.uint8).copy() if n else np.zeros(0, np.uint8))
            return 1
        sink = EvalSink(None, EVAL_VERDICTS_CB(on_verdicts))
        counts = (C.c_int64 * 12)()
        hist = (C.c_int64 * 512)()
        query = bytes(query)
        _check(self.lib.pbsim_truth_bam_eval(self.h, arr, len(keep), query, len(query), C.byref(opts), C.byref(sink) if verdicts else None,
                                             counts, hist))
        cd = dict(zip(EVAL_COUNTS, (int(v) for v in counts)))
        hd = np.array(list(hist), dtype=np.int64).reshape(256, 2)
        out = (cd, hd, eval_report(cd, hd))
        return out + (got[0],) if verdicts else out

    def bam_depth(self, data, fmt="bedgraph", window=0, min_mapq=0, exclude_flags=0x704, deletions=True, arrays=False, piece_bytes=0):
        """The depth of coverage of a BAM (pbsim_bam_depth; the rule: include/pbsim3_amd.h).  data: the bytes of a truth BAM
        or a mapper's BAM; fmt: "bedgraph" (runs of equal depth) or "window" (sums over windows of `window` positions).  Returns
        (text, counts, refs, hist, report): the text's bytes, a dict, a list of (name, l_ref, covered, sum, max), a numpy
        int64[256] and the report text -- and with `arrays` a sixth item, a list of numpy int32 arrays, one per reference."""
        import numpy as np
        if fmt not in DEPTH_FORMATS:
            raise ValueError("fmt must be bedgraph or window")
        parts, at, refs, depth = [], [0], [], []

        def on_text(user, ptr, n, offset):
            if offset != at[0]:      # (the pieces come in offset order)
                return 0
            parts.append(C.string_at(ptr, n))
            at[0] += n
            return 1

        def on_refs(user, n_ref, names, rows):
            refs.extend((names[r],) + tuple(int(rows[4 * r + k]) for k in range(4)) for r in range(n_ref))
            return 1

        def on_depth(user, ref, ptr, l_ref):
            depth.append(np.frombuffer(C.string_at(ptr, 4 * l_ref), dtype=np.int32).copy() if l_ref else np.zeros(0, np.int32))
            return 1
        sink = DepthSink(None, DEPTH_TEXT_CB(on_text), DEPTH_REFS_CB(on_refs), DEPTH_ARRAY_CB(on_depth) if arrays else DEPTH_ARRAY_CB())
        opts = DepthOpts(int(exclude_flags), int(min_mapq), 1 if deletions else 0, DEPTH_FORMATS[fmt], int(window), int(piece_bytes))
        counts = (C.c_int64 * 6)()
        hist = (C.c_int64 * 256)()
        data = bytes(data)
        _check(self.lib.pbsim_bam_depth(self.h, data, len(data), C.byref(opts), C.byref(sink), counts, hist))
        cd = dict(zip(DEPTH_COUNTS, (int(v) for v in counts)))
        hd = np.array(list(hist), dtype=np.int64)
        out = (b"".join(parts), cd, refs, hd, depth_report(cd, refs, hd))
        return out + (depth,) if arrays else out

    def bam_stats(self, files, min_mapq=0, exclude_flags=0x900, text=False, piece_bytes=0):
        """A summary of the reads of BAM files (pbsim_bam_stats; the rule: include/pbsim3_amd.h).  files: the bytes of one
        file, or a list of them, summed into one result.  Returns (counts, len_row, totals, hist_q, hist_identity, hist_qacc,
        report): three dicts, three numpy int64 arrays (128, 1001 and 1001 bins) and the report text -- and with `text` an
        eighth item, the per-read lines."""
        import numpy as np
        if isinstance(files, (bytes, bytearray, memoryview)):
            files = [files]
        files = [bytes(f) for f in files]
        arr = (StatsFile * max(len(files), 1))(*[StatsFile(C.cast(C.c_char_p(f), C.c_void_p), len(f)) for f in files])
        parts, at = [], [0]

        def on_text(user, ptr, n, offset):
            if offset != at[0]:      # (the pieces come in offset order)
                return 0
            parts.append(C.string_at(ptr, n))
            at[0] += n
            return 1
        sink = StatsSink(None, STATS_TEXT_CB(on_text) if text else STATS_TEXT_CB())
        opts = StatsOpts(int(exclude_flags), int(min_mapq), int(piece_bytes))
        out = [(C.c_int64 * k)() for k in (10, 16, 12, 128, 1001, 1001)]
        _check(self.lib.pbsim_bam_stats(self.h, arr, len(files), C.byref(opts), C.byref(sink), *out))
        cd = dict(zip(STATS_COUNTS, (int(v) for v in out[0])))
        ld = dict(zip(STATS_LEN_ROW, (int(v) for v in out[1])))
        td = dict(zip(STATS_TOTALS, (int(v) for v in out[2])))
        hists = tuple(np.array(list(h), dtype=np.int64) for h in out[3:])
        res = (cd, ld, td) + hists + (stats_report(cd, ld, td, *hists),)
        return res + (b"".join(parts),) if text else res

    def bam_errors(self, files, genome, ref_names=None, text=False, min_mapq=0, exclude_flags=0x900, piece_bytes=0):
        """The error profile of the aligned reads of BAM files against their genome (pbsim_bam_errors; the rule:
        include/pbsim3_amd.h).  files: the bytes of one file, or a list of them, summed into one result; genome: a list of (name,
        sequence lines) with names as str or bytes, line feeds allowed in the lines; ref_names: per file None or the name its only
        reference has in the genome.  Returns (result, report): a dict -- counts and totals as dicts by name, the arrays pair,
        hp_cols, hp_sub, hp_del, ins_len, del_len, ins_base, del_base, qcal (128 x 3, flat) and hist_identity as lists, fit_ok,
        fit_bias_milli, fit_suggest_milli -- and the report text; with `text` a third item, the per-read lines."""
        if isinstance(files, (bytes, bytearray, memoryview)):
            files = [files]
        files = [bytes(f) for f in files]
        names = list(ref_names) if ref_names is not None else [None] * len(files)
        if len(names) != len(files):
            raise ValueError("ref_names: one entry per file (%d given for %d files)" % (len(names), len(files)))
        names = [None if nm is None else (nm.encode() if isinstance(nm, str) else bytes(nm)) for nm in names]
        genome = [((nm.encode() if isinstance(nm, str) else bytes(nm)), bytes(lines)) for nm, lines in genome]
        refs = (ErrorsRef * max(len(genome), 1))(*[ErrorsRef(nm, C.cast(C.c_char_p(lines), C.c_void_p), len(lines)) for nm, lines in genome])
        arr = (ErrorsFile * max(len(files), 1))(*[ErrorsFile(C.cast(C.c_char_p(f), C.c_void_p), len(f), nm) for f, nm in zip(files, names)])
        parts, at = [], [0]

        def on_text(user, ptr, n, offset):
            if offset != at[0]:      # (the pieces come in offset order)
                return 0
            parts.append(C.string_at(ptr, n))
            at[0] += n
            return 1
        sink = ErrorsSink(None, ERRORS_TEXT_CB(on_text) if text else ERRORS_TEXT_CB())
        opts = ErrorsOpts(int(exclude_flags), int(min_mapq), int(piece_bytes))
        res = ErrorsResult()
        _check(self.lib.pbsim_bam_errors(self.h, refs, len(genome), arr, len(files), C.byref(opts), C.byref(sink), C.byref(res)))
        out = _errors_dict(res)
        got = (out, errors_report(out))
        return got + (b"".join(parts),) if text else got

    def bam_pileup(self, files, genome, ref_names=None, text=False, fmt="sites", min_mapq=0, exclude_flags=0x900, min_baseq=0, min_depth=1,
                   arrays=False, piece_bytes=0):
        """The pileup of the aligned reads of BAM files against their genome (pbsim_bam_pileup; the rule: include/pbsim3_amd.h).
        files, genome and ref_names as bam_errors takes them; fmt: "sites" (the discordant sites) or "all" (every position).
        Returns (result, report): a dict -- counts, sites and cell_sums as dicts by name, ins_unanchored, max_depth, and hp_called,
        hp_sub, hp_del, hp_ins as lists -- and the report text; with `text` a further item, the lines; with `arrays` a further
        item, a list with one uint32 tensor [l_ref, 8] per genome record: the cells A C G T other del ins masked."""
        import numpy as np
        if arrays:
            import torch
        if fmt not in PILEUP_FORMATS:
            raise ValueError("fmt must be sites or all")
        if isinstance(files, (bytes, bytearray, memoryview)):
            files = [files]
        files = [bytes(f) for f in files]
        names = list(ref_names) if ref_names is not None else [None] * len(files)
        if len(names) != len(files):
            raise ValueError("ref_names: one entry per file (%d given for %d files)" % (len(names), len(files)))
        names = [None if nm is None else (nm.encode() if isinstance(nm, str) else bytes(nm)) for nm in names]
        genome = [((nm.encode() if isinstance(nm, str) else bytes(nm)), bytes(lines)) for nm, lines in genome]
        refs = (ErrorsRef * max(len(genome), 1))(*[ErrorsRef(nm, C.cast(C.c_char_p(lines), C.c_void_p), len(lines)) for nm, lines in genome])
        arr = (ErrorsFile * max(len(files), 1))(*[ErrorsFile(C.cast(C.c_char_p(f), C.c_void_p), len(f), nm) for f, nm in zip(files, names)])
        parts, at, cells = [], [0], []

        def on_text(user, ptr, n, offset):
            if offset != at[0]:      # (the pieces come in offset order)
                return 0
            parts.append(C.string_at(ptr, n))
            at[0] += n
            return 1

        def on_cells(user, ref, ptr, l_ref):
            a = np.frombuffer(C.string_at(ptr, 32 * l_ref), dtype=np.uint32).copy() if l_ref else np.zeros(0, np.uint32)
            cells.append(torch.from_numpy(a.reshape(l_ref, 8)))
            return 1
        sink = PileupSink(None, PILEUP_TEXT_CB(on_text) if text else PILEUP_TEXT_CB(), PILEUP_CELLS_CB(on_cells) if arrays else PILEUP_CELLS_CB())
        opts = PileupOpts(int(exclude_flags), int(min_mapq), int(min_baseq), PILEUP_FORMATS[fmt], int(min_depth), int(piece_bytes))
        res = PileupResult()
        _check(self.lib.pbsim_bam_pileup(self.h, refs, len(genome), arr, len(files), C.byref(opts), C.byref(sink), C.byref(res)))
        out = _pileup_dict(res)
        got = (out, pileup_report(out))
        if text:
            got += (b"".join(parts),)
        return got + (cells,) if arrays else got

    def bam_consensus(self, files, genome, ref_names=None, text=True, min_mapq=0, exclude_flags=0x900, min_baseq=0, min_depth=1, fill="n",
                      max_ins=1024, line_width=60, piece_bytes=0):
        """The consensus FASTA of the aligned reads of BAM files against their genome (pbsim_bam_consensus; the rule:
        include/pbsim3_amd.h).  files, genome and ref_names as bam_pileup takes them; fill: "n" (N at a site that is not called) or
        "ref" (the genome's base there).  Returns (result, report): a dict -- counts, sites and bases as dicts by name, ins_len as a
        list, ins_unanchored, max_depth, ins_sites, ins_longest, ins_capped, text_bytes -- and the report text; with `text` two
        further items, the FASTA and a list of (l_ref, l_cons) per genome record."""
        if fill not in CONSENSUS_FILL:
            raise ValueError("fill must be n or ref")
        if isinstance(files, (bytes, bytearray, memoryview)):
            files = [files]
        files = [bytes(f) for f in files]
        names = list(ref_names) if ref_names is not None else [None] * len(files)
        if len(names) != len(files):
            raise ValueError("ref_names: one entry per file (%d given for %d files)" % (len(names), len(files)))
        names = [None if nm is None else (nm.encode() if isinstance(nm, str) else bytes(nm)) for nm in names]
        genome = [((nm.encode() if isinstance(nm, str) else bytes(nm)), bytes(lines)) for nm, lines in genome]
        refs = (ErrorsRef * max(len(genome), 1))(*[ErrorsRef(nm, C.cast(C.c_char_p(lines), C.c_void_p), len(lines)) for nm, lines in genome])
        arr = (ErrorsFile * max(len(files), 1))(*[ErrorsFile(C.cast(C.c_char_p(f), C.c_void_p), len(f), nm) for f, nm in zip(files, names)])
        parts, at, lengths = [], [0], []

        def on_text(user, ptr, n, offset):
            if offset != at[0]:      # (the pieces come in offset order)
                return 0
            parts.append(C.string_at(ptr, n))
            at[0] += n
            return 1

        def on_record(user, ref, l_ref, l_cons):
            lengths.append((int(l_ref), int(l_cons)))
            return 1
        sink = ConsensusSink(None, CONSENSUS_TEXT_CB(on_text) if text else CONSENSUS_TEXT_CB(),
                             CONSENSUS_RECORD_CB(on_record) if text else CONSENSUS_RECORD_CB())
        opts = ConsensusOpts(int(exclude_flags), int(min_mapq), int(min_baseq), CONSENSUS_FILL[fill], int(min_depth), int(max_ins), int(line_width),
                             int(piece_bytes))
        res = ConsensusResult()
        _check(self.lib.pbsim_bam_consensus(self.h, refs, len(genome), arr, len(files), C.byref(opts), C.byref(sink), C.byref(res)))
        out = _consensus_dict(res)
        got = (out, consensus_report(out))
        return got + (b"".join(parts), lengths) if text else got

    def bam_call(self, files, genome, ref_names=None, text=True, min_mapq=0, exclude_flags=0x900, min_baseq=0, min_depth=1, max_ins=1024, piece_bytes=0):
        """The differences between the genome and what the pile of aligned reads of BAM files spells, as VCF (pbsim_bam_call; the
        rule: include/pbsim3_amd.h).  files, genome and ref_names as bam_consensus takes them.  Returns (result, report): a dict --
        counts, sites and types as dicts by name, ins_unanchored, max_depth, variants, ref_bases, alt_bases, longest_ref, longest_alt,
        unplaced_records, unplaced_sites, header_bytes, text_bytes -- and the report text; with `text` two further items, the VCF and
        a list of (l_ref, n_variants) per genome record."""
        if isinstance(files, (bytes, bytearray, memoryview)):
            files = [files]
        files = [bytes(f) for f in files]
        names = list(ref_names) if ref_names is not None else [None] * len(files)
        if len(names) != len(files):
            raise ValueError("ref_names: one entry per file (%d given for %d files)" % (len(names), len(files)))
        names = [None if nm is None else (nm.encode() if isinstance(nm, str) else bytes(nm)) for nm in names]
        genome = [((nm.encode() if isinstance(nm, str) else bytes(nm)), bytes(lines)) for nm, lines in genome]
        refs = (ErrorsRef * max(len(genome), 1))(*[ErrorsRef(nm, C.cast(C.c_char_p(lines), C.c_void_p), len(lines)) for nm, lines in genome])
        arr = (ErrorsFile * max(len(files), 1))(*[ErrorsFile(C.cast(C.c_char_p(f), C.c_void_p), len(f), nm) for f, nm in zip(files, names)])
        parts, at, records = [], [0], []

        def on_text(user, ptr, n, offset):
            if offset != at[0]:      # (the pieces come in offset order)
                return 0
            parts.append(C.string_at(ptr, n))
            at[0] += n
            return 1

        def on_record(user, ref, l_ref, n_variants):
            records.append((int(l_ref), int(n_variants)))
            return 1
        sink = CallSink(None, CALL_TEXT_CB(on_text) if text else CALL_TEXT_CB(), CALL_RECORD_CB(on_record) if text else CALL_RECORD_CB())
        opts = CallOpts(int(exclude_flags), int(min_mapq), int(min_baseq), int(max_ins), int(min_depth), int(piece_bytes))
        res = CallResult()
        _check(self.lib.pbsim_bam_call(self.h, refs, len(genome), arr, len(files), C.byref(opts), C.byref(sink), C.byref(res)))
        out = _call_dict(res)
        got = (out, call_report(out))
        return got + (b"".join(parts), records) if text else got

    def mutate_genome(self, genome, seed=1, snv_ppm=1000, ins_ppm=100, del_ppm=100, ext_ppm=500000, max_indel=50, line_width=60, text=True,
                      origin=False, piece_bytes=0):
        """A variant genome and its truth variants drawn from `genome` -- a list of (name, sequence lines) -- and a seed
        (pbsim_genome_mutate; the rule: include/pbsim3_amd.h).  Returns (result, report): a dict -- drawn and types as dicts by name,
        records, bases_in, eligible, bases_out, void_del, dropped, merged, substituted, inserted, deleted, variants, ref_bases,
        alt_bases, longest_ref, longest_alt, header_bytes, vcf_bytes, fasta_bytes -- and the report text; with `text` three further
        items, the FASTA, the VCF and a list of (l_ref, l_out, n_variants) per genome record; with `origin` one more, a list of numpy
        int32 arrays, per record and written base the genome position it stands for, -1 - p for a base inserted behind p."""
        import numpy as np
        genome = [((nm.encode() if isinstance(nm, str) else bytes(nm)), bytes(lines)) for nm, lines in genome]
        refs = (ErrorsRef * max(len(genome), 1))(*[ErrorsRef(nm, C.cast(C.c_char_p(lines), C.c_void_p), len(lines)) for nm, lines in genome])
        texts, at, records, origins = ([], []), [0, 0], [], []

        def on_text(which):
            def take(user, ptr, n, offset):
                if offset != at[which]:      # (the pieces come in offset order)
                    return 0
                texts[which].append(C.string_at(ptr, n))
                at[which] += n
                return 1
            return take

        def on_record(user, ref, l_ref, l_out, n_variants):
            records.append((int(l_ref), int(l_out), int(n_variants)))
            return 1

        def on_origin(user, ref, ptr, l_out):
            origins.append(np.frombuffer(C.string_at(ptr, 4 * l_out), dtype=np.int32).copy() if l_out else np.zeros(0, np.int32))
            return 1
        sink = MutateSink(None, MUTATE_TEXT_CB(on_text(0)) if text else MUTATE_TEXT_CB(), MUTATE_TEXT_CB(on_text(1)) if text else MUTATE_TEXT_CB(),
                          MUTATE_RECORD_CB(on_record) if text else MUTATE_RECORD_CB(), MUTATE_ORIGIN_CB(on_origin) if origin else MUTATE_ORIGIN_CB())
        for name, v in (("seed", seed), ("snv_ppm", snv_ppm), ("ins_ppm", ins_ppm), ("del_ppm", del_ppm), ("ext_ppm", ext_ppm),
                        ("max_indel", max_indel), ("line_width", line_width)):
            if not (0 <= int(v) < 2 ** 32 if name == "seed" else -2 ** 31 <= int(v) < 2 ** 31):
                raise ValueError("%s: %d does not fit its 32-bit field" % (name, int(v)))
        opts = MutateOpts(int(seed), int(snv_ppm), int(ins_ppm), int(del_ppm), int(ext_ppm), int(max_indel), int(line_width), int(piece_bytes))
        res = MutateResult()
        _check(self.lib.pbsim_genome_mutate(self.h, refs, len(genome), C.byref(opts), C.byref(sink), C.byref(res)))
        out = _mutate_dict(res)
        got = (out, mutate_report(out))
        if text:
            got += (b"".join(texts[0]), b"".join(texts[1]), records)
        return got + (origins,) if origin else got

    def compare_vcf(self, truth, calls, genome, ref_names=None, lines="discordant", min_ms=0, text=True, piece_bytes=0):
        """A call set scored against the truth variants, both VCF texts over `genome` -- a list of (name, sequence lines) --, every
        indel moved to its leftmost placement first (pbsim_vcf_compare; the rule: include/pbsim3_amd.h).  ref_names: per genome
        record the contig name the VCFs use for it (None: the records' own).  lines: "discordant" or "all" (or 0, 1).  Returns
        (result, report): a dict of nested lists -- files, types, lengths, ms -- with text_bytes, and the report text; with `text`
        one further item, the annotated text."""
        truth, calls = bytes(truth), bytes(calls)
        genome = [((nm.encode() if isinstance(nm, str) else bytes(nm)), bytes(ls)) for nm, ls in genome]
        refs = (ErrorsRef * max(len(genome), 1))(*[ErrorsRef(nm, C.cast(C.c_char_p(ls), C.c_void_p), len(ls)) for nm, ls in genome])
        names = None
        if ref_names is not None:
            used = [nm.encode() if isinstance(nm, str) else bytes(nm) for nm in ref_names]
            if len(used) != len(genome):
                raise ValueError("ref_names: one entry per genome record (%d given for %d records)" % (len(used), len(genome)))
            names = (C.c_char_p * max(len(used), 1))(*used)
        for name, v in (("lines", COMPARE_LINES.get(lines, lines)), ("min_ms", min_ms)):
            if not -2 ** 31 <= int(v) < 2 ** 31:
                raise ValueError("%s: %d does not fit its 32-bit field" % (name, int(v)))
        parts, at = [], [0]

        def on_text(user, ptr, n, offset):
            if offset != at[0]:      # (the pieces come in offset order)
                return 0
            parts.append(C.string_at(ptr, n))
            at[0] += n
            return 1
        sink = CompareSink(None, COMPARE_TEXT_CB(on_text) if text else COMPARE_TEXT_CB())
        opts = CompareOpts(int(COMPARE_LINES.get(lines, lines)), int(min_ms), int(piece_bytes))
        res = CompareResult()
        _check(self.lib.pbsim_vcf_compare(self.h, refs, len(genome), names, truth, len(truth), calls, len(calls), C.byref(opts), C.byref(sink),
                                          C.byref(res)))
        out = _compare_dict(res)
        got = (out, compare_report(out))
        return got + (b"".join(parts),) if text else got

    def apply_vcf(self, vcf, genome, ref_names=None, haplotype=0, sample=0, lines="discordant", line_width=60, fasta=True, text=True,
                  origin=False, piece_bytes=0):
        """The lines of a VCF text applied to `genome` -- a list of (name, sequence lines) --, per haplotype (pbsim_vcf_apply; the
        rule: include/pbsim3_amd.h).  ref_names: per genome record the contig name the VCF uses for it (None: the records' own).
        haplotype: 0 the first ALT of every line, 1 or 2 that allele of the sample's GT.  sample: the 0-based sample column, or the
        sample's name in the #CHROM line.  lines: "discordant" or "all" (or 0, 1).  Returns (result, report): a dict -- types as a
        dict by name, lines, the classes, overlap, applied, bases_in, bases_out, inserted, deleted, substituted, longest_cluster,
        fasta_bytes, text_bytes -- and the report text; with `fasta` two further items, the FASTA and a list of (l_ref, l_out,
        n_applied) per genome record; with `text` one more, the annotated text; with `origin` one more, a list of numpy int32 arrays
        per record (the header states the encoding)."""
        import numpy as np
        vcf = bytes(vcf)
        genome = [((nm.encode() if isinstance(nm, str) else bytes(nm)), bytes(ls)) for nm, ls in genome]
        refs = (ErrorsRef * max(len(genome), 1))(*[ErrorsRef(nm, C.cast(C.c_char_p(ls), C.c_void_p), len(ls)) for nm, ls in genome])
        names = None
        if ref_names is not None:
            used = [nm.encode() if isinstance(nm, str) else bytes(nm) for nm in ref_names]
            if len(used) != len(genome):
                raise ValueError("ref_names: one entry per genome record (%d given for %d records)" % (len(used), len(genome)))
            names = (C.c_char_p * max(len(used), 1))(*used)
        if isinstance(sample, (str, bytes)):
            column = apply_sample(vcf, sample)
            if column < 0:
                raise ValueError("sample: the #CHROM line names no sample %r" % (sample,))
            sample = column
        for name, v in (("haplotype", haplotype), ("sample", sample), ("lines", APPLY_LINES.get(lines, lines)), ("line_width", line_width)):
            if not -2 ** 31 <= int(v) < 2 ** 31:
                raise ValueError("%s: %d does not fit its 32-bit field" % (name, int(v)))
        texts, at, records, origins = ([], []), [0, 0], [], []

        def on_text(which):
            def take(user, ptr, n, offset):
                if offset != at[which]:      # (the pieces come in offset order)
                    return 0
                texts[which].append(C.string_at(ptr, n))
                at[which] += n
                return 1
            return take

        def on_record(user, ref, l_ref, l_out, n_applied):
            records.append((int(l_ref), int(l_out), int(n_applied)))
            return 1

        def on_origin(user, ref, ptr, l_out):
            origins.append(np.frombuffer(C.string_at(ptr, 4 * l_out), dtype=np.int32).copy() if l_out else np.zeros(0, np.int32))
            return 1
        sink = ApplySink(None, APPLY_TEXT_CB(on_text(0)) if fasta else APPLY_TEXT_CB(), APPLY_TEXT_CB(on_text(1)) if text else APPLY_TEXT_CB(),
                         APPLY_RECORD_CB(on_record) if fasta else APPLY_RECORD_CB(), APPLY_ORIGIN_CB(on_origin) if origin else APPLY_ORIGIN_CB())
        opts = ApplyOpts(int(haplotype), int(sample), int(APPLY_LINES.get(lines, lines)), int(line_width), int(piece_bytes))
        res = ApplyResult()
        _check(self.lib.pbsim_vcf_apply(self.h, refs, len(genome), names, vcf, len(vcf), C.byref(opts), C.byref(sink), C.byref(res)))
        out = _apply_dict(res)
        got = (out, apply_report(out))
        if fasta:
            got += (b"".join(texts[0]), records)
        if text:
            got += (b"".join(texts[1]),)
        return got + (origins,) if origin else got

    def lift_bam(self, bam, genome, origin, ref_names=None, ref_name=None):
        """An aligned BAM whose records lie on a variant genome, placed on the original `genome` -- a list of (name, sequence lines)
        -- through `origin`, the list of int32 arrays per genome record that mutate_genome(origin=True) or apply_vcf(origin=True)
        returns (pbsim_bam_lift; the rule: include/pbsim3_amd.h).  ref_names: per genome record the name the BAM's header uses for it
        (None: the records' own); ref_name: the genome name of the only reference of a file that calls it otherwise (`ref` in a wgs
        truth BAM).  Returns (result, report, lifted_bytes): a dict of the counts and totals by name, the report text, and the lifted
        file, BGZF."""
        import numpy as np
        bam = bytes(bam)
        genome = [((nm.encode() if isinstance(nm, str) else bytes(nm)), bytes(ls)) for nm, ls in genome]
        if ref_names is not None:
            used = [nm.encode() if isinstance(nm, str) else bytes(nm) for nm in ref_names]
            if len(used) != len(genome):
                raise ValueError("ref_names: one entry per genome record (%d given for %d records)" % (len(used), len(genome)))
            genome = [(nm, ls) for nm, (_, ls) in zip(used, genome)]
        if len(origin) != len(genome):
            raise ValueError("origin: one map per genome record (%d given for %d records)" % (len(origin), len(genome)))
        maps = [np.ascontiguousarray(o, dtype=np.int32) for o in origin]
        refs = (ErrorsRef * max(len(genome), 1))(*[ErrorsRef(nm, C.cast(C.c_char_p(ls), C.c_void_p), len(ls)) for nm, ls in genome])
        origins = (LiftOrigin * max(len(maps), 1))(*[LiftOrigin(m.ctypes.data if m.size else None, m.size) for m in maps])
        if ref_name is not None:
            ref_name = ref_name.encode() if isinstance(ref_name, str) else bytes(ref_name)
        file = ErrorsFile(C.cast(C.c_char_p(bam), C.c_void_p), len(bam), ref_name)
        parts, at = [], [0]

        def on_bam(user, ptr, n, offset):
            if offset != at[0]:      # (the pieces come in offset order)
                return 0
            parts.append(C.string_at(ptr, n))
            at[0] += n
            return 1
        sink = LiftSink(None, LIFT_BAM_CB(on_bam))
        res = LiftResult()
        _check(self.lib.pbsim_bam_lift(self.h, refs, len(genome), origins, C.byref(file), C.byref(sink), C.byref(res)))
        out = _lift_dict(res)
        return out, lift_report(out), b"".join(parts)

    def set_transcripts(self, ids, plus, minus, seqs):
        """ids: list[str]; plus/minus: expression counts; seqs: list[bytes]."""
        n = len(ids)
        c_ids = (C.c_char_p * n)(*[i.encode() for i in ids])
        c_plus = (C.c_int64 * n)(*plus)
        c_minus = (C.c_int64 * n)(*minus)
        self._keep = [C.create_string_buffer(s, len(s)) for s in seqs]
        c_seqs = (C.c_void_p * n)(*[C.cast(b, C.c_void_p).value for b in self._keep])
        c_lens = (C.c_int64 * n)(*[len(s) for s in seqs])
        _check(self.lib.pbsim_set_transcripts(self.h, n, c_ids, c_plus, c_minus, c_seqs, c_lens))
        self._keep = None

    def set_templates(self, ids, seqs):
        """ids: list[str]; seqs: list[bytes] -- every template is one unit with one read over its whole length."""
        n = len(ids)
        c_ids = (C.c_char_p * n)(*[i.encode() for i in ids])
        keep = [C.create_string_buffer(s, len(s)) for s in seqs]
        c_seqs = (C.c_void_p * n)(*[C.cast(b, C.c_void_p).value for b in keep])
        c_lens = (C.c_int64 * n)(*[len(s) for s in seqs])
        _check(self.lib.pbsim_set_templates(self.h, n, c_ids, c_seqs, c_lens))

    def load_transcript_file(self, path):
        """--transcript file -> units; returns (transcripts, total expression value)"""
        st = (C.c_int64 * 2)()
        _check(self.lib.pbsim_load_transcript_file(self.h, os.fsencode(path), st))
        return st[0], st[1]

    def load_template_file(self, path):
        """--template FASTA -> units; returns (templates, total length)"""
        st = (C.c_int64 * 2)()
        _check(self.lib.pbsim_load_template_file(self.h, os.fsencode(path), st))
        return st[0], st[1]

    def unit_reads(self):
        return self.lib.pbsim_unit_reads(self.h)

    def simulate_units_range(self, first_read, n_reads):
        """reads first_read .. first_read + n_reads - 1 of the unit set (one rank's shard); returns (read text, maf text)"""
        reads, mafs = [], []

        def on_read(user, text, n):
            reads.append(C.string_at(text, n))
            return 1

        def on_maf(user, text, n):
            mafs.append(C.string_at(text, n))
            return 1

        sink = Sink(None, SINK_CB(on_read), SINK_CB(on_maf))
        _check(self.lib.pbsim_simulate_units_range(self.h, first_read, n_reads, C.byref(sink)))
        return b"".join(reads), b"".join(mafs)

    def simulate_trans(self, collect=True):
        reads, mafs = [], []

        def on_read(user, text, n):
            reads.append(C.string_at(text, n))
            return 1

        def on_maf(user, text, n):
            mafs.append(C.string_at(text, n))
            return 1

        sink = Sink(None, SINK_CB(on_read), SINK_CB(on_maf))
        _check(self.lib.pbsim_simulate_trans(self.h, C.byref(sink) if collect else None))
        return b"".join(reads), b"".join(mafs)

    def stats(self):
        s = Stats()
        _check(self.lib.pbsim_get_stats(self.h, C.byref(s)))
        return s

    def batch_walk(self, first_read, n_reads, truncate_remaining=-1):
        out = C.c_int64(0)
        _check(self.lib.pbsim_batch_walk(self.h, first_read, n_reads, truncate_remaining, C.byref(out)))
        return out.value

    def select_slot(self, slot):
        _check(self.lib.pbsim_select_slot(self.h, slot))

    def batch_walk_begin(self, first_read, n_reads, truncate_remaining=-1):
        _check(self.lib.pbsim_batch_walk_begin(self.h, first_read, n_reads, truncate_remaining))

    def batch_walk_end(self):
        out = C.c_int64(0)
        _check(self.lib.pbsim_batch_walk_end(self.h, C.byref(out)))
        return out.value

    def batch_finalize(self, len_total_before):
        bi = BatchInfo()
        _check(self.lib.pbsim_batch_finalize(self.h, len_total_before, C.byref(bi)))
        return bi

    def batch_fetch(self, info):
        r = C.create_string_buffer(max(1, info.read_text_bytes))
        m = C.create_string_buffer(max(1, info.maf_text_bytes))
        _check(self.lib.pbsim_batch_fetch(self.h, C.cast(r, C.c_void_p), C.cast(m, C.c_void_p)))
        return r.raw[:info.read_text_bytes], m.raw[:info.maf_text_bytes]

    def batch_fetch_deflated(self, info):
        """(read members, maf members): the batch's text as BGZF-framed gzip members compressed on the GPU"""
        cr = self.lib.pbsim_deflate_bound(info.read_text_bytes) + 16
        cm = self.lib.pbsim_deflate_bound(info.maf_text_bytes) + 16
        r, m = C.create_string_buffer(cr), C.create_string_buffer(cm)
        nr, nm = C.c_int64(0), C.c_int64(0)
        _check(self.lib.pbsim_batch_fetch_deflated(self.h, C.cast(r, C.c_void_p), cr, C.cast(m, C.c_void_p), cm,
                                                   C.byref(nr), C.byref(nm)))
        return r.raw[:nr.value], m.raw[:nm.value]

    def set_bam_output(self, on=True):
        _check(self.lib.pbsim_set_bam_output(self.h, 1 if on else 0))

    def bam_header(self):
        n = self.lib.pbsim_bam_header(self.h, None, 0)
        buf = C.create_string_buffer(n)
        self.lib.pbsim_bam_header(self.h, buf, n)
        return buf.raw[:n]

    def set_truth_bam(self, on=True):
        """the MAF stream carries aligned BAM records (one per task) instead of MAF blocks"""
        _check(self.lib.pbsim_set_truth_bam(self.h, 1 if on else 0))

    def truth_bam_header(self):
        n = self.lib.pbsim_truth_bam_header(self.h, None, 0)
        buf = C.create_string_buffer(n)
        self.lib.pbsim_truth_bam_header(self.h, buf, n)
        return buf.raw[:n]

    def job_truth_bam_header(self, record):
        n = self.lib.pbsim_job_truth_bam_header(self.h, record, None, 0)
        if n < 0:
            raise PbsimError("no record %d in the job" % record)
        buf = C.create_string_buffer(n)
        self.lib.pbsim_job_truth_bam_header(self.h, record, buf, n)
        return buf.raw[:n]

    # ---- the whole job (pbsim_job_*)
    def job_begin(self, first_record=1):
        _check(self.lib.pbsim_job_begin(self.h, first_record))

    def job_add_record(self, seq: bytes):
        buf = C.create_string_buffer(seq, len(seq))
        _check(self.lib.pbsim_job_add_record(self.h, C.cast(buf, C.c_void_p), len(seq)))

    def job_add_record_lines(self, lines: bytes):
        """the record as its FASTA sequence lines (line feeds included); they are squeezed out on the GPU"""
        buf = C.create_string_buffer(lines, len(lines))
        _check(self.lib.pbsim_job_add_record_lines(self.h, C.cast(buf, C.c_void_p), len(lines), len(lines) - lines.count(b"\n")))

    def job_expect(self, lens):
        """announce the job's records (their lengths): job_run may start before they have all been added, another thread adds them"""
        a = (C.c_int64 * len(lens))(*lens)
        _check(self.lib.pbsim_job_expect(self.h, len(lens), a))

    def job_feed_abort(self, why="the feeding thread gave up"):
        _check(self.lib.pbsim_job_feed_abort(self.h, why.encode()))

    def job_add_record_device(self, ptr: int, length: int):
        _check(self.lib.pbsim_job_add_record_device(self.h, C.c_void_p(ptr), length))

    def job_run(self, comm=None, collect=True, on_done=None):
        """Runs every record of the job.  collect: returns {record: [read bytes, maf bytes]} assembled from the positional
        pieces this rank received (holes stay zero: other ranks' ranges), plus {record: (Stats, read_bytes, maf_bytes)}."""
        pieces, done = {}, {}

        def put(which, rec, text, n, off):
            pieces.setdefault(rec, [[], []])[which].append((off, C.string_at(text, n)))
            return 1

        def fin(user, rec, st, rb, mb):
            s = Stats()
            C.memmove(C.byref(s), st, C.sizeof(Stats))
            done[rec] = (s, rb, mb)
            if on_done:
                on_done(rec, s, rb, mb)
            return 1

        cbs = (REC_TEXT_CB(lambda u, r, t, n, o: put(0, r, t, n, o)), REC_TEXT_CB(lambda u, r, t, n, o: put(1, r, t, n, o)),
               REC_DONE_CB(fin))
        sink = RecordSink(None, *cbs) if collect else RecordSink(None, REC_TEXT_CB(), REC_TEXT_CB(), cbs[2])
        _check(self.lib.pbsim_job_run(self.h, C.byref(comm) if comm is not None else None, C.byref(sink)))
        out = {}
        for rec, (s, rb, mb) in done.items():
            bufs = [bytearray(rb), bytearray(mb)]
            for which in (0, 1):
                for off, data in pieces.get(rec, [[], []])[which]:
                    bufs[which][off:off + len(data)] = data
            out[rec] = bufs
        return out, done

    def job_progress(self):
        """(phase, record, first_read, n_per, world, len_total, quota, next_read) of the exchange pbsim_job_run is about to enter"""
        a = (C.c_int64 * 8)()
        _check(self.lib.pbsim_job_progress(self.h, a))
        return tuple(a)

    def batch_fetch_lengths(self, n_reads):
        """(rawlen, len, pass-0 bases) of the reads of the walked batch on the selected slot, numpy int32 arrays"""
        import numpy as np
        r, l, o = (np.empty(n_reads, dtype=np.int32) for _ in range(3))
        _check(self.lib.pbsim_batch_fetch_lengths(self.h, r.ctypes.data, l.ctypes.data, o.ctypes.data))
        return r, l, o

    def scratch_state(self):
        """(factor the next batches' rows are laid out with, largest need seen, batches walked twice)"""
        a = (C.c_double * 3)()
        _check(self.lib.pbsim_scratch_state(self.h, a))
        return tuple(a)

    def job_counters(self):
        a = (C.c_int64 * 8)()
        _check(self.lib.pbsim_job_counters(self.h, a))
        return dict(reads_walked=a[0], reads_delivered=a[1], rounds=a[2], bases=a[3], wall_us=a[4], comm_us=a[5],
                    ref_bases=a[6], maf_columns=a[7])

    BREAKDOWN = ("wall", "wait_walk", "finalize", "wait_bytes", "collectives", "account", "tail_block", "drain", "slot_wait",
                 "merge", "begin", "tail_steps", "worker_busy", "topup_rounds", "tail_reads", "depth")

    def job_breakdown(self):
        """where the round loop of the last job_run spent its wall time: {name: microseconds} (+ three counters)"""
        a = (C.c_double * 16)()
        _check(self.lib.pbsim_job_breakdown(self.h, a))
        return dict(zip(self.BREAKDOWN, a))

    def job_sam_header(self, record):
        n = self.lib.pbsim_job_sam_header(self.h, record, None, 0)
        buf = C.create_string_buffer(n + 1)
        self.lib.pbsim_job_sam_header(self.h, record, buf, n + 1)
        return buf.raw[:n]

    def stats_keep_values(self, on=True):
        _check(self.lib.pbsim_stats_keep_values(self.h, 1 if on else 0))

    def stats_merge(self, comm):
        _check(self.lib.pbsim_stats_merge(self.h, C.byref(comm)))

    def stats_add_tasks(self, first_task, out_len, nsub, nins, ndel, qsum=None):
        import numpy as np
        a = [np.ascontiguousarray(x, dtype=np.int32) for x in (out_len, nsub, nins, ndel)]
        q = np.ascontiguousarray(qsum, dtype=np.float64) if qsum is not None else None
        p32 = C.POINTER(C.c_int32)
        _check(self.lib.pbsim_stats_add_tasks(self.h, first_task, len(a[0]), *[x.ctypes.data_as(p32) for x in a],
                                              q.ctypes.data_as(C.POINTER(C.c_double)) if q is not None else None))

    def format_stats(self, stats, unit=0):
        buf = C.create_string_buffer(2048)
        n = self.lib.pbsim_format_stats(C.byref(self.params), C.byref(stats), unit, buf, 2048)
        return buf.raw[:n].decode()

    def batch_account(self):
        _check(self.lib.pbsim_batch_account(self.h))

    def reset_stats(self):
        _check(self.lib.pbsim_reset_stats(self.h))

    def unit_quota(self):
        return self.lib.pbsim_unit_quota(self.h)

    def batch_capacity(self):
        return self.lib.pbsim_batch_capacity(self.h)

    def set_scratch_bytes(self, n):
        _check(self.lib.pbsim_set_scratch_bytes(self.h, n))

    def release_pools(self):
        _check(self.lib.pbsim_release_pools(self.h))

    def prof_reset(self):
        _check(self.lib.pbsim_prof_reset(self.h))

    def prof_get(self):
        a, b, c = C.c_double(0), C.c_int64(0), C.c_double(0)
        _check(self.lib.pbsim_prof_get(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def prof_tail(self):
        a, b = C.c_double(0), C.c_int64(0)
        _check(self.lib.pbsim_prof_tail(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def prof_secondary(self):
        a = (C.c_double * 8)()
        _check(self.lib.pbsim_prof_secondary(self.h, a))
        return dict(text_ms=a[0], text_launches=int(a[1]), text_in=int(a[2]), text_out=int(a[3]),
                    deflate_ms=a[4], deflate_launches=int(a[5]), deflate_in=int(a[6]), deflate_out=int(a[7]))

    def prof_wave_launches(self):
        return self.lib.pbsim_prof_wave_launches(self.h)

    def prof_walk_busy(self):
        a = C.c_double(0)
        _check(self.lib.pbsim_prof_walk_busy(self.h, C.byref(a)))
        return a.value

    def dump_table(self, which):
        """pbsim_dump_table (test infrastructure): 0 prob2len, 1 prob2acc, 2 class tables; of the current unit as the
        preparation kernels left it: 3 sequence bytes, 4 hp bytes (PbsimError when bit 7 of the sequence bytes carries
        hp == 11 instead), 5 its census (12 int64), 6 the census pbsim_add_hp_census has accumulated (12 int64)"""
        n = self.lib.pbsim_dump_table(self.h, which, None, 0)
        if n < 0:
            raise PbsimError(self.lib.pbsim_last_error().decode(errors="replace"))
        buf = C.create_string_buffer(n)
        if self.lib.pbsim_dump_table(self.h, which, C.cast(buf, C.c_void_p), n) != n:
            raise PbsimError(self.lib.pbsim_last_error().decode(errors="replace"))
        return buf.raw
