"""ctypes binding of include/slacken_amd.h (one Python method per C entry point; no compute happens in Python).
In a process that also uses PyTorch-ROCm, `import torch` before the first slacken_amd call: torch bundles its own HIP runtime,
and whichever runtime is loaded first is the one that can open the GPU."""
import ctypes as C
import os
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

DEFAULT_TOGGLE_MASK = 0xE37E28C4271B5A2D
E_INVALID, E_UNSUPPORTED, E_HIP, E_NO_GPU, E_CAPACITY, E_STATE = -1, -2, -3, -4, -5, -6   # SLK_E_* of the header
TAXON_NONE, TAXON_ROOT, TAXON_AMBIGUOUS, TAXON_MATE_PAIR_BORDER = 0, 1, -1, -2
FLAG_SEQUENCE, FLAG_AMBIGUOUS, FLAG_MATE_PAIR_BORDER = 1, 2, 3


class SlackenError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"slacken_amd error {code}: {msg}")
        self.code = code


class _Params(C.Structure):
    _fields_ = [("k", C.c_int32), ("m", C.c_int32), ("spaces", C.c_int32), ("canonical", C.c_int32),
                ("xor_mask", C.c_uint64), ("id_longs", C.c_int32), ("reserved", C.c_int32)]


class _TableConfig(C.Structure):
    _fields_ = [("expected_records", C.c_uint64), ("max_taxon", C.c_int32), ("load_factor", C.c_float)]


class IndexInfo(C.Structure):
    _fields_ = [("records", C.c_uint64), ("buckets", C.c_uint64), ("table_bytes", C.c_uint64),
                ("bucket_bits", C.c_int32), ("taxon_bits", C.c_int32), ("disp_bits", C.c_int32),
                ("max_displacement", C.c_int32), ("duplicate_keys", C.c_uint64), ("taxonomy_size", C.c_int32),
                ("device", C.c_int32), ("dense_taxa", C.c_int32), ("bucket_cells", C.c_int32), ("load_factor", C.c_float),
                ("grown", C.c_int32)]


class _ShardBatch(C.Structure):
    _fields_ = [("bases", C.c_void_p), ("offsets", C.c_void_p), ("mate_bases", C.c_void_p), ("mate_offsets", C.c_void_p),
                ("R", C.c_uint64), ("out_taxon", C.c_void_p), ("out_classified", C.c_void_p), ("out_num_distinct", C.c_void_p),
                ("out_total_kmers", C.c_void_p), ("out_hit_offsets", C.c_void_p), ("out_hits", C.c_void_p),
                ("hits_capacity", C.c_uint64)]


class ShardLists(C.Structure):
    """slk_shard_lists: a batch and the lists its EMIT job leaves on its rank (all device addresses)"""
    _fields_ = [("d_bases", C.c_void_p), ("d_offsets", C.c_void_p), ("d_mate_bases", C.c_void_p), ("d_mate_offsets", C.c_void_p),
                ("R", C.c_uint64), ("total_bases", C.c_uint64), ("total_mate_bases", C.c_uint64), ("n_shards", C.c_uint32),
                ("reserved", C.c_uint32), ("capacity_per_owner", C.c_uint64),
                ("d_send_keys", C.c_void_p), ("d_send_meta", C.c_void_p), ("d_cursors", C.c_void_p), ("d_batch_log", C.c_void_p),
                ("d_tile_rows", C.c_void_p), ("d_read_info", C.c_void_p), ("d_defer", C.c_void_p), ("d_span_meta", C.c_void_p),
                ("d_span_taxon", C.c_void_p), ("d_span_count", C.c_void_p)]


class ShardLookup(C.Structure):
    _fields_ = [("d_keys", C.c_void_p), ("n", C.c_uint64), ("d_out_taxa", C.c_void_p)]


class ShardResults(C.Structure):
    _fields_ = [("d_taxa", C.c_void_p), ("min_hit_groups", C.c_int32), ("C", C.c_int32), ("thresholds", C.POINTER(C.c_double)),
                ("d_out_taxon", C.c_void_p), ("d_out_classified", C.c_void_p), ("d_out_num_distinct", C.c_void_p),
                ("d_out_total_kmers", C.c_void_p), ("d_out_num_hits", C.c_void_p)]


EXCHANGE_AUTO, EXCHANGE_RCCL, EXCHANGE_COPY = 0, 1, 2
class _Reads(C.Structure):   # slk_reads: one side of a batch of slk_pipe_submit
    _fields_ = [("bases", C.c_void_p), ("codes", C.c_void_p), ("valid", C.c_void_p), ("exc_word", C.c_void_p), ("exc_bits", C.c_void_p),
                ("n_exc", C.c_uint64), ("offsets", C.c_void_p), ("lengths", C.c_void_p), ("uniform_len", C.c_uint32)]


SPAN_DTYPE = np.dtype([("key", "<i8"), ("kmers", "<i4"), ("flag", "i1"), ("distinct", "u1"), ("pad", "<u2")])
HIT_DTYPE = np.dtype([("taxon", "<i4"), ("count", "<i4")])

# every symbol include/slacken_amd.h declares
EXPORTS = ["slk_device_count", "slk_last_error", "slk_version", "slk_host_alloc", "slk_host_register", "slk_host_free", "slk_index_create", "slk_index_append",
           "slk_index_append_device", "slk_index_set_shard", "slk_index_set_taxonomy", "slk_index_finalize", "slk_index_get_info",
           "slk_index_lookup", "slk_index_add_sequences", "slk_index_add_sequences_device", "slk_index_export", "slk_index_export_range", "slk_index_taxon_counts", "slk_index_respace",
           "slk_index_set_merge_remap", "slk_index_merge_records", "slk_index_merge_records_device", "slk_index_merge_index", "slk_index_destroy", "slk_stream_create", "slk_stream_synchronize",
           "slk_stream_hip_stream", "slk_stream_destroy", "slk_spans_batch", "slk_spans_batch_wide", "slk_classify_batch",
           "slk_classify_batch_packed", "slk_pack_bases",
           "slk_classify_batch_device", "slk_classify_hits", "slk_stream_last_stage_ms", "slk_scan_device", "slk_lookup_device",
           "slk_shard_of", "slk_stream_set_merged_hits", "slk_classify_hits_device", "slk_shard_batch_rows", "slk_shard_chunk", "slk_shard_step_device",
           "slk_stream_last_deferred", "slk_stream_last_route", "slk_table_slot", "slk_table_hash_of",
           "slk_shardset_create", "slk_shardset_classify", "slk_shardset_classify_rounds", "slk_shardset_exchange_mode", "slk_shardset_staged_pairs", "slk_shardset_destroy", "slk_bracken_create", "slk_bracken_add", "slk_bracken_result", "slk_bracken_destroy",
           "slk_migration_create", "slk_migration_add", "slk_migration_add_device", "slk_migration_result", "slk_migration_destroy",
           "slk_coverage_create", "slk_coverage_add", "slk_coverage_fold", "slk_coverage_result", "slk_coverage_totals", "slk_coverage_budget",
           "slk_coverage_destroy",
           "slk_support_create", "slk_support_add", "slk_support_result", "slk_support_totals", "slk_support_destroy",
           "slk_parse_tile_bytes", "slk_parse_device", "slk_parse_text", "slk_classify_text",
           "slk_pair_device", "slk_parse_text_paired", "slk_classify_text_paired",
           "slk_pipe_create", "slk_pipe_set_merged_hits", "slk_pipe_submit", "slk_pipe_collect", "slk_pipe_pending", "slk_pipe_destroy",
           "slk_pack_bases_sparse",
           "slk_mask_tile_bases", "slk_mask_device", "slk_mask_sequences", "slk_index_add_sequences_masked",
           "slk_stream_set_split_long", "slk_stream_set_split_hits", "slk_stream_last_split", "slk_stream_split_info",
           "slk_compare_create", "slk_compare_add_reference", "slk_compare_add_reference_device", "slk_compare_begin_test",
           "slk_compare_add_test", "slk_compare_add_test_device", "slk_compare_pairs", "slk_compare_reference_taxa", "slk_compare_totals",
           "slk_compare_error", "slk_compare_destroy"]

# SLK_ROUTE_* of the header: the kernels a classify call launched (Stream.last_route)
ROUTE_LANE, ROUTE_ROUTING, ROUTE_LONG, ROUTE_SEGMENT, ROUTE_PIECES, ROUTE_WAVE, ROUTE_STAGED, ROUTE_RERUN = (1 << i for i in range(8))
ROUTE_NAMES = {ROUTE_LANE: "lane", ROUTE_ROUTING: "routing", ROUTE_LONG: "long", ROUTE_SEGMENT: "segment", ROUTE_PIECES: "pieces",
               ROUTE_WAVE: "wave", ROUTE_STAGED: "staged", ROUTE_RERUN: "rerun"}

COMPARE_BAD_LINE, COMPARE_DUPLICATE_REFERENCE, COMPARE_DUPLICATE_TEST = 1, 2, 3   # SLK_COMPARE_* of the header

PAIR_FIELDS = ("P", "mismatch", "consumed1", "consumed2", "R1", "R2", "n_bases", "n_mate_bases")   # slk_pair_record, in order

FORMAT_FASTA, FORMAT_FASTQ = 0, 1   # SLK_FORMAT_* of the header


def _format(fmt):
    if fmt in (FORMAT_FASTA, FORMAT_FASTQ):
        return int(fmt)
    try:
        return {"fasta": FORMAT_FASTA, "fa": FORMAT_FASTA, "fastq": FORMAT_FASTQ, "fq": FORMAT_FASTQ}[str(fmt).lower()]
    except KeyError:
        raise ValueError(f"format {fmt!r}: 'fasta' or 'fastq'") from None


class MaskConfig(C.Structure):   # slk_mask_config
    _fields_ = [("window", C.c_uint32), ("threshold", C.c_uint32), ("replacement", C.c_uint8)]


def mask_tile_bases():
    """The interval starts one workgroup of the masker takes at a time (slk_mask_tile_bases)"""
    return int(lib().slk_mask_tile_bases())


def parse_tile_bytes():
    """The bytes of text one workgroup of the device parser takes at a time (slk_parse_tile_bytes)"""
    return int(lib().slk_parse_tile_bytes())


def lib_path():
    # SLACKEN_AMD_LIB: another build of the same library (A/B experiments with different compile-time settings)
    return os.environ.get("SLACKEN_AMD_LIB") or os.path.join(_HERE, "lib", "libslacken_amd.so")


_lib = None


def lib():
    """Load libslacken_amd.so; raises loudly if it has not been built (there is no fallback implementation)."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with `make` (or __graft_entry__.build()). "
                          "slacken_amd has no CPU/Python fallback for the classify path.")
    L = C.CDLL(path)
    vp, u8p, i32p, i64p, u64p = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p
    L.slk_device_count.restype = C.c_int32
    L.slk_last_error.restype = C.c_char_p
    L.slk_version.restype = C.c_char_p
    L.slk_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.slk_host_register.argtypes = [vp, C.c_size_t]
    L.slk_host_free.argtypes = [vp]
    L.slk_index_create.argtypes = [C.POINTER(_Params), C.POINTER(_TableConfig), C.c_int32, C.POINTER(vp)]
    L.slk_index_append.argtypes = [vp, i64p, i32p, C.c_uint64]
    L.slk_index_append_device.argtypes = [vp, i64p, i32p, C.c_uint64]
    L.slk_index_set_taxonomy.argtypes = [vp, i32p, C.c_int32]
    L.slk_table_slot.argtypes = [C.c_uint64, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
    L.slk_table_hash_of.argtypes = [C.c_uint64, C.c_uint32, C.c_uint64, C.POINTER(C.c_uint64)]
    L.slk_shardset_create.argtypes = [C.POINTER(vp), C.c_int32, C.c_int32, C.POINTER(vp)]
    L.slk_shardset_classify.argtypes = [vp, C.POINTER(_ShardBatch), C.c_int32, C.POINTER(C.c_double), C.c_int32]
    L.slk_shardset_classify_rounds.argtypes = [vp, C.POINTER(_ShardBatch), C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_int32]
    L.slk_shardset_exchange_mode.argtypes = [vp]
    L.slk_shardset_staged_pairs.argtypes = [vp]
    L.slk_shardset_destroy.argtypes = [vp]
    L.slk_shardset_destroy.restype = None
    L.slk_index_set_shard.argtypes = [vp, C.c_uint32, C.c_uint32]
    L.slk_index_finalize.argtypes = [vp]
    L.slk_index_get_info.argtypes = [vp, C.POINTER(IndexInfo)]
    L.slk_index_lookup.argtypes = [vp, i64p, C.c_uint64, i32p]
    L.slk_index_add_sequences.argtypes = [vp, u8p, u64p, i32p, C.c_uint64]
    L.slk_index_add_sequences_device.argtypes = [vp, u8p, u64p, i32p, C.c_uint64]
    L.slk_index_export.argtypes = [vp, i64p, i32p, C.c_uint64, C.POINTER(C.c_uint64)]
    L.slk_index_export_range.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_int32, i64p, i32p, C.c_uint64, u64p, C.POINTER(C.c_uint64)]
    L.slk_index_taxon_counts.argtypes = [vp, i32p, u64p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.slk_index_respace.argtypes = [vp, C.c_int32, C.POINTER(_TableConfig), C.POINTER(vp)]
    L.slk_index_set_merge_remap.argtypes = [vp, i32p, C.c_int32]
    L.slk_index_merge_records.argtypes = [vp, i64p, i32p, C.c_uint64]
    L.slk_index_merge_records_device.argtypes = [vp, i64p, i32p, C.c_uint64]
    L.slk_index_merge_index.argtypes = [vp, vp]
    L.slk_index_destroy.argtypes = [vp]
    L.slk_index_destroy.restype = None
    L.slk_stream_create.argtypes = [vp, C.POINTER(vp)]
    L.slk_stream_synchronize.argtypes = [vp]
    L.slk_stream_set_merged_hits.argtypes = [vp, C.c_int32]
    L.slk_stream_hip_stream.argtypes = [vp]
    L.slk_stream_hip_stream.restype = C.c_void_p
    L.slk_stream_destroy.argtypes = [vp]
    L.slk_stream_destroy.restype = None
    L.slk_spans_batch.argtypes = [vp, vp, u8p, u64p, u8p, u64p, C.c_uint64, u64p, vp, C.c_uint64]
    L.slk_spans_batch_wide.argtypes = [vp, vp, u8p, u64p, u8p, u64p, C.c_uint64, u64p, vp, i64p, C.c_uint64]
    L.slk_classify_batch.argtypes = [vp, vp, u8p, u64p, u8p, u64p, C.c_uint64, C.c_int32, C.POINTER(C.c_double),
                                     C.c_int32, i32p, u8p, i32p, i32p, u64p, vp, C.c_uint64]
    L.slk_classify_batch_packed.argtypes = [vp, vp, vp, vp, u64p, vp, vp, u64p, C.c_uint64, C.c_int32, C.POINTER(C.c_double),
                                            C.c_int32, i32p, u8p, i32p, i32p, u64p, vp, C.c_uint64]
    L.slk_pack_bases.argtypes = [u8p, C.c_uint64, vp, vp]
    L.slk_classify_batch_device.argtypes = [vp, vp, u8p, u64p, u8p, u64p, C.c_uint64, C.c_uint64, C.c_uint64,
                                            C.c_int32, C.POINTER(C.c_double), C.c_int32, i32p, u8p, i32p, i32p, i32p, i32p]
    L.slk_classify_hits.argtypes = [vp, vp, C.c_uint64, u64p, vp, u8p, C.c_int32, C.POINTER(C.c_double), C.c_int32, i32p, u8p,
                                    i32p, i32p]
    L.slk_stream_last_stage_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.slk_scan_device.argtypes = [vp, vp, u8p, u64p, u8p, u64p, C.c_uint64, u64p, i32p, i32p]
    L.slk_lookup_device.argtypes = [vp, vp, i64p, C.c_uint64, i32p]
    L.slk_shard_of.argtypes = [C.c_int64, C.c_uint32]
    L.slk_shard_of.restype = C.c_uint32
    L.slk_classify_hits_device.argtypes = [vp, vp, u64p, u64p, C.c_uint64, i32p, i32p, i32p, u64p, C.c_int32,
                                           C.POINTER(C.c_double), C.c_int32, i32p, u8p, i32p, i32p, i32p]
    L.slk_shard_batch_rows.argtypes = [C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32]
    L.slk_shard_batch_rows.restype = C.c_uint64
    L.slk_shard_chunk.argtypes = [C.c_uint32]
    L.slk_shard_chunk.restype = C.c_uint32
    L.slk_shard_step_device.argtypes = [vp, vp, C.POINTER(ShardLists), C.POINTER(ShardLookup), C.POINTER(ShardLists), C.POINTER(ShardResults)]
    L.slk_stream_last_deferred.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.slk_stream_last_route.argtypes = [vp, C.POINTER(C.c_uint32)]
    L.slk_stream_set_split_long.argtypes = [vp, C.c_int64]
    L.slk_stream_set_split_hits.argtypes = [vp, C.c_int32]
    L.slk_stream_last_split.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.slk_stream_split_info.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.slk_bracken_create.argtypes = [vp, C.c_int32, C.c_uint64, C.POINTER(vp)]
    L.slk_bracken_add.argtypes = [vp, vp, u8p, u64p, i32p, C.c_uint64]
    L.slk_bracken_result.argtypes = [vp, C.POINTER(C.c_uint64), i32p, i32p, u64p, C.c_uint64]
    L.slk_bracken_destroy.argtypes = [vp]
    L.slk_bracken_destroy.restype = None
    L.slk_migration_create.argtypes = [vp, i32p, C.c_int32, C.POINTER(vp)]
    L.slk_migration_add.argtypes = [vp, vp, i64p, i32p, C.c_uint64]
    L.slk_migration_add_device.argtypes = [vp, vp, i64p, i32p, C.c_uint64]
    L.slk_migration_result.argtypes = [vp, C.POINTER(C.c_uint64), i32p, i32p, i32p, u64p, C.c_uint64, C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_uint64)]
    L.slk_migration_destroy.argtypes = [vp]
    L.slk_migration_destroy.restype = None
    L.slk_coverage_create.argtypes = [vp, i32p, C.c_int32, C.c_uint64, C.POINTER(vp)]
    L.slk_coverage_add.argtypes = [vp, vp, u8p, u64p, i32p, C.c_uint64]
    L.slk_coverage_fold.argtypes = [vp, vp]
    L.slk_coverage_result.argtypes = [vp, C.POINTER(C.c_uint64), i32p, i32p, u64p, u64p, C.c_uint64]
    L.slk_coverage_totals.argtypes = [vp, C.POINTER(C.c_uint64), i32p, u64p, u64p, C.c_uint64]
    L.slk_coverage_budget.argtypes = [vp]
    L.slk_coverage_budget.restype = C.c_uint64
    L.slk_coverage_destroy.argtypes = [vp]
    L.slk_coverage_destroy.restype = None
    L.slk_support_create.argtypes = [vp, i32p, C.c_int32, C.c_int32, C.c_int32, C.POINTER(vp)]
    L.slk_support_add.argtypes = [vp, vp, u8p, u64p, C.c_uint64]
    L.slk_support_result.argtypes = [vp, C.POINTER(C.c_uint64), i32p, u64p, u64p, u64p, C.c_uint64]
    L.slk_support_totals.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 4
    L.slk_support_destroy.argtypes = [vp]
    L.slk_support_destroy.restype = None
    L.slk_parse_tile_bytes.argtypes = []
    L.slk_parse_tile_bytes.restype = C.c_uint32
    L.slk_parse_device.argtypes = [vp, u8p, C.c_uint64, C.c_int32, C.c_int32, u8p, C.c_uint64, u64p, u64p, vp, C.c_uint64, u64p]
    L.slk_parse_text.argtypes = [vp, u8p, C.c_uint64, C.c_int32, C.c_int32, u8p, u64p, u64p, vp, C.c_uint64, C.c_uint64,
                                 C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    L.slk_classify_text.argtypes = [vp, vp, u8p, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_double), C.c_int32, i32p, u8p,
                                    i32p, i32p, u64p, u64p, vp, u64p, vp, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_uint64)]
    L.slk_pair_device.argtypes = [vp, u8p, C.c_uint64, u64p, vp, u64p, u64p, C.c_uint64, u8p, C.c_uint64, u64p, vp, u64p, u64p, C.c_uint64, u64p]
    L.slk_parse_text_paired.argtypes = [vp, u8p, C.c_uint64, C.c_int32, C.c_int32, u8p, C.c_uint64, C.c_int32, C.c_int32, u8p, u64p, u8p, u64p,
                                        u64p, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, u64p]
    L.slk_classify_text_paired.argtypes = [vp, vp, u8p, C.c_uint64, C.c_int32, C.c_int32, u8p, C.c_uint64, C.c_int32, C.c_int32, C.c_int32,
                                           C.POINTER(C.c_double), C.c_int32, i32p, u8p, i32p, i32p, u64p, u64p, u64p, vp, u64p, vp,
                                           C.c_uint64, C.c_uint64, u64p]
    L.slk_pipe_create.argtypes = [vp, C.c_int32, C.POINTER(vp)]
    L.slk_pipe_set_merged_hits.argtypes = [vp, C.c_int32]
    L.slk_pipe_submit.argtypes = [vp, C.c_uint64, C.POINTER(_Reads), C.POINTER(_Reads), C.c_int32, C.POINTER(C.c_double), C.c_int32, C.c_int32,
                                  C.POINTER(C.c_uint64)]
    L.slk_pipe_collect.argtypes = [vp, C.c_uint64, i32p, u8p, i32p, i32p, u64p, vp, C.c_uint64]
    L.slk_pipe_pending.argtypes = [vp, C.POINTER(C.c_int32)]
    L.slk_pipe_destroy.argtypes = [vp]
    L.slk_pipe_destroy.restype = None
    L.slk_pack_bases_sparse.argtypes = [u8p, C.c_uint64, vp, vp, vp, C.c_uint64, C.POINTER(C.c_uint64)]
    L.slk_mask_tile_bases.argtypes = []
    L.slk_mask_tile_bases.restype = C.c_uint32
    L.slk_mask_device.argtypes = [vp, u8p, u64p, C.c_uint64, C.POINTER(MaskConfig), u64p]
    L.slk_mask_sequences.argtypes = [vp, u8p, u64p, C.c_uint64, C.POINTER(MaskConfig), C.POINTER(C.c_uint64)]
    L.slk_index_add_sequences_masked.argtypes = [vp, vp, u8p, u64p, i32p, C.c_uint64, C.POINTER(MaskConfig), C.POINTER(C.c_uint64)]
    L.slk_compare_create.argtypes = [vp, C.POINTER(vp)]
    L.slk_compare_add_reference.argtypes = [vp, vp, u8p, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint64)]
    L.slk_compare_add_reference_device.argtypes = [vp, vp, u8p, C.c_uint64, C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_uint64)]
    L.slk_compare_begin_test.argtypes = [vp]
    L.slk_compare_add_test.argtypes = [vp, vp, u8p, C.c_uint64, C.c_int32, C.POINTER(C.c_uint64)]
    L.slk_compare_add_test_device.argtypes = [vp, vp, u8p, C.c_uint64, C.c_int32, C.POINTER(C.c_uint64)]
    L.slk_compare_pairs.argtypes = [vp, C.POINTER(C.c_uint64), i32p, i32p, u64p, C.c_uint64]
    L.slk_compare_reference_taxa.argtypes = [vp, C.POINTER(C.c_uint64), i32p, u64p, C.c_uint64]
    L.slk_compare_totals.argtypes = [vp] + [C.POINTER(C.c_uint64)] * 5
    L.slk_compare_error.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]
    L.slk_compare_destroy.argtypes = [vp]
    L.slk_compare_destroy.restype = None
    for name in EXPORTS:
        fn = getattr(L, name)
        if fn.restype is C.c_int:  # default: int32 status
            fn.restype = C.c_int32
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise SlackenError(rc, lib().slk_last_error().decode())


def _np(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _ptr(a):
    return a.ctypes.data if a is not None else None


def pack_bases(bases, pinned=False):
    """ASCII bases -> (codes uint32 [ceil(n / 16)], valid uint16 [ceil(n / 16)]): the engine's 3-bit form (slk_pack_bases)"""
    bases = _np(bases, np.uint8)
    words = (bases.size + 15) // 16
    make = (lambda n, dt: pinned_array((n,), dt)) if pinned else (lambda n, dt: np.zeros(n, dt))
    codes, valid = make(max(words, 1), np.uint32), make(max(words, 1), np.uint16)
    _check(lib().slk_pack_bases(_ptr(bases), bases.size, _ptr(codes), _ptr(valid)))
    return codes, valid


def pack_bases_sparse(bases, pinned=False):
    """ASCII bases -> (codes uint32 [ceil(n / 16)], exc_word uint32 [n_exc], exc_bits uint16 [n_exc]): the codes of pack_bases and
    the validity as the list of the words that hold an invalid base (slk_pack_bases_sparse; Pipe.submit takes it)"""
    bases = _np(bases, np.uint8)
    words = (bases.size + 15) // 16
    make = (lambda n, dt: pinned_array((n,), dt)) if pinned else (lambda n, dt: np.zeros(n, dt))
    codes = make(max(words, 1), np.uint32)
    cap, n = max(16, words // 64), C.c_uint64(0)
    while True:
        exc_word, exc_bits = make(cap, np.uint32), make(cap, np.uint16)
        rc = lib().slk_pack_bases_sparse(_ptr(bases), bases.size, _ptr(codes), _ptr(exc_word), _ptr(exc_bits), cap, C.byref(n))
        if rc != -5:   # SLK_E_CAPACITY: n says what the list needs
            _check(rc)
            return codes, exc_word[:n.value], exc_bits[:n.value]
        cap = int(n.value)


def pinned_array(shape, dtype):
    """A numpy array in pinned host memory (slk_host_alloc): the host entry points DMA from and to it directly.
    Keep the array (or a view of it) alive while it is in use; the memory is freed with the array's base object."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    p = C.c_void_p()
    _check(lib().slk_host_alloc(max(n, 1), C.byref(p)))

    class _Owner:
        def __init__(self, addr):
            self.addr = addr

        def __del__(self):
            try:
                lib().slk_host_free(self.addr)
            except Exception:
                pass

    buf = (C.c_uint8 * max(n, 1)).from_address(p.value)
    buf._owner = _Owner(p.value)   # freed when the last view goes
    return np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)


@dataclass
class ClassifyParams:
    """Mirror of ClassifyParams (S/slacken/Classifier.scala:60-61)."""
    minHitGroups: int = 2
    withUnclassified: bool = True
    thresholds: List[float] = field(default_factory=lambda: [0.0])
    sampleRegex: Optional[str] = None
    perReadOutput: bool = True


class Index:
    """HBM-resident minimizer->taxon records + taxonomy (the engine-side KeyValueIndex)."""

    def __init__(self, k=35, m=31, spaces=7, xor_mask=DEFAULT_TOGGLE_MASK, canonical=True, expected_records=1 << 20,
                 max_taxon=0, load_factor=0.0, device=0):
        self.k, self.m, self.spaces = k, m, spaces
        self.W = (m + 31) // 32   # id columns: keys are rows of W int64 words
        p = _Params(k, m, spaces, int(bool(canonical)), C.c_uint64(xor_mask & (2**64 - 1)), (m + 31) // 32, 0)
        cfg = _TableConfig(int(expected_records), int(max_taxon), float(load_factor))
        h = C.c_void_p()
        _check(lib().slk_index_create(C.byref(p), C.byref(cfg), device, C.byref(h)))
        self.h = h

    def append(self, keys, taxa):
        keys, taxa = _np(keys, np.int64), _np(taxa, np.int32)
        assert keys.size == taxa.size * self.W
        _check(lib().slk_index_append(self.h, _ptr(keys), _ptr(taxa), taxa.size))

    def append_device(self, d_keys_ptr, d_taxa_ptr, n):
        _check(lib().slk_index_append_device(self.h, d_keys_ptr, d_taxa_ptr, n))

    def set_shard(self, shard, n_shards):
        """Table-sharded library: keep only the records whose key falls to `shard` of `n_shards` (before the first record)."""
        _check(lib().slk_index_set_shard(self.h, shard, n_shards))

    def set_taxonomy(self, parents):
        parents = _np(parents, np.int32)
        _check(lib().slk_index_set_taxonomy(self.h, _ptr(parents), parents.size))

    def add_sequences(self, bases, offsets, taxa):
        """Library construction (KeyValueIndex.makeRecords): minimizers of taxon-labelled sequences, LCA-merged."""
        bases, offsets, taxa = _np(bases, np.uint8), _np(offsets, np.uint64), _np(taxa, np.int32)
        assert offsets.size == taxa.size + 1
        _check(lib().slk_index_add_sequences(self.h, _ptr(bases), _ptr(offsets), _ptr(taxa), taxa.size))

    def add_sequences_device(self, d_bases_ptr, offsets, taxa):
        """add_sequences with the bases resident on the index's GPU (raw device address, 16 readable bytes past the end)."""
        offsets, taxa = _np(offsets, np.uint64), _np(taxa, np.int32)
        assert offsets.size == taxa.size + 1
        _check(lib().slk_index_add_sequences_device(self.h, d_bases_ptr, _ptr(offsets), _ptr(taxa), taxa.size))

    def export(self):
        """(keys, taxa) of every record in the table, sorted by key."""
        n = C.c_uint64(0)
        _check(lib().slk_index_export(self.h, None, None, 0, C.byref(n)))
        keys, taxa = np.zeros(n.value * self.W, np.int64), np.zeros(n.value, np.int32)
        if n.value:
            _check(lib().slk_index_export(self.h, _ptr(keys), _ptr(taxa), n.value, C.byref(n)))
        if self.W > 1:   # rows of W words, sorted as unsigned numbers, word by word
            rows = keys.reshape(-1, self.W)
            order = np.lexsort(rows.view(np.uint64).T[::-1])
            return rows[order], taxa[order]
        order = np.argsort(keys, kind="stable")
        return keys[order], taxa[order]

    def export_range(self, bucket0, bucket1, n_groups=0):
        """The records of table buckets [bucket0, bucket1) (slk_index_export_range; info().buckets bounds the range), as they
        leave the device: (keys, taxa) in any order, or with n_groups >= 1 (keys, taxa, group_offsets) ordered by Spark's bucket
        pmod(Murmur3 hashLong(key, 42), n_groups), group g at [group_offsets[g], group_offsets[g + 1])."""
        cap = max(0, int(bucket1) - int(bucket0)) * self.info().bucket_cells   # an upper bound: never SLK_E_CAPACITY
        keys, taxa = np.zeros(max(cap, 1), np.int64), np.zeros(max(cap, 1), np.int32)
        offs = np.zeros(int(n_groups) + 1, np.uint64) if n_groups > 0 else None
        n = C.c_uint64(0)
        _check(lib().slk_index_export_range(self.h, int(bucket0), int(bucket1), int(n_groups), _ptr(keys), _ptr(taxa), max(cap, 1),
                                            _ptr(offs), C.byref(n)))
        keys, taxa = keys[:n.value].copy(), taxa[:n.value].copy()
        return (keys, taxa, offs) if n_groups > 0 else (keys, taxa)

    def export_pieces(self, piece_buckets, n_groups=0):
        """export_range over the whole table, piece_buckets buckets at a time: a generator of its results."""
        nb, step = int(self.info().buckets), max(1, int(piece_buckets))
        for b0 in range(0, nb, step):
            yield self.export_range(b0, min(nb, b0 + step), n_groups)

    def taxon_counts(self):
        """(taxa int32, counts uint64) of the resident table: records per taxon, ascending taxon, the caller's ids
        (slk_index_taxon_counts: counted on the device, only the pairs come to the host)."""
        n, total = C.c_uint64(0), C.c_uint64(0)
        _check(lib().slk_index_taxon_counts(self.h, None, None, 0, C.byref(n), C.byref(total)))
        taxa, counts = np.zeros(n.value, np.int32), np.zeros(n.value, np.uint64)
        if n.value:
            _check(lib().slk_index_taxon_counts(self.h, _ptr(taxa), _ptr(counts), n.value, C.byref(n), C.byref(total)))
        return taxa, counts

    def respace(self, spaces, expected_records=None):
        """A new finalized Index with `spaces` (> this one's) mask spaces, derived on the device from this one's table
        (slk_index_respace: KeyValueIndex.respace); expected_records: sizing of its table, default this index's record count."""
        cfg = C.byref(_TableConfig(int(expected_records), 0, 0.0)) if expected_records is not None else None
        h = C.c_void_p()
        _check(lib().slk_index_respace(self.h, int(spaces), cfg, C.byref(h)))
        new = Index.__new__(Index)
        new.k, new.m, new.spaces, new.W, new.h = self.k, self.m, int(spaces), self.W, h
        return new

    def set_merge_remap(self, remap):
        """Later merge calls translate every source taxon t as remap[t] (t >= len(remap) or remap[t] == 0: the destination has no
        such node); None clears it (slk_index_set_merge_remap)."""
        remap = _np(remap, np.int32) if remap is not None else None
        _check(lib().slk_index_set_merge_remap(self.h, _ptr(remap), remap.size if remap is not None else 0))

    def merge_records(self, keys, taxa):
        """Records merged into what the table holds, per key by LCA (slk_index_merge_records): any order, any chunking, keys may
        repeat and may be in the table already.  Needs the taxonomy and an unfinalized index."""
        keys, taxa = _np(keys, np.int64), _np(taxa, np.int32)
        assert keys.size == taxa.size
        _check(lib().slk_index_merge_records(self.h, _ptr(keys), _ptr(taxa), taxa.size))

    def merge_records_device(self, d_keys_ptr, d_taxa_ptr, n):
        """merge_records with both arrays resident on the index's GPU (raw device addresses)."""
        _check(lib().slk_index_merge_records_device(self.h, d_keys_ptr, d_taxa_ptr, n))

    def merge_index(self, src):
        """The records of another resident Index on the same device merged into this one (slk_index_merge_index): its table is
        walked on the device; the source is only read."""
        _check(lib().slk_index_merge_index(self.h, src.h))

    def finalize(self):
        _check(lib().slk_index_finalize(self.h))

    def info(self):
        out = IndexInfo()
        _check(lib().slk_index_get_info(self.h, C.byref(out)))
        return out

    def lookup(self, keys):
        keys = _np(keys, np.int64)
        out = np.zeros(keys.size // self.W, np.int32)
        _check(lib().slk_index_lookup(self.h, _ptr(keys), out.size, _ptr(out)))
        return out

    def stream(self):
        return Stream(self)

    def close(self):
        if getattr(self, "h", None):
            lib().slk_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BrackenWeights:
    """Bracken weights against an index (slk_bracken_*: BrackenWeights.buildWeights, S/slacken/BrackenWeights.scala:294-352).
    add() takes whole records (no whitespace) with the taxon each came from; result() gives (dest, source, count) as numpy
    arrays, dest ascending then source ascending."""

    def __init__(self, index, read_len, max_fragment=0, stream=None):
        self.index = index
        self.stream = stream if stream is not None else index.stream()
        h = C.c_void_p()
        _check(lib().slk_bracken_create(index.h, int(read_len), int(max_fragment), C.byref(h)))
        self.h = h

    def add(self, bases, offsets, source_taxa):
        bases, offsets, taxa = _np(bases, np.uint8), _np(offsets, np.uint64), _np(source_taxa, np.int32)
        assert offsets.size == taxa.size + 1
        _check(lib().slk_bracken_add(self.h, self.stream.h, _ptr(bases), _ptr(offsets), _ptr(taxa), taxa.size))

    def result(self):
        n = C.c_uint64(0)
        _check(lib().slk_bracken_result(self.h, C.byref(n), None, None, None, 0))
        dest, source, count = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32), np.zeros(n.value, np.uint64)
        if n.value:
            _check(lib().slk_bracken_result(self.h, C.byref(n), _ptr(dest), _ptr(source), _ptr(count), n.value))
        return dest, source, count

    def close(self):
        if getattr(self, "h", None):
            lib().slk_bracken_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MinimizerMigration:
    """Minimizer migration of a subject library against a reference index (slk_migration_*: MinimizerMigration.taxaDistances,
    S/slacken/analysis/MinimizerMigration.scala:38-66).  depths[t] = Taxonomy.depth(t) of the reference's taxonomy (None: steps
    are 0).  add() takes the subject's records; result() gives (t1, t2, steps, count, matched, unmatched): numpy arrays sorted by
    t1 then t2, and two ints."""

    def __init__(self, reference_index, depths=None, stream=None):
        self.index = reference_index
        self.stream = stream if stream is not None else reference_index.stream()
        h = C.c_void_p()
        d = _np(depths, np.int32) if depths is not None else None
        _check(lib().slk_migration_create(reference_index.h, _ptr(d), d.size if d is not None else 0, C.byref(h)))
        self.h = h

    def add(self, keys, taxa):
        keys, taxa = _np(keys, np.int64), _np(taxa, np.int32)
        assert keys.size == taxa.size
        _check(lib().slk_migration_add(self.h, self.stream.h, _ptr(keys), _ptr(taxa), taxa.size))

    def add_device(self, d_keys_ptr, d_taxa_ptr, n):
        _check(lib().slk_migration_add_device(self.h, self.stream.h, d_keys_ptr, d_taxa_ptr, n))

    def result(self):
        n, matched, unmatched = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().slk_migration_result(self.h, C.byref(n), None, None, None, None, 0, C.byref(matched), C.byref(unmatched)))
        t1, t2, steps = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
        count = np.zeros(n.value, np.uint64)
        if n.value:
            _check(lib().slk_migration_result(self.h, C.byref(n), _ptr(t1), _ptr(t2), _ptr(steps), _ptr(count), n.value,
                                              C.byref(matched), C.byref(unmatched)))
        return t1, t2, steps, count, matched.value, unmatched.value

    def close(self):
        if getattr(self, "h", None):
            lib().slk_migration_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Coverage:
    """Genome coverage of labelled sequences against an index (slk_coverage_*: IndexStatistics.showTaxonFullCoverageStats,
    S/slacken/IndexStatistics.scala:86-111, and the k-mers per source of totalKmerCountReport, :38-52).  depths[t] =
    Taxonomy.depth(t) of the index's taxonomy.  add() takes whole sequences (no whitespace) with the taxon each came from; fold()
    closes a group of sources; result() gives (source, depth, all, distinct) sorted by source then depth, totals() gives
    (source, kmers, supermers) sorted by source: numpy arrays."""

    def __init__(self, index, depths=None, max_pairs=0, stream=None):
        self.index = index
        self.stream = stream if stream is not None else index.stream()
        h = C.c_void_p()
        d = _np(depths, np.int32) if depths is not None else None
        _check(lib().slk_coverage_create(index.h, _ptr(d), d.size if d is not None else 0, int(max_pairs), C.byref(h)))
        self.h = h

    def budget(self):
        return int(lib().slk_coverage_budget(self.h))

    def add(self, bases, offsets, source_taxa):
        bases, offsets, taxa = _np(bases, np.uint8), _np(offsets, np.uint64), _np(source_taxa, np.int32)
        assert offsets.size == taxa.size + 1
        _check(lib().slk_coverage_add(self.h, self.stream.h, _ptr(bases), _ptr(offsets), _ptr(taxa), taxa.size))

    def fold(self):
        _check(lib().slk_coverage_fold(self.h, self.stream.h))

    def result(self):
        n = C.c_uint64(0)
        _check(lib().slk_coverage_result(self.h, C.byref(n), None, None, None, None, 0))
        source, depth = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
        count, distinct = np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint64)
        if n.value:
            _check(lib().slk_coverage_result(self.h, C.byref(n), _ptr(source), _ptr(depth), _ptr(count), _ptr(distinct), n.value))
        return source, depth, count, distinct

    def totals(self):
        n = C.c_uint64(0)
        _check(lib().slk_coverage_totals(self.h, C.byref(n), None, None, None, 0))
        source, kmers, supermers = np.zeros(n.value, np.int32), np.zeros(n.value, np.uint64), np.zeros(n.value, np.uint64)
        if n.value:
            _check(lib().slk_coverage_totals(self.h, C.byref(n), _ptr(source), _ptr(kmers), _ptr(supermers), n.value))
        return source, kmers, supermers

    def close(self):
        if getattr(self, "h", None):
            lib().slk_coverage_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Support:
    """A sample's minimizers counted per taxon against an index (slk_support_*: Dynamic.minimizersInSubjects and multiStatsPerTaxon,
    S/slacken/Dynamic.scala:95-117, 152-180).  depths[t] = Taxonomy.depth(t) of the index's taxonomy; hits of taxa below min_depth are
    dropped.  add() takes sequences (no whitespace; the mates of paired reads are sequences of their own); result() gives
    (taxon, kmers, minimizers, distinct) sorted by taxon as numpy arrays, totals() gives (sequences, supermers, matched, kept)."""

    def __init__(self, index, depths=None, min_depth=0, want_distinct=True, stream=None):
        self.index = index
        self.stream = stream if stream is not None else index.stream()
        h = C.c_void_p()
        d = _np(depths, np.int32) if depths is not None else None
        _check(lib().slk_support_create(index.h, _ptr(d), d.size if d is not None else 0, int(min_depth), 1 if want_distinct else 0, C.byref(h)))
        self.h = h

    def add(self, bases, offsets):
        bases, offsets = _np(bases, np.uint8), _np(offsets, np.uint64)
        assert offsets.size >= 1
        _check(lib().slk_support_add(self.h, self.stream.h, _ptr(bases), _ptr(offsets), offsets.size - 1))

    def result(self):
        n = C.c_uint64(0)
        _check(lib().slk_support_result(self.h, C.byref(n), None, None, None, None, 0))
        taxa = np.zeros(n.value, np.int32)
        kmers, minimizers, distinct = (np.zeros(n.value, np.uint64) for _ in range(3))
        if n.value:
            _check(lib().slk_support_result(self.h, C.byref(n), _ptr(taxa), _ptr(kmers), _ptr(minimizers), _ptr(distinct), n.value))
        return taxa, kmers, minimizers, distinct

    def totals(self):
        v = [C.c_uint64(0) for _ in range(4)]
        _check(lib().slk_support_totals(self.h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def close(self):
        if getattr(self, "h", None):
            lib().slk_support_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Compare:
    """Classifications joined with a truth mapping on the read id (slk_compare_*: the join of MappingComparison,
    S/slacken/analysis/MappingComparison.scala:157-159, 216-217).  The reference mapping's rows stay on the device; each test text
    is a begin_test(), its add_test() calls, then pairs().  Taxa are RAW, as the texts have them: primary(), isDefined and the rank
    arithmetic are the caller's, over the distinct pairs.

    No Index or Stream is needed: Compare(device=0) makes the small empty index and the stream that own the handle.

        c = Compare()
        c.add_reference(open("reads_mapping.tsv", "rb").read())          # columns 2 and 3, or id_col= / taxon_col=
        c.begin_test()
        c.add_test(open("part-00000.txt", "rb").read())                  # the per-read lines `classify` writes
        ref_taxon, test_taxon, rows = c.pairs()

    add_reference / add_test take a whole text, or, with final=False, a chunk: they return the bytes consumed, where the next chunk
    starts (0: the chunk holds no whole line and must grow).  A bad line or a duplicated id raises SlackenError (code -1); error()
    then gives (byte offset of the line in its whole text, kind)."""

    def __init__(self, stream=None, device=0):
        self._index = None
        if stream is None:
            self._index = Index(expected_records=1024, device=device)
            stream = self._index.stream()
        self.stream = stream
        h = C.c_void_p()
        _check(lib().slk_compare_create(stream.h, C.byref(h)))
        self.h = h

    def _add(self, fn, text, args, final):
        text = np.frombuffer(bytes(text), np.uint8) if not isinstance(text, np.ndarray) else _np(text, np.uint8)
        consumed = C.c_uint64(0)
        _check(fn(self.h, self.stream.h, _ptr(text) if text.size else None, text.size, *args, 1 if final else 0, C.byref(consumed)))
        return int(consumed.value)

    def add_reference(self, text, id_col=2, taxon_col=3, final=True):
        return self._add(lib().slk_compare_add_reference, text, (int(id_col), int(taxon_col)), final)

    def begin_test(self):
        _check(lib().slk_compare_begin_test(self.h))

    def add_test(self, text, final=True):
        return self._add(lib().slk_compare_add_test, text, (), final)

    def add_reference_device(self, d_text_ptr, n, id_col=2, taxon_col=3, final=True):
        """add_reference with the text resident on the handle's GPU (raw device address, aligned to 16 bytes)"""
        consumed = C.c_uint64(0)
        _check(lib().slk_compare_add_reference_device(self.h, self.stream.h, d_text_ptr, n, int(id_col), int(taxon_col), 1 if final else 0,
                                                      C.byref(consumed)))
        return int(consumed.value)

    def add_test_device(self, d_text_ptr, n, final=True):
        consumed = C.c_uint64(0)
        _check(lib().slk_compare_add_test_device(self.h, self.stream.h, d_text_ptr, n, 1 if final else 0, C.byref(consumed)))
        return int(consumed.value)

    def pairs(self):
        """(reference taxon, test taxon, joined rows) of the current test, ascending, as numpy arrays"""
        n = C.c_uint64(0)
        _check(lib().slk_compare_pairs(self.h, C.byref(n), None, None, None, 0))
        ref, test, count = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32), np.zeros(n.value, np.uint64)
        if n.value:
            _check(lib().slk_compare_pairs(self.h, C.byref(n), _ptr(ref), _ptr(test), _ptr(count), n.value))
        return ref, test, count

    def reference_taxa(self):
        """(raw taxon, kept reference rows), ascending"""
        n = C.c_uint64(0)
        _check(lib().slk_compare_reference_taxa(self.h, C.byref(n), None, None, 0))
        taxa, count = np.zeros(n.value, np.int32), np.zeros(n.value, np.uint64)
        if n.value:
            _check(lib().slk_compare_reference_taxa(self.h, C.byref(n), _ptr(taxa), _ptr(count), n.value))
        return taxa, count

    def totals(self):
        """(reference rows, dropped as "/2", kept ids, test rows, joined rows)"""
        v = [C.c_uint64(0) for _ in range(5)]
        _check(lib().slk_compare_totals(self.h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def error(self):
        """(byte offset, kind) of the bad line or duplicate that ended an add; kind 0: none"""
        off, kind = C.c_uint64(0), C.c_int32(0)
        _check(lib().slk_compare_error(self.h, C.byref(off), C.byref(kind)))
        return int(off.value), int(kind.value)

    def close(self):
        if getattr(self, "h", None):
            lib().slk_compare_destroy(self.h)
            self.h = None
            if self._index is not None:   # (the index and the stream made for this handle alone)
                self.stream.close()
                self._index.close()
                self._index = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class ShardSet:
    """Table-sharded classification in one process (slk_shardset_*): members[g] is an Index with set_shard(g, n), finalized."""

    def __init__(self, members, exchange=EXCHANGE_AUTO):
        self.members = list(members)
        arr = (C.c_void_p * len(self.members))(*[m.h for m in self.members])
        h = C.c_void_p()
        _check(lib().slk_shardset_create(arr, len(self.members), exchange, C.byref(h)))
        self.h = h

    @property
    def exchange_mode(self):
        return int(lib().slk_shardset_exchange_mode(self.h))

    @property
    def staged_pairs(self):
        """ordered pairs of members whose copies go through pinned host memory (slk_shardset_staged_pairs)"""
        return int(lib().slk_shardset_staged_pairs(self.h))

    def classify(self, batches, min_hit_groups=2, thresholds=(0.0,), with_hits=True):
        """One round: batches[g] = (bases, offsets) or (bases, offsets, mate_bases, mate_offsets) or None for member g.
        -> list of result dicts as Stream.classify_batch returns them (None for members without a batch)."""
        n = len(self.members)
        assert len(batches) == n
        Cn = len(thresholds)
        thr = (C.c_double * Cn)(*thresholds)
        arr = (_ShardBatch * n)()
        keep, outs = [], []
        for g, b in enumerate(batches):
            if b is None:
                outs.append(None)
                continue
            bases, offsets = _np(b[0], np.uint8), _np(b[1], np.uint64)
            mb = mo = None
            if len(b) > 2 and b[2] is not None:
                mb, mo = _np(b[2], np.uint8), _np(b[3], np.uint64)
            R = offsets.size - 1
            o = dict(taxon=np.zeros((Cn, R), np.int32), classified=np.zeros((Cn, R), np.uint8), num_distinct=np.zeros(R, np.int32),
                     total_kmers=np.zeros(R, np.int32))
            hit_off = hits = None
            cap = 0
            if with_hits:
                cap = int(bases.size + (mb.size + R if mb is not None else 0)) + 1
                hit_off, hits = np.zeros(R + 1, np.uint64), np.zeros(cap, HIT_DTYPE)
            keep.append((bases, offsets, mb, mo, hit_off, hits))
            arr[g] = _ShardBatch(_ptr(bases), _ptr(offsets), _ptr(mb), _ptr(mo), R, _ptr(o["taxon"]), _ptr(o["classified"]),
                                 _ptr(o["num_distinct"]), _ptr(o["total_kmers"]), _ptr(hit_off), _ptr(hits), cap)
            o["_hit"] = (hit_off, hits)
            outs.append(o)
        _check(lib().slk_shardset_classify(self.h, arr, min_hit_groups, thr, Cn))
        for o in outs:
            if o is None:
                continue
            hit_off, hits = o.pop("_hit")
            if hit_off is not None:
                o["hit_offsets"] = hit_off
                o["hits"] = hits[:int(hit_off[-1])]
                o["num_hits"] = np.diff(hit_off.astype(np.int64)).astype(np.int32)
        return outs

    def classify_rounds_device(self, rounds, min_hit_groups=2, thresholds=(0.0,)):
        """Pipelined rounds over DEVICE-resident batches (slk_shardset_classify_rounds, device_resident = 1): rounds[r][g] is a dict of
        raw device addresses on member g's GPU -- bases, offsets, R, out_taxon, out_classified and optionally mate_bases,
        mate_offsets, out_num_distinct, out_total_kmers -- or None.  Synchronous: returns when every round is done."""
        n = len(self.members)
        Cn = len(thresholds)
        thr = (C.c_double * Cn)(*thresholds)
        arr = (_ShardBatch * (n * len(rounds)))()
        for r, rnd in enumerate(rounds):
            assert len(rnd) == n
            for g, b in enumerate(rnd):
                if b is None:
                    continue
                arr[r * n + g] = _ShardBatch(b["bases"], b["offsets"], b.get("mate_bases"), b.get("mate_offsets"), b["R"], b["out_taxon"],
                                             b["out_classified"], b.get("out_num_distinct"), b.get("out_total_kmers"),
                                             b.get("out_hit_offsets"), b.get("out_hits"), 0)   # (hit lists: refused, SLK_E_UNSUPPORTED)
        _check(lib().slk_shardset_classify_rounds(self.h, arr, len(rounds), 1, min_hit_groups, thr, Cn))

    def classify_rounds(self, rounds, min_hit_groups=2, thresholds=(0.0,), with_hits=True, hits_capacity=None):
        """Several rounds of classify() in ONE pipelined call (slk_shardset_classify_rounds, host pointers): rounds[r][g] as
        classify()'s batches[g].  with_hits: one bool for the call, or a [rounds][members] matrix of bools (a batch asks for its
        hit lists or not).  hits_capacity: None, or a [rounds][members] matrix of entry counts (None: what the batch can need at
        most).  -> list (per round) of lists (per member) of result dicts."""
        n = len(self.members)
        Cn = len(thresholds)
        thr = (C.c_double * Cn)(*thresholds)
        arr = (_ShardBatch * (n * len(rounds)))()
        keep, outs = [], []
        want = with_hits if isinstance(with_hits, (list, tuple)) else [[bool(with_hits)] * n for _ in rounds]
        assert len(want) == len(rounds) and all(len(w) == n for w in want)
        for r, rnd in enumerate(rounds):
            assert len(rnd) == n
            row = []
            for g, b in enumerate(rnd):
                with_hits = bool(want[r][g])
                if b is None:
                    row.append(None)
                    continue
                bases, offsets = _np(b[0], np.uint8), _np(b[1], np.uint64)
                mb = mo = None
                if len(b) > 2 and b[2] is not None:
                    mb, mo = _np(b[2], np.uint8), _np(b[3], np.uint64)
                R = offsets.size - 1
                o = dict(taxon=np.zeros((Cn, R), np.int32), classified=np.zeros((Cn, R), np.uint8), num_distinct=np.zeros(R, np.int32),
                         total_kmers=np.zeros(R, np.int32))
                hit_off = hits = None
                cap = 0
                if with_hits:
                    cap = int(bases.size + (mb.size + R if mb is not None else 0)) + 1
                    if hits_capacity is not None and hits_capacity[r][g] is not None:
                        cap = int(hits_capacity[r][g])
                    hit_off, hits = np.zeros(R + 1, np.uint64), np.zeros(max(cap, 1), HIT_DTYPE)
                keep.append((bases, offsets, mb, mo, hit_off, hits))
                arr[r * n + g] = _ShardBatch(_ptr(bases), _ptr(offsets), _ptr(mb), _ptr(mo), R, _ptr(o["taxon"]), _ptr(o["classified"]),
                                             _ptr(o["num_distinct"]), _ptr(o["total_kmers"]), _ptr(hit_off), _ptr(hits), cap)
                o["_hit"] = (hit_off, hits)
                row.append(o)
            outs.append(row)
        _check(lib().slk_shardset_classify_rounds(self.h, arr, len(rounds), 0, min_hit_groups, thr, Cn))
        for row in outs:
            for o in row:
                if o is None:
                    continue
                hit_off, hits = o.pop("_hit")
                if hit_off is not None:
                    o["hit_offsets"] = hit_off
                    o["hits"] = hits[:int(hit_off[-1])]
                    o["num_hits"] = np.diff(hit_off.astype(np.int64)).astype(np.int32)
        return outs

    def close(self):
        if getattr(self, "h", None):
            lib().slk_shardset_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Pipe:
    """slk_pipe: `depth` batches in flight from one thread.  submit() queues a batch and returns its ticket at once; collect()
    waits for that ticket alone and returns what Stream.classify_batch returns.  A side of a batch is a dict with
      bases (ASCII)  or  codes with valid (pack_bases)  or  codes with exc_word, exc_bits (pack_bases_sparse; both may be absent)
      and one of offsets [R + 1], lengths [R], uniform_len
    Every array a ticket was submitted with is kept alive here until the ticket is collected (pinned arrays are read by DMA
    after submit returns: do not change them before)."""

    _DTYPES = dict(bases=np.uint8, codes=np.uint32, valid=np.uint16, exc_word=np.uint32, exc_bits=np.uint16, offsets=np.uint64,
                   lengths=np.uint32)

    def __init__(self, index, depth=2):
        self.index = index
        h = C.c_void_p()
        _check(lib().slk_pipe_create(index.h, depth, C.byref(h)))
        self.h = h
        self._tickets = {}    # ticket -> (R, C, hits, default hits capacity, the input arrays)

    def set_merged_hits(self, on=True):
        _check(lib().slk_pipe_set_merged_hits(self.h, 1 if on else 0))

    def pending(self):
        n = C.c_int32(0)
        _check(lib().slk_pipe_pending(self.h, C.byref(n)))
        return int(n.value)

    @classmethod
    def _side(cls, d):
        """-> (slk_reads, the arrays it points to, the R the side implies or None, its bases)"""
        keep = {k: _np(d[k], dt) for k, dt in cls._DTYPES.items() if d.get(k) is not None}
        R = keep["offsets"].size - 1 if "offsets" in keep else keep["lengths"].size if "lengths" in keep else None
        n_exc = keep["exc_word"].size if "exc_word" in keep else 0
        for k in keep:   # (an empty array may have no address: the call tells present from absent by the pointer)
            if keep[k].size == 0:
                keep[k] = np.zeros(1, cls._DTYPES[k])
        r = _Reads()
        for k, a in keep.items():
            setattr(r, k, a.ctypes.data)
        r.n_exc = int(d["n_exc"]) if "n_exc" in d else n_exc
        r.uniform_len = int(d.get("uniform_len") or 0)
        return r, keep, R

    @staticmethod
    def _total(keep, r, R):
        if "offsets" in keep:
            return int(keep["offsets"][R])
        if "lengths" in keep:
            return int(keep["lengths"][:R].sum(dtype=np.uint64))
        return R * int(r.uniform_len)

    def submit(self, reads, mates=None, R=None, min_hit_groups=2, thresholds=(0.0,), hits=2):
        """hits: 0 = none, 1 = num_hits only, 2 = the hit lists.  R is needed where no array says it (uniform_len).  -> ticket"""
        r, keep, Rr = self._side(reads)
        m = mkeep = None
        if mates is not None:
            m, mkeep, Rm = self._side(mates)
            if Rr is not None and Rm is not None and Rr != Rm:
                raise SlackenError(-1, f"the mates describe {Rm} reads, the reads {Rr}")
            Rr = Rr if Rr is not None else Rm
        if R is not None and Rr is not None and int(R) != Rr:
            raise SlackenError(-1, f"R = {R}, the arrays describe {Rr} reads")
        R = int(R) if R is not None else Rr
        if R is None:
            raise ValueError("uniform_len needs R")
        Cn = len(thresholds)
        thr = (C.c_double * Cn)(*thresholds)
        ticket = C.c_uint64(0)
        _check(lib().slk_pipe_submit(self.h, R, C.byref(r), C.byref(m) if m is not None else None, min_hit_groups, thr, Cn, hits,
                                     C.byref(ticket)))
        cap = self._total(keep, r, R) + (self._total(mkeep, m, R) + R if m is not None else 0) + 1
        self._tickets[ticket.value] = (R, Cn, hits, cap, (keep, mkeep))
        return int(ticket.value)

    def collect(self, ticket, hits_capacity=None, out=None):
        """-> the dict of Stream.classify_batch (hits 2: with hit_offsets, hits, num_hits; hits 1: with num_hits).  out: optional
        dict of preallocated result arrays, as there.  SLK_E_CAPACITY (hits_capacity too small) leaves the ticket collectable."""
        R, Cn, hits, cap, _ = self._tickets.get(ticket, (0, 1, 0, 0, None))
        if out is not None:
            taxon, cls, nd, tk = out["taxon"], out["classified"], out["num_distinct"], out["total_kmers"]
            assert taxon.shape == (Cn, R) and taxon.dtype == np.int32 and cls.shape == (Cn, R) and cls.dtype == np.uint8
            assert all(a.flags.c_contiguous for a in (taxon, cls, nd, tk))
        else:
            taxon, cls = np.zeros((Cn, R), np.int32), np.zeros((Cn, R), np.uint8)
            nd, tk = np.zeros(R, np.int32), np.zeros(R, np.int32)
        hit_off = hit_arr = None
        if hits:
            hit_off = np.zeros(R + 1, np.uint64)
        if hits == 2:
            cap = hits_capacity if hits_capacity is not None else cap
            hit_arr = np.zeros(max(cap, 1), HIT_DTYPE)
        rc = lib().slk_pipe_collect(self.h, ticket, _ptr(taxon), _ptr(cls), _ptr(nd), _ptr(tk), _ptr(hit_off), _ptr(hit_arr),
                                    cap if hits == 2 else 0)
        if rc == -5:   # SLK_E_CAPACITY: the offsets say what the lists need
            err = SlackenError(rc, lib().slk_last_error().decode())
            err.hit_offsets = hit_off
            raise err
        self._tickets.pop(ticket, None)
        _check(rc)
        res = dict(taxon=taxon, classified=cls, num_distinct=nd, total_kmers=tk)
        if hits:
            res["num_hits"] = np.diff(hit_off.astype(np.int64)).astype(np.int32)
        if hits == 2:
            res["hit_offsets"] = hit_off
            res["hits"] = hit_arr[:int(hit_off[R])]
        return res

    def close(self):
        """slk_pipe_destroy: waits for what is pending and drops it"""
        if getattr(self, "h", None):
            lib().slk_pipe_destroy(self.h)
            self.h = None
            self._tickets.clear()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_deferred_streams = []   # engine streams whose destruction was put off because torch still held a view of them (Stream.close)


class Stream:
    def __init__(self, index):
        self.index = index
        h = C.c_void_p()
        _check(lib().slk_stream_create(index.h, C.byref(h)))
        self.h = h
        self._views = []     # weak references to the torch ExternalStream wrappers handed out

    def external_stream(self, torch, device):
        """The torch view of this stream (torch.cuda.ExternalStream).  torch's caching allocator ties every block to the stream it was
        allocated on and records events on the streams a tensor was used on when the tensor dies -- on a stream that no longer
        exists that is a crash -- so the engine stream is NOT destroyed while a view of it is alive: close() puts the destruction
        off (see below), and whoever hands views out drops them, after torch.cuda.empty_cache(), before it closes the stream
        (slacken_amd.sharded.ShardedClassifier.close)."""
        import weakref
        ext = torch.cuda.ExternalStream(self.hip_stream, device=device)
        self._views.append(weakref.ref(ext))
        return ext

    def views_alive(self):
        return any(r() is not None for r in self._views)

    @property
    def hip_stream(self):
        return lib().slk_stream_hip_stream(self.h)

    def synchronize(self):
        _check(lib().slk_stream_synchronize(self.h))

    def set_merged_hits(self, on=True):
        """hit lists of classify_batch as TaxonCounts.fromHits merges them (adjacent hits of one taxon summed); `num_hits` then counts
        the merged entries"""
        _check(lib().slk_stream_set_merged_hits(self.h, 1 if on else 0))

    def last_deferred(self):
        n = C.c_uint64(0)
        _check(lib().slk_stream_last_deferred(self.h, C.byref(n)))
        return int(n.value)

    def last_route(self):
        """the ROUTE_* bits of the kernels the last classify call on this stream launched, ROUTE_RERUN among them once a synchronisation
        classified it again after a taxon-map overflow (slk_stream_last_route)"""
        m = C.c_uint32(0)
        _check(lib().slk_stream_last_route(self.h, C.byref(m)))
        return int(m.value)

    def set_split_long(self, min_len=-1):
        """Unpaired fragments of at least min_len bases are split over many waves (slk_stream_set_split_long):
        -1 the engine's own choice (300 000 bases, in batches of long fragments), 0 off.  Holds for every later classify call on this stream."""
        _check(lib().slk_stream_set_split_long(self.h, int(min_len)))

    def set_split_hits(self, on=True):
        """Calls that want hit lists take the piece route too, where set_split_long(LEN > 0) would send a call without them
        (slk_stream_set_split_hits; off by default, and never with the engine's own threshold).  The lists are those of the other routes."""
        _check(lib().slk_stream_set_split_hits(self.h, 1 if on else 0))

    def last_split(self):
        """(fragments, pieces, spills) of the last classify call: the fragments that were split, the pieces they made, and how often a
        wave emptied a full 128-entry taxon map before its piece ended (slk_stream_last_split)"""
        f, p, s = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        _check(lib().slk_stream_last_split(self.h, C.byref(f), C.byref(p), C.byref(s)))
        return int(f.value), int(p.value), int(s.value)

    def split_info(self):
        """(waves of the piece kernel's fixed grid, bytes of scratch the piece route holds on this stream) (slk_stream_split_info)"""
        g, b = C.c_uint64(0), C.c_uint64(0)
        _check(lib().slk_stream_split_info(self.h, C.byref(g), C.byref(b)))
        return int(g.value), int(b.value)

    def mask_sequences(self, bases, offsets, window=64, threshold=20, replacement=ord("x")):
        """Low-complexity masking (symmetric DUST; slk_mask_sequences) of sequences in the layout of add_sequences
        -> (masked copy of bases, letters changed).  replacement 0: lower case."""
        bases, offsets = _np(bases, np.uint8).copy(), _np(offsets, np.uint64)
        cfg = MaskConfig(window, threshold, replacement)
        masked = C.c_uint64(0)
        _check(lib().slk_mask_sequences(self.h, _ptr(bases), _ptr(offsets), offsets.size - 1, C.byref(cfg), C.byref(masked)))
        return bases, int(masked.value)

    def spans_batch(self, bases, offsets, mate_bases=None, mate_offsets=None, capacity=None):
        """-> (span_offsets u64[R+1], spans structured array SPAN_DTYPE)"""
        bases, offsets = _np(bases, np.uint8), _np(offsets, np.uint64)
        R = offsets.size - 1
        if mate_bases is not None:
            mate_bases, mate_offsets = _np(mate_bases, np.uint8), _np(mate_offsets, np.uint64)
        if capacity is None:
            capacity = int(bases.size + (mate_bases.size + R if mate_bases is not None else 0)) + 1
        out_off = np.zeros(R + 1, np.uint64)
        out = np.zeros(capacity, SPAN_DTYPE)
        _check(lib().slk_spans_batch(self.index.h, self.h, _ptr(bases), _ptr(offsets), _ptr(mate_bases),
                                     _ptr(mate_offsets), R, _ptr(out_off), _ptr(out), capacity))
        return out_off, out[:int(out_off[R])]

    def spans_batch_wide(self, bases, offsets, mate_bases=None, mate_offsets=None):
        """-> (span_offsets u64[R+1], spans SPAN_DTYPE, keys int64 [n_spans, id_longs])"""
        bases, offsets = _np(bases, np.uint8), _np(offsets, np.uint64)
        R = offsets.size - 1
        if mate_bases is not None:
            mate_bases, mate_offsets = _np(mate_bases, np.uint8), _np(mate_offsets, np.uint64)
        capacity = int(bases.size + (mate_bases.size + R if mate_bases is not None else 0)) + 1
        out_off = np.zeros(R + 1, np.uint64)
        out = np.zeros(capacity, SPAN_DTYPE)
        keys = np.zeros((capacity, self.index.W), np.int64)
        _check(lib().slk_spans_batch_wide(self.index.h, self.h, _ptr(bases), _ptr(offsets), _ptr(mate_bases), _ptr(mate_offsets), R,
                                          _ptr(out_off), _ptr(out), _ptr(keys), capacity))
        n = int(out_off[R])
        return out_off, out[:n], keys[:n]

    def classify_batch(self, bases, offsets, mate_bases=None, mate_offsets=None, min_hit_groups=2,
                       thresholds=(0.0,), with_hits=True, hits_capacity=None, with_num_hits=False, out=None, packed=False):
        """out: optional dict of preallocated result arrays (taxon [C,R] int32, classified [C,R] uint8, num_distinct [R],
        total_kmers [R]) -- e.g. pinned_array()s, which the library fills by DMA.
        packed: True = the reads travel in the engine's 3-bit form (packed here by slk_pack_bases; slk_classify_batch_packed), or a
        tuple (codes, valid[, mate_codes, mate_valid]) of arrays packed beforehand (bases may then be None)."""
        offsets = _np(offsets, np.uint64)
        R = offsets.size - 1
        pk = None
        if packed:
            if packed is True:
                pk = pack_bases(bases) + (pack_bases(mate_bases) if mate_bases is not None else (None, None))
            else:
                pk = tuple(packed) + (None, None) * (len(packed) == 2)
            n_bases = int(offsets[R])
            n_mates = int(_np(mate_offsets, np.uint64)[R]) if mate_offsets is not None else 0
        else:
            bases = _np(bases, np.uint8)
            n_bases, n_mates = bases.size, (np.asarray(mate_bases).size if mate_bases is not None else 0)
        if mate_offsets is not None:
            mate_offsets = _np(mate_offsets, np.uint64)
            if not packed:
                mate_bases = _np(mate_bases, np.uint8)
        Cn = len(thresholds)
        thr = (C.c_double * Cn)(*thresholds)
        if out is not None:
            taxon, cls, nd, tk = out["taxon"], out["classified"], out["num_distinct"], out["total_kmers"]
            assert taxon.shape == (Cn, R) and taxon.dtype == np.int32 and cls.shape == (Cn, R) and cls.dtype == np.uint8
            assert all(a.flags.c_contiguous for a in (taxon, cls, nd, tk))
        else:
            taxon = np.zeros((Cn, R), np.int32)
            cls = np.zeros((Cn, R), np.uint8)
            nd, tk = np.zeros(R, np.int32), np.zeros(R, np.int32)
        hit_off = hits = None
        cap = 0
        if with_hits:
            cap = hits_capacity if hits_capacity is not None else \
                int(n_bases + (n_mates + R if mate_offsets is not None else 0)) + 1
            hit_off = np.zeros(R + 1, np.uint64)
            hits = np.zeros(cap, HIT_DTYPE)
        elif with_num_hits:   # the number of spans per fragment without the lists: offsets only
            hit_off = np.zeros(R + 1, np.uint64)
        if pk is not None:
            _check(lib().slk_classify_batch_packed(self.index.h, self.h, _ptr(pk[0]), _ptr(pk[1]), _ptr(offsets), _ptr(pk[2]), _ptr(pk[3]),
                                                   _ptr(mate_offsets), R, min_hit_groups, thr, Cn, _ptr(taxon), _ptr(cls),
                                                   _ptr(nd), _ptr(tk), _ptr(hit_off), _ptr(hits), cap))
        else:
            _check(lib().slk_classify_batch(self.index.h, self.h, _ptr(bases), _ptr(offsets), _ptr(mate_bases),
                                            _ptr(mate_offsets), R, min_hit_groups, thr, Cn, _ptr(taxon), _ptr(cls),
                                            _ptr(nd), _ptr(tk), _ptr(hit_off), _ptr(hits), cap))
        out = dict(taxon=taxon, classified=cls, num_distinct=nd, total_kmers=tk)
        if with_hits:
            out["hit_offsets"] = hit_off
            out["hits"] = hits[:int(hit_off[R])]
            out["num_hits"] = np.diff(hit_off.astype(np.int64)).astype(np.int32)
        elif with_num_hits:
            out["num_hits"] = np.diff(hit_off.astype(np.int64)).astype(np.int32)
        return out

    def parse_text_raw(self, data, fmt, final=True, bases_capacity=None, records_capacity=None, guard=0):
        """slk_parse_text as it stands: -> dict(bases, offsets, title_pos, title_len, R, n_bases, consumed).  The output arrays are
        allocated with `guard` extra elements behind the capacities, filled with 0xA5 bytes, and returned whole under the keys
        raw_*: what the call must not touch."""
        data = np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else _np(data, np.uint8)
        n = data.size
        bcap = n if bases_capacity is None else int(bases_capacity)
        rcap = n // 2 + 2 if records_capacity is None else int(records_capacity)
        bases = np.full(bcap + guard, 0xA5, np.uint8)
        offsets = np.full(rcap + 1 + guard, 0xA5A5A5A5A5A5A5A5, np.uint64)
        tpos = np.full(rcap + guard, 0xA5A5A5A5A5A5A5A5, np.uint64)
        tlen = np.full(rcap + guard, 0xA5A5A5A5, np.uint32)
        R, nb, consumed = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        rc = lib().slk_parse_text(self.h, _ptr(data), n, _format(fmt), 1 if final else 0, _ptr(bases), _ptr(offsets), _ptr(tpos), _ptr(tlen),
                                  bcap, rcap, C.byref(R), C.byref(nb), C.byref(consumed))
        out = dict(raw_bases=bases, raw_offsets=offsets, raw_title_pos=tpos, raw_title_len=tlen, R=int(R.value), n_bases=int(nb.value),
                   consumed=int(consumed.value), bases_capacity=bcap, records_capacity=rcap)
        if rc != 0:
            err = SlackenError(rc, lib().slk_last_error().decode())
            err.partial = out
            raise err
        out.update(bases=bases[:out["n_bases"]], offsets=offsets[:out["R"] + 1], title_pos=tpos[:out["R"]], title_len=tlen[:out["R"]])
        return out

    def parse_text(self, data, fmt, final=True):
        """FASTA / FASTQ text (bytes) parsed on the device (slk_parse_text) -> (titles, seqs, consumed): two lists of str, and where the
        caller's next chunk starts (len(data) when final)."""
        data = bytes(data)
        o = self.parse_text_raw(data, fmt, final)
        off = o["offsets"]
        seqs = [o["bases"][int(off[r]):int(off[r + 1])].tobytes().decode("latin-1") for r in range(o["R"])]
        titles = [data[int(p):int(p) + int(l)].decode("latin-1") for p, l in zip(o["title_pos"], o["title_len"])]
        return titles, seqs, o["consumed"]

    def classify_text(self, data, fmt, final=True, min_hit_groups=2, thresholds=(0.0,), with_hits=True, records_capacity=None,
                      hits_capacity=None):
        """classify_batch on the records of a FASTA / FASTQ text that is parsed on the device (slk_classify_text): the result dict of
        classify_batch plus offsets [R+1], title_pos, title_len, titles (list of str), R and consumed."""
        data = bytes(data)
        text = np.frombuffer(data, np.uint8)
        n = text.size
        rcap = n // 2 + 2 if records_capacity is None else int(records_capacity)
        Cn = len(thresholds)
        thr = (C.c_double * Cn)(*thresholds)
        taxon, cls = np.zeros(Cn * rcap, np.int32), np.zeros(Cn * rcap, np.uint8)
        nd, tk = np.zeros(rcap, np.int32), np.zeros(rcap, np.int32)
        offsets, tpos, tlen = np.zeros(rcap + 1, np.uint64), np.zeros(rcap, np.uint64), np.zeros(rcap, np.uint32)
        hit_off = hits = None
        cap = 0
        if with_hits:
            cap = hits_capacity if hits_capacity is not None else n + 1
            hit_off, hits = np.zeros(rcap + 1, np.uint64), np.zeros(cap, HIT_DTYPE)
        R, consumed = C.c_uint64(0), C.c_uint64(0)
        _check(lib().slk_classify_text(self.index.h, self.h, _ptr(text), n, _format(fmt), 1 if final else 0, min_hit_groups, thr, Cn,
                                       _ptr(taxon), _ptr(cls), _ptr(nd), _ptr(tk), _ptr(offsets), _ptr(tpos), _ptr(tlen), _ptr(hit_off),
                                       _ptr(hits), rcap, cap, C.byref(R), C.byref(consumed)))
        R = int(R.value)
        out = dict(taxon=taxon[:Cn * R].reshape(Cn, R), classified=cls[:Cn * R].reshape(Cn, R), num_distinct=nd[:R], total_kmers=tk[:R],
                   offsets=offsets[:R + 1], title_pos=tpos[:R], title_len=tlen[:R], R=R, consumed=int(consumed.value))
        out["titles"] = [data[int(p):int(p) + int(l)].decode("latin-1") for p, l in zip(out["title_pos"], out["title_len"])]
        if with_hits:
            out["hit_offsets"] = hit_off[:R + 1]
            out["hits"] = hits[:int(hit_off[R])]
            out["num_hits"] = np.diff(hit_off[:R + 1].astype(np.int64)).astype(np.int32)
        return out

    def parse_text_paired_raw(self, data1, fmt1, final1, data2, fmt2, final2, bases_capacity=(None, None), records_capacity=(None, None), guard=0):
        """slk_parse_text_paired as it stands: -> dict(bases, offsets, mate_bases, mate_offsets, title_pos, title_len and the fields of the
        pair record: P, mismatch, consumed1, consumed2, R1, R2, n_bases, n_mate_bases).  The output arrays are allocated with `guard`
        extra elements behind the capacities, filled with 0xA5 bytes, and returned whole under the keys raw_*."""
        d1 = np.frombuffer(bytes(data1), np.uint8)
        d2 = np.frombuffer(bytes(data2), np.uint8)
        bcap = [d.size if c is None else int(c) for d, c in zip((d1, d2), bases_capacity)]
        rcap = [d.size // 2 + 2 if c is None else int(c) for d, c in zip((d1, d2), records_capacity)]
        A5 = 0xA5A5A5A5A5A5A5A5
        bases, mbases = np.full(bcap[0] + guard, 0xA5, np.uint8), np.full(bcap[1] + guard, 0xA5, np.uint8)
        offsets, moffsets = np.full(rcap[0] + 1 + guard, A5, np.uint64), np.full(rcap[1] + 1 + guard, A5, np.uint64)
        tpos, tlen = np.full(rcap[0] + guard, A5, np.uint64), np.full(rcap[0] + guard, 0xA5A5A5A5, np.uint32)
        pair = np.zeros(8, np.uint64)
        rc = lib().slk_parse_text_paired(self.h, _ptr(d1), d1.size, _format(fmt1), 1 if final1 else 0, _ptr(d2), d2.size, _format(fmt2),
                                         1 if final2 else 0, _ptr(bases), _ptr(offsets), _ptr(mbases), _ptr(moffsets), _ptr(tpos), _ptr(tlen),
                                         bcap[0], rcap[0], bcap[1], rcap[1], _ptr(pair))
        out = dict(raw_bases=bases, raw_offsets=offsets, raw_mate_bases=mbases, raw_mate_offsets=moffsets, raw_title_pos=tpos, raw_title_len=tlen,
                   bases_capacity=tuple(bcap), records_capacity=tuple(rcap))
        out.update({k: int(v) for k, v in zip(PAIR_FIELDS, pair)})
        out["mismatch"] = bool(out["mismatch"])
        if rc != 0:
            err = SlackenError(rc, lib().slk_last_error().decode())
            err.partial = out
            raise err
        P = out["P"]
        out.update(bases=bases[:out["n_bases"]], offsets=offsets[:P + 1], mate_bases=mbases[:out["n_mate_bases"]], mate_offsets=moffsets[:P + 1],
                   title_pos=tpos[:out["R1"]], title_len=tlen[:out["R1"]])
        return out

    def parse_text_paired(self, data1, fmt1, final1, data2, fmt2, final2):
        """Two mate texts parsed and paired in lockstep on the device (slk_parse_text_paired) -> dict(titles: the stripped titles of ALL R1
        records of text 1 -- the first P are the pairs' --, seqs, mate_seqs: lists of str for the P pairs, P, mismatch, consumed1,
        consumed2, R1, R2)."""
        data1 = bytes(data1)
        o = self.parse_text_paired_raw(data1, fmt1, final1, data2, fmt2, final2)
        off, moff = o["offsets"], o["mate_offsets"]
        out = {k: o[k] for k in ("P", "mismatch", "consumed1", "consumed2", "R1", "R2")}
        out["seqs"] = [o["bases"][int(off[r]):int(off[r + 1])].tobytes().decode("latin-1") for r in range(o["P"])]
        out["mate_seqs"] = [o["mate_bases"][int(moff[r]):int(moff[r + 1])].tobytes().decode("latin-1") for r in range(o["P"])]
        out["titles"] = [data1[int(p):int(p) + int(l)].decode("latin-1") for p, l in zip(o["title_pos"], o["title_len"])]
        return out

    def classify_text_paired(self, data1, fmt1, final1, data2, fmt2, final2, min_hit_groups=2, thresholds=(0.0,), with_hits=True,
                             records_capacity=None, hits_capacity=None):
        """classify_batch with mates on the pairs of two mate texts that are parsed and paired on the device (slk_classify_text_paired): the
        result dict of classify_batch for the P pairs plus offsets, mate_offsets [P+1], title_pos, title_len, titles (all R1 records of
        text 1, stripped) and the fields of the pair record."""
        data1, data2 = bytes(data1), bytes(data2)
        t1, t2 = np.frombuffer(data1, np.uint8), np.frombuffer(data2, np.uint8)
        rcap = max(t1.size, t2.size) // 2 + 2 if records_capacity is None else int(records_capacity)
        Cn = len(thresholds)
        thr = (C.c_double * Cn)(*thresholds)
        taxon, cls = np.zeros(Cn * rcap, np.int32), np.zeros(Cn * rcap, np.uint8)
        nd, tk = np.zeros(rcap, np.int32), np.zeros(rcap, np.int32)
        offsets, moffsets = np.zeros(rcap + 1, np.uint64), np.zeros(rcap + 1, np.uint64)
        tpos, tlen = np.zeros(rcap, np.uint64), np.zeros(rcap, np.uint32)
        hit_off = hits = None
        cap = 0
        if with_hits:
            cap = hits_capacity if hits_capacity is not None else t1.size + t2.size + rcap + 1
            hit_off, hits = np.zeros(rcap + 1, np.uint64), np.zeros(cap, HIT_DTYPE)
        pair = np.zeros(8, np.uint64)
        rc = lib().slk_classify_text_paired(self.index.h, self.h, _ptr(t1), t1.size, _format(fmt1), 1 if final1 else 0, _ptr(t2), t2.size,
                                            _format(fmt2), 1 if final2 else 0, min_hit_groups, thr, Cn, _ptr(taxon), _ptr(cls), _ptr(nd), _ptr(tk),
                                            _ptr(offsets), _ptr(moffsets), _ptr(tpos), _ptr(tlen), _ptr(hit_off), _ptr(hits), rcap, cap, _ptr(pair))
        out = {k: int(v) for k, v in zip(PAIR_FIELDS, pair)}
        out["mismatch"] = bool(out["mismatch"])
        if rc != 0:
            err = SlackenError(rc, lib().slk_last_error().decode())
            err.partial = out
            raise err
        P, R1 = out["P"], out["R1"]
        out.update(taxon=taxon[:Cn * P].reshape(Cn, P), classified=cls[:Cn * P].reshape(Cn, P), num_distinct=nd[:P], total_kmers=tk[:P],
                   offsets=offsets[:P + 1], mate_offsets=moffsets[:P + 1], title_pos=tpos[:R1], title_len=tlen[:R1])
        out["titles"] = [data1[int(p):int(p) + int(l)].decode("latin-1") for p, l in zip(out["title_pos"], out["title_len"])]
        if with_hits:
            out["hit_offsets"] = hit_off[:P + 1]
            out["hits"] = hits[:int(hit_off[P])]
            out["num_hits"] = np.diff(hit_off[:P + 1].astype(np.int64)).astype(np.int32)
        return out

    def classify_hits(self, hit_offsets, hits, distinct=None, min_hit_groups=2, thresholds=(0.0,)):
        """Classifier.classify on caller-assembled hit lists (HIT_DTYPE array + offsets); distinct: uint8 per hit or None."""
        hit_offsets = _np(hit_offsets, np.uint64)
        hits = np.ascontiguousarray(hits, dtype=HIT_DTYPE)
        if distinct is not None:
            distinct = _np(distinct, np.uint8)
        R = hit_offsets.size - 1
        Cn = len(thresholds)
        thr = (C.c_double * Cn)(*thresholds)
        taxon, cls = np.zeros((Cn, R), np.int32), np.zeros((Cn, R), np.uint8)
        nd, tk = np.zeros(R, np.int32), np.zeros(R, np.int32)
        _check(lib().slk_classify_hits(self.index.h, self.h, R, _ptr(hit_offsets), _ptr(hits), _ptr(distinct), min_hit_groups,
                                       thr, Cn, _ptr(taxon), _ptr(cls), _ptr(nd), _ptr(tk)))
        return dict(taxon=taxon, classified=cls, num_distinct=nd, total_kmers=tk)

    def classify_batch_device(self, d_bases, d_offsets, R, total_bases, d_out_taxon, d_out_classified,
                              d_out_num_distinct=None, d_out_total_kmers=None, d_out_num_hits=None, d_out_num_probes=None,
                              d_mate_bases=None, d_mate_offsets=None, total_mate_bases=0, min_hit_groups=2,
                              thresholds=(0.0,)):
        """All d_* are raw device addresses (ints), e.g. torch.Tensor.data_ptr(). Asynchronous on this stream."""
        Cn = len(thresholds)
        thr = (C.c_double * Cn)(*thresholds)
        _check(lib().slk_classify_batch_device(self.index.h, self.h, d_bases, d_offsets, d_mate_bases,
                                               d_mate_offsets, R, total_bases, total_mate_bases, min_hit_groups, thr,
                                               Cn, d_out_taxon, d_out_classified, d_out_num_distinct,
                                               d_out_total_kmers, d_out_num_hits, d_out_num_probes))

    def scan_device(self, d_bases, d_offsets, R, d_span_keys, d_span_meta, d_span_count, d_mate_bases=None,
                    d_mate_offsets=None):
        _check(lib().slk_scan_device(self.index.h, self.h, d_bases, d_offsets, d_mate_bases, d_mate_offsets, R,
                                     d_span_keys, d_span_meta, d_span_count))

    def lookup_device(self, d_keys, n, d_out_taxa):
        _check(lib().slk_lookup_device(self.index.h, self.h, d_keys, n, d_out_taxa))

    def shard_step(self, emit=None, lookup=None, apply_lists=None, apply=None):
        """One pipeline step of the table-sharded mode (slk_shard_step_device): emit / apply_lists: ShardLists, lookup: ShardLookup,
        apply: ShardResults -- any may be None.  Asynchronous on this stream."""
        _check(lib().slk_shard_step_device(self.index.h, self.h, C.byref(emit) if emit is not None else None,
                                           C.byref(lookup) if lookup is not None else None,
                                           C.byref(apply_lists) if apply_lists is not None else None,
                                           C.byref(apply) if apply is not None else None))

    def classify_hits_device(self, d_offsets, R, d_span_meta, d_span_taxon, d_span_count, d_scratch, d_out_taxon,
                             d_out_classified, d_out_num_distinct=None, d_out_total_kmers=None, d_out_num_hits=None,
                             d_mate_offsets=None, min_hit_groups=2, thresholds=(0.0,)):
        Cn = len(thresholds)
        thr = (C.c_double * Cn)(*thresholds)
        _check(lib().slk_classify_hits_device(self.index.h, self.h, d_offsets, d_mate_offsets, R, d_span_meta,
                                              d_span_taxon, d_span_count, d_scratch, min_hit_groups, thr, Cn,
                                              d_out_taxon, d_out_classified, d_out_num_distinct, d_out_total_kmers,
                                              d_out_num_hits))

    def last_stage_ms(self):
        out = (C.c_float * 3)()
        _check(lib().slk_stream_last_stage_ms(self.h, out))
        return list(out)

    def close(self):
        """Destroys the engine stream -- unless torch still holds a view of it (external_stream): then the handle is parked in
        capi._deferred_streams, alive, and release_deferred_streams() destroys it once the views are gone."""
        if getattr(self, "h", None):
            if self.views_alive():
                _deferred_streams.append((self.h, list(self._views), self.index))
                self.h = None
                return
            lib().slk_stream_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def release_deferred_streams():
    """Destroys the parked streams whose torch views have all died; -> how many are still parked."""
    keep = []
    for h, views, index in _deferred_streams:
        if any(r() is not None for r in views):
            keep.append((h, views, index))
        else:
            lib().slk_stream_destroy(h)
    _deferred_streams[:] = keep
    return len(keep)
