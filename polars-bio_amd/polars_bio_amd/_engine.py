"""ctypes binding of libivjoin_hip.so (include/ivjoin.h).

This is the only place the package touches the native library.  There is no
CPU fallback: if the library is missing or no MI355X is usable the engine
raises -- it never routes through the oracle or numpy.

Replaces the reference's PyO3 entry point
``polars_bio.polars_bio.range_operation_frame`` (/root/reference/src/lib.rs:79-145).
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Optional, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libivjoin_hip.so")

FILTER_WEAK = 0    # FilterOp.Weak   (1-based closed)    src/option.rs:95-100
FILTER_STRICT = 1  # FilterOp.Strict (0-based half-open)

# every symbol include/ivjoin.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = [
    "ivj_last_error", "ivj_version", "ivj_abi_version", "ivj_device_count", "ivj_host_mem_available", "ivj_ctx_create", "ivj_ctx_destroy",
    "ivj_ctx_set_stream", "ivj_ctx_sync", "ivj_ctx_enable_timing", "ivj_ctx_get_timings", "ivj_ctx_profile_mark",
    "ivj_overlap", "ivj_pairs_free", "ivj_count_overlaps", "ivj_nearest",
    "ivj_index_build_dev", "ivj_index_free", "ivj_overlap_count_dev", "ivj_overlap_fill_dev", "ivj_overlap_fused_dev",
    "ivj_count_overlaps_dev", "ivj_nearest_dev",
    "ivj_overlap_thresh", "ivj_count_overlaps_thresh", "ivj_overlap_thresh_dev", "ivj_count_overlaps_thresh_dev",
    "ivj_overlap_window", "ivj_window_dist_free", "ivj_count_window", "ivj_overlap_window_dev", "ivj_count_window_dev",
    "ivj_overlap_select", "ivj_rowsel_free", "ivj_overlap_select_dev", "ivj_overlap_outer",
    "ivj_side_from_arrow", "ivj_materialize_dev", "ivj_overlap_fused_rows_dev", "ivj_take_dev", "ivj_take", "ivj_overlap_rows", "ivj_rows_free", "ivj_rows_export_arrow",
    "ivj_subtract", "ivj_complement", "ivj_pieces_free", "ivj_subtract_dev",
    "ivj_merge", "ivj_merged_free", "ivj_cluster", "ivj_coverage", "ivj_cluster_dev", "ivj_merge_dev", "ivj_coverage_dev",
    "ivj_merge_agg", "ivj_merge_agg_free", "ivj_merge_agg_dev",
    "ivj_overlap_agg", "ivj_overlap_agg_dev", "ivj_overlap_quantiles", "ivj_overlap_quantiles_dev", "ivj_permute_overlaps", "ivj_permute_overlaps_dev",
    "ivj_overlap_wagg", "ivj_overlap_wagg_dev", "ivj_signal_profile", "ivj_signal_profile_dev",
    "ivj_overlap_bases", "ivj_overlap_bases_dev", "ivj_depth_profile", "ivj_depth_profile_dev",
    "ivj_depth", "ivj_blocks_free", "ivj_depth_dev", "ivj_depth_summary", "ivj_depth_summary_dev",
    "ivj_depth_hist", "ivj_depth_hist_contigs", "ivj_depth_hist_dev", "ivj_depth_hist_contigs_dev",
    "ivj_depth_quantiles", "ivj_depth_quantiles_dev",
    "ivj_setop", "ivj_regions_free", "ivj_set_stats", "ivj_setop_dev", "ivj_set_stats_dev",
    "ivj_multi_inter", "ivj_segments_free", "ivj_multi_inter_dev", "ivj_multi_pairwise", "ivj_multi_pairwise_dev",
    "ivj_stream_open", "ivj_stream_submit", "ivj_stream_flush", "ivj_stream_set_nearest_ignore", "ivj_stream_close",
    "ivj_dev_alloc", "ivj_dev_free", "ivj_memcpy_h2d", "ivj_memcpy_d2h",
    "ivj_comm_unique_id", "ivj_comm_create", "ivj_comm_create_local", "ivj_comm_destroy", "ivj_comm_info",
    "ivj_allgather_counts", "ivj_allgatherv_dev", "ivj_overlap_allgather_dev",
    "ivj_count_overlaps_allgather_dev", "ivj_nearest_allgather_dev",
    "ivj_overlap_arrow_stream", "ivj_count_overlaps_arrow_stream", "ivj_nearest_arrow_stream", "ivj_arrow_encode_keys", "ivj_arrow_keys_free",
    "ivj_overlap_arrow_stream_lazy", "ivj_count_overlaps_arrow_stream_lazy", "ivj_nearest_arrow_stream_lazy",
    "ivj_arrow_take_stream",
    "ivj_host_shard", "ivj_host_contig_hist", "ivj_group_ids_dev", "ivj_host_group_ids",
    "ivj_host_narrow_i32", "ivj_host_encode_utf8", "ivj_host_encode_keys64", "ivj_host_remap_i32", "ivj_host_take", "ivj_host_scatter", "ivj_host_widen_i32",
]

ABI_VERSION = 6            # include/ivjoin.h: IVJ_ABI_VERSION (struct layouts and signatures this binding assumes)
STREAM_OVERLAP, STREAM_COUNT, STREAM_NEAREST = 0, 1, 2
# ivj_opts.nearest_ignore: the candidate classes a nearest call leaves out (rows before / after the probe; overlapping rows always count)
NEAREST_IGNORE_LEFT, NEAREST_IGNORE_RIGHT = 1, 2
DEPTH_PROFILE_MAX_BINS = 4096        # include/ivjoin.h: ivj_depth_profile accepts 1 .. this many bins
MAX_HIST_DEPTH = 1023                # include/ivjoin.h: IVJ_MAX_HIST_DEPTH, ivj_depth_hist accepts max_depth in 1 .. this
HIST_LDS_BYTES, HIST_MAX_TILE = 65536, 512      # include/ivjoin.h: IVJ_HIST_LDS_BYTES, IVJ_HIST_MAX_TILE


def depth_hist_tile(max_depth: int) -> int:
    """probe rows one workgroup of ivj_depth_hist owns (include/ivjoin.h); informative: the result does not depend on it"""
    return min(max(HIST_LDS_BYTES // ((int(max_depth) + 1) * 8), 1), HIST_MAX_TILE)


MAX_QUANT_RANKS = 16                 # include/ivjoin.h: IVJ_MAX_QUANT_RANKS, ivj_depth_quantiles accepts 1 .. this many ranks per row
QUANT_BITS, QUANT_LDS_BYTES, QUANT_MAX_TILE = 4, 65536, 512      # include/ivjoin.h: IVJ_QUANT_BITS, IVJ_QUANT_LDS_BYTES, IVJ_QUANT_MAX_TILE


def depth_quant_tile(n_ranks: int) -> int:
    """probe rows one workgroup of ivj_depth_quantiles owns (include/ivjoin.h); informative: the result does not depend on it"""
    return min(max(QUANT_LDS_BYTES // (int(n_ranks) * (1 << QUANT_BITS) * 8), 1), QUANT_MAX_TILE)

MAX_OVQ_RANKS = 16                   # include/ivjoin.h: IVJ_MAX_OVQ_RANKS, ivj_overlap_quantiles accepts 1 .. this many requests per call
OVQ_BITS, OVQ_LDS_BYTES, OVQ_MAX_TILE = 4, 49152, 512            # include/ivjoin.h: IVJ_OVQ_BITS, IVJ_OVQ_LDS_BYTES, IVJ_OVQ_MAX_TILE


def overlap_quant_tile(n_q: int) -> int:
    """probe rows one workgroup of ivj_overlap_quantiles owns (include/ivjoin.h); informative: the result does not depend on it"""
    return min(max(OVQ_LDS_BYTES // (int(n_q) * (1 << OVQ_BITS) * 4), 1), OVQ_MAX_TILE)


# the operations of ivj_setop / ivj_setop_dev (include/ivjoin.h: IVJ_SETOP_*)
SETOP_INTERSECTION, SETOP_UNION, SETOP_DIFFERENCE, SETOP_SYMMETRIC_DIFFERENCE = 0, 1, 2, 3
SETOPS = {"intersection": SETOP_INTERSECTION, "union": SETOP_UNION, "difference": SETOP_DIFFERENCE,
          "symmetric_difference": SETOP_SYMMETRIC_DIFFERENCE}

# ivj_multi_inter / ivj_multi_inter_dev (include/ivjoin.h: IVJ_MAX_FRAMES, IVJ_MULTI_*)
MAX_FRAMES = 64
MULTI_SEGMENTS, MULTI_CONSENSUS = 0, 1

# ivj_merge_agg / ivj_merge_agg_dev (include/ivjoin.h: IVJ_AGG_*, IVJ_MAX_AGG_COLS)
AGG_SUM, AGG_MIN, AGG_MAX, AGG_MEAN, AGG_COUNT = 1, 2, 4, 8, 16
AGG_OPS = {"sum": AGG_SUM, "min": AGG_MIN, "max": AGG_MAX, "mean": AGG_MEAN, "count": AGG_COUNT}
AGG_I64, AGG_F64 = 0, 1
MAX_AGG_COLS = 16

ROW_COLUMNS = ("probe_idx", "build_idx", "contig", "start_1", "end_1", "start_2", "end_2")


IVJ_ECAPACITY, IVJ_ESTATE, IVJ_EPEER = -4, -5, -6

# ivj_overlap_select / ivj_overlap_select_dev (include/ivjoin.h: IVJ_SELECT_*)
SELECT_SEMI, SELECT_ANTI = 0, 1
SELECT_MODES = {"semi": SELECT_SEMI, "anti": SELECT_ANTI}

# ivj_thresholds minima (include/ivjoin.h): uint32 base counts, 0 = no requirement, THRESH_NEVER = the row never matches
THRESH_NEVER = 0xFFFFFFFF


class EngineError(RuntimeError):
    """HIP / engine failure (the reference surfaces these as PanicException).  ``code`` = the IVJ_E* status."""
    code = 0


class PeerError(EngineError):
    """A multi-rank call completed on this rank but ANOTHER rank failed (IVJ_EPEER): the gathered result is incomplete."""


class _Side(C.Structure):
    _fields_ = [("contig", C.c_void_p), ("start", C.c_void_p), ("end", C.c_void_p), ("n", C.c_int64),
                ("row_id", C.c_void_p)]


class _ArrowStream(C.Structure):
    """struct ArrowArrayStream (Arrow C stream interface): five pointers."""
    _fields_ = [("get_schema", C.c_void_p), ("get_next", C.c_void_p), ("get_last_error", C.c_void_p), ("release", C.c_void_p),
                ("private_data", C.c_void_p)]


class _ArrowKeys(C.Structure):
    _fields_ = [("n1", C.c_int64), ("n2", C.c_int64), ("contig1", C.c_void_p), ("start1", C.c_void_p), ("end1", C.c_void_p),
                ("contig2", C.c_void_p), ("start2", C.c_void_p), ("end2", C.c_void_p), ("n_contigs", C.c_int32),
                ("name_offsets", C.c_void_p), ("name_bytes", C.c_void_p)]


class _Opts(C.Structure):
    _fields_ = [("filter_op", C.c_int32), ("n_contigs", C.c_int32), ("nearest_k", C.c_int32),
                ("include_overlaps", C.c_int32), ("partition_mode", C.c_int32), ("table_mode", C.c_int32), ("slice_rows", C.c_int32), ("slice_chunk", C.c_int32),
                ("deterministic", C.c_int32), ("nearest_ignore", C.c_int32)]


class _Thresholds(C.Structure):
    _fields_ = [("min_overlap", C.c_uint32), ("probe_min", C.c_void_p), ("build_min", C.c_void_p)]


class _Window(C.Structure):
    _fields_ = [("left", C.c_uint32), ("right", C.c_uint32), ("probe_left", C.c_void_p), ("probe_right", C.c_void_p),
                ("min_distance", C.c_uint32)]


class _RowSel(C.Structure):
    _fields_ = [("rows", C.POINTER(C.c_int32)), ("n", C.c_int64)]


class _Pairs(C.Structure):
    _fields_ = [("n_pairs", C.c_int64), ("probe_idx", C.POINTER(C.c_int32)), ("build_idx", C.POINTER(C.c_int32))]


class _Rows(C.Structure):
    _fields_ = [("n_pairs", C.c_int64)] + [(name, C.POINTER(C.c_int32)) for name in
                                            ("probe_idx", "build_idx", "contig", "start_1", "end_1", "start_2", "end_2")]


class _Merged(C.Structure):
    _fields_ = [("n", C.c_int64), ("contig", C.POINTER(C.c_int32)), ("start", C.POINTER(C.c_int32)), ("end", C.POINTER(C.c_int32)),
                ("n_intervals", C.POINTER(C.c_int64))]


class _AggIn(C.Structure):
    _fields_ = [("values", C.c_void_p), ("valid", C.c_void_p), ("dtype", C.c_int32), ("ops", C.c_uint32)]


class _AggOut(C.Structure):
    _fields_ = [("sum", C.c_void_p), ("min", C.c_void_p), ("max", C.c_void_p), ("mean", C.c_void_p), ("count", C.c_void_p)]


class _Blocks(C.Structure):
    _fields_ = [("n", C.c_int64), ("contig", C.POINTER(C.c_int32)), ("start", C.POINTER(C.c_int32)), ("end", C.POINTER(C.c_int32)),
                ("depth", C.POINTER(C.c_int32))]


class _Regions(C.Structure):
    _fields_ = [("n", C.c_int64), ("contig", C.POINTER(C.c_int32)), ("start", C.POINTER(C.c_int32)), ("end", C.POINTER(C.c_int32))]


class _Segments(C.Structure):
    _fields_ = [("n", C.c_int64), ("contig", C.POINTER(C.c_int32)), ("start", C.POINTER(C.c_int32)), ("end", C.POINTER(C.c_int32)),
                ("mask", C.POINTER(C.c_uint64))]


class _Pieces(C.Structure):
    _fields_ = [("n", C.c_int64), ("row", C.POINTER(C.c_int32)), ("start", C.POINTER(C.c_int32)), ("end", C.POINTER(C.c_int32))]


class _ArrowSchema(C.Structure):     # Arrow C Data Interface, opaque to Python: only its address is handed on
    _fields_ = [("format", C.c_char_p), ("name", C.c_char_p), ("metadata", C.c_char_p), ("flags", C.c_int64),
                ("n_children", C.c_int64), ("children", C.c_void_p), ("dictionary", C.c_void_p), ("release", C.c_void_p),
                ("private_data", C.c_void_p)]


class _ArrowArray(C.Structure):
    _fields_ = [("length", C.c_int64), ("null_count", C.c_int64), ("offset", C.c_int64), ("n_buffers", C.c_int64),
                ("n_children", C.c_int64), ("buffers", C.c_void_p), ("children", C.c_void_p), ("dictionary", C.c_void_p),
                ("release", C.c_void_p), ("private_data", C.c_void_p)]


class _StreamResult(C.Structure):
    _fields_ = [("batch", C.c_int64), ("n_probe", C.c_int64), ("n", C.c_int64), ("probe_idx", C.POINTER(C.c_int32)),
                ("build_idx", C.POINTER(C.c_int32)), ("counts", C.POINTER(C.c_int64)), ("dist", C.POINTER(C.c_int64)),
                ("n_found", C.POINTER(C.c_int32))]


class _Timing(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("launches", C.c_int32), ("ms", C.c_float)]


_lib = None
_lib_lock = threading.Lock()


def load_library() -> C.CDLL:
    """dlopen the in-tree HIP library; raise loudly when it is absent."""
    global _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise EngineError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        P, O = C.POINTER(_Side), C.POINTER(_Opts)
        vp = C.c_void_p
        L.ivj_last_error.restype = C.c_char_p
        if not hasattr(L, "ivj_abi_version") or L.ivj_abi_version() != ABI_VERSION:
            raise EngineError(f"{LIB_PATH} speaks ABI version {L.ivj_abi_version() if hasattr(L, 'ivj_abi_version') else '?'}, this binding was written "
                              f"against {ABI_VERSION} (include/ivjoin.h: IVJ_ABI_VERSION): rebuild the library")
        L.ivj_version.restype = C.c_char_p
        L.ivj_host_mem_available.restype = C.c_int64
        L.ivj_device_count.argtypes = [C.POINTER(C.c_int)]
        L.ivj_ctx_create.argtypes = [C.c_int, C.POINTER(vp)]
        L.ivj_ctx_destroy.argtypes = [vp]
        L.ivj_ctx_destroy.restype = None
        L.ivj_ctx_set_stream.argtypes = [vp, vp]
        L.ivj_ctx_sync.argtypes = [vp]
        L.ivj_ctx_enable_timing.argtypes = [vp, C.c_int]
        L.ivj_ctx_profile_mark.argtypes = [vp]
        L.ivj_ctx_get_timings.argtypes = [vp, C.POINTER(_Timing), C.c_int, C.POINTER(C.c_int)]
        L.ivj_overlap.argtypes = [vp, P, P, O, C.POINTER(_Pairs)]
        L.ivj_pairs_free.argtypes = [C.POINTER(_Pairs)]
        L.ivj_pairs_free.restype = None
        L.ivj_count_overlaps.argtypes = [vp, P, P, O, vp]
        L.ivj_nearest.argtypes = [vp, P, P, O, vp, vp, vp]
        L.ivj_index_build_dev.argtypes = [vp, P, O, C.c_int, C.POINTER(vp)]
        L.ivj_index_free.argtypes = [vp]
        L.ivj_index_free.restype = None
        L.ivj_overlap_count_dev.argtypes = [vp, vp, P, O, C.POINTER(C.c_int64)]
        L.ivj_overlap_fill_dev.argtypes = [vp, vp, P, O, vp, vp, C.c_int64]
        L.ivj_overlap_fused_dev.argtypes = [vp, vp, P, O, vp, vp, C.c_int64, C.POINTER(C.c_int64)]
        L.ivj_count_overlaps_dev.argtypes = [vp, vp, P, O, vp]
        L.ivj_nearest_dev.argtypes = [vp, vp, P, O, vp, vp, vp]
        T = C.POINTER(_Thresholds)
        L.ivj_overlap_thresh.argtypes = [vp, P, P, O, T, C.POINTER(_Pairs)]
        L.ivj_count_overlaps_thresh.argtypes = [vp, P, P, O, T, vp]
        L.ivj_overlap_thresh_dev.argtypes = [vp, vp, P, O, T, vp, vp, C.c_int64, C.POINTER(C.c_int64)]
        L.ivj_count_overlaps_thresh_dev.argtypes = [vp, vp, P, O, T, vp]
        W = C.POINTER(_Window)
        L.ivj_overlap_window.argtypes = [vp, P, P, O, W, C.POINTER(_Pairs), C.POINTER(C.POINTER(C.c_int64))]
        L.ivj_window_dist_free.argtypes = [C.POINTER(C.c_int64)]
        L.ivj_window_dist_free.restype = None
        L.ivj_count_window.argtypes = [vp, P, P, O, W, vp]
        L.ivj_overlap_window_dev.argtypes = [vp, vp, P, O, W, vp, vp, vp, C.c_int64, C.POINTER(C.c_int64)]
        L.ivj_count_window_dev.argtypes = [vp, vp, P, O, W, vp]
        L.ivj_overlap_select.argtypes = [vp, P, P, O, T, C.c_int32, C.POINTER(_RowSel)]
        L.ivj_rowsel_free.argtypes = [C.POINTER(_RowSel)]
        L.ivj_rowsel_free.restype = None
        L.ivj_overlap_select_dev.argtypes = [vp, vp, P, O, T, C.c_int32, vp, vp, C.c_int64, C.POINTER(C.c_int64)]
        L.ivj_overlap_outer.argtypes = [vp, P, P, O, T, C.POINTER(_Pairs)]
        L.ivj_materialize_dev.argtypes = [vp, P, P, C.POINTER(_Rows)]
        L.ivj_overlap_fused_rows_dev.argtypes = [vp, vp, P, O, C.POINTER(_Rows), C.POINTER(C.c_int64)]
        L.ivj_take_dev.argtypes = [vp, vp, C.c_int32, vp, C.c_int64, vp, vp]
        L.ivj_take.argtypes = [vp, vp, C.c_int64, C.c_int32, vp, vp, vp, vp, vp]
        L.ivj_overlap_rows.argtypes = [vp, P, P, O, C.POINTER(_Rows)]
        L.ivj_rows_free.argtypes = [C.POINTER(_Rows)]
        L.ivj_rows_free.restype = None
        L.ivj_rows_export_arrow.argtypes = [C.POINTER(_Rows), vp, vp]
        L.ivj_side_from_arrow.argtypes = [vp, vp, P]
        L.ivj_subtract.argtypes = [vp, P, P, O, C.POINTER(_Pieces)]
        L.ivj_complement.argtypes = [vp, P, P, O, C.POINTER(_Pieces)]
        L.ivj_pieces_free.argtypes = [C.POINTER(_Pieces)]
        L.ivj_pieces_free.restype = None
        L.ivj_subtract_dev.argtypes = [vp, vp, P, O, C.c_int64, vp, vp, vp, C.POINTER(C.c_int64)]
        L.ivj_merge.argtypes = [vp, P, O, C.c_int64, C.POINTER(_Merged)]
        L.ivj_merged_free.argtypes = [C.POINTER(_Merged)]
        L.ivj_merged_free.restype = None
        L.ivj_cluster.argtypes = [vp, P, O, C.c_int64, vp, vp, vp, C.POINTER(C.c_int64)]
        L.ivj_coverage.argtypes = [vp, P, P, O, vp]
        L.ivj_cluster_dev.argtypes = [vp, vp, O, C.c_int64, vp, vp, vp, C.POINTER(C.c_int64)]
        L.ivj_merge_dev.argtypes = [vp, vp, O, C.c_int64, C.c_int64, vp, vp, vp, vp, C.POINTER(C.c_int64)]
        L.ivj_merge_agg.argtypes = [vp, P, O, C.c_int64, C.c_int32, C.POINTER(_AggIn), C.POINTER(_Merged), C.POINTER(_AggOut)]
        L.ivj_merge_agg_free.argtypes = [C.POINTER(_Merged), C.POINTER(_AggOut), C.c_int32]
        L.ivj_merge_agg_free.restype = None
        L.ivj_merge_agg_dev.argtypes = [vp, vp, O, C.c_int64, C.c_int64, vp, vp, vp, vp, C.c_int64, C.c_int32, C.POINTER(_AggIn),
                                        C.POINTER(_AggOut), C.POINTER(C.c_int64)]
        L.ivj_overlap_agg.argtypes = [vp, P, P, O, T, C.c_int32, C.POINTER(_AggIn), C.POINTER(_AggOut)]
        L.ivj_overlap_agg_dev.argtypes = [vp, vp, P, O, T, C.c_int64, C.c_int32, C.POINTER(_AggIn), C.POINTER(_AggOut)]
        L.ivj_overlap_wagg.argtypes = L.ivj_overlap_agg.argtypes
        L.ivj_overlap_quantiles.argtypes = [vp, P, P, O, T, C.POINTER(_AggIn), C.c_int32, vp, vp, vp, vp]
        L.ivj_overlap_quantiles_dev.argtypes = [vp, vp, P, O, T, C.c_int64, C.POINTER(_AggIn), C.c_int32, vp, vp, vp, vp]
        L.ivj_overlap_wagg_dev.argtypes = L.ivj_overlap_agg_dev.argtypes
        L.ivj_signal_profile.argtypes = [vp, P, vp, C.c_int32, P, O, C.c_int32, C.POINTER(_AggIn), C.POINTER(_AggOut)]
        L.ivj_signal_profile_dev.argtypes = [vp, vp, P, vp, C.c_int32, O, C.c_int64, C.c_int32, C.POINTER(_AggIn), C.POINTER(_AggOut)]
        L.ivj_permute_overlaps.argtypes = [vp, P, P, O, vp, vp, C.c_int64, vp, vp]
        L.ivj_permute_overlaps_dev.argtypes = [vp, vp, P, O, vp, vp, C.c_int64, vp, vp]
        L.ivj_depth.argtypes = [vp, P, O, C.POINTER(_Blocks)]
        L.ivj_blocks_free.argtypes = [C.POINTER(_Blocks)]
        L.ivj_blocks_free.restype = None
        L.ivj_depth_dev.argtypes = [vp, vp, O, C.c_int64, vp, vp, vp, vp, C.POINTER(C.c_int64)]
        L.ivj_setop.argtypes = [vp, P, P, O, C.c_int32, C.POINTER(_Regions)]
        L.ivj_regions_free.argtypes = [C.POINTER(_Regions)]
        L.ivj_regions_free.restype = None
        L.ivj_set_stats.argtypes = [vp, P, P, O, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.ivj_setop_dev.argtypes = [vp, vp, vp, O, C.c_int32, C.c_int64, vp, vp, vp, C.POINTER(C.c_int64)]
        L.ivj_set_stats_dev.argtypes = [vp, vp, vp, O, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.ivj_multi_inter.argtypes = [vp, P, C.c_int32, O, C.c_int32, C.c_int32, C.POINTER(_Segments)]
        L.ivj_segments_free.argtypes = [C.POINTER(_Segments)]
        L.ivj_segments_free.restype = None
        L.ivj_multi_inter_dev.argtypes = [vp, C.POINTER(vp), C.c_int32, O, C.c_int32, C.c_int32, C.c_int64, vp, vp, vp, vp, C.POINTER(C.c_int64)]
        L.ivj_multi_pairwise.argtypes = [vp, P, C.c_int32, O, vp, vp]
        L.ivj_multi_pairwise_dev.argtypes = [vp, C.POINTER(vp), C.c_int32, O, vp, vp]
        L.ivj_coverage_dev.argtypes = [vp, vp, P, O, vp]
        L.ivj_overlap_bases.argtypes = [vp, P, P, O, vp]
        L.ivj_overlap_bases_dev.argtypes = [vp, vp, P, O, vp]
        L.ivj_depth_profile.argtypes = [vp, P, vp, C.c_int32, P, O, vp]
        L.ivj_depth_profile_dev.argtypes = [vp, vp, P, vp, C.c_int32, O, vp]
        L.ivj_depth_summary.argtypes = [vp, P, P, O, vp, C.c_int32, vp, vp]
        L.ivj_depth_summary_dev.argtypes = [vp, vp, P, O, vp, C.c_int32, vp, vp]
        L.ivj_depth_hist.argtypes = [vp, P, P, O, C.c_int32, vp]
        L.ivj_depth_hist_contigs.argtypes = [vp, P, O, C.c_int32, vp]
        L.ivj_depth_hist_dev.argtypes = [vp, vp, P, O, C.c_int32, vp]
        L.ivj_depth_hist_contigs_dev.argtypes = [vp, vp, O, C.c_int32, vp]
        L.ivj_depth_quantiles.argtypes = [vp, P, P, O, C.c_int32, vp, vp]
        L.ivj_depth_quantiles_dev.argtypes = [vp, vp, P, O, C.c_int32, vp, vp]
        L.ivj_stream_open.argtypes = [vp, P, O, C.c_int, C.c_int64, C.POINTER(vp)]
        L.ivj_stream_submit.argtypes = [vp, P, C.POINTER(_StreamResult)]
        L.ivj_stream_flush.argtypes = [vp, C.POINTER(_StreamResult)]
        L.ivj_stream_set_nearest_ignore.argtypes = [vp, C.c_int32]
        L.ivj_stream_close.argtypes = [vp]
        L.ivj_stream_close.restype = None
        L.ivj_dev_alloc.argtypes = [vp, C.c_int64, C.POINTER(vp)]
        L.ivj_dev_free.argtypes = [vp, vp]
        L.ivj_memcpy_h2d.argtypes = [vp, vp, vp, C.c_int64]
        L.ivj_memcpy_d2h.argtypes = [vp, vp, vp, C.c_int64]
        L.ivj_comm_unique_id.argtypes = [vp]
        L.ivj_comm_create.argtypes = [vp, vp, C.c_int, C.c_int, C.POINTER(vp)]
        L.ivj_comm_create_local.argtypes = [C.POINTER(vp), C.c_int, C.POINTER(vp)]
        L.ivj_comm_destroy.argtypes = [vp]
        L.ivj_comm_destroy.restype = None
        L.ivj_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.ivj_allgather_counts.argtypes = [vp, C.c_int64, C.POINTER(C.c_int64)]
        L.ivj_allgatherv_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.c_int, C.c_int, C.POINTER(C.c_int64)]
        L.ivj_overlap_allgather_dev.argtypes = [vp, vp, P, O, C.c_int, vp, vp, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.ivj_count_overlaps_allgather_dev.argtypes = [vp, vp, P, O, C.c_int64, vp]
        L.ivj_nearest_allgather_dev.argtypes = [vp, vp, P, O, C.c_int64, vp, vp, vp]
        L.ivj_host_narrow_i32.argtypes = [vp, C.c_int32, C.c_int32, C.c_int64, vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32]
        L.ivj_host_encode_utf8.argtypes = [vp, C.c_int32, vp, vp, C.c_int64, C.c_int64, vp, vp, C.c_int32, C.POINTER(C.c_int32), C.c_int32]
        L.ivj_host_encode_keys64.argtypes = [vp, C.c_int64, vp, vp, C.c_int32, C.POINTER(C.c_int32), C.c_int32]
        L.ivj_host_remap_i32.argtypes = [vp, C.c_int32, C.c_int64, vp, C.c_int64, vp, vp, C.c_int32]
        L.ivj_host_take.argtypes = [vp, C.c_int32, C.c_int64, vp, C.c_int64, vp, C.c_int32]
        L.ivj_host_scatter.argtypes = [vp, C.c_int32, C.c_int64, vp, C.c_int64, vp, vp, C.c_int64, C.c_int32]
        L.ivj_host_widen_i32.argtypes = [vp, C.c_int64, vp, C.c_int32]
        L.ivj_host_shard.argtypes = [vp, vp, vp, C.c_int64, vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, C.c_int32]
        L.ivj_host_contig_hist.argtypes = [vp, C.c_int64, C.c_int32, vp, C.c_int32]
        L.ivj_group_ids_dev.argtypes = [vp, vp, C.POINTER(vp), C.c_int64, vp, C.POINTER(vp), C.c_int64, C.c_int32, vp, C.c_int32, vp, vp, vp,
                                        C.c_int64, C.POINTER(C.c_int32)]
        L.ivj_host_group_ids.argtypes = [vp, C.POINTER(vp), C.c_int64, vp, C.POINTER(vp), C.c_int64, C.c_int32, vp, C.c_int32, vp, vp, vp,
                                         C.c_int64, C.POINTER(C.c_int32), C.c_int32]
        names3 = C.POINTER(C.c_char_p)
        L.ivj_overlap_arrow_stream.argtypes = [vp, vp, vp, names3, names3, O, C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, vp]
        L.ivj_count_overlaps_arrow_stream.argtypes = [vp, vp, vp, names3, names3, O, C.c_char_p, C.c_int64, C.c_int64, vp]
        L.ivj_nearest_arrow_stream.argtypes = [vp, vp, vp, names3, names3, O, C.c_char_p, C.c_char_p, C.c_int32, C.c_int64, C.c_int64, vp]
        L.ivj_overlap_arrow_stream_lazy.argtypes = [vp, vp, vp, names3, names3, O, C.c_char_p, C.c_char_p, C.c_int64, C.c_int64, C.c_int64, vp]
        L.ivj_count_overlaps_arrow_stream_lazy.argtypes = [vp, vp, vp, names3, names3, O, C.c_char_p, C.c_int64, C.c_int64, C.c_int64, vp]
        L.ivj_nearest_arrow_stream_lazy.argtypes = [vp, vp, vp, names3, names3, O, C.c_char_p, C.c_char_p, C.c_int32, C.c_int64, C.c_int64, C.c_int64, vp]
        L.ivj_arrow_encode_keys.argtypes = [vp, vp, names3, names3, C.POINTER(_ArrowKeys)]
        L.ivj_arrow_keys_free.argtypes = [C.POINTER(_ArrowKeys)]
        L.ivj_arrow_keys_free.restype = None
        L.ivj_arrow_take_stream.argtypes = [vp, vp, C.c_int64, C.c_int64, vp]
        _lib = L
        return L


def _check(L, rc: int, what: str):
    if rc != 0:
        msg = L.ivj_last_error()
        err = (PeerError if rc == IVJ_EPEER else EngineError)(f"{what} failed ({rc}): {msg.decode() if msg else ''}")
        err.code = rc
        raise err


def device_count() -> int:
    L = load_library()
    n = C.c_int(0)
    rc = L.ivj_device_count(C.byref(n))
    return n.value if rc == 0 else 0


def _i32(a) -> np.ndarray:
    a = np.asarray(a)
    if a.dtype != np.int32 or not a.flags.c_contiguous:
        a = np.ascontiguousarray(a, dtype=np.int32)
    return a


def agg_ops_mask(ops) -> int:
    """A name or a list of names of AGG_OPS -> the mask of AGG_* (ValueError on an unknown name or an empty list).  An int is
    taken as the mask itself and handed on unchecked: the library validates it."""
    if isinstance(ops, (int, np.integer)) and not isinstance(ops, (bool, np.bool_)):
        return int(ops) & 0xFFFFFFFF
    names = [ops] if isinstance(ops, str) else list(ops)
    if not names:
        raise ValueError(f"no aggregate operation given: expected some of {sorted(AGG_OPS)}")
    mask = 0
    for name in names:
        if not isinstance(name, str) or name not in AGG_OPS:
            raise ValueError(f"unknown aggregate {name!r}: expected one of {sorted(AGG_OPS)}")
        mask |= AGG_OPS[name]
    return mask


def _agg_column(values, valid, ops, n: int):
    """One value column of merge_agg as the library reads it: contiguous int64 / float64 values, uint8 validity or None."""
    values = np.asarray(values)
    if values.dtype not in (np.int64, np.float64):
        raise ValueError(f"value columns must be int64 or float64 arrays, got {values.dtype}")
    values = np.ascontiguousarray(values)
    if values.shape != (n,):
        raise ValueError(f"a value column has shape {values.shape}, the frame has {n} rows")
    if valid is not None:
        valid = np.ascontiguousarray(np.asarray(valid).astype(bool, copy=False)).view(np.uint8)
        if valid.shape != (n,):
            raise ValueError(f"a validity column has shape {valid.shape}, the frame has {n} rows")
    return values, valid, agg_ops_mask(ops)


def _host_side(contig, start, end) -> Tuple[_Side, tuple]:
    c, s, e = _i32(contig), _i32(start), _i32(end)
    if not (c.shape == s.shape == e.shape and c.ndim == 1):
        raise ValueError("contig/start/end must be 1-D arrays of equal length")
    return _Side(c.ctypes.data, s.ctypes.data, e.ctypes.data, c.shape[0], None), (c, s, e)


def side_from_arrow(batch) -> Tuple[_Side, tuple]:
    """pyarrow.RecordBatch / StructArray with int32 children contig / start / end -> ivj_side viewing the Arrow
    buffers (ivj_side_from_arrow, zero copy).  Returns (side, keep-alive); needs no device."""
    L = load_library()
    arr, sch = _ArrowArray(), _ArrowSchema()
    batch._export_to_c(C.addressof(arr), C.addressof(sch))
    side = _Side()
    _check(L, L.ivj_side_from_arrow(C.addressof(arr), C.addressof(sch), C.byref(side)), "ivj_side_from_arrow")
    return side, (batch, arr, sch)


def _ignore_mask(mask) -> int:
    mask = int(mask)
    if mask < 0 or mask > (NEAREST_IGNORE_LEFT | NEAREST_IGNORE_RIGHT):
        raise ValueError(f"nearest_ignore must be 0 or a mask of NEAREST_IGNORE_LEFT (1) and NEAREST_IGNORE_RIGHT (2), got {mask}")
    return mask


def _u32_min(a, n: int, what: str):
    """A column of per-row minima (ivj_thresholds) as contiguous uint32, or None."""
    if a is None:
        return None
    a = np.ascontiguousarray(a, dtype=np.uint32)
    if a.shape != (n,):
        raise ValueError(f"{what} must hold one uint32 per row ({n}), got shape {a.shape}")
    return a


def make_thresholds(min_overlap: int = 0, probe_min_ptr: int = 0, build_min_ptr: int = 0) -> _Thresholds:
    """ivj_thresholds from a scalar and two (host or device) addresses; 0 = not set."""
    if not 0 <= int(min_overlap) <= THRESH_NEVER:
        raise ValueError(f"min_overlap must fit uint32, got {min_overlap}")
    return _Thresholds(int(min_overlap), probe_min_ptr or None, build_min_ptr or None)


WINDOW_MAX = 0xFFFFFFFF     # ivj_window: extents and min_distance are uint32


def make_window(left: int = 0, right: int = 0, probe_left_ptr: int = 0, probe_right_ptr: int = 0, min_distance: int = 0) -> _Window:
    """ivj_window from the scalar extents, two (host or device) addresses of per-row uint32 extent columns (0 = the scalar holds) and
    the minimum distance."""
    for what, v in (("left", left), ("right", right), ("min_distance", min_distance)):
        if not 0 <= int(v) <= WINDOW_MAX:
            raise ValueError(f"{what} must fit uint32, got {v}")
    return _Window(int(left), int(right), probe_left_ptr or None, probe_right_ptr or None, int(min_distance))


def select_mode(mode) -> int:
    """"semi" / "anti" or SELECT_SEMI / SELECT_ANTI -> the IVJ_SELECT_* code (ValueError otherwise)."""
    if isinstance(mode, str):
        if mode not in SELECT_MODES:
            raise ValueError(f"unknown selection mode '{mode}': one of {sorted(SELECT_MODES)}")
        return SELECT_MODES[mode]
    if isinstance(mode, (bool, np.bool_)) or int(mode) not in SELECT_MODES.values():
        raise ValueError(f"unknown selection mode {mode!r}")
    return int(mode)


def _setop_code(op) -> int:
    if isinstance(op, str):
        if op not in SETOPS:
            raise ValueError(f"unknown set operation '{op}': one of {sorted(SETOPS)}")
        return SETOPS[op]
    if int(op) not in SETOPS.values():
        raise ValueError(f"unknown set operation {op}")
    return int(op)


def check_multi(n_frames: int, min_frames, mode=MULTI_SEGMENTS) -> int:
    """The argument rules of ivj_multi_inter, checked before the library is touched -> min_frames as an int."""
    if n_frames < 1 or n_frames > MAX_FRAMES:
        raise ValueError(f"between 1 and {MAX_FRAMES} frames are expected, got {n_frames}")
    if isinstance(min_frames, (bool, np.bool_)) or not isinstance(min_frames, (int, np.integer)):
        raise ValueError(f"min_frames must be an int, got {min_frames!r}")
    if min_frames < 1 or min_frames > n_frames:
        raise ValueError(f"min_frames must be in 1 .. {n_frames} (the number of frames), got {min_frames}")
    if mode not in (MULTI_SEGMENTS, MULTI_CONSENSUS):
        raise ValueError(f"mode must be MULTI_SEGMENTS (0) or MULTI_CONSENSUS (1), got {mode!r}")
    return int(min_frames)


def make_opts(strict: bool, n_contigs: int, k: int = 1, include_overlaps: bool = True, partition_mode: int = 0,
              table_mode: int = 0, slice_rows: int = 0, slice_chunk: int = 0, deterministic: bool = False, nearest_ignore: int = 0) -> _Opts:
    o = _Opts()
    o.nearest_ignore = _ignore_mask(nearest_ignore)
    o.deterministic = 1 if deterministic else 0
    o.slice_rows = int(slice_rows)
    o.slice_chunk = int(slice_chunk)
    o.table_mode = int(table_mode)
    o.partition_mode = int(partition_mode)
    o.filter_op = FILTER_STRICT if strict else FILTER_WEAK
    o.n_contigs = int(n_contigs)
    o.nearest_k = int(k)
    o.include_overlaps = 1 if include_overlaps else 0
    return o


class _LockedLib:
    """The native library as one Engine sees it: every call is made under that engine's lock.

    An ivj_ctx is not thread-safe (include/ivjoin.h: arena, count -> fill state, pinned totals and the index
    cache are per context) and ctypes releases the GIL during a call, so two Python threads sharing an Engine
    would otherwise race inside the library.  Multi-call sequences (count -> fill, streaming tiles) take
    ``Engine.lock`` around the whole sequence as well (it is re-entrant)."""

    def __init__(self, lib: C.CDLL, lock):
        self._lib, self._lock = lib, lock

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        lock = self._lock

        def call(*args):
            with lock:
                return fn(*args)
        call.__name__ = name
        setattr(self, name, call)
        return call


class _DistOwner:
    """Keeps the distance column of ivj_overlap_window alive for the numpy array that views it."""

    def __init__(self, lib, ptr):
        self.lib, self.ptr = lib, ptr

    def __del__(self):
        try:
            self.lib.ivj_window_dist_free(self.ptr)
        except Exception:
            pass


class _PairsOwner:
    """Keeps an ivj_pairs result alive for the numpy arrays that view its buffers."""

    def __init__(self, lib, pairs):
        self.lib, self.pairs = lib, pairs

    def __del__(self):
        try:
            self.lib.ivj_pairs_free(C.byref(self.pairs))
        except Exception:
            pass


def _owned_view(ptr, n, owner) -> np.ndarray:
    """numpy view of `n` int32 at `ptr` whose base object keeps `owner` alive (views of the view chain back to it)."""
    buf = (C.c_int32 * n).from_address(C.addressof(ptr.contents))
    buf._owner = owner                       # the ctypes array is the numpy array's base: its attribute pins the owner
    return np.frombuffer(buf, dtype=np.int32)


# ---- what the host-buffer methods of Engine share: sides in, columns out ----

def _host_sides(a, b):
    """Both sides of a two-sided host call -> (ivj_side of a, ivj_side of b, the arrays they point into: keep them until the
    call returned)."""
    sa, keep_a = _host_side(*a)
    sb, keep_b = _host_side(*b)
    return sa, sb, (keep_a, keep_b)


def _frames(frames):
    """The frames of a multi-frame host call -> (ivj_side array, keep-alive)."""
    sides = (_Side * len(frames))()
    keep = []
    for f, frame in enumerate(frames):
        sides[f], arrays = _host_side(*frame)
        keep.append(arrays)
    return sides, keep


def _reverse_flags(reverse, n: int):
    """The ``reverse`` argument of the profile calls as contiguous uint8 flags, one per window, or None."""
    if reverse is None:
        return None
    rev = np.ascontiguousarray(np.asarray(reverse).astype(bool).astype(np.uint8))
    if rev.shape != (n,):
        raise ValueError(f"reverse must hold one flag per window ({n}), got shape {rev.shape}")
    return rev


def _agg_in(values, valid, ops, n: int):
    """One (values, valid, ops) value column of ``n`` rows -> (its ivj_agg_in, the checked values array, keep-alive)."""
    values, valid, ops = _agg_column(values, valid, ops, n)
    col = _AggIn(values.ctypes.data if n else None, valid.ctypes.data if valid is not None and n else None,
                 AGG_I64 if values.dtype == np.int64 else AGG_F64, ops)
    return col, values, (values, valid)


def _quantile_requests(q, upper):
    """The (q, upper) requests of ivj_overlap_quantiles as contiguous float64 / uint8 arrays of one length; the library
    validates their number and values."""
    qs = np.ascontiguousarray(np.atleast_1d(np.asarray(q, np.float64)).ravel())
    up = np.ascontiguousarray(np.atleast_1d(np.asarray(upper)).astype(bool).astype(np.uint8).ravel())
    if qs.shape != up.shape:
        raise ValueError(f"q has {qs.size} entries, upper has {up.size}")
    return qs, up


def _copy_columns(out, names, dtypes, free=None):
    """The named columns of a library-allocated result struct (``out.n`` rows) as numpy copies -- empty arrays of ``dtypes`` when
    it has no rows -- after which ``free(pointer to out)`` releases the struct, whatever happened."""
    try:
        n = out.n
        return tuple(np.ctypeslib.as_array(getattr(out, name), shape=(n,)).copy() if n else np.empty(0, dtype)
                     for name, dtype in zip(names, dtypes))
    finally:
        if free is not None:
            free(C.byref(out))


_I32x3 = (np.int32,) * 3
_MERGED_COLUMNS, _MERGED_DTYPES = ("contig", "start", "end", "n_intervals"), _I32x3 + (np.int64,)


class ProbeStream:
    """Streaming probe session (ivj_stream_*): the build side is indexed once, probe batches are submitted one at a time;
    every submit overlaps the H2D copy of its batch, the join of the previous batch and the D2H copy of the one before.

    submit() / flush() return None or a dict: ``batch`` (index of the batch the results belong to), ``n_probe`` and
        overlap         ``probe_idx`` (rows INSIDE that batch), ``build_idx``
        count_overlaps  ``counts``
        nearest         ``build_idx`` (n_probe x k, -1 = none), ``dist`` (n_probe x k), ``n_found``
    The arrays are copies unless ``copy=False`` (then they view the stream's pinned result slot and are valid until the
    next call on the stream).  nearest: ``nearest_ignore`` is the direction mask of the first batches, set_nearest_ignore()
    changes it for the batches submitted after the call."""

    def __init__(self, engine: "Engine", build, strict: bool, n_contigs: int, op: int, max_batch_rows: int, k: int = 1,
                 include_overlaps: bool = True, partition_mode: int = 0, copy: bool = True, nearest_ignore: int = 0):
        self.engine, self.op, self.k, self.copy = engine, int(op), int(k), copy
        self.opts = make_opts(strict, n_contigs, k, include_overlaps, partition_mode=partition_mode, nearest_ignore=nearest_ignore)
        bs, keep = _host_side(*build)
        h = C.c_void_p()
        _check(engine.L, engine.L.ivj_stream_open(engine.h, C.byref(bs), C.byref(self.opts), self.op, int(max_batch_rows), C.byref(h)),
               "ivj_stream_open")
        del keep
        self.h = h
        self.max_batch_rows = int(max_batch_rows)

    def _result(self, r: _StreamResult):
        if r.batch < 0:
            return None
        def arr(ptr, n, dtype, shape=None):
            if n == 0:
                a = np.empty(0, dtype)
            else:
                a = np.ctypeslib.as_array(ptr, shape=(n,))
                a = a.copy() if self.copy else a
            return a.reshape(shape) if shape else a
        out = {"batch": int(r.batch), "n_probe": int(r.n_probe)}
        n, k = int(r.n_probe), self.k
        if self.op == STREAM_OVERLAP:
            out["probe_idx"] = arr(r.probe_idx, int(r.n), np.int32)
            out["build_idx"] = arr(r.build_idx, int(r.n), np.int32)
        elif self.op == STREAM_COUNT:
            out["counts"] = arr(r.counts, n, np.int64)
        else:
            out["build_idx"] = arr(r.build_idx, n * k, np.int32, (n, k))
            out["dist"] = arr(r.dist, n * k, np.int64, (n, k))
            out["n_found"] = arr(r.n_found, n, np.int32)
        return out

    def submit(self, batch):
        """batch: (contig, start, end) int32 arrays, or an ivj_side made by side_from_arrow (zero copy from Arrow)."""
        keep = None
        if isinstance(batch, _Side):
            side = batch
        else:
            side, keep = _host_side(*batch)
        r = _StreamResult()
        _check(self.engine.L, self.engine.L.ivj_stream_submit(self.h, C.byref(side), C.byref(r)), "ivj_stream_submit")
        del keep
        return self._result(r)

    def set_nearest_ignore(self, mask: int):
        """Direction mask (NEAREST_IGNORE_LEFT | NEAREST_IGNORE_RIGHT) of the batches submitted from now on; a batch already
        submitted keeps the mask it was submitted under."""
        mask = _ignore_mask(mask)
        _check(self.engine.L, self.engine.L.ivj_stream_set_nearest_ignore(self.h, mask), "ivj_stream_set_nearest_ignore")
        self.opts.nearest_ignore = mask

    def flush(self):
        r = _StreamResult()
        _check(self.engine.L, self.engine.L.ivj_stream_flush(self.h, C.byref(r)), "ivj_stream_flush")
        return self._result(r)

    def close(self):
        if getattr(self, "h", None):
            self.engine.L.ivj_stream_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceIndex:
    """Sorted build side resident in HBM (ivj_index)."""

    def __init__(self, engine: "Engine", handle: int, n: int):
        self.engine, self.handle, self.n = engine, handle, n

    def close(self):
        if self.handle:
            self.engine.L.ivj_index_free(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """One HIP device + stream + scratch arena (ivj_ctx)."""

    def __init__(self, device: int = 0):
        self.lock = threading.RLock()
        self.L = _LockedLib(load_library(), self.lock)
        h = C.c_void_p()
        _check(self.L, self.L.ivj_ctx_create(int(device), C.byref(h)), "ivj_ctx_create")
        self.h = h
        self.device = device

    def close(self):
        """Destroys the context.  Indexes built on it stay valid handles (the library detaches them) and are
        released by their own close()."""
        with self.lock:
            if getattr(self, "h", None):
                self.L.ivj_ctx_destroy(self.h)
                self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- host-buffer entry points (numpy in, numpy out) --------------------
    def _pairs_result(self, out: _Pairs):
        """An ivj_pairs result -> (probe_idx, build_idx).  No copy: the arrays view the library's (pre-faulted, huge-page) result
        buffers, which are freed when the last view of either array is gone."""
        n = out.n_pairs
        if n == 0:
            self.L.ivj_pairs_free(C.byref(out))
            return np.empty(0, np.int32), np.empty(0, np.int32)
        owner = _PairsOwner(load_library(), out)
        return _owned_view(out.probe_idx, n, owner), _owned_view(out.build_idx, n, owner)

    def overlap(self, probe, build, strict: bool, n_contigs: int, partition_mode: int = 0, table_mode: int = 0, slice_rows: int = 0,
                slice_chunk: int = 0, deterministic: bool = False):
        """probe/build: (contig_id, start, end) int32 arrays -> (probe_idx, build_idx).
        partition_mode: 0 auto, 1 256 buckets + window scan, 2 never (pairs then come in probe-row order), 6 index slices in LDS.
        deterministic: the slice path's output is identical from run to run (stable partition; ivj_opts.deterministic)."""
        ps, bs, keep = _host_sides(probe, build)
        o = make_opts(strict, n_contigs, partition_mode=partition_mode, table_mode=table_mode, slice_rows=slice_rows, slice_chunk=slice_chunk,
                      deterministic=deterministic)
        out = _Pairs()
        _check(self.L, self.L.ivj_overlap(self.h, C.byref(ps), C.byref(bs), C.byref(o), C.byref(out)), "ivj_overlap")
        del keep
        return self._pairs_result(out)

    def take_columns(self, idx: np.ndarray, columns, nullable: bool = False):
        """Arrow ``take`` of fixed-width host columns through HBM (ivj_take): ``columns`` = numpy arrays of 4- or 8-byte
        items sharing the int32 index column ``idx``.  -> list of (values, validity) with validity = None, or (nullable) a
        uint64 bitmap (Arrow layout) whose cleared bits mark the negative-index slots."""
        idx = np.ascontiguousarray(idx, np.int32)
        n, k = int(idx.shape[0]), len(columns)
        cols = [np.ascontiguousarray(c) for c in columns]
        for c in cols:
            if c.dtype.itemsize not in (4, 8) or c.ndim != 1:
                raise ValueError("take_columns: 1-d columns of 4- or 8-byte items only")
        outs = [np.empty(n, c.dtype) for c in cols]
        vals = [np.empty((n + 63) // 64, np.uint64) if nullable else None for _ in cols]
        if n == 0 or k == 0:
            return list(zip(outs, vals))
        VP = C.c_void_p * k
        src = VP(*[c.ctypes.data for c in cols])
        dst = VP(*[o.ctypes.data for o in outs])
        val = VP(*[(v.ctypes.data if v is not None else None) for v in vals])
        rows = (C.c_int64 * k)(*[int(c.shape[0]) for c in cols])
        eb = (C.c_int32 * k)(*[int(c.dtype.itemsize) for c in cols])
        _check(self.L, self.L.ivj_take(self.h, C.c_void_p(idx.ctypes.data), n, k, src, rows, eb, dst, val if nullable else None), "ivj_take")
        return list(zip(outs, vals))

    def overlap_rows(self, probe, build, strict: bool, n_contigs: int, partition_mode: int = 0, as_arrow: bool = False):
        """overlap + row materialisation on the device (ivj_overlap_rows): the pair indices AND the key
        columns of both sides for every pair.  -> dict of int32 numpy arrays keyed by ROW_COLUMNS, or
        (as_arrow=True) a pyarrow.RecordBatch that owns the library's host buffers through the Arrow C
        Data interface (ivj_rows_export_arrow; no copy)."""
        ps, bs, keep = _host_sides(probe, build)
        o = make_opts(strict, n_contigs, partition_mode=partition_mode)
        out = _Rows()
        _check(self.L, self.L.ivj_overlap_rows(self.h, C.byref(ps), C.byref(bs), C.byref(o), C.byref(out)), "ivj_overlap_rows")
        del keep
        try:
            if as_arrow:
                import pyarrow as pa
                arr, sch = _ArrowArray(), _ArrowSchema()
                _check(self.L, self.L.ivj_rows_export_arrow(C.byref(out), C.addressof(arr), C.addressof(sch)),
                       "ivj_rows_export_arrow")
                return pa.RecordBatch._import_from_c(C.addressof(arr), C.addressof(sch))
            n = out.n_pairs
            return {name: (np.ctypeslib.as_array(getattr(out, name), shape=(n,)).copy() if n else np.empty(0, np.int32))
                    for name in ROW_COLUMNS}
        finally:
            self.L.ivj_rows_free(C.byref(out))

    # ---- sort-scan family ---------------------------------------------
    def merge(self, frame, strict: bool, n_contigs: int, min_dist: int = 0):
        """pb.merge: -> (contig id, start, end, n_intervals) of the merged intervals, (contig id, start) order."""
        fs, keep = _host_side(*frame)
        o = make_opts(strict, n_contigs)
        out = _Merged()
        _check(self.L, self.L.ivj_merge(self.h, C.byref(fs), C.byref(o), int(min_dist), C.byref(out)), "ivj_merge")
        del keep
        return _copy_columns(out, _MERGED_COLUMNS, _MERGED_DTYPES, self.L.ivj_merged_free)

    def merge_agg(self, frame, strict: bool, n_contigs: int, agg, min_dist: int = 0):
        """pb.merge(agg=...): ``agg`` = a list of (values, valid, ops) per value column -- values an int64 or float64 array with
        one element per frame row (other dtypes are refused), valid a bool / uint8 array or None, ops a mask of AGG_* or a list
        of names of AGG_OPS.  -> (contig id, start, end, n_intervals, [dict per column]); the dict maps each requested name
        ("sum", "min", "max", "mean", "count") to its array: sum int64 (wrapped) / float64, min / max the column's type, mean
        float64, count int64.  min / max / mean are unspecified where count is 0."""
        fs, keep = _host_side(*frame)
        o = make_opts(strict, n_contigs)
        agg = list(agg)
        cols = (_AggIn * max(len(agg), 1))()
        outs = (_AggOut * max(len(agg), 1))()
        dtypes = []
        for k, (values, valid, ops) in enumerate(agg):
            cols[k], values, arrays = _agg_in(values, valid, ops, fs.n)
            keep += arrays
            dtypes.append(values.dtype)
        out = _Merged()
        _check(self.L, self.L.ivj_merge_agg(self.h, C.byref(fs), C.byref(o), int(min_dist), len(agg), cols, C.byref(out), outs), "ivj_merge_agg")
        del keep
        try:
            n = out.n

            def column(ptr, dtype):
                if n == 0:
                    return np.empty(0, dtype)
                return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_int64)), shape=(n,)).view(dtype).copy()

            table = _copy_columns(out, _MERGED_COLUMNS, _MERGED_DTYPES)      # (freed below, with the aggregates)
            results = []
            for k in range(len(agg)):
                kinds = {"sum": dtypes[k], "min": dtypes[k], "max": dtypes[k], "mean": np.float64, "count": np.int64}
                results.append({name: column(getattr(outs[k], name), kinds[name]) for name, bit in AGG_OPS.items() if cols[k].ops & bit})
            return (*table, results)
        finally:
            self.L.ivj_merge_agg_free(C.byref(out), outs, len(agg))

    def depth(self, frame, strict: bool, n_contigs: int):
        """pb.depth: -> (contig id, start, end, depth) int32 arrays of the blocks of constant coverage >= 1, (contig id, start)
        order; block bounds in the mode's own convention (Strict half-open, Weak closed)."""
        fs, keep = _host_side(*frame)
        o = make_opts(strict, n_contigs)
        out = _Blocks()
        _check(self.L, self.L.ivj_depth(self.h, C.byref(fs), C.byref(o), C.byref(out)), "ivj_depth")
        del keep
        return _copy_columns(out, ("contig", "start", "end", "depth"), (np.int32,) * 4, self.L.ivj_blocks_free)

    def setop(self, a, b, op, strict: bool, n_contigs: int):
        """pb.set_intersect / set_union / set_difference / set_symmetric_difference: -> (contig id, start, end) int32 arrays of
        the maximal runs of op(U(a), U(b)), (contig id, start) order, bounds in the mode's own convention.  ``op``: a name of
        SETOPS or its number."""
        sa, sb, keep = _host_sides(a, b)
        o = make_opts(strict, n_contigs)
        out = _Regions()
        _check(self.L, self.L.ivj_setop(self.h, C.byref(sa), C.byref(sb), C.byref(o), _setop_code(op), C.byref(out)), "ivj_setop")
        del keep
        return _copy_columns(out, ("contig", "start", "end"), _I32x3, self.L.ivj_regions_free)

    def set_stats(self, a, b, strict: bool, n_contigs: int):
        """-> (only_a, only_b, both, n_intersections): the positions only U(a), only U(b), both cover (exact ints) and the
        number of regions of the intersection, from one walk."""
        sa, sb, keep = _host_sides(a, b)
        o = make_opts(strict, n_contigs)
        bases = (C.c_int64 * 3)()
        ni = C.c_int64(0)
        _check(self.L, self.L.ivj_set_stats(self.h, C.byref(sa), C.byref(sb), C.byref(o), bases, C.byref(ni)), "ivj_set_stats")
        del keep
        return int(bases[0]), int(bases[1]), int(bases[2]), int(ni.value)

    def multi_inter(self, frames, min_frames: int, mode: int, strict: bool, n_contigs: int):
        """pb.multi_intersect (mode MULTI_SEGMENTS) / pb.consensus (MULTI_CONSENSUS) over a list of (contig, start, end) frames:
        -> (contig id, start, end) int32 arrays and the uint64 membership mask per segment (bit f = frame f; None for
        consensus), (contig id, start) order, bounds in the mode's own convention."""
        frames = list(frames)
        min_frames = check_multi(len(frames), min_frames, mode)
        sides, keep = _frames(frames)
        o = make_opts(strict, n_contigs)
        out = _Segments()
        _check(self.L, self.L.ivj_multi_inter(self.h, sides, len(frames), C.byref(o), min_frames, int(mode), C.byref(out)), "ivj_multi_inter")
        del keep
        if mode == MULTI_SEGMENTS:
            return _copy_columns(out, ("contig", "start", "end", "mask"), _I32x3 + (np.uint64,), self.L.ivj_segments_free)
        return (*_copy_columns(out, ("contig", "start", "end"), _I32x3, self.L.ivj_segments_free), None)

    def multi_pairwise(self, frames, strict: bool, n_contigs: int):
        """pb.pairwise_jaccard over a list of (contig, start, end) frames: -> (bases, runs), two (F, F) int64 arrays, symmetric;
        bases[i, j] = the positions frames i and j both cover (the diagonal: what frame i covers), runs[i, j] = the regions of
        their intersection (set_stats' n_intersections), from one walk over all frames."""
        frames = list(frames)
        check_multi(len(frames), 1)
        sides, keep = _frames(frames)
        o = make_opts(strict, n_contigs)
        bases = np.zeros((len(frames), len(frames)), np.int64)
        runs = np.zeros((len(frames), len(frames)), np.int64)
        _check(self.L, self.L.ivj_multi_pairwise(self.h, sides, len(frames), C.byref(o), bases.ctypes.data, runs.ctypes.data), "ivj_multi_pairwise")
        del keep
        return bases, runs

    def cluster(self, frame, strict: bool, n_contigs: int, min_dist: int = 0):
        """pb.cluster: -> (cluster id int64, cluster_start, cluster_end) per input row + number of clusters."""
        fs, keep = _host_side(*frame)
        o = make_opts(strict, n_contigs)
        cid = np.empty(fs.n, np.int64)
        cs = np.empty(fs.n, np.int32)
        ce = np.empty(fs.n, np.int32)
        ncl = C.c_int64(0)
        _check(self.L, self.L.ivj_cluster(self.h, C.byref(fs), C.byref(o), int(min_dist), cid.ctypes.data, cs.ctypes.data,
                                           ce.ctypes.data, C.byref(ncl)), "ivj_cluster")
        del keep
        return cid, cs, ce, ncl.value

    def coverage(self, probe, build, strict: bool, n_contigs: int, partition_mode: int = 0) -> np.ndarray:
        """pb.coverage: covered positions of every probe row (int64, probe order)."""
        ps, bs, keep = _host_sides(probe, build)
        o = make_opts(strict, n_contigs, partition_mode=partition_mode)
        cov = np.empty(ps.n, np.int64)
        _check(self.L, self.L.ivj_coverage(self.h, C.byref(ps), C.byref(bs), C.byref(o), cov.ctypes.data), "ivj_coverage")
        del keep
        return cov

    def overlap_bases(self, probe, build, strict: bool, n_contigs: int, partition_mode: int = 0) -> np.ndarray:
        """pb.mean_depth: for every probe row the positions shared with each build row of its contig, summed (int64, probe order)."""
        ps, bs, keep = _host_sides(probe, build)
        o = make_opts(strict, n_contigs, partition_mode=partition_mode)
        bases = np.empty(ps.n, np.int64)
        _check(self.L, self.L.ivj_overlap_bases(self.h, C.byref(ps), C.byref(bs), C.byref(o), bases.ctypes.data), "ivj_overlap_bases")
        del keep
        return bases

    def depth_profile(self, windows, reverse, n_bins: int, build, strict: bool, n_contigs: int) -> np.ndarray:
        """pb.depth_profile: every window row cut into n_bins bins (edges S + floor(j L / n_bins)), per bin the positions shared with
        each build row of the window's contig, summed -> int64 (n, n_bins), window order.  ``reverse``: None or one flag per window;
        a flagged row comes back right to left."""
        ws, bs, keep = _host_sides(windows, build)
        o = make_opts(strict, n_contigs)
        rev = _reverse_flags(reverse, ws.n)
        n_bins = int(n_bins)
        # a bin count the entry refuses gets no matrix: the entry checks n_bins before it looks at the output
        bases = np.empty((ws.n, n_bins if 1 <= n_bins <= DEPTH_PROFILE_MAX_BINS else 0), np.int64)
        _check(self.L, self.L.ivj_depth_profile(self.h, C.byref(ws), rev.ctypes.data if rev is not None and ws.n else None, int(n_bins),
                                                 C.byref(bs), C.byref(o), bases.ctypes.data if bases.size else None), "ivj_depth_profile")
        del keep
        return bases

    def depth_summary(self, probe, build, strict: bool, n_contigs: int, thresholds=(1,), partition_mode: int = 0, want_max: bool = True):
        """pb.depth_summary: -> (max_depth int32[n], bases_ge int64[K, n]): per probe row the largest number of build rows of its
        contig that cover one of its positions, and per threshold T = thresholds[k] the number of its positions covered by at
        least T build rows (row k of bases_ge, the caller's order).  want_max=False: thresholds only, max_depth comes back None."""
        ps, bs, keep = _host_sides(probe, build)
        o = make_opts(strict, n_contigs, partition_mode=partition_mode)
        thr = np.ascontiguousarray(np.asarray(list(thresholds), dtype=np.int64).astype(np.int32))
        k = int(thr.shape[0])
        md = np.empty(ps.n, np.int32) if want_max else None
        bg = np.empty((k, ps.n), np.int64)
        _check(self.L, self.L.ivj_depth_summary(self.h, C.byref(ps), C.byref(bs), C.byref(o), thr.ctypes.data if k else None, k,
                                                 md.ctypes.data if want_max else None, bg.ctypes.data if k else None), "ivj_depth_summary")
        del keep
        return md, bg

    def depth_hist(self, probe, build, strict: bool, n_contigs: int, max_depth: int, partition_mode: int = 0) -> np.ndarray:
        """pb.depth_histogram: -> int64 (n, max_depth + 1), probe order: bin d of a row = its positions that exactly d build rows of
        its contig cover, the last bin = max_depth or more; a row sums to its positions, bin 0 holds the uncovered ones."""
        ps, bs, keep = _host_sides(probe, build)
        o = make_opts(strict, n_contigs, partition_mode=partition_mode)
        max_depth = int(max_depth)
        # a depth the entry refuses gets no matrix: the entry checks max_depth before it looks at the output
        ok = 1 <= max_depth <= MAX_HIST_DEPTH
        hist = np.empty((ps.n, max_depth + 1 if ok else 0), np.int64)
        keep_h = hist if hist.size else np.empty(1, np.int64)        # (an array without elements still has to pass a non-NULL address)
        _check(self.L, self.L.ivj_depth_hist(self.h, C.byref(ps), C.byref(bs), C.byref(o), max_depth, keep_h.ctypes.data if ok else None),
               "ivj_depth_hist")
        del keep
        return hist

    def depth_hist_contigs(self, frame, strict: bool, n_contigs: int, max_depth: int) -> np.ndarray:
        """pb.genome_depth_histogram: -> int64 (n_contigs, max_depth + 1): bin d >= 1 of a contig = its positions that exactly d rows
        of the frame cover, the last bin = max_depth or more; bin 0 is 0 (the engine does not know a contig's length)."""
        fs, keep_f = _host_side(*frame)
        o = make_opts(strict, n_contigs)
        max_depth = int(max_depth)
        ok = 1 <= max_depth <= MAX_HIST_DEPTH
        hist = np.empty((int(n_contigs), max_depth + 1 if ok else 0), np.int64)
        keep = hist if hist.size else np.empty(1, np.int64)
        _check(self.L, self.L.ivj_depth_hist_contigs(self.h, C.byref(fs), C.byref(o), max_depth, keep.ctypes.data if ok else None),
               "ivj_depth_hist_contigs")
        del keep_f
        return hist

    def depth_quantiles(self, probe, build, strict: bool, n_contigs: int, ranks, partition_mode: int = 0) -> np.ndarray:
        """pb.depth_quantiles: ranks int64 (n, K), 0-based, K in 1 .. MAX_QUANT_RANKS -> int32 (n, K), probe order: cell (i, j) =
        the ranks[i, j]-th smallest depth of the build side over the positions of probe row i (uncovered positions count at
        depth 0); -1 for a rank outside [0, positions of the row) and for a row without a position or outside the dictionary."""
        ps, bs, keep = _host_sides(probe, build)
        o = make_opts(strict, n_contigs, partition_mode=partition_mode)
        ranks = np.ascontiguousarray(ranks, dtype=np.int64)
        if ranks.ndim != 2 or ranks.shape[0] != ps.n:
            raise ValueError(f"ranks must be an (n, K) matrix with one row per probe row, got shape {ranks.shape} for {ps.n} rows")
        k = ranks.shape[1]
        out = np.empty((ps.n, k), np.int32)
        # (an array without elements still has to pass a non-NULL address: the entry checks its pointers before the row count)
        keep_r = ranks if ranks.size else np.zeros(1, np.int64)
        keep_o = out if out.size else np.empty(1, np.int32)
        _check(self.L, self.L.ivj_depth_quantiles(self.h, C.byref(ps), C.byref(bs), C.byref(o), k, keep_r.ctypes.data, keep_o.ctypes.data),
               "ivj_depth_quantiles")
        del keep
        return out

    def _pieces(self, fn, name, a, b, strict, n_contigs, partition_mode=0):
        sa, sb, keep = _host_sides(a, b)
        o = make_opts(strict, n_contigs, partition_mode=partition_mode)
        out = _Pieces()
        _check(self.L, fn(self.h, C.byref(sa), C.byref(sb), C.byref(o), C.byref(out)), name)
        del keep
        return _copy_columns(out, ("row", "start", "end"), _I32x3, self.L.ivj_pieces_free)

    def subtract(self, left, right, strict: bool, n_contigs: int, partition_mode: int = 0):
        """pb.subtract: every left interval minus the union of the right ones -> (left row, start, end) pieces.
        partition_mode 0 auto / 1 bucket the left rows first / 2 never: same result, same order."""
        return self._pieces(self.L.ivj_subtract, "ivj_subtract", left, right, strict, n_contigs, partition_mode)

    def complement(self, frame, view, strict: bool, n_contigs: int, partition_mode: int = 0):
        """pb.complement: the gaps of ``frame`` inside every view interval -> (view row, start, end)."""
        return self._pieces(self.L.ivj_complement, "ivj_complement", frame, view, strict, n_contigs, partition_mode)

    def count_overlaps(self, probe, build, strict: bool, n_contigs: int, table_mode: int = 0, partition_mode: int = 0) -> np.ndarray:
        ps, bs, keep = _host_sides(probe, build)
        o = make_opts(strict, n_contigs, table_mode=table_mode, partition_mode=partition_mode)
        counts = np.empty(ps.n, np.int64)
        _check(self.L, self.L.ivj_count_overlaps(self.h, C.byref(ps), C.byref(bs), C.byref(o), counts.ctypes.data),
               "ivj_count_overlaps")
        del keep
        return counts

    def _host_thresholds(self, ps, bs, min_overlap, probe_min, build_min):
        pm, bm = _u32_min(probe_min, ps.n, "probe_min"), _u32_min(build_min, bs.n, "build_min")
        t = make_thresholds(min_overlap, pm.ctypes.data if pm is not None else 0, bm.ctypes.data if bm is not None else 0)
        return t, (pm, bm)

    def overlap_thresh(self, probe, build, strict: bool, n_contigs: int, min_overlap: int = 0, probe_min=None, build_min=None,
                       partition_mode: int = 0):
        """pb.overlap with overlap thresholds (ivj_overlap_thresh): the pairs with ov >= max(1, min_overlap, probe_min[probe row],
        build_min[build row]); the minima are uint32 base counts per row (0 none, THRESH_NEVER never) -> (probe_idx, build_idx)."""
        ps, bs, keep = _host_sides(probe, build)
        t, keep_t = self._host_thresholds(ps, bs, min_overlap, probe_min, build_min)
        o = make_opts(strict, n_contigs, partition_mode=partition_mode)
        out = _Pairs()
        _check(self.L, self.L.ivj_overlap_thresh(self.h, C.byref(ps), C.byref(bs), C.byref(o), C.byref(t), C.byref(out)), "ivj_overlap_thresh")
        del keep, keep_t
        return self._pairs_result(out)

    def count_overlaps_thresh(self, probe, build, strict: bool, n_contigs: int, min_overlap: int = 0, probe_min=None, build_min=None,
                              partition_mode: int = 0) -> np.ndarray:
        """pb.count_overlaps with overlap thresholds (ivj_count_overlaps_thresh): int64 per probe row, probe order kept."""
        ps, bs, keep = _host_sides(probe, build)
        t, keep_t = self._host_thresholds(ps, bs, min_overlap, probe_min, build_min)
        o = make_opts(strict, n_contigs, partition_mode=partition_mode)
        counts = np.zeros(ps.n, np.int64)
        _check(self.L, self.L.ivj_count_overlaps_thresh(self.h, C.byref(ps), C.byref(bs), C.byref(o), C.byref(t), counts.ctypes.data),
               "ivj_count_overlaps_thresh")
        del keep, keep_t
        return counts

    def _host_window(self, ps, left, right, probe_left, probe_right, min_distance):
        pl, pr = _u32_min(probe_left, ps.n, "probe_left"), _u32_min(probe_right, ps.n, "probe_right")
        w = make_window(left, right, pl.ctypes.data if pl is not None and ps.n else 0, pr.ctypes.data if pr is not None and ps.n else 0, min_distance)
        return w, (pl, pr)

    def overlap_window(self, probe, build, strict: bool, n_contigs: int, left: int = 0, right: int = 0, min_distance: int = 0,
                       probe_left=None, probe_right=None, distance: bool = True, partition_mode: int = 0):
        """pb.window (ivj_overlap_window): every build row within ``left`` bases before / ``right`` bases after each probe row (or the
        row's entry of the uint32 columns ``probe_left`` / ``probe_right``) and at least ``min_distance`` away; the semantics are
        those of include/ivjoin.h -> (probe_idx, build_idx, dist): dist the signed int64 distances (negative: the build row lies
        before the probe row), or None with ``distance=False``."""
        ps, bs, keep = _host_sides(probe, build)
        w, keep_w = self._host_window(ps, left, right, probe_left, probe_right, min_distance)
        o = make_opts(strict, n_contigs, partition_mode=partition_mode)
        out = _Pairs()
        dist = C.POINTER(C.c_int64)()
        _check(self.L, self.L.ivj_overlap_window(self.h, C.byref(ps), C.byref(bs), C.byref(o), C.byref(w), C.byref(out),
                                                 C.byref(dist) if distance else None), "ivj_overlap_window")
        del keep, keep_w
        n = out.n_pairs
        d = None
        if distance and n == 0:
            d = np.empty(0, np.int64)
        elif distance:
            buf = (C.c_int64 * n).from_address(C.addressof(dist.contents))
            buf._owner = _DistOwner(load_library(), dist)
            d = np.frombuffer(buf, dtype=np.int64)
        return (*self._pairs_result(out), d)

    def count_window(self, probe, build, strict: bool, n_contigs: int, left: int = 0, right: int = 0, min_distance: int = 0,
                     probe_left=None, probe_right=None, partition_mode: int = 0) -> np.ndarray:
        """pb.count_window (ivj_count_window): the number of pairs ``overlap_window`` reports per probe row, int64, probe order kept."""
        ps, bs, keep = _host_sides(probe, build)
        w, keep_w = self._host_window(ps, left, right, probe_left, probe_right, min_distance)
        o = make_opts(strict, n_contigs, partition_mode=partition_mode)
        counts = np.zeros(ps.n, np.int64)
        _check(self.L, self.L.ivj_count_window(self.h, C.byref(ps), C.byref(bs), C.byref(o), C.byref(w), counts.ctypes.data), "ivj_count_window")
        del keep, keep_w
        return counts

    def permute_overlaps(self, probe, build, strict: bool, n_contigs: int, contig_len, offsets, partition_mode: int = 0):
        """pb.permutation_test (ivj_permute_overlaps): ``contig_len`` int32[n_contigs] (>= 1), ``offsets`` int32[n_perm, n_contigs]
        with 0 <= offsets[p, c] < contig_len[c].  -> (n_pairs int64[n_perm], n_rows int64[n_perm]): per permutation the matches
        summed over the circularly shifted probe rows and their pieces, and the probe rows with a match (include/ivjoin.h)."""
        ps, bs, keep = _host_sides(probe, build)
        o = make_opts(strict, n_contigs, partition_mode=partition_mode)
        lens = np.ascontiguousarray(contig_len, dtype=np.int32).reshape(-1)
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        if off.ndim != 2 or off.shape[1] != n_contigs or lens.shape[0] != n_contigs:
            raise ValueError(f"offsets must be [n_perm, {n_contigs}] and contig_len [{n_contigs}], got {off.shape} and {lens.shape}")
        n_perm = int(off.shape[0])
        pairs, rows = np.zeros(n_perm, np.int64), np.zeros(n_perm, np.int64)
        _check(self.L, self.L.ivj_permute_overlaps(self.h, C.byref(ps), C.byref(bs), C.byref(o), lens.ctypes.data if n_contigs else None,
                                                   off.ctypes.data if off.size else None, n_perm, pairs.ctypes.data, rows.ctypes.data),
               "ivj_permute_overlaps")
        del keep
        return pairs, rows

    def _optional_thresholds(self, ps, bs, min_overlap, probe_min, build_min):
        """-> (pointer to an ivj_thresholds or None for the plain predicate, keep-alive)."""
        if not min_overlap and probe_min is None and build_min is None:
            return None, None
        t, keep = self._host_thresholds(ps, bs, min_overlap, probe_min, build_min)
        return C.byref(t), (t, keep)

    def _agg_columns(self, agg, n_build: int, shape):
        """The ivj_agg_in / ivj_agg_out arrays of a host call: ``agg`` = a list of (values, valid, ops) per value column of the build
        side; every result array has ``shape``.  -> (n_cols, cols, outs, results, keep-alive)."""
        agg = list(agg)
        cols = (_AggIn * max(len(agg), 1))()
        outs = (_AggOut * max(len(agg), 1))()
        keep, results = [], []
        size = int(np.prod(shape))
        for k, (values, valid, ops) in enumerate(agg):
            cols[k], values, arrays = _agg_in(values, valid, ops, n_build)
            keep.append(arrays)
            kinds = {"sum": values.dtype, "min": values.dtype, "max": values.dtype, "mean": np.float64, "count": np.int64}
            res = {name: np.zeros(shape, kinds[name]) for name, bit in AGG_OPS.items() if cols[k].ops & bit}
            outs[k] = _AggOut(*(res[name].ctypes.data if name in res and size else None for name in ("sum", "min", "max", "mean", "count")))
            results.append(res)
        return len(agg), cols, outs, results, keep

    def overlap_agg(self, probe, build, strict: bool, n_contigs: int, agg, min_overlap: int = 0, probe_min=None, build_min=None,
                    partition_mode: int = 0):
        """pb.map_overlaps (ivj_overlap_agg): ``agg`` = a list of (values, valid, ops) per value column of the BUILD side, as in
        ``merge_agg``.  Every probe row reduces the valid values of the build rows it matches -- under the plain predicate, or the
        thresholded one when min_overlap / probe_min / build_min are given -> [dict per column] mapping each requested name to an
        array of one entry per probe row, probe order kept: sum int64 (wrapped) / float64, min / max the column's type, mean
        float64, count int64.  sum and count are 0 where nothing valid matches; min / max / mean are unspecified there."""
        return self._overlap_agg_call("ivj_overlap_agg", probe, build, strict, n_contigs, agg, min_overlap, probe_min, build_min, partition_mode)

    def overlap_wagg(self, probe, build, strict: bool, n_contigs: int, agg, min_overlap: int = 0, probe_min=None, build_min=None,
                     partition_mode: int = 0):
        """pb.signal_summary (ivj_overlap_wagg): as ``overlap_agg``, but a build row contributes iff it shares ov >= max(1, minima)
        positions with the probe row, and then weighs ov: ``count`` receives the bases (sum of ov), ``sum`` the sum of value * ov
        (int64 wrapped / float64), ``mean`` = sum / bases; ``min`` / ``max`` are over the contributing values, unweighted."""
        return self._overlap_agg_call("ivj_overlap_wagg", probe, build, strict, n_contigs, agg, min_overlap, probe_min, build_min, partition_mode)

    def _overlap_agg_call(self, entry, probe, build, strict, n_contigs, agg, min_overlap, probe_min, build_min, partition_mode):
        ps, bs, keep = _host_sides(probe, build)
        t, keep_t = self._optional_thresholds(ps, bs, min_overlap, probe_min, build_min)
        o = make_opts(strict, n_contigs, partition_mode=partition_mode)
        k, cols, outs, results, keep_a = self._agg_columns(agg, bs.n, (ps.n,))
        _check(self.L, getattr(self.L, entry)(self.h, C.byref(ps), C.byref(bs), C.byref(o), t, k, cols, outs), entry)
        del keep, keep_t, keep_a
        return results

    def overlap_quantiles(self, probe, build, strict: bool, n_contigs: int, values, valid, q, upper, min_overlap: int = 0, probe_min=None,
                          build_min=None, partition_mode: int = 0):
        """pb.map_quantiles (ivj_overlap_quantiles): ``values`` (int64 / float64) and ``valid`` (or None) = ONE value column of the
        BUILD side; ``q`` = 1 .. MAX_OVQ_RANKS floats in [0, 1] and ``upper`` = one flag per q, shared by all rows.  Every probe row
        sorts the valid values of the build rows it matches (predicate as ``overlap_agg``; int64 signed, doubles as np.sort with
        NaN last) and answers v[floor(q (m - 1))], or v[ceil(q (m - 1))] where ``upper`` is set -> (out (n, n_q) in the values'
        dtype, count int64 (n,) = m), probe order kept; a row with m == 0 holds zeros."""
        ps, bs, keep = _host_sides(probe, build)
        t, keep_t = self._optional_thresholds(ps, bs, min_overlap, probe_min, build_min)
        o = make_opts(strict, n_contigs, partition_mode=partition_mode)
        col, values, keep_a = _agg_in(values, valid, AGG_COUNT, bs.n)
        qs, up = _quantile_requests(q, upper)
        n_q = len(qs)
        out = np.zeros((ps.n, n_q if 1 <= n_q <= MAX_OVQ_RANKS else 0), values.dtype)
        count = np.zeros(ps.n, np.int64)
        _check(self.L, self.L.ivj_overlap_quantiles(self.h, C.byref(ps), C.byref(bs), C.byref(o), t, C.byref(col), n_q, qs.ctypes.data,
                                                    up.ctypes.data, out.ctypes.data if out.size else None,
                                                    count.ctypes.data if ps.n else None), "ivj_overlap_quantiles")
        del keep, keep_t, keep_a
        return out, count

    def signal_profile(self, windows, reverse, n_bins: int, build, strict: bool, n_contigs: int, agg):
        """pb.signal_profile (ivj_signal_profile): every window row cut into n_bins bins as by ``depth_profile``, every bin a probe of
        ``overlap_wagg`` without thresholds -> [dict per column] of (n, n_bins) arrays, window order; ``reverse``: None or one flag
        per window, a flagged row comes back right to left."""
        ws, bs, keep = _host_sides(windows, build)
        o = make_opts(strict, n_contigs)
        rev = _reverse_flags(reverse, ws.n)
        n_bins = int(n_bins)
        # a bin count the entry refuses gets no matrix: the entry checks n_bins before it looks at the outputs
        k, cols, outs, results, keep_a = self._agg_columns(agg, bs.n, (ws.n, n_bins if 1 <= n_bins <= DEPTH_PROFILE_MAX_BINS else 0))
        _check(self.L, self.L.ivj_signal_profile(self.h, C.byref(ws), rev.ctypes.data if rev is not None and ws.n else None, n_bins,
                                                  C.byref(bs), C.byref(o), k, cols, outs), "ivj_signal_profile")
        del keep, keep_a
        return results

    def overlap_select(self, probe, build, strict: bool, n_contigs: int, mode, min_overlap: int = 0, probe_min=None, build_min=None,
                       partition_mode: int = 0) -> np.ndarray:
        """Semi / anti join (ivj_overlap_select): the probe rows with at least one (mode "semi" / SELECT_SEMI) or no (mode "anti" /
        SELECT_ANTI) build row under the predicate -- the plain one, or the thresholded one when min_overlap / probe_min / build_min
        are given -- as an ascending int32 array.  The counts stay on the device; no pair is enumerated."""
        mode = select_mode(mode)
        ps, bs, keep = _host_sides(probe, build)
        t, keep_t = self._optional_thresholds(ps, bs, min_overlap, probe_min, build_min)
        o = make_opts(strict, n_contigs, partition_mode=partition_mode)
        out = _RowSel()
        _check(self.L, self.L.ivj_overlap_select(self.h, C.byref(ps), C.byref(bs), C.byref(o), t, mode, C.byref(out)), "ivj_overlap_select")
        del keep, keep_t
        return _copy_columns(out, ("rows",), (np.int32,), self.L.ivj_rowsel_free)[0]

    def overlap_outer(self, probe, build, strict: bool, n_contigs: int, min_overlap: int = 0, probe_min=None, build_min=None,
                      partition_mode: int = 0):
        """Left outer join (ivj_overlap_outer): the inner pairs as ``overlap`` (``overlap_thresh`` with thresholds) returns them,
        then (row, -1) for every probe row without a match, ascending -> (probe_idx, build_idx)."""
        ps, bs, keep = _host_sides(probe, build)
        t, keep_t = self._optional_thresholds(ps, bs, min_overlap, probe_min, build_min)
        o = make_opts(strict, n_contigs, partition_mode=partition_mode)
        out = _Pairs()
        _check(self.L, self.L.ivj_overlap_outer(self.h, C.byref(ps), C.byref(bs), C.byref(o), t, C.byref(out)), "ivj_overlap_outer")
        del keep, keep_t
        return self._pairs_result(out)

    def nearest(self, probe, build, strict: bool, n_contigs: int, k: int = 1, include_overlaps: bool = True,
                table_mode: int = 0, partition_mode: int = 0, nearest_ignore: int = 0):
        """partition_mode 0 auto / 1 bucket the probe side first / 2 never: same result, probe order kept.
        nearest_ignore: NEAREST_IGNORE_LEFT (1) leaves out the rows before the probe, NEAREST_IGNORE_RIGHT (2) the rows after it
        (overlapping rows always count); the rest of the ordered candidate list, cut to k."""
        ps, bs, keep = _host_sides(probe, build)
        if k < 1:
            raise ValueError("k must be >= 1")
        o = make_opts(strict, n_contigs, k, include_overlaps, table_mode=table_mode, partition_mode=partition_mode, nearest_ignore=nearest_ignore)
        idx = np.empty((ps.n, k), np.int32)
        dist = np.empty((ps.n, k), np.int64)
        nf = np.empty(ps.n, np.int32)
        _check(self.L, self.L.ivj_nearest(self.h, C.byref(ps), C.byref(bs), C.byref(o), idx.ctypes.data,
                                           dist.ctypes.data, nf.ctypes.data), "ivj_nearest")
        del keep
        return idx, dist, nf

    # ---- device-resident entry points (raw device pointers) -----------------
    def set_stream(self, hip_stream: Optional[int]):
        """hipStream_t handle as an int (0 = the legacy default stream torch uses); None restores
        the engine's own stream."""
        h = C.c_void_p(-1) if hip_stream is None else C.c_void_p(hip_stream)
        _check(self.L, self.L.ivj_ctx_set_stream(self.h, h), "ivj_ctx_set_stream")

    def sync(self):
        _check(self.L, self.L.ivj_ctx_sync(self.h), "ivj_ctx_sync")

    def enable_timing(self, level: int = 2):
        """0 off, 1 probe kernels only, 2 every kernel (HIP events on the launch stream)."""
        _check(self.L, self.L.ivj_ctx_enable_timing(self.h, int(level)), "ivj_ctx_enable_timing")

    def profile_mark(self):
        """An empty marker kernel on the context's stream (step boundary for a profiler)."""
        _check(self.L, self.L.ivj_ctx_profile_mark(self.h), "ivj_ctx_profile_mark")

    def timings(self) -> dict:
        arr = (_Timing * 64)()
        n = C.c_int(0)
        _check(self.L, self.L.ivj_ctx_get_timings(self.h, arr, 64, C.byref(n)), "ivj_ctx_get_timings")
        return {arr[i].name.decode(): {"launches": arr[i].launches, "ms": arr[i].ms} for i in range(min(n.value, 64))}

    @staticmethod
    def dev_side(contig_ptr: int, start_ptr: int, end_ptr: int, n: int, row_id_ptr: int = 0) -> _Side:
        return _Side(contig_ptr or None, start_ptr or None, end_ptr or None, n, row_id_ptr or None)

    def index_build_dev(self, build: _Side, opts: _Opts, with_end_order: bool = False, sweep_only: bool = False) -> DeviceIndex:
        """sweep_only: index for merge_dev / cluster_dev only (no lookup tables)."""
        h = C.c_void_p()
        with_end_order = int(bool(with_end_order)) | (2 if sweep_only else 0)
        _check(self.L, self.L.ivj_index_build_dev(self.h, C.byref(build), C.byref(opts), int(with_end_order), C.byref(h)),
               "ivj_index_build_dev")
        return DeviceIndex(self, h, build.n)

    def overlap_count_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts) -> int:
        n = C.c_int64(0)
        _check(self.L, self.L.ivj_overlap_count_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), C.byref(n)),
               "ivj_overlap_count_dev")
        return n.value

    def overlap_fill_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts, probe_idx_ptr: int, build_idx_ptr: int,
                         capacity: int):
        _check(self.L, self.L.ivj_overlap_fill_dev(self.h, ix.handle, C.byref(probe), C.byref(opts),
                                                    C.c_void_p(probe_idx_ptr), C.c_void_p(build_idx_ptr), capacity),
               "ivj_overlap_fill_dev")

    def overlap_fused_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts, probe_idx_ptr: int, build_idx_ptr: int,
                          capacity: int):
        """-> (n_pairs, fits).  fits=False: nothing usable was written, grow the buffers to n_pairs."""
        n = C.c_int64(0)
        rc = self.L.ivj_overlap_fused_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), C.c_void_p(probe_idx_ptr),
                                          C.c_void_p(build_idx_ptr), capacity, C.byref(n))
        if rc == -4:      # IVJ_ECAPACITY
            return n.value, False
        _check(self.L, rc, "ivj_overlap_fused_dev")
        return n.value, True

    def overlap_thresh_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts, thr: _Thresholds, probe_idx_ptr: int, build_idx_ptr: int,
                           capacity: int):
        """Thresholded join on an index (ivj_overlap_thresh_dev; thr from make_thresholds with device addresses) -> (n_pairs, fits).
        fits=False: nothing was written, grow the buffers to n_pairs.  Null buffers with capacity 0 count only."""
        n = C.c_int64(0)
        rc = self.L.ivj_overlap_thresh_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), C.byref(thr), C.c_void_p(probe_idx_ptr or None),
                                           C.c_void_p(build_idx_ptr or None), capacity, C.byref(n))
        if rc == IVJ_ECAPACITY:
            return n.value, False
        _check(self.L, rc, "ivj_overlap_thresh_dev")
        return n.value, True

    def count_overlaps_thresh_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts, thr: _Thresholds, counts_ptr: int):
        _check(self.L, self.L.ivj_count_overlaps_thresh_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), C.byref(thr),
                                                            C.c_void_p(counts_ptr)), "ivj_count_overlaps_thresh_dev")

    def overlap_window_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts, win: _Window, probe_idx_ptr: int, build_idx_ptr: int, dist_ptr: int,
                           capacity: int):
        """Distance-window join on an index (ivj_overlap_window_dev; win from make_window with device addresses) -> (n_pairs, fits).
        fits=False: nothing was written, grow the buffers to n_pairs.  Null buffers with capacity 0 count only; dist_ptr 0 = no
        distance column."""
        n = C.c_int64(0)
        rc = self.L.ivj_overlap_window_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), C.byref(win), C.c_void_p(probe_idx_ptr or None),
                                           C.c_void_p(build_idx_ptr or None), C.c_void_p(dist_ptr or None), capacity, C.byref(n))
        if rc == IVJ_ECAPACITY:
            return n.value, False
        _check(self.L, rc, "ivj_overlap_window_dev")
        return n.value, True

    def count_window_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts, win: _Window, counts_ptr: int):
        _check(self.L, self.L.ivj_count_window_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), C.byref(win), C.c_void_p(counts_ptr)),
               "ivj_count_window_dev")

    def overlap_select_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts, thr: Optional[_Thresholds], mode: int, rows_ptr: int,
                           pad_ptr: int, capacity: int):
        """Semi / anti selection on an index (ivj_overlap_select_dev; thr from make_thresholds with device addresses, or None for the
        plain predicate) -> (n_rows, fits).  fits=False: nothing was written, grow the buffers to n_rows.  Null buffers with capacity
        0 count only.  pad_ptr (0 = none) receives -1 wherever rows_ptr receives a row."""
        n = C.c_int64(0)
        rc = self.L.ivj_overlap_select_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), C.byref(thr) if thr is not None else None,
                                           int(mode), C.c_void_p(rows_ptr or None), C.c_void_p(pad_ptr or None), capacity, C.byref(n))
        if rc == IVJ_ECAPACITY:
            return n.value, False
        _check(self.L, rc, "ivj_overlap_select_dev")
        return n.value, True

    def materialize_dev(self, probe: _Side, build: _Side, n_pairs: int, probe_idx_ptr: int, build_idx_ptr: int,
                        contig_ptr: int = 0, start_1_ptr: int = 0, end_1_ptr: int = 0, start_2_ptr: int = 0, end_2_ptr: int = 0):
        """ivj_materialize_dev: gather the key columns of both sides for every pair (device pointers;
        0 skips a column)."""
        r = _Rows()
        r.n_pairs = int(n_pairs)
        for name, ptr in zip(ROW_COLUMNS, (probe_idx_ptr, build_idx_ptr, contig_ptr, start_1_ptr, end_1_ptr, start_2_ptr, end_2_ptr)):
            setattr(r, name, C.cast(C.c_void_p(ptr or None), C.POINTER(C.c_int32)))
        _check(self.L, self.L.ivj_materialize_dev(self.h, C.byref(probe), C.byref(build), C.byref(r)), "ivj_materialize_dev")

    def overlap_fused_rows_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts, capacity: int, probe_idx_ptr: int = 0,
                               build_idx_ptr: int = 0, contig_ptr: int = 0, start_1_ptr: int = 0, end_1_ptr: int = 0,
                               start_2_ptr: int = 0, end_2_ptr: int = 0):
        """ivj_overlap_fused_rows_dev: join + key-column materialisation in one pass.  -> (n_rows, fits)."""
        r = _Rows()
        r.n_pairs = int(capacity)
        for name, ptr in zip(ROW_COLUMNS, (probe_idx_ptr, build_idx_ptr, contig_ptr, start_1_ptr, end_1_ptr, start_2_ptr, end_2_ptr)):
            setattr(r, name, C.cast(C.c_void_p(ptr or None), C.POINTER(C.c_int32)))
        n = C.c_int64(0)
        rc = self.L.ivj_overlap_fused_rows_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), C.byref(r), C.byref(n))
        if rc == -4:      # IVJ_ECAPACITY
            return n.value, False
        _check(self.L, rc, "ivj_overlap_fused_rows_dev")
        return n.value, True

    def take_dev(self, src_ptr: int, elem_bytes: int, idx_ptr: int, n: int, dst_ptr: int, validity_ptr: int = 0):
        """ivj_take_dev: Arrow take of one 4- or 8-byte device column; negative indices -> 0 / null bit."""
        _check(self.L, self.L.ivj_take_dev(self.h, C.c_void_p(src_ptr), int(elem_bytes), C.c_void_p(idx_ptr), int(n),
                                            C.c_void_p(dst_ptr), C.c_void_p(validity_ptr or None)), "ivj_take_dev")

    def group_ids_dev(self, probe_contig_ptr: int, probe_code_ptrs, n_probe: int, build_contig_ptr: int, build_code_ptrs, n_build: int,
                      cards, n_contigs: int, probe_gid_ptr: int, build_gid_ptr: int, keys_ptr: int, keys_cap: int) -> int:
        """ivj_group_ids_dev (device pointers; the code pointer lists and ``cards`` are host values) -> number of groups."""
        k = len(cards)
        cards_a = (C.c_int32 * max(k, 1))(*[int(c) for c in cards])
        pc = (C.c_void_p * max(k, 1))(*[C.c_void_p(int(p)) for p in probe_code_ptrs])
        bc = (C.c_void_p * max(k, 1))(*[C.c_void_p(int(p)) for p in build_code_ptrs])
        g = C.c_int32(0)
        _check(self.L, self.L.ivj_group_ids_dev(self.h, C.c_void_p(probe_contig_ptr or None), C.cast(pc, C.POINTER(C.c_void_p)), int(n_probe),
                                                 C.c_void_p(build_contig_ptr or None), C.cast(bc, C.POINTER(C.c_void_p)), int(n_build), k,
                                                 C.cast(cards_a, C.c_void_p), int(n_contigs), C.c_void_p(probe_gid_ptr or None),
                                                 C.c_void_p(build_gid_ptr or None), C.c_void_p(keys_ptr or None), int(keys_cap), C.byref(g)),
               "ivj_group_ids_dev")
        return g.value

    def cluster_dev(self, ix: DeviceIndex, opts: _Opts, min_dist: int, cluster_ptr: int, start_ptr: int, end_ptr: int) -> int:
        n = C.c_int64(0)
        _check(self.L, self.L.ivj_cluster_dev(self.h, ix.handle, C.byref(opts), int(min_dist), C.c_void_p(cluster_ptr),
                                               C.c_void_p(start_ptr), C.c_void_p(end_ptr), C.byref(n)), "ivj_cluster_dev")
        return n.value

    def merge_dev(self, ix: DeviceIndex, opts: _Opts, min_dist: int, capacity: int, contig_ptr: int, start_ptr: int, end_ptr: int,
                  n_intervals_ptr: int):
        """-> (n_merged, fits)"""
        n = C.c_int64(0)
        rc = self.L.ivj_merge_dev(self.h, ix.handle, C.byref(opts), int(min_dist), int(capacity), C.c_void_p(contig_ptr or None),
                                  C.c_void_p(start_ptr or None), C.c_void_p(end_ptr or None), C.c_void_p(n_intervals_ptr or None), C.byref(n))
        if rc == -4:
            return n.value, False
        _check(self.L, rc, "ivj_merge_dev")
        return n.value, True

    def merge_agg_dev(self, ix: DeviceIndex, opts: _Opts, min_dist: int, capacity: int, contig_ptr: int, start_ptr: int, end_ptr: int,
                      n_intervals_ptr: int, n_values: int, cols, outs):
        """ivj_merge_agg_dev.  ``cols``: per value column (values_ptr, valid_ptr or 0, dtype AGG_I64 / AGG_F64, ops mask);
        ``outs``: per value column a dict name -> device address of the caller's column (names of AGG_OPS; missing = NULL).
        -> (n_merged, fits); fits=False: nothing was written, grow the buffers to n_merged."""
        k = len(cols)
        cin = (_AggIn * max(k, 1))()
        cout = (_AggOut * max(k, 1))()
        for i, (values_ptr, valid_ptr, dtype, ops) in enumerate(cols):
            cin[i] = _AggIn(values_ptr or None, valid_ptr or None, int(dtype), int(ops))
            cout[i] = _AggOut(*(outs[i].get(name) or None for name in ("sum", "min", "max", "mean", "count")))
        n = C.c_int64(0)
        rc = self.L.ivj_merge_agg_dev(self.h, ix.handle, C.byref(opts), int(min_dist), int(capacity), C.c_void_p(contig_ptr or None),
                                      C.c_void_p(start_ptr or None), C.c_void_p(end_ptr or None), C.c_void_p(n_intervals_ptr or None),
                                      int(n_values), k, cin, cout, C.byref(n))
        if rc == IVJ_ECAPACITY:
            return n.value, False
        _check(self.L, rc, "ivj_merge_agg_dev")
        return n.value, True

    def overlap_agg_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts, thr: Optional[_Thresholds], n_values: int, cols, outs):
        """ivj_overlap_agg_dev; ``thr`` None = the plain predicate.  ``cols`` / ``outs`` as in ``merge_agg_dev``, the value columns
        being the build side's and every output column holding probe.n entries."""
        k = len(cols)
        cin = (_AggIn * max(k, 1))()
        cout = (_AggOut * max(k, 1))()
        for i, (values_ptr, valid_ptr, dtype, ops) in enumerate(cols):
            cin[i] = _AggIn(values_ptr or None, valid_ptr or None, int(dtype), int(ops))
            cout[i] = _AggOut(*(outs[i].get(name) or None for name in ("sum", "min", "max", "mean", "count")))
        _check(self.L, self.L.ivj_overlap_agg_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), C.byref(thr) if thr is not None else None,
                                                  int(n_values), k, cin, cout), "ivj_overlap_agg_dev")

    def overlap_quantiles_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts, thr: Optional[_Thresholds], n_values: int, col, q, upper,
                              out_ptr: int, count_ptr: int):
        """ivj_overlap_quantiles_dev; ``thr`` None = the plain predicate.  ``col`` = (values_ptr, valid_ptr or 0, dtype AGG_I64 /
        AGG_F64) of the build side's value column; ``q`` / ``upper`` are host sequences; ``out_ptr``: probe.n x len(q) elements of
        the column's type, ``count_ptr``: probe.n int64 or 0."""
        values_ptr, valid_ptr, dtype = col
        cin = _AggIn(values_ptr or None, valid_ptr or None, int(dtype), 0)
        qs, up = _quantile_requests(q, upper)
        _check(self.L, self.L.ivj_overlap_quantiles_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), C.byref(thr) if thr is not None else None,
                                                        int(n_values), C.byref(cin), len(qs), qs.ctypes.data, up.ctypes.data,
                                                        C.c_void_p(out_ptr or None), C.c_void_p(count_ptr or None)), "ivj_overlap_quantiles_dev")

    def overlap_wagg_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts, thr: Optional[_Thresholds], n_values: int, cols, outs):
        """ivj_overlap_wagg_dev; ``thr`` None = every row that shares a position.  Arguments as ``overlap_agg_dev``; the ``count``
        column receives the bases."""
        k = len(cols)
        cin = (_AggIn * max(k, 1))()
        cout = (_AggOut * max(k, 1))()
        for i, (values_ptr, valid_ptr, dtype, ops) in enumerate(cols):
            cin[i] = _AggIn(values_ptr or None, valid_ptr or None, int(dtype), int(ops))
            cout[i] = _AggOut(*(outs[i].get(name) or None for name in ("sum", "min", "max", "mean", "count")))
        _check(self.L, self.L.ivj_overlap_wagg_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), C.byref(thr) if thr is not None else None,
                                                   int(n_values), k, cin, cout), "ivj_overlap_wagg_dev")

    def signal_profile_dev(self, ix: DeviceIndex, windows: _Side, reverse_ptr: int, n_bins: int, opts: _Opts, n_values: int, cols, outs):
        """ivj_signal_profile_dev.  ``cols`` / ``outs`` as in ``overlap_wagg_dev``, every output a row-major windows.n x n_bins matrix."""
        k = len(cols)
        cin = (_AggIn * max(k, 1))()
        cout = (_AggOut * max(k, 1))()
        for i, (values_ptr, valid_ptr, dtype, ops) in enumerate(cols):
            cin[i] = _AggIn(values_ptr or None, valid_ptr or None, int(dtype), int(ops))
            cout[i] = _AggOut(*(outs[i].get(name) or None for name in ("sum", "min", "max", "mean", "count")))
        _check(self.L, self.L.ivj_signal_profile_dev(self.h, ix.handle, C.byref(windows), C.c_void_p(reverse_ptr or None), int(n_bins),
                                                     C.byref(opts), int(n_values), k, cin, cout), "ivj_signal_profile_dev")

    def depth_dev(self, ix: DeviceIndex, opts: _Opts, capacity: int, contig_ptr: int, start_ptr: int, end_ptr: int, depth_ptr: int):
        """-> (n_blocks, fits).  fits=False: nothing was written, grow the buffers to n_blocks."""
        n = C.c_int64(0)
        rc = self.L.ivj_depth_dev(self.h, ix.handle, C.byref(opts), int(capacity), C.c_void_p(contig_ptr or None),
                                  C.c_void_p(start_ptr or None), C.c_void_p(end_ptr or None), C.c_void_p(depth_ptr or None), C.byref(n))
        if rc == -4:
            return n.value, False
        _check(self.L, rc, "ivj_depth_dev")
        return n.value, True

    def setop_dev(self, ix_a: DeviceIndex, ix_b: DeviceIndex, opts: _Opts, op, capacity: int, contig_ptr: int, start_ptr: int, end_ptr: int):
        """-> (n_regions, fits).  fits=False: nothing was written, grow the buffers to n_regions."""
        n = C.c_int64(0)
        rc = self.L.ivj_setop_dev(self.h, ix_a.handle, ix_b.handle, C.byref(opts), _setop_code(op), int(capacity),
                                  C.c_void_p(contig_ptr or None), C.c_void_p(start_ptr or None), C.c_void_p(end_ptr or None), C.byref(n))
        if rc == -4:
            return n.value, False
        _check(self.L, rc, "ivj_setop_dev")
        return n.value, True

    def multi_inter_dev(self, indexes, opts: _Opts, min_frames: int, mode: int, capacity: int, contig_ptr: int, start_ptr: int, end_ptr: int,
                        mask_ptr: int):
        """-> (n, fits).  fits=False: nothing was written, grow the buffers to n.  ``indexes``: one DeviceIndex (or None = an empty
        frame) per frame; ``mask_ptr`` may be 0 for MULTI_CONSENSUS."""
        indexes = list(indexes)
        min_frames = check_multi(len(indexes), min_frames, mode)
        handles = (C.c_void_p * len(indexes))(*(None if ix is None else getattr(ix.handle, "value", ix.handle) for ix in indexes))
        n = C.c_int64(0)
        rc = self.L.ivj_multi_inter_dev(self.h, handles, len(indexes), C.byref(opts), min_frames, int(mode), int(capacity),
                                        C.c_void_p(contig_ptr or None), C.c_void_p(start_ptr or None), C.c_void_p(end_ptr or None),
                                        C.c_void_p(mask_ptr or None), C.byref(n))
        if rc == -4:
            return n.value, False
        _check(self.L, rc, "ivj_multi_inter_dev")
        return n.value, True

    def multi_pairwise_dev(self, indexes, opts: _Opts, bases_ptr: int, runs_ptr: int):
        """``indexes``: one DeviceIndex (or None = an empty frame) per frame; the pointers: F * F int64 each in HBM, row-major."""
        indexes = list(indexes)
        check_multi(len(indexes), 1)
        handles = (C.c_void_p * len(indexes))(*(None if ix is None else getattr(ix.handle, "value", ix.handle) for ix in indexes))
        _check(self.L, self.L.ivj_multi_pairwise_dev(self.h, handles, len(indexes), C.byref(opts), C.c_void_p(bases_ptr or None),
                                                     C.c_void_p(runs_ptr or None)), "ivj_multi_pairwise_dev")

    def set_stats_dev(self, ix_a: DeviceIndex, ix_b: DeviceIndex, opts: _Opts):
        """-> (only_a, only_b, both, n_intersections)"""
        bases = (C.c_int64 * 3)()
        ni = C.c_int64(0)
        _check(self.L, self.L.ivj_set_stats_dev(self.h, ix_a.handle, ix_b.handle, C.byref(opts), bases, C.byref(ni)), "ivj_set_stats_dev")
        return int(bases[0]), int(bases[1]), int(bases[2]), int(ni.value)

    def subtract_dev(self, right_ix: DeviceIndex, left: _Side, opts: _Opts, capacity: int, row_ptr: int, start_ptr: int, end_ptr: int):
        """-> (n_pieces, fits)"""
        n = C.c_int64(0)
        rc = self.L.ivj_subtract_dev(self.h, right_ix.handle, C.byref(left), C.byref(opts), int(capacity), C.c_void_p(row_ptr or None),
                                     C.c_void_p(start_ptr or None), C.c_void_p(end_ptr or None), C.byref(n))
        if rc == -4:
            return n.value, False
        _check(self.L, rc, "ivj_subtract_dev")
        return n.value, True

    def coverage_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts, coverage_ptr: int):
        _check(self.L, self.L.ivj_coverage_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), C.c_void_p(coverage_ptr)),
               "ivj_coverage_dev")

    def depth_summary_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts, thresholds, max_depth_ptr: int, bases_ge_ptr: int):
        """thresholds: host ints; max_depth_ptr / bases_ge_ptr: device addresses (0 = NULL) of int32[n] / column-major int64[K, n]."""
        thr = np.ascontiguousarray(np.asarray(list(thresholds), dtype=np.int64).astype(np.int32))
        k = int(thr.shape[0])
        _check(self.L, self.L.ivj_depth_summary_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), thr.ctypes.data if k else None, k,
                                                     C.c_void_p(max_depth_ptr or None), C.c_void_p(bases_ge_ptr or None)), "ivj_depth_summary_dev")

    def depth_hist_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts, max_depth: int, hist_ptr: int):
        """hist_ptr: device address (0 = NULL) of row-major int64[n, max_depth + 1]."""
        _check(self.L, self.L.ivj_depth_hist_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), int(max_depth), C.c_void_p(hist_ptr or None)),
               "ivj_depth_hist_dev")

    def depth_hist_contigs_dev(self, ix: DeviceIndex, opts: _Opts, max_depth: int, hist_ptr: int):
        """hist_ptr: device address (0 = NULL) of row-major int64[n_contigs, max_depth + 1]."""
        _check(self.L, self.L.ivj_depth_hist_contigs_dev(self.h, ix.handle, C.byref(opts), int(max_depth), C.c_void_p(hist_ptr or None)),
               "ivj_depth_hist_contigs_dev")

    def depth_quantiles_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts, n_ranks: int, ranks_ptr: int, out_ptr: int):
        """ranks_ptr / out_ptr: device addresses (0 = NULL) of row-major int64[n, n_ranks] and int32[n, n_ranks]."""
        _check(self.L, self.L.ivj_depth_quantiles_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), int(n_ranks), C.c_void_p(ranks_ptr or None),
                                                       C.c_void_p(out_ptr or None)), "ivj_depth_quantiles_dev")

    def permute_overlaps_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts, contig_len_ptr: int, offsets_ptr: int, n_perm: int,
                             n_pairs_ptr: int, n_rows_ptr: int):
        """ivj_permute_overlaps_dev: device addresses of int32[n_contigs], int32[n_perm, n_contigs] and two int64[n_perm] outputs."""
        _check(self.L, self.L.ivj_permute_overlaps_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), C.c_void_p(contig_len_ptr or None),
                                                       C.c_void_p(offsets_ptr or None), int(n_perm), C.c_void_p(n_pairs_ptr or None),
                                                       C.c_void_p(n_rows_ptr or None)), "ivj_permute_overlaps_dev")

    def overlap_bases_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts, bases_ptr: int):
        _check(self.L, self.L.ivj_overlap_bases_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), C.c_void_p(bases_ptr)),
               "ivj_overlap_bases_dev")

    def depth_profile_dev(self, ix: DeviceIndex, windows: _Side, reverse_ptr: int, n_bins: int, opts: _Opts, bases_ptr: int):
        """reverse_ptr: device address of one byte per window (0 = NULL: none reversed); bases_ptr: row-major int64[n, n_bins]."""
        _check(self.L, self.L.ivj_depth_profile_dev(self.h, ix.handle, C.byref(windows), C.c_void_p(reverse_ptr or None), int(n_bins),
                                                     C.byref(opts), C.c_void_p(bases_ptr or None)), "ivj_depth_profile_dev")

    def count_overlaps_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts, counts_ptr: int):
        _check(self.L, self.L.ivj_count_overlaps_dev(self.h, ix.handle, C.byref(probe), C.byref(opts),
                                                      C.c_void_p(counts_ptr)), "ivj_count_overlaps_dev")

    def nearest_dev(self, ix: DeviceIndex, probe: _Side, opts: _Opts, idx_ptr: int, dist_ptr: int, nf_ptr: int):
        _check(self.L, self.L.ivj_nearest_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), C.c_void_p(idx_ptr),
                                               C.c_void_p(dist_ptr), C.c_void_p(nf_ptr)), "ivj_nearest_dev")

    # ---- streaming: build side resident, probe side in bounded batches ---------
    def probe_stream(self, build, strict: bool, n_contigs: int, op: int = STREAM_OVERLAP, max_batch_rows: int = 8_000_000, k: int = 1,
                     include_overlaps: bool = True, partition_mode: int = 0, copy: bool = True, nearest_ignore: int = 0) -> ProbeStream:
        """Open a streaming probe session (ivj_stream_open): see ProbeStream."""
        return ProbeStream(self, build, strict, n_contigs, op, max_batch_rows, k, include_overlaps, partition_mode, copy, nearest_ignore)

    def overlap_batches(self, probe, build, strict: bool, n_contigs: int, batch_rows: int = 8_000_000):
        """Generator of (probe_idx, build_idx) numpy batches over a probe side that is already in host arrays.

        The build side is sorted once and stays in HBM; the probe side goes through the device in batches of
        ``batch_rows`` rows with H2D / join / D2H of consecutive batches overlapped (ProbeStream), so device memory and
        the size of every result batch are bounded (the reference's streaming probe side + ``low_memory``:
        docs/developers.md:641-646, polars_bio/range_op.py:168).  probe_idx are rows of the WHOLE probe side."""
        pc, ps, pe = (_i32(a) for a in probe)
        n = pc.shape[0]
        if n == 0 or len(build[0]) == 0:
            return
        rows = int(min(batch_rows, n))
        with self.probe_stream(build, strict, n_contigs, STREAM_OVERLAP, rows, copy=False) as st:
            def emit(res):
                lo = res["batch"] * rows
                return (res["probe_idx"] + np.int32(lo)), res["build_idx"].copy()
            for lo in range(0, n, rows):
                hi = min(lo + rows, n)
                res = st.submit((pc[lo:hi], ps[lo:hi], pe[lo:hi]))
                if res is not None:
                    yield emit(res)
            while True:
                res = st.flush()
                if res is None:
                    break
                yield emit(res)

    # ---- raw device memory (callers without torch) --------------------------
    def dev_alloc(self, nbytes: int) -> int:
        p = C.c_void_p()
        _check(self.L, self.L.ivj_dev_alloc(self.h, nbytes, C.byref(p)), "ivj_dev_alloc")
        return p.value or 0

    def dev_free(self, ptr: int):
        _check(self.L, self.L.ivj_dev_free(self.h, C.c_void_p(ptr)), "ivj_dev_free")

    def h2d(self, dst_ptr: int, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        _check(self.L, self.L.ivj_memcpy_h2d(self.h, C.c_void_p(dst_ptr), arr.ctypes.data, arr.nbytes), "ivj_memcpy_h2d")

    def d2h(self, arr: np.ndarray, src_ptr: int):
        assert arr.flags.c_contiguous
        _check(self.L, self.L.ivj_memcpy_d2h(self.h, arr.ctypes.data, C.c_void_p(src_ptr), arr.nbytes), "ivj_memcpy_d2h")


UNIQUE_ID_BYTES = 128


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the library: rank 0 makes it, every other rank receives the 128 bytes by whatever channel
    the host has (a file, MPI, a torch.distributed object broadcast ...)."""
    L = load_library()
    buf = C.create_string_buffer(UNIQUE_ID_BYTES)
    _check(L, L.ivj_comm_unique_id(buf), "ivj_comm_unique_id")
    return buf.raw


class Comm:
    """RCCL communicator of the library (include/ivjoin.h, ivj_comm_*): one rank per GPU; the all-gatherv of result batches
    and the sharded overlap with the exchange overlapping the join run inside libivjoin_hip.so, no PyTorch on the data path."""

    def __init__(self, engine: Engine, unique_id: Optional[bytes], rank: int, world: int, _handle=None):
        self.engine, self.rank, self.world = engine, rank, world
        self.L = load_library()
        if _handle is not None:
            self.h = _handle
            return
        h = C.c_void_p()
        idbuf = C.create_string_buffer(unique_id, UNIQUE_ID_BYTES) if unique_id is not None else None
        _check(self.L, self.L.ivj_comm_create(engine.h, idbuf, int(rank), int(world), C.byref(h)), "ivj_comm_create")
        self.h = h

    @staticmethod
    def create_local(engines):
        """One process, one Engine per device: ncclCommInitAll.  Collective calls on the returned communicators must come
        from one host thread per rank."""
        L = load_library()
        n = len(engines)
        ctxs = (C.c_void_p * n)(*[e.h for e in engines])
        out = (C.c_void_p * n)()
        _check(L, L.ivj_comm_create_local(ctxs, n, out), "ivj_comm_create_local")
        return [Comm(e, None, i, n, _handle=C.c_void_p(out[i])) for i, e in enumerate(engines)]

    def close(self):
        if getattr(self, "h", None):
            self.L.ivj_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def allgather_counts(self, n_local: int):
        counts = (C.c_int64 * self.world)()
        _check(self.L, self.L.ivj_allgather_counts(self.h, int(n_local), counts), "ivj_allgather_counts")
        return [int(x) for x in counts]

    def allgatherv_dev(self, send_ptrs, recv_ptrs, elem_bytes: int, counts):
        n = len(send_ptrs)
        sp = (C.c_void_p * n)(*[C.c_void_p(p) for p in send_ptrs])
        rp = (C.c_void_p * n)(*[C.c_void_p(p) for p in recv_ptrs])
        cn = (C.c_int64 * self.world)(*[int(x) for x in counts])
        with self.engine.lock:
            _check(self.L, self.L.ivj_allgatherv_dev(self.h, sp, rp, n, int(elem_bytes), cn), "ivj_allgatherv_dev")

    def overlap_allgather_dev(self, ix: "DeviceIndex", probe: _Side, opts: _Opts, n_chunks: int, probe_idx_ptr: int, build_idx_ptr: int,
                              capacity: int):
        """-> (n_total, n_local, fits): this rank's shard joined and all-gathered, the exchange overlapping the join."""
        nt, nl = C.c_int64(0), C.c_int64(0)
        with self.engine.lock:
            rc = self.L.ivj_overlap_allgather_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), int(n_chunks), C.c_void_p(probe_idx_ptr),
                                                  C.c_void_p(build_idx_ptr), int(capacity), C.byref(nt), C.byref(nl))
        if rc == -4:
            return nt.value, nl.value, False
        _check(self.L, rc, "ivj_overlap_allgather_dev")
        return nt.value, nl.value, True

    def count_overlaps_allgather_dev(self, ix: "DeviceIndex", probe: _Side, opts: _Opts, n_total: int, counts_ptr: int):
        """count_overlaps of this rank's shard (probe.row_id = global rows) + the exchange of the per-probe results: the int64
        column counts_ptr[n_total] holds every probe row's count, in global probe order, on every rank."""
        with self.engine.lock:
            _check(self.L, self.L.ivj_count_overlaps_allgather_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), int(n_total), C.c_void_p(counts_ptr)),
                   "ivj_count_overlaps_allgather_dev")

    def nearest_allgather_dev(self, ix: "DeviceIndex", probe: _Side, opts: _Opts, n_total: int, idx_ptr: int, dist_ptr: int, nf_ptr: int):
        """nearest of this rank's shard + the exchange: idx_ptr[n_total * k] (int32), dist_ptr[n_total * k] (int64),
        nf_ptr[n_total] (int32) in global probe order on every rank."""
        with self.engine.lock:
            _check(self.L, self.L.ivj_nearest_allgather_dev(self.h, ix.handle, C.byref(probe), C.byref(opts), int(n_total), C.c_void_p(idx_ptr),
                                                            C.c_void_p(dist_ptr), C.c_void_p(nf_ptr)), "ivj_nearest_allgather_dev")


# ---- the one-call Arrow entry (include/ivjoin.h: ivj_*_arrow_stream): what a C / Rust host binds, driven from Python -------------
def _export_stream(src):
    """Anything Arrow-streamable (pyarrow.Table / RecordBatchReader / an object with __arrow_c_stream__) -> a filled
    struct ArrowArrayStream (the library drains and releases it)."""
    import pyarrow as pa
    if isinstance(src, pa.Table):
        src = src.to_reader()
    elif not isinstance(src, pa.RecordBatchReader):
        src = pa.RecordBatchReader.from_stream(src)
    s = _ArrowStream()
    src._export_to_c(C.addressof(s))
    return s


def _import_stream(s: _ArrowStream):
    import pyarrow as pa
    return pa.RecordBatchReader._import_from_c(C.addressof(s))


def _names3(cols):
    if cols is None:
        return None
    return (C.c_char_p * 3)(*[str(c).encode() for c in cols])


def arrow_encode_keys(df1, df2, cols1=None, cols2=None):
    """ivj_arrow_encode_keys: -> ((contig, start, end) of df1, of df2, dictionary names); host only."""
    L = load_library()
    s1, s2 = _export_stream(df1), _export_stream(df2)
    k = _ArrowKeys()
    _check(L, L.ivj_arrow_encode_keys(C.addressof(s1), C.addressof(s2), _names3(cols1), _names3(cols2), C.byref(k)), "ivj_arrow_encode_keys")
    try:
        col = lambda p, n: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), shape=(n,)).copy() if n else np.empty(0, np.int32)
        side1 = (col(k.contig1, k.n1), col(k.start1, k.n1), col(k.end1, k.n1))
        side2 = (col(k.contig2, k.n2), col(k.start2, k.n2), col(k.end2, k.n2))
        offs = np.ctypeslib.as_array(C.cast(k.name_offsets, C.POINTER(C.c_int64)), shape=(k.n_contigs + 1,))
        raw = C.string_at(k.name_bytes, int(offs[-1]))
        names = [raw[offs[i]:offs[i + 1]].decode() for i in range(k.n_contigs)]
        return side1, side2, names
    finally:
        L.ivj_arrow_keys_free(C.byref(k))


def arrow_take_stream(src, idx, batch_rows: int = 0):
    """ivj_arrow_take_stream: rows idx (negative: a null row) of an Arrow stream as a new pyarrow.RecordBatchReader; host only."""
    L = load_library()
    s, out = _export_stream(src), _ArrowStream()
    idx = np.ascontiguousarray(idx, np.int64)
    _check(L, L.ivj_arrow_take_stream(C.addressof(s), C.c_void_p(idx.ctypes.data), len(idx), int(batch_rows), C.addressof(out)), "ivj_arrow_take_stream")
    return _import_stream(out)


def _arrow_stream_call(engine, op: str, df1, df2, cols1, cols2, strict: bool, suffixes, k: int = 1, include_overlaps: bool = True,
                       distance: bool = True, batch_rows: int = 0, limit=None, lazy: bool = False, max_batch_rows: int = 0, nearest_ignore: int = 0):
    L = load_library()
    opts = make_opts(strict, 0, k, include_overlaps, nearest_ignore=nearest_ignore)
    s1, s2, out = _export_stream(df1), _export_stream(df2), _ArrowStream()
    lim = -1 if limit is None else int(limit)
    sfx = [None if x is None else str(x).encode() for x in suffixes]
    a = (engine.h, C.addressof(s1), C.addressof(s2), _names3(cols1), _names3(cols2), C.byref(opts))
    with engine.lock:
        if op == "overlap":
            rc = (L.ivj_overlap_arrow_stream_lazy(*a, sfx[0], sfx[1], int(batch_rows), int(max_batch_rows), lim, C.addressof(out)) if lazy else
                  L.ivj_overlap_arrow_stream(*a, sfx[0], sfx[1], int(batch_rows), lim, C.addressof(out)))
        elif op == "count_overlaps":
            rc = (L.ivj_count_overlaps_arrow_stream_lazy(*a, sfx[0], int(batch_rows), int(max_batch_rows), lim, C.addressof(out)) if lazy else
                  L.ivj_count_overlaps_arrow_stream(*a, sfx[0], int(batch_rows), lim, C.addressof(out)))
        else:
            rc = (L.ivj_nearest_arrow_stream_lazy(*a, sfx[0], sfx[1], 1 if distance else 0, int(batch_rows), int(max_batch_rows), lim, C.addressof(out)) if lazy else
                  L.ivj_nearest_arrow_stream(*a, sfx[0], sfx[1], 1 if distance else 0, int(batch_rows), lim, C.addressof(out)))
    _check(L, rc, f"ivj_{op}_arrow_stream" + ("_lazy" if lazy else ""))
    reader = _import_stream(out)
    if not lazy:
        return reader
    # the lazy stream works on the engine's context whenever a batch is pulled: every pull is made under the engine's lock
    import pyarrow as pa

    def pull():
        while True:
            with engine.lock:
                try:
                    b = reader.read_next_batch()
                except StopIteration:
                    return
            yield b
    return pa.RecordBatchReader.from_batches(reader.schema, pull())


def overlap_arrow_stream(engine, df1, df2, strict: bool, cols1=None, cols2=None, suffixes=("_1", "_2"), batch_rows: int = 0, limit=None,
                         lazy: bool = False, max_batch_rows: int = 0):
    """ivj_overlap_arrow_stream[_lazy] -> pyarrow.RecordBatchReader of the joined rows (every column of both sides, suffixed).
    lazy: df1 is pulled batch by batch while the result is read (host memory bounded by max_batch_rows, not by len(df1))."""
    return _arrow_stream_call(engine, "overlap", df1, df2, cols1, cols2, strict, suffixes, batch_rows=batch_rows, limit=limit, lazy=lazy, max_batch_rows=max_batch_rows)


def count_overlaps_arrow_stream(engine, df1, df2, strict: bool, cols1=None, cols2=None, suffix="", batch_rows: int = 0, limit=None,
                                lazy: bool = False, max_batch_rows: int = 0):
    return _arrow_stream_call(engine, "count_overlaps", df1, df2, cols1, cols2, strict, (suffix, None), batch_rows=batch_rows, limit=limit, lazy=lazy,
                              max_batch_rows=max_batch_rows)


def nearest_arrow_stream(engine, df1, df2, strict: bool, cols1=None, cols2=None, suffixes=("_1", "_2"), k: int = 1, include_overlaps: bool = True,
                         distance: bool = True, batch_rows: int = 0, limit=None, lazy: bool = False, max_batch_rows: int = 0, nearest_ignore: int = 0):
    """nearest_ignore: ONE direction mask for every df1 row (the one-call entries have no per-row orientation)."""
    return _arrow_stream_call(engine, "nearest", df1, df2, cols1, cols2, strict, suffixes, k, include_overlaps, distance, batch_rows, limit, lazy, max_batch_rows,
                              nearest_ignore)


_default_engine: Optional[Engine] = None
_default_lock = threading.Lock()


def default_engine() -> Engine:
    """Process-wide engine (its native calls are serialised by Engine.lock; use one Engine per thread for
    concurrent joins).  One device: the ``ivj.device`` option when it was set explicitly, else LOCAL_RANK (one
    process per GPU under torch.distributed.run), else 0.  Several devices (``ivj.devices`` = "0,1,..", or
    ``ivj.num_gpus`` > 1 on a host with that many GPUs): a
    ``multi.MultiEngine`` -- one context and one host thread per device, contigs dealt to the devices."""
    global _default_engine
    with _default_lock:
        if _default_engine is None:
            from .multi import MultiEngine, requested_devices
            devs = requested_devices()
            _default_engine = MultiEngine(devs) if len(devs) > 1 else Engine(devs[0])
        return _default_engine


def reset_default_engine():
    """Drop the process-wide engine (the next call creates a new one, e.g. after ``ivj.device`` changed).  The old engine is
    NOT closed here: another thread or an unconsumed lazy reader may still be running on it -- its context goes when the last
    reference does (Engine.__del__)."""
    global _default_engine
    with _default_lock:
        _default_engine = None
