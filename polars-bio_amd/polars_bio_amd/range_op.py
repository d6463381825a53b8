"""pb.overlap / pb.nearest / pb.count_overlaps on the MI355X engine.

Same names, argument meaning and error behaviour as the reference's
``IntervalOperations`` (/root/reference/polars_bio/range_op.py:117-256, 259-340,
418-511) and its dispatcher ``range_operation``
(/root/reference/polars_bio/range_op_helpers.py:171-376); the executor behind
them is libivjoin_hip.so instead of DataFusion's IntervalJoinExec + COITrees.

Side roles: probe = df1, build = df2 for all three
operations -- i.e. the state after the reference's swaps in range_op.py:511
(count_overlaps) and src/operation.rs:143-158 (nearest).
"""
from __future__ import annotations

import logging
import os
from typing import Literal, Union

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc

from . import _arrow as A
from ._engine import DEPTH_PROFILE_MAX_BINS, WINDOW_MAX, EngineError, default_engine
from ._metadata import validate_coordinate_system_single, validate_coordinate_systems
from .constants import DEFAULT_INTERVAL_COLUMNS

logger = logging.getLogger("polars_bio_amd")

__all__ = ["overlap", "window", "count_window", "window_extents", "overlap_batches", "count_overlaps_batches", "nearest_batches", "nearest", "count_overlaps", "coverage", "mean_depth", "depth_profile", "depth_summary", "depth_histogram", "genome_depth_histogram", "depth_quantiles", "median_depth", "quantile_ranks", "merge", "cluster", "complement", "subtract", "map_overlaps", "map_quantiles", "map_median", "signal_summary", "signal_profile",
           "set_intersect", "set_union", "set_difference", "set_symmetric_difference", "jaccard", "multi_intersect", "consensus", "pairwise_jaccard",
           "FilterOp", "RangeOp", "OverlapOutputMode"]


class FilterOp:      # src/option.rs:95-100
    Weak = 0
    Strict = 1


class RangeOp:       # src/option.rs:102-112 (hot-path members only)
    Overlap = 0
    Nearest = 3
    Coverage = 4
    CountOverlapsNaive = 6
    Merge = 7
    Cluster = 8
    Complement = 9
    Subtract = 10


class OverlapOutputMode:  # src/option.rs:87-92
    Join = 0
    Left = 1


def _parse_overlap_output_mode(overlap_output: str) -> int:
    normalized = overlap_output.lower()
    if normalized == "join":
        return OverlapOutputMode.Join
    if normalized == "left":
        return OverlapOutputMode.Left
    raise ValueError("overlap_output must be either 'join' or 'left'")


def _validate_overlap_input(col1, col2, on_cols, suffixes, output_type):
    """reference: range_op_helpers.py:379-399.  -> on_cols as a list, or None for no extra join keys ([] is None)."""
    assert output_type in A.OUTPUT_TYPES, (
        "Only polars.LazyFrame, polars.DataFrame and pandas DataFrame are supported")
    if on_cols is None:
        return None
    if isinstance(on_cols, str):
        on_cols = [on_cols]
    on_cols = list(on_cols)
    if not on_cols:
        return None
    assert all(isinstance(c, str) for c in on_cols), "on_cols must be a list of column names"
    assert len(set(on_cols)) == len(on_cols), "on_cols names a column twice"
    interval = set(DEFAULT_INTERVAL_COLUMNS if col1 is None else col1) | set(DEFAULT_INTERVAL_COLUMNS if col2 is None else col2)
    bad = [c for c in on_cols if c in interval]
    assert not bad, f"on_cols may not name the interval columns: {bad}"
    return on_cols


def _schema_names(df):
    from . import _streaming as S
    sch = S.source_schema(df)
    if sch is None:
        return None
    return list(sch.names)


def _check_on_cols_present(on_cols, *frames):
    """Every on_col must exist in every frame (AssertionError otherwise, as the reference's own checks fail)."""
    if not on_cols:
        return
    for df in frames:
        names = _schema_names(df)
        if names is None:
            continue                                          # a bare stream: checked when its first batch is encoded
        missing = [c for c in on_cols if c not in names]
        assert not missing, f"on_cols {missing} not found in {names}"


def _low_memory_batch_rows() -> int:
    from .context import get_option
    try:
        return max(1024, int(get_option("ivj.low_memory_batch_rows") or 8_000_000))
    except ValueError:
        return 8_000_000


def _key_columns_from_device(t1, t2, cols1, cols2) -> bool:
    """The key columns of a joined result can come back from the device (int32 in pair order) when the frames' coordinate
    columns are plain integers (any width: the engine computes in int32) and the engine offers ivj_overlap_rows;
    ``ivj.materialize = pairs`` keeps the index-pair path (the result rows are then gathered on the host)."""
    from .context import get_option
    if str(get_option("ivj.materialize") or "host").lower() == "pairs":
        return False
    c1 = list(DEFAULT_INTERVAL_COLUMNS if cols1 is None else cols1)
    c2 = list(DEFAULT_INTERVAL_COLUMNS if cols2 is None else cols2)
    for t, c in ((t1, c1), (t2, c2)):
        for name in c[1:]:
            if not pa.types.is_integer(t.schema.field(name).type):
                return False
    eng = default_engine()
    # several devices (multi.MultiEngine): the shards' results are merged as index pairs
    return hasattr(eng, "overlap_rows") and not hasattr(eng, "last_shards")


def _materialize_on_device() -> bool:
    from .context import get_option
    return str(get_option("ivj.materialize") or "host").lower() == "device"


def _overlap_join_rows(t1, t2, probe, build, n_contigs, keys, cols1, cols2, suffixes, zero_based, others_on_device) -> pa.Table:
    """Join-mode overlap whose key columns are materialised in HBM (ivj_overlap_rows) and arrive
    through the Arrow C Data interface as int32 columns in pair order: the six key columns of the result are then sequential
    passes (a widening back to the frame's dtype, a gather out of the chrom dictionary) instead of six random gathers out of the
    10^7-row inputs; only the non-key columns are gathered by the pair indices -- on the host (native threaded gather) or,
    with ``ivj.materialize = device``, in HBM (ivj_take).  Same output contract as the host path (src/operation.rs:272-301)."""
    c1 = list(DEFAULT_INTERVAL_COLUMNS if cols1 is None else cols1)
    c2 = list(DEFAULT_INTERVAL_COLUMNS if cols2 is None else cols2)
    dictionary = keys[4]
    eng = default_engine()
    rows = eng.overlap_rows(probe, build, strict=zero_based, n_contigs=n_contigs, as_arrow=True)
    col = lambda name: rows.column(name).to_numpy(zero_copy_only=False)     # views of the library's buffers (owned by `rows`)
    p_idx, b_idx, contig = col("probe_idx"), col("build_idx"), col("contig")
    if len(keys) > 5 and keys[5] is not None:
        contig = A.H.take(keys[5], np.ascontiguousarray(contig, np.int32))  # on_cols: the ids are group ids -> chrom ids of the group table
    other1 = [n for n in t1.column_names if n not in c1]
    other2 = [n for n in t2.column_names if n not in c2]
    take = (lambda t, idx: A.take_rows_device(eng, t, idx)) if others_on_device else (lambda t, idx: A.take_rows(t, idx))

    def coord(values, typ):
        if pa.types.is_int32(typ):
            return pa.array(values, type=typ)
        if pa.types.is_int64(typ):
            return pa.Array.from_buffers(typ, len(values), [None, pa.py_buffer(A.H.widen_i64(values))])
        return pc.cast(pa.array(values, type=pa.int32()), typ)

    def side(args):
        src, cols, others, idx, start, end = args
        taken = take(src.select(others), idx) if others else None
        arrays = []
        for name in src.column_names:
            typ = src.schema.field(name).type
            if name == cols[0]:
                arrays.append(A._chrom_from_ids(contig, dictionary, typ))
            elif name == cols[1]:
                arrays.append(coord(start, typ))
            elif name == cols[2]:
                arrays.append(coord(end, typ))
            else:
                arrays.append(taken.column(name))
        return pa.Table.from_arrays(arrays, names=src.column_names)

    jobs = [(t1, c1, other1, p_idx, col("start_1"), col("end_1")), (t2, c2, other2, b_idx, col("start_2"), col("end_2"))]
    res1, res2 = A._pmap(side, jobs, A.SIDES) if len(p_idx) >= A._PAR_MIN_ROWS else [side(j) for j in jobs]
    return A.hconcat(A.with_suffix(res1, suffixes[0]), A.with_suffix(res2, suffixes[1]))


# ---- result assembly (shared by the eager and the streaming paths) ------------------------------------------------

def _assemble_overlap(t1, t2, p_idx, b_idx, mode, distinct_output, suffixes, keys=None) -> pa.Table:
    """src/operation.rs:272-301: df1 columns + suffixes[0], df2 columns + suffixes[1]; "left": df1 columns only.
    keys = (chrom column of df1, its per-row dictionary ids, chrom column of df2, its ids, the shared dictionary) from the key
    encoding: the two chrom columns of the result are then gathered out of the dictionary, not out of the input strings."""
    k1 = (keys[0], keys[1], keys[4]) if keys is not None else None
    k2 = (keys[2], keys[3], keys[4]) if keys is not None else None
    if mode == OverlapOutputMode.Left:
        if distinct_output:
            p_idx = np.unique(p_idx)
        return A.take_rows(t1, p_idx, chrom=k1)
    left, right = A._pmap(lambda a: A.take_rows(a[0], a[1], chrom=a[2]), [(t1, p_idx, k1), (t2, b_idx, k2)], A.SIDES)
    return A.hconcat(A.with_suffix(left, suffixes[0]), A.with_suffix(right, suffixes[1]))


def _assemble_nearest(t1, t2, idx, dist, nf, suffixes, distance, keys=None) -> pa.Table:
    """src/operation.rs:170-197: one output row per filled slot; rows without any candidate keep a single null slot."""
    n1 = t1.num_rows
    k1 = (keys[0], keys[1], keys[4]) if keys is not None else None
    k2 = (keys[2], keys[3], keys[4]) if keys is not None else None
    if idx.ndim == 2 and idx.shape[1] == 1:
        # k = 1: exactly one slot per df1 row -- the left side IS df1 (no gather, no copy), the right side one gather
        left = t1
        b_sel = np.ascontiguousarray(idx.reshape(-1))
        d_sel = np.array(dist.reshape(-1), copy=True)          # becomes a result column: must not alias a streaming session's recycled slot
    else:
        slots = np.maximum(nf, 1)
        rep = np.repeat(np.arange(n1, dtype=np.int32), slots)
        first = np.cumsum(slots) - slots
        within = np.arange(rep.shape[0], dtype=np.int64) - np.repeat(first, slots)
        b_sel = idx[rep, within] if n1 else np.empty(0, np.int32)
        d_sel = dist[rep, within] if n1 else np.empty(0, np.int64)
        left = A.take_rows(t1, rep, chrom=k1)
    res = A.hconcat(A.with_suffix(left, suffixes[0]), A.with_suffix(A.take_rows(t2, b_sel, nullable=True, chrom=k2), suffixes[1]))
    if distance:
        res = res.append_column("distance", pa.array(d_sel, type=pa.int64(), mask=(b_sel < 0)))
    return res


def _assemble_count(t1, counts, naive_query, cols1, suffixes, on_cols=None) -> pa.Table:
    if naive_query:
        return t1.append_column("count", pa.array(counts, type=pa.int64()))
    # the reference sweep's select list (range_op.py:583-592): suffixed key columns, the on_cols (df1's values), count
    res = pa.table({f"{c}{suffixes[0]}": t1.column(c) for c in cols1})
    for c in on_cols or ():
        res = res.append_column(c, t1.column(c))
    return res.append_column("count", pa.array(counts, type=pa.int64()))


# ---- streaming / lazy front end ----------------------------------------------------

def _stream(op, df1, df2, cols1, cols2, assemble, batch_rows, limit, k=1, include_overlaps=True, zero_based=None, on_cols=None, **directed):
    from . import _streaming as S
    if zero_based is None:
        zero_based = validate_coordinate_systems(df1, df2)
    cols1 = list(DEFAULT_INTERVAL_COLUMNS if cols1 is None else cols1)
    cols2 = list(DEFAULT_INTERVAL_COLUMNS if cols2 is None else cols2)
    rows = int(batch_rows) if batch_rows else _low_memory_batch_rows()
    return zero_based, S.range_batches(default_engine(), op, df1, df2, cols1, cols2, zero_based, assemble, batch_rows=rows, limit=limit,
                                       k=k, include_overlaps=include_overlaps, on_cols=on_cols, **directed)


def _lazy_reader(df1, df2, zero_based, batches, assemble_empty):
    """The streaming result as a pyarrow.RecordBatchReader (= an ArrowArrayStream, ``__arrow_c_stream__``); its schema comes
    from assembling an EMPTY result, so nothing is read or joined before the consumer pulls."""
    from . import _streaming as S
    from ._metadata import set_coordinate_system
    sch1 = S.source_schema(df1)
    if sch1 is None:                                      # a producer that only reveals its schema with its first batch
        batches = iter(batches)
        first = next(batches, None)
        schema = first.schema if first is not None else pa.schema([])
        import itertools
        batches = itertools.chain([first] if first is not None else [], batches)
    else:
        t2 = A.to_arrow(df2) if not isinstance(df2, pa.Table) else df2
        schema = assemble_empty(sch1.empty_table(), t2.slice(0, 0)).schema
    # the marker type of pandas object-string columns (_arrow._OBJECT_DICT) never leaves through an Arrow stream
    schema = set_coordinate_system(A._decode_object_dict(schema.empty_table()), zero_based).schema
    return S.range_reader(schema, (A._decode_object_dict(b) for b in batches))


def overlap_batches(df1, df2, suffixes=("_1", "_2"), cols1=None, cols2=None, batch_rows: int = 8_000_000, limit=None,
                    overlap_output: str = "join", distinct_output: bool = False, as_reader: bool = False, _zero_based=None, on_cols=None):
    """Streaming form of ``overlap``: df2 is indexed once on the device, df1 is CONSUMED batch by batch -- an Arrow C stream
    producer (``__arrow_c_stream__`` / ``pyarrow.RecordBatchReader``), a Parquet / CSV / BED path, or an in-memory frame --
    and one pyarrow.Table of joined rows is yielded per probe batch (H2D, join and D2H of consecutive batches overlap).
    ``limit`` bounds the number of result rows and stops reading df1 early.  ``as_reader=True`` returns a
    pyarrow.RecordBatchReader instead of a generator.  Counterpart of the reference's lazy ``range_lazy_scan`` generator
    (/root/reference/polars_bio/range_op_io.py:100-174) and ``range_operation_lazy`` (src/lib.rs:154-214).
    ``on_cols``: extra join keys; df2 fixes their dictionaries, a df1 value df2 lacks matches nothing."""
    mode = _parse_overlap_output_mode(overlap_output)
    asm = lambda bt, t2, res: _assemble_overlap(bt, t2, res["probe_idx"], res["build_idx"], mode, distinct_output, suffixes)
    zero_based, gen = _stream("overlap", df1, df2, cols1, cols2, asm, batch_rows, limit, zero_based=_zero_based, on_cols=on_cols)
    if as_reader:
        e = np.empty(0, np.int32)
        return _lazy_reader(df1, df2, zero_based, gen, lambda a, b: _assemble_overlap(a, b, e, e, mode, distinct_output, suffixes))
    return gen


def count_overlaps_batches(df1, df2, suffixes=("", "_"), cols1=None, cols2=None, batch_rows: int = 8_000_000, limit=None,
                           naive_query: bool = True, as_reader: bool = False, _zero_based=None, on_cols=None):
    """Streaming form of ``count_overlaps`` (see ``overlap_batches``): df1 rows + ``count`` per probe batch, df1 order kept."""
    c1 = list(DEFAULT_INTERVAL_COLUMNS if cols1 is None else cols1)
    asm = lambda bt, t2, res: _assemble_count(bt, res["counts"], naive_query, c1, suffixes, on_cols)
    zero_based, gen = _stream("count_overlaps", df1, df2, cols1, cols2, asm, batch_rows, limit, zero_based=_zero_based, on_cols=on_cols)
    if as_reader:
        return _lazy_reader(df1, df2, zero_based, gen, lambda a, b: _assemble_count(a, np.empty(0, np.int64), naive_query, c1, suffixes, on_cols))
    return gen


def _direction(df1, ignore_upstream, ignore_downstream, direction_col):
    """-> (engine mask of the "+" rows, mask of the "-" rows or None when every row takes the same mask).  Upstream of a "+" row is
    lower coordinates (the engine's class "left"), downstream higher ("right"); a "-" row has the two swapped, so its mask is the
    other one's mirror -- which only differs when exactly one of the two flags is set."""
    from ._engine import NEAREST_IGNORE_LEFT, NEAREST_IGNORE_RIGHT
    if direction_col is not None:
        if not isinstance(direction_col, str):
            raise ValueError("direction_col must be the name of a df1 column")
        names = _schema_names(df1)                            # None: a bare stream, checked when its first batch is split
        if names is not None and direction_col not in names:
            raise ValueError(f"direction_col '{direction_col}' not found in {names}")
    up, down = bool(ignore_upstream), bool(ignore_downstream)
    plus = (NEAREST_IGNORE_LEFT if up else 0) | (NEAREST_IGNORE_RIGHT if down else 0)
    minus = (NEAREST_IGNORE_RIGHT if up else 0) | (NEAREST_IGNORE_LEFT if down else 0)
    return plus, (minus if direction_col is not None and minus != plus else None)


def _directed_kw(plus, minus, direction_col):
    """Keywords of the streaming session for a directed nearest; none for the undirected call (which then is today's call)."""
    if minus is not None:
        return {"nearest_ignore": plus, "direction": (direction_col, minus)}
    return {"nearest_ignore": plus} if plus else {}


def _nearest_oriented(eng, t1, probe, build, n_contigs, zero_based, k, overlap, direction_col, plus, minus):
    """The eager engine call(s) of a directed nearest: the engine's mask is uniform per call, so df1 rows of both orientations are
    partitioned into two calls (the mask and its mirror) and the results scattered back to df1 row order (ivj_host_scatter)."""
    run = lambda side, mask: eng.nearest(side, build, strict=zero_based, n_contigs=n_contigs, k=k, include_overlaps=overlap, nearest_ignore=mask)
    if minus is None:
        return run(probe, plus)
    is_minus = A.minus_rows(t1.column(direction_col))
    n_minus = int(is_minus.sum())
    if n_minus == 0 or n_minus == len(is_minus):
        return run(probe, minus if n_minus else plus)
    n = len(is_minus)
    idx, dist, nf = np.empty((n, k), np.int32), np.empty((n, k), np.int64), np.empty(n, np.int32)
    for rows, mask in ((np.flatnonzero(~is_minus).astype(np.int32), plus), (np.flatnonzero(is_minus).astype(np.int32), minus)):
        i, d, f = run(tuple(A.H.take(np.ascontiguousarray(c, np.int32), rows) for c in probe), mask)
        A.H.scatter(idx, rows, np.ascontiguousarray(i, np.int32).reshape(len(rows), k))
        A.H.scatter(dist, rows, np.ascontiguousarray(d, np.int64).reshape(len(rows), k))
        A.H.scatter(nf, rows, f)
    return idx, dist, nf


def nearest_batches(df1, df2, suffixes=("_1", "_2"), cols1=None, cols2=None, k: int = 1, overlap: bool = True, distance: bool = True,
                    batch_rows: int = 8_000_000, limit=None, as_reader: bool = False, _zero_based=None, on_cols=None, *,
                    ignore_upstream: bool = False, ignore_downstream: bool = False, direction_col=None):
    """Streaming form of ``nearest`` (see ``overlap_batches``).  ``ignore_upstream`` / ``ignore_downstream`` / ``direction_col``: as
    in ``nearest``.  When df1 rows of both orientations meet in one input batch, the batch is submitted as two sub-batches (its
    "+" rows, then its "-" rows) to the same session, and the two come out as SEPARATE result batches, each in df1 order: the
    rows of one input batch are then not contiguous in df1 order (the reference leaves the row order unspecified)."""
    plus, minus = _direction(df1, ignore_upstream, ignore_downstream, direction_col)
    asm = lambda bt, t2, res: _assemble_nearest(bt, t2, res["build_idx"], res["dist"], res["n_found"], suffixes, distance)
    zero_based, gen = _stream("nearest", df1, df2, cols1, cols2, asm, batch_rows, limit, k=int(k), include_overlaps=bool(overlap), zero_based=_zero_based,
                              on_cols=on_cols, **_directed_kw(plus, minus, direction_col))
    if as_reader:
        kk = int(k)
        return _lazy_reader(df1, df2, zero_based, gen, lambda a, b: _assemble_nearest(a, b, np.empty((0, kk), np.int32), np.empty((0, kk), np.int64),
                                                                                     np.empty(0, np.int32), suffixes, distance))
    return gen


def _is_one_shot(df) -> bool:
    """True for a source that can be streamed only once: a pyarrow.RecordBatchReader, or an object that only offers
    ``__arrow_c_stream__`` (tables, frames and paths can be opened again)."""
    if isinstance(df, pa.RecordBatchReader):
        return True
    if isinstance(df, (pa.Table, pa.RecordBatch, str)) or hasattr(df, "to_arrow") or hasattr(df, "collect") or hasattr(df, "iloc"):
        return False
    return hasattr(df, "__arrow_c_stream__")


def _polars_lazy_result(df1, df2, zero_based, limit, batches_fn, **kw):
    """``output_type="polars.LazyFrame"`` (the reference's default) with polars installed: a ``register_io_source`` LazyFrame
    over the streaming session -- nothing is read or joined until polars pulls, every collect() runs a fresh stream, a LazyFrame
    df1 is streamed through the device batch by batch instead of being collected (reference: range_lazy_scan /
    _prepare_lazy_stream_input, polars_bio/range_op_io.py:31-174, 185-283).  None: df1 reveals its schema only with its first
    batch (a bare Arrow C stream): the caller keeps the eager path."""
    from . import _polars_lazy as PL
    from . import _streaming as S
    from ._metadata import set_coordinate_system
    if A.pl is None or S.source_schema(df1) is None:
        return None
    if _is_one_shot(df1):
        # a pyarrow.RecordBatchReader / a bare Arrow C stream can be read ONCE, a LazyFrame may be collected any number of times
        # (and the schema probe below would already pull from it): such a source is materialised once, like the build side
        df1 = A.to_arrow(df1)
    t2 = df2 if isinstance(df2, pa.Table) else A.to_arrow(df2)      # the build side is read ONCE, whatever the number of collects
    probe = batches_fn(df1, t2, as_reader=True, limit=0, _zero_based=zero_based, **kw)      # schema only: assembles an empty result
    schema = probe.schema
    probe.close()

    def make(n_rows):
        lim = limit if n_rows is None else (n_rows if limit is None else min(limit, n_rows))
        return (A._decode_object_dict(b) for b in batches_fn(df1, t2, limit=lim, _zero_based=zero_based, **kw))
    return set_coordinate_system(PL.range_lazy_scan(make, schema), zero_based)


# ---- overlap thresholds (include/ivjoin.h: ivj_thresholds) -------------------------------------------------------

THRESH_NEVER = 0xFFFFFFFF      # the per-row minimum of a row that can never match


def _validate_overlap_thresholds(min_overlap, min_frac1, min_frac2):
    """-> (min_overlap as int or 0, min_frac1, min_frac2 as float or None).  ValueError: a min_overlap that is not an int >= 1
    (bools are refused), a fraction outside (0, 1] or NaN."""
    if min_overlap is None:
        mo = 0
    else:
        if isinstance(min_overlap, (bool, np.bool_)) or not isinstance(min_overlap, (int, np.integer)):
            raise ValueError(f"min_overlap must be an int >= 1, got {min_overlap!r}")
        if min_overlap < 1:
            raise ValueError(f"min_overlap must be >= 1, got {min_overlap}")
        mo = min(int(min_overlap), THRESH_NEVER)           # minima are uint32: 2^32 - 1 and above read as "never" (see min_bases)
    fr = []
    for name, f in (("min_frac1", min_frac1), ("min_frac2", min_frac2)):
        if f is None:
            fr.append(None)
            continue
        if isinstance(f, (bool, np.bool_)) or not isinstance(f, (int, float, np.integer, np.floating)):
            raise ValueError(f"{name} must be a float in (0, 1], got {f!r}")
        f = float(f)
        if not (f > 0.0 and f <= 1.0):                     # NaN fails both comparisons
            raise ValueError(f"{name} must be in (0, 1], got {f}")
        fr.append(f)
    return mo, fr[0], fr[1]


def min_bases(length, frac: float) -> np.ndarray:
    """Per-row minimum base count of a fractional overlap threshold: m(r) = the smallest integer m >= 1 with
    m / len(r) >= frac evaluated in IEEE float64, as uint32; THRESH_NEVER for rows with len <= 0.  ``length``: int64 lengths.
    Computed as ceil(frac * len) and corrected by one in either direction with the literal division test; float64 division is
    monotone in m, so one step each way suffices -- asserted."""
    length = np.asarray(length, dtype=np.int64)
    out = np.full(length.shape, THRESH_NEVER, dtype=np.uint32)
    ok = length > 0
    ln = length[ok]
    lf = ln.astype(np.float64)
    m = np.maximum(np.ceil(frac * lf).astype(np.int64), 1)
    m = np.minimum(m, ln)                                  # frac <= 1: m = len always passes (len / len = 1.0)
    up = (m.astype(np.float64) / lf) < frac                # the product rounded down: one more base
    m = m + up
    down = (m > 1) & (((m - 1).astype(np.float64) / lf) >= frac)   # the product rounded up: one base fewer still passes
    m = m - down
    assert ((m.astype(np.float64) / lf) >= frac).all() and ((m == 1) | (((m - 1).astype(np.float64) / lf) < frac)).all(), \
        "min_bases: one correction step did not reach the smallest passing count"
    assert (m >= 1).all() and (m <= ln).all()
    # minima are uint32 and 2^32 - 1 is "never": a minimum that large (a row spanning all but a few of the 2^32 int32 positions)
    # is stored as never
    out[ok] = np.minimum(m, THRESH_NEVER).astype(np.uint32)
    return out


def _side_lengths(side, zero_based: bool) -> np.ndarray:
    """len(r) of the semantics: end - start, + 1 for 1-based closed frames (int64)."""
    return side[2].astype(np.int64) - side[1].astype(np.int64) + (0 if zero_based else 1)


def _threshold_engine():
    eng = default_engine()
    if not hasattr(eng, "overlap_thresh") or not hasattr(eng, "count_overlaps_thresh"):
        raise NotImplementedError(f"min_overlap / min_frac1 / min_frac2 need a single-device engine; the default engine is a "
                                  f"{type(eng).__name__} (several devices), which has no thresholded join")
    return eng


def _threshold_minima(probe, build, zero_based, min_frac1, min_frac2):
    pm = min_bases(_side_lengths(probe, zero_based), min_frac1) if min_frac1 is not None else None
    bm = min_bases(_side_lengths(build, zero_based), min_frac2) if min_frac2 is not None else None
    return pm, bm


def _finish_eager(table, output_type, zero_based, limit):
    """An eagerly computed result as the requested output kind: ``limit`` takes its head, a RecordBatchReader reads it."""
    if limit is not None:
        table = table.slice(0, max(int(limit), 0))
    if output_type == "pyarrow.RecordBatchReader":
        from ._metadata import set_coordinate_system
        table = set_coordinate_system(A._decode_object_dict(table), zero_based)
        return pa.RecordBatchReader.from_batches(table.schema, table.to_batches())
    return A.from_arrow(table, output_type, zero_based)


def _prepare(df1, df2, cols1, cols2, on_cols=None):
    """-> (t1, t2, probe, build, n_contigs, keys).  With on_cols the sides carry GROUP ids over (chrom, on values) as contig and
    n_contigs is the number of groups (ivj_host_group_ids); keys keeps the per-row chrom ids (the result's chrom columns) and, as
    a sixth item, the chrom id of every group id (None without on_cols)."""
    cols1 = list(DEFAULT_INTERVAL_COLUMNS if cols1 is None else cols1)
    cols2 = list(DEFAULT_INTERVAL_COLUMNS if cols2 is None else cols2)
    t1, t2 = A.to_arrow(df1), A.to_arrow(df2)
    probe, build, n_contigs, dictionary = A.encode_keys(t1, cols1, t2, cols2, with_dictionary=True)
    keys = (cols1[0], probe[0], cols2[0], build[0], dictionary, None)
    if on_cols:
        for t in (t1, t2):
            missing = [c for c in on_cols if c not in t.column_names]
            assert not missing, f"on_cols {missing} not found in {t.column_names}"
        (codes1, codes2), cards, _, _ = A.encode_on_cols([t1, t2], on_cols)
        probe, build, groups, table = A.group_sides(probe, build, n_contigs, codes1, codes2, cards, on_cols)
        n_contigs = max(groups, 1)
        keys = keys[:5] + (np.ascontiguousarray(table[:, 0]) if groups else np.zeros(1, np.int32),)
    return t1, t2, probe, build, n_contigs, keys


def overlap(
    df1,
    df2,
    suffixes: tuple = ("_1", "_2"),
    on_cols: Union[list, None] = None,
    cols1: Union[list, None] = ["chrom", "start", "end"],
    cols2: Union[list, None] = ["chrom", "start", "end"],
    algorithm: str = "Coitrees",
    low_memory: bool = False,
    overlap_output: Literal["join", "left"] = "join",
    distinct_output: bool = False,
    output_type: str = "polars.LazyFrame",
    read_options1=None,
    read_options2=None,
    projection_pushdown: bool = True,
    limit: Union[int, None] = None,
    *,
    min_overlap: Union[int, None] = None,
    min_frac1: Union[float, None] = None,
    min_frac2: Union[float, None] = None,
    how: Literal["inner", "left", "semi", "anti"] = "inner",
):
    """Find pairs of overlapping genomic intervals (reference: range_op.py:117-256).

    ``output_type="pyarrow.RecordBatchReader"`` returns the LAZY result (an ArrowArrayStream: df1 is streamed through the
    device batch by batch when the consumer pulls); ``limit`` (the reference carries it through its FFI, src/lib.rs:80-88,
    125-130) bounds the number of result rows -- both take the streaming path (``overlap_batches``).

    ``algorithm`` / ``low_memory`` are accepted for call compatibility; the result is
    algorithm-invariant in the reference (tests/test_overlap_algorithms.py:128-171) and the
    HIP engine is always used.  Output: every df1 column + suffixes[0], then every df2
    column + suffixes[1] (src/operation.rs:277-292); ``overlap_output="left"`` returns df1
    columns only, one row per matching pair, or once per df1 row with ``distinct_output``
    (src/operation.rs:224-233, 294-298).

    ``on_cols``: further columns both frames must agree on (e.g. ``["strand"]``): pairs are formed within groups of equal
    (chrom, on values) only; a null on-value matches nothing, like a null chrom.

    Overlap thresholds (keyword-only; bedtools ``intersect -f / -F / -r`` and a minimum base count).  With
    ``ov = min(end1, end2) - max(start1, start2)`` and ``len = end - start`` for 0-based half-open frames (both + 1 for 1-based
    closed frames): ``min_overlap`` (int >= 1) keeps a pair iff ``ov >= min_overlap``; ``min_frac1`` (float in (0, 1]) iff
    ``ov >= 1`` and ``ov / len(df1 row) >= min_frac1``, the division evaluated in IEEE float64 (``-f``); ``min_frac2`` the same
    against the df2 row (``-F``; both equal is ``-r``).  All thresholds that are set must hold; an "either fraction suffices"
    mode (``-e``) is not offered.  Any threshold implies ``ov >= 1``: rows that cover no position (zero-length, start > end),
    intervals that only touch, and rows with a null chrom or on-value never match.  The fractions become per-row minimum base
    counts on the host (``min_bases``); the device tests ``ov >= max(min_overlap, m1[df1 row], m2[df2 row])`` on every candidate
    pair, so nothing is materialised only to be filtered.  ``on_cols``, ``overlap_output``, ``distinct_output`` and ``suffixes``
    behave as without thresholds.  A thresholded call is EAGER whatever the ``output_type``: the finished table is converted,
    ``limit`` takes its head, and ``pyarrow.RecordBatchReader`` is a reader over it; ``low_memory`` is not applied.  The streaming
    entries (``overlap_batches``) and a multi-device default engine take no thresholds (the latter raises NotImplementedError).
    Invalid thresholds raise ValueError.

    Join kinds (keyword-only ``how``; bedtools ``intersect -u / -v / -loj``).  ``"inner"`` (default) is everything above.
    ``"semi"``: the df1 rows that overlap at least one df2 row, each once (``-u``); ``"anti"``: the df1 rows that overlap none
    (``-v``) -- both return df1's columns as they are (no suffix), in df1 order.  ``"left"``: the joined columns of the inner
    join, followed by one row per unmatched df1 row whose df2 columns are all null (``-loj``).  "Overlap" is the predicate of the
    call: with ``min_overlap`` / ``min_frac1`` / ``min_frac2`` the thresholded one.  Rows that can match nothing (null chrom or
    on-value, and under thresholds rows that cover no position) are unmatched rows; an empty df2 leaves every df1 row unmatched.
    The selection runs on the device over the per-row counts of ``count_overlaps``; no pair is enumerated for semi / anti.  A
    non-inner ``how`` composes with ``on_cols``, ``cols1`` / ``cols2``, ``suffixes`` and the thresholds; it is EAGER whatever the
    ``output_type`` (``limit`` takes the head), ``low_memory`` is not applied, ``overlap_output`` must be "join" and
    ``distinct_output`` False (ValueError otherwise, as for an unknown ``how``); a multi-device default engine raises
    NotImplementedError.  ``overlap_batches`` takes no ``how``."""
    how = _validate_how(how, overlap_output, distinct_output)
    if how != "inner":
        return _overlap_join_kind(how, df1, df2, suffixes, on_cols, cols1, cols2, output_type, limit, min_overlap, min_frac1, min_frac2)
    if min_overlap is not None or min_frac1 is not None or min_frac2 is not None:
        return _overlap_thresholded(df1, df2, suffixes, on_cols, cols1, cols2, overlap_output, distinct_output, output_type, limit,
                                    min_overlap, min_frac1, min_frac2)
    on_cols = _validate_overlap_input(cols1, cols2, on_cols, suffixes, output_type)
    _check_on_cols_present(on_cols, df1, df2)
    zero_based = validate_coordinate_systems(df1, df2)
    mode = _parse_overlap_output_mode(overlap_output)
    logger.info("Optimizing into IntervalJoinExec using %s algorithm (executed by the HIP engine)", algorithm)
    if output_type == "polars.LazyFrame":
        lf = _polars_lazy_result(df1, df2, zero_based, limit, overlap_batches, suffixes=suffixes, cols1=cols1, cols2=cols2,
                                 batch_rows=_low_memory_batch_rows(), overlap_output=overlap_output, distinct_output=distinct_output,
                                 on_cols=on_cols)
        if lf is not None:
            return lf
    if output_type == "pyarrow.RecordBatchReader" or limit is not None:
        lazy = overlap_batches(df1, df2, suffixes, cols1, cols2, batch_rows=_low_memory_batch_rows(), limit=limit,
                               overlap_output=overlap_output, distinct_output=distinct_output, as_reader=True, on_cols=on_cols)
        return lazy if output_type == "pyarrow.RecordBatchReader" else A.from_arrow(lazy.read_all(), output_type, zero_based)
    t1, t2, probe, build, n_contigs, keys = _prepare(df1, df2, cols1, cols2, on_cols)
    if mode == OverlapOutputMode.Join and not low_memory and _key_columns_from_device(t1, t2, cols1, cols2):
        try:
            return A.from_arrow(_overlap_join_rows(t1, t2, probe, build, n_contigs, keys, cols1, cols2, suffixes, zero_based, _materialize_on_device()),
                                output_type, zero_based)
        except EngineError as e:
            # seven int32 columns per pair did not fit the host (28 bytes per pair; the index pairs below need 8): keep going
            if "does not fit the available host memory" not in str(e):
                raise
    if low_memory:
        # bounded device footprint and result batches: the probe side streams through the GPU in
        # tiles against the resident build index (reference: low_memory caps the output batch size)
        parts = list(default_engine().overlap_batches(probe, build, strict=zero_based, n_contigs=n_contigs,
                                                      batch_rows=_low_memory_batch_rows()))
        p_idx = np.concatenate([p for p, _ in parts]) if parts else np.empty(0, np.int32)
        b_idx = np.concatenate([b for _, b in parts]) if parts else np.empty(0, np.int32)
    else:
        p_idx, b_idx = default_engine().overlap(probe, build, strict=zero_based, n_contigs=n_contigs)
    return A.from_arrow(_assemble_overlap(t1, t2, p_idx, b_idx, mode, distinct_output, suffixes, keys), output_type, zero_based)


def _overlap_thresholded(df1, df2, suffixes, on_cols, cols1, cols2, overlap_output, distinct_output, output_type, limit,
                         min_overlap, min_frac1, min_frac2):
    mo, f1, f2 = _validate_overlap_thresholds(min_overlap, min_frac1, min_frac2)
    on_cols = _validate_overlap_input(cols1, cols2, on_cols, suffixes, output_type)
    _check_on_cols_present(on_cols, df1, df2)
    zero_based = validate_coordinate_systems(df1, df2)
    mode = _parse_overlap_output_mode(overlap_output)
    eng = _threshold_engine()
    t1, t2, probe, build, n_contigs, keys = _prepare(df1, df2, cols1, cols2, on_cols)
    pm, bm = _threshold_minima(probe, build, zero_based, f1, f2)
    p_idx, b_idx = eng.overlap_thresh(probe, build, strict=zero_based, n_contigs=n_contigs, min_overlap=mo, probe_min=pm, build_min=bm)
    return _finish_eager(_assemble_overlap(t1, t2, p_idx, b_idx, mode, distinct_output, suffixes, keys), output_type, zero_based, limit)


JOIN_KINDS = ("inner", "left", "semi", "anti")


def _validate_how(how, overlap_output, distinct_output) -> str:
    """ValueError: an unknown ``how``; a non-inner ``how`` together with ``overlap_output != "join"`` or ``distinct_output``."""
    if not isinstance(how, str) or how not in JOIN_KINDS:
        raise ValueError(f"how must be one of {list(JOIN_KINDS)}, got {how!r}")
    if how != "inner":
        if _parse_overlap_output_mode(overlap_output) != OverlapOutputMode.Join:
            raise ValueError(f"how='{how}' takes overlap_output='join' only: semi / anti already return df1's columns")
        if distinct_output:
            raise ValueError(f"how='{how}' does not take distinct_output: semi / anti report every df1 row once")
    return how


def _join_kind_engine():
    eng = default_engine()
    if not hasattr(eng, "overlap_select") or not hasattr(eng, "overlap_outer"):
        raise NotImplementedError(f"how='left' / 'semi' / 'anti' need a single-device engine; the default engine is a "
                                  f"{type(eng).__name__} (several devices), which has no semi, anti or outer join")
    return eng


def _overlap_join_kind(how, df1, df2, suffixes, on_cols, cols1, cols2, output_type, limit, min_overlap, min_frac1, min_frac2):
    mo, f1, f2 = _validate_overlap_thresholds(min_overlap, min_frac1, min_frac2)
    on_cols = _validate_overlap_input(cols1, cols2, on_cols, suffixes, output_type)
    _check_on_cols_present(on_cols, df1, df2)
    zero_based = validate_coordinate_systems(df1, df2)
    eng = _join_kind_engine()
    t1, t2, probe, build, n_contigs, keys = _prepare(df1, df2, cols1, cols2, on_cols)
    pm, bm = _threshold_minima(probe, build, zero_based, f1, f2)
    kw = dict(strict=zero_based, n_contigs=n_contigs, min_overlap=mo, probe_min=pm, build_min=bm)
    k1, k2 = (keys[0], keys[1], keys[4]), (keys[2], keys[3], keys[4])
    if how == "left":
        p_idx, b_idx = eng.overlap_outer(probe, build, **kw)
        left, right = A.take_rows(t1, p_idx, chrom=k1), A.take_rows(t2, b_idx, nullable=True, chrom=k2)
        table = A.hconcat(A.with_suffix(left, suffixes[0]), A.with_suffix(right, suffixes[1]))
    else:
        table = A.take_rows(t1, eng.overlap_select(probe, build, mode=how, **kw), chrom=k1)
    return _finish_eager(table, output_type, zero_based, limit)


def nearest(
    df1,
    df2,
    suffixes: tuple = ("_1", "_2"),
    on_cols: Union[list, None] = None,
    cols1: Union[list, None] = ["chrom", "start", "end"],
    cols2: Union[list, None] = ["chrom", "start", "end"],
    k: int = 1,
    overlap: bool = True,
    distance: bool = True,
    output_type: str = "polars.LazyFrame",
    read_options=None,
    projection_pushdown: bool = True,
    limit: Union[int, None] = None,
    *,
    ignore_upstream: bool = False,
    ignore_downstream: bool = False,
    direction_col: Union[str, None] = None,
):
    """Find the k closest df2 intervals of every df1 interval (reference: range_op.py:259-340;
    column order df1+suffix[0], df2+suffix[1], distance: src/operation.rs:170-197).

    A df1 row with no candidate on its contig yields one row with null df2 columns and a null
    distance (unpinned in the reference; tests/test_native.py:133-140 drops such rows).  ``on_cols``: the k nearest df2
    intervals within the df1 row's group of equal (chrom, on values); a row whose group df2 lacks gets the one null row.

    Directional nearest: ``ignore_upstream`` leaves out the df2 intervals that lie before the df1 interval without
    overlapping it, ``ignore_downstream`` those that lie after it; overlapping intervals always count (unless
    ``overlap=False``), and the answer is the k closest of what remains, distances non-negative as ever.  Without
    ``direction_col`` every df1 row reads as "+": upstream = lower coordinates.  ``direction_col`` names a df1 column (usually
    the strand): a row whose value is the string "-" has upstream and downstream swapped, every other value ("+", ".", null)
    is "+"; a column df1 lacks is a ValueError.  ``on_cols=["strand"], direction_col="strand"`` is the strand-matched,
    strand-oriented nearest.  With both flags set only overlapping intervals are reported.  On the lazy / streaming outputs
    (``pyarrow.RecordBatchReader``, ``polars.LazyFrame``, ``limit``) the two orientations of one df1 batch may come out as
    separate result batches, each in df1 order (see ``nearest_batches``)."""
    on_cols = _validate_overlap_input(cols1, cols2, on_cols, suffixes, output_type)
    _check_on_cols_present(on_cols, df1, df2)
    plus, minus = _direction(df1, ignore_upstream, ignore_downstream, direction_col)
    directed = dict(ignore_upstream=ignore_upstream, ignore_downstream=ignore_downstream, direction_col=direction_col) if (plus or minus is not None) else {}
    zero_based = validate_coordinate_systems(df1, df2)
    if output_type == "polars.LazyFrame":
        lf = _polars_lazy_result(df1, df2, zero_based, limit, nearest_batches, suffixes=suffixes, cols1=cols1, cols2=cols2, k=k, overlap=overlap,
                                 distance=distance, batch_rows=_low_memory_batch_rows(), on_cols=on_cols, **directed)
        if lf is not None:
            return lf
    if output_type == "pyarrow.RecordBatchReader" or limit is not None:
        lazy = nearest_batches(df1, df2, suffixes, cols1, cols2, k=k, overlap=overlap, distance=distance,
                               batch_rows=_low_memory_batch_rows(), limit=limit, as_reader=True, on_cols=on_cols, **directed)
        return lazy if output_type == "pyarrow.RecordBatchReader" else A.from_arrow(lazy.read_all(), output_type, zero_based)
    t1, t2, probe, build, n_contigs, keys = _prepare(df1, df2, cols1, cols2, on_cols)
    if directed:
        idx, dist, nf = _nearest_oriented(default_engine(), t1, probe, build, n_contigs, zero_based, int(k), bool(overlap), direction_col, plus, minus)
    else:
        idx, dist, nf = default_engine().nearest(probe, build, strict=zero_based, n_contigs=n_contigs, k=int(k),
                                                 include_overlaps=bool(overlap))
    return A.from_arrow(_assemble_nearest(t1, t2, idx, dist, nf, suffixes, distance, keys), output_type, zero_based)


def count_overlaps(
    df1,
    df2,
    suffixes: tuple = ("", "_"),
    cols1: Union[list, None] = ["chrom", "start", "end"],
    cols2: Union[list, None] = ["chrom", "start", "end"],
    on_cols: Union[list, None] = None,
    output_type: str = "polars.LazyFrame",
    naive_query: bool = True,
    projection_pushdown: bool = True,
    limit: Union[int, None] = None,
    *,
    min_overlap: Union[int, None] = None,
    min_frac1: Union[float, None] = None,
    min_frac2: Union[float, None] = None,
):
    """Count the df2 intervals overlapping every df1 interval (reference: range_op.py:418-597).
    Output = df1 columns + ``count`` (Int64), df1 row order kept
    (tests/test_coordinate_system_metadata.py:1504-1506).  ``naive_query=False`` selects the
    reference's SQL sweep (range_op.py:512-597), which computes the same two-rank formula the
    device kernel uses; both values run the same kernel here, the sweep's output naming
    (key columns + suffixes[0]) is honoured, followed by the ``on_cols`` (df1's values).  ``on_cols``: only df2 intervals of
    the df1 row's group of equal (chrom, on values) are counted.

    ``min_overlap`` / ``min_frac1`` / ``min_frac2`` (keyword-only): count only the df2 intervals that pass the overlap
    thresholds -- the semantics, the float64 rule and the limits are those of ``overlap`` (which see); the count of a df1 row
    equals the number of its rows in the thresholded ``overlap``.  The pairs are counted on the device, never enumerated.  A
    thresholded call is eager whatever the ``output_type`` (``limit`` takes the head of the finished table,
    ``pyarrow.RecordBatchReader`` reads it); ``count_overlaps_batches`` takes no thresholds."""
    if min_overlap is not None or min_frac1 is not None or min_frac2 is not None:
        mo, f1, f2 = _validate_overlap_thresholds(min_overlap, min_frac1, min_frac2)
        on_cols = _validate_overlap_input(cols1, cols2, on_cols, suffixes, output_type)
        _check_on_cols_present(on_cols, df1, df2)
        zero_based = validate_coordinate_systems(df1, df2)
        eng = _threshold_engine()
        t1, t2, probe, build, n_contigs, _keys = _prepare(df1, df2, cols1, cols2, on_cols)
        pm, bm = _threshold_minima(probe, build, zero_based, f1, f2)
        counts = eng.count_overlaps_thresh(probe, build, strict=zero_based, n_contigs=n_contigs, min_overlap=mo, probe_min=pm, build_min=bm)
        c1 = list(DEFAULT_INTERVAL_COLUMNS if cols1 is None else cols1)
        return _finish_eager(_assemble_count(t1, counts, naive_query, c1, suffixes, on_cols), output_type, zero_based, limit)
    on_cols = _validate_overlap_input(cols1, cols2, on_cols, suffixes, output_type)
    _check_on_cols_present(on_cols, df1, df2)
    zero_based = validate_coordinate_systems(df1, df2)
    if output_type == "polars.LazyFrame":
        lf = _polars_lazy_result(df1, df2, zero_based, limit, count_overlaps_batches, suffixes=suffixes, cols1=cols1, cols2=cols2,
                                 batch_rows=_low_memory_batch_rows(), naive_query=naive_query, on_cols=on_cols)
        if lf is not None:
            return lf
    if output_type == "pyarrow.RecordBatchReader" or limit is not None:
        lazy = count_overlaps_batches(df1, df2, suffixes, cols1, cols2, batch_rows=_low_memory_batch_rows(), limit=limit,
                                      naive_query=naive_query, as_reader=True, on_cols=on_cols)
        return lazy if output_type == "pyarrow.RecordBatchReader" else A.from_arrow(lazy.read_all(), output_type, zero_based)
    t1, t2, probe, build, n_contigs, _keys = _prepare(df1, df2, cols1, cols2, on_cols)
    counts = default_engine().count_overlaps(probe, build, strict=zero_based, n_contigs=n_contigs)
    c1 = list(DEFAULT_INTERVAL_COLUMNS if cols1 is None else cols1)
    return A.from_arrow(_assemble_count(t1, counts, naive_query, c1, suffixes, on_cols), output_type, zero_based)


# ---- distance window: pb.window / pb.count_window ------------------------------------------------------

def _window_int(name, v) -> int:
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)):
        raise ValueError(f"{name} must be an int in [0, 2^32 - 1], got {v!r}")
    if v < 0 or v > WINDOW_MAX:
        raise ValueError(f"{name} must be in [0, 2^32 - 1], got {v}")
    return int(v)


def _validate_window(window, upstream, downstream, min_distance):
    """-> (upstream, downstream, min_distance) as ints; ``upstream`` / ``downstream`` default to ``window``.  ValueError: a value
    that is not an int (bools are refused), negative, or above 2^32 - 1."""
    w = _window_int("window", window)
    up = w if upstream is None else _window_int("upstream", upstream)
    down = w if downstream is None else _window_int("downstream", downstream)
    return up, down, _window_int("min_distance", min_distance)


def window_extents(is_minus, upstream: int, downstream: int):
    """The engine's extents of a call: -> (left, right, probe_left, probe_right).  Upstream of a "+" row is lower coordinates, so
    left = upstream and right = downstream; a "-" row (``is_minus``: bool per df1 row, or None without a direction column) has
    the two swapped.  Scalars when every row agrees (probe_left / probe_right are None then), else the two uint32 per-row columns
    (the scalars are then 0 and not read)."""
    if is_minus is None or upstream == downstream or not is_minus.any():
        return upstream, downstream, None, None
    if is_minus.all():
        return downstream, upstream, None, None
    up, down = np.uint32(upstream), np.uint32(downstream)
    return 0, 0, np.where(is_minus, down, up).astype(np.uint32), np.where(is_minus, up, down).astype(np.uint32)


def _window_setup(df1, df2, window, upstream, downstream, direction_col, min_distance, suffixes, on_cols, cols1, cols2, output_type):
    up, down, md = _validate_window(window, upstream, downstream, min_distance)
    on_cols = _validate_overlap_input(cols1, cols2, on_cols, suffixes, output_type)
    _check_on_cols_present(on_cols, df1, df2)
    if direction_col is not None:
        if not isinstance(direction_col, str):
            raise ValueError("direction_col must be the name of a df1 column")
        names = _schema_names(df1)
        if names is not None and direction_col not in names:
            raise ValueError(f"direction_col '{direction_col}' not found in {names}")
    zero_based = validate_coordinate_systems(df1, df2)
    t1, t2, probe, build, n_contigs, keys = _prepare(df1, df2, cols1, cols2, on_cols)
    is_minus = None
    if direction_col is not None:
        if direction_col not in t1.column_names:
            raise ValueError(f"direction_col '{direction_col}' not found in {t1.column_names}")
        is_minus = A.minus_rows(t1.column(direction_col))
    left, right, pl, pr = window_extents(is_minus, up, down)
    kw = dict(strict=zero_based, n_contigs=n_contigs, left=left, right=right, min_distance=md, probe_left=pl, probe_right=pr)
    return zero_based, t1, t2, probe, build, keys, is_minus, kw


def window(
    df1,
    df2,
    window: int = 1000,
    *,
    upstream: Union[int, None] = None,
    downstream: Union[int, None] = None,
    direction_col: Union[str, None] = None,
    min_distance: int = 0,
    distance: bool = True,
    signed_distance: bool = False,
    suffixes: tuple = ("_1", "_2"),
    on_cols: Union[list, None] = None,
    cols1: Union[list, None] = ["chrom", "start", "end"],
    cols2: Union[list, None] = ["chrom", "start", "end"],
    output_type: str = "polars.LazyFrame",
    limit: Union[int, None] = None,
):
    """Every df2 interval within a distance of every df1 interval, with the distance (bedtools ``window -w / -l / -r / -sw``,
    pyranges ``join(slack=)``, bioframe ``pair_by_distance``): the join between ``overlap`` ("shares a position") and ``nearest``
    ("the k closest").

    The distance ``d`` is ``nearest``'s, evaluated in 64 bits: 0 when the two intervals overlap, else the gap between them
    (``start2 - end1`` for a df2 interval after the df1 one, ``start1 - end2`` for one before it).  Bookended 0-based half-open
    intervals do not overlap and have d = 0; adjacent 1-based closed intervals have d = 1.  A pair is kept iff both intervals
    cover at least one position (zero-length rows and rows with start > end never pair), ``d >= min_distance`` (with
    ``min_distance >= 1`` overlapping intervals drop out), and the df2 interval overlaps the df1 one, or lies downstream of it
    with ``d <= downstream``, or upstream with ``d <= upstream``.  Rows with a null chrom or on-value never pair.
    ``bedtools window -w W`` is ``window=W - 1`` on 0-based half-open frames and ``window=W`` on 1-based closed ones.

    ``upstream`` / ``downstream`` default to ``window``; all three and ``min_distance`` are ints in [0, 2^32 - 1] (ValueError
    otherwise).  Without ``direction_col`` upstream is the lower coordinates.  ``direction_col`` names a df1 column (usually the
    strand; a column df1 lacks is a ValueError): a row whose value is the string "-" has upstream and downstream swapped, every
    other value ("+", ".", null) reads as "+" -- ``nearest``'s rule and bedtools ``-sw``.  ``min_distance`` above both extents
    is legal and gives the empty result.

    Output: every df1 column + suffixes[0], every df2 column + suffixes[1], then ``distance`` (Int64; dropped with
    ``distance=False``), one row per pair; the pairs of one df1 row are contiguous and ordered by (start, row) of the df2
    interval.  ``signed_distance=True``: negative for a df2 interval upstream of the df1 row, read along the row's strand when
    ``direction_col`` is set; otherwise the distance is non-negative.  ``on_cols``: pairs are formed within groups of equal
    (chrom, on values) only.

    The extents widen the candidate range of each df1 row on the device and the distance test runs there on every candidate;
    the distances come back with the pairs, nothing is padded, clamped or filtered on the host.  The call is EAGER whatever the
    ``output_type``: the finished table is converted, ``limit`` takes its head and ``pyarrow.RecordBatchReader`` reads it.  Out
    of scope: streaming entries (there is no ``window_batches``), sharding over several devices (the call runs on one), join
    kinds (``how=``) and the overlap thresholds of ``overlap``."""
    zero_based, t1, t2, probe, build, keys, is_minus, kw = _window_setup(df1, df2, window, upstream, downstream, direction_col, min_distance,
                                                                         suffixes, on_cols, cols1, cols2, output_type)
    p_idx, b_idx, dist = default_engine().overlap_window(probe, build, distance=bool(distance), **kw)
    table = _assemble_overlap(t1, t2, p_idx, b_idx, OverlapOutputMode.Join, False, suffixes, keys)
    if distance:
        if not signed_distance:
            dist = np.abs(dist)
        elif is_minus is not None and is_minus.any():
            dist = np.where(is_minus[p_idx], -dist, dist)
        table = table.append_column("distance", pa.array(dist, type=pa.int64()))
    return _finish_eager(table, output_type, zero_based, limit)


def count_window(
    df1,
    df2,
    window: int = 1000,
    *,
    upstream: Union[int, None] = None,
    downstream: Union[int, None] = None,
    direction_col: Union[str, None] = None,
    min_distance: int = 0,
    suffixes: tuple = ("", "_"),
    on_cols: Union[list, None] = None,
    cols1: Union[list, None] = ["chrom", "start", "end"],
    cols2: Union[list, None] = ["chrom", "start", "end"],
    output_type: str = "polars.LazyFrame",
    limit: Union[int, None] = None,
):
    """Count the df2 intervals within a distance of every df1 interval: df1's columns + ``count`` (Int64), df1 row order kept, as
    ``count_overlaps``.  The semantics and the arguments are those of ``window`` (which see); the count of a df1 row equals the
    number of its rows in ``window``.  The pairs are counted on the device, never enumerated.  Eager, one device, no streaming
    entry."""
    zero_based, t1, _t2, probe, build, _keys, _m, kw = _window_setup(df1, df2, window, upstream, downstream, direction_col, min_distance,
                                                                     suffixes, on_cols, cols1, cols2, output_type)
    counts = default_engine().count_window(probe, build, **kw)
    return _finish_eager(t1.append_column("count", pa.array(counts, type=pa.int64())), output_type, zero_based, limit)


# ---- sort-scan family ----------------------------------------------------

def coverage(
    df1,
    df2,
    suffixes: tuple = ("_1", "_2"),
    on_cols: Union[list, None] = None,
    cols1: Union[list, None] = ["chrom", "start", "end"],
    cols2: Union[list, None] = ["chrom", "start", "end"],
    output_type: str = "polars.LazyFrame",
    read_options=None,
    projection_pushdown: bool = True,
):
    """Covered positions of every df1 interval by the union of the df2 intervals (reference:
    range_op.py:342-415; executed by CountOverlapsProvider(coverage=true), src/operation.rs:306-350).
    Output = df1 columns + ``coverage`` (Int64), df1 row order kept (range_op_helpers.py:214-222, 317-318).
    ``on_cols``: only df2 intervals of the df1 row's group of equal (chrom, on values) cover it."""
    on_cols = _validate_overlap_input(cols1, cols2, on_cols, suffixes, output_type)
    _check_on_cols_present(on_cols, df1, df2)
    zero_based = validate_coordinate_systems(df1, df2)
    t1, t2, probe, build, n_contigs, _keys = _prepare(df1, df2, cols1, cols2, on_cols)
    cov = default_engine().coverage(probe, build, strict=zero_based, n_contigs=n_contigs)
    return A.from_arrow(t1.append_column("coverage", pa.array(cov, type=pa.int64())), output_type, zero_based)


def mean_depth(
    df1,
    df2,
    suffixes: tuple = ("_1", "_2"),
    on_cols: Union[list, None] = None,
    cols1: Union[list, None] = ["chrom", "start", "end"],
    cols2: Union[list, None] = ["chrom", "start", "end"],
    output_type: str = "polars.LazyFrame",
    read_options=None,
    projection_pushdown: bool = True,
):
    """Total overlap and mean depth of df2 over every df1 interval: ``bases`` = the positions the df1 row shares with each df2
    interval of its contig, summed over the df2 intervals (the integral of df2's ``depth`` over the row; ``coverage`` is the
    integral of min(depth, 1), so coverage <= bases <= count_overlaps * length), ``mean_depth`` = bases / length of the row.
    The per-window summary of ``mosdepth --by`` / ``bedtools coverage -mean`` for an interval frame of reads or fragments.

    Output = df1 columns + ``bases`` (Int64) + ``mean_depth`` (Float64, null where the df1 row covers no position), df1 row
    order kept.  0-based frames are half-open (intervals that only touch share nothing), 1-based frames closed.  Rows of
    either frame that cover no position, and rows with a null chrom, share nothing.
    ``on_cols``: only df2 intervals of the df1 row's group of equal (chrom, on values) count; a null on-value matches nothing."""
    on_cols = _validate_overlap_input(cols1, cols2, on_cols, suffixes, output_type)
    _check_on_cols_present(on_cols, df1, df2)
    zero_based = validate_coordinate_systems(df1, df2)
    t1, t2, probe, build, n_contigs, _keys = _prepare(df1, df2, cols1, cols2, on_cols)
    bases = default_engine().overlap_bases(probe, build, strict=zero_based, n_contigs=n_contigs)
    length = np.asarray(probe[2], np.int64) - np.asarray(probe[1], np.int64) + (0 if zero_based else 1)
    has_positions = length > 0
    mean = np.divide(bases.astype(np.float64), length.astype(np.float64), out=np.zeros(len(bases), np.float64), where=has_positions)
    t = t1.append_column("bases", pa.array(bases, type=pa.int64()))
    t = t.append_column("mean_depth", pa.array(mean, type=pa.float64(), mask=~has_positions))
    return A.from_arrow(t, output_type, zero_based)


_PROFILE_ANCHORS = ("start", "end", "center")


def profile_windows(start, end, zero_based: bool, anchor=None, upstream: int = 0, downstream: int = 0, is_minus=None):
    """The window of every df1 row of ``depth_profile`` -> (window start, window end) as int64 arrays in the frames' own coordinate
    convention.  ``anchor=None``: the row itself.  Otherwise, in half-open position space with S the row's first position and L its
    number of positions, the window is [a - upstream, a + downstream) around a = S ("start"), S + L ("end": one past the last
    position) or S + L // 2 ("center"); for a row flagged in ``is_minus`` "start" / "end" and upstream / downstream swap.  A row
    that covers no position (end before start) reads as L = 0 from its start: all three anchors are S."""
    s = np.asarray(start, np.int64)
    e = np.asarray(end, np.int64)
    if anchor is None:
        return s.copy(), e.copy()
    w = 0 if zero_based else 1
    length = np.maximum(e - s + w, 0)
    minus = np.zeros(len(s), bool) if is_minus is None else np.asarray(is_minus, bool)
    if anchor == "center":
        a = s + length // 2
    else:
        a = np.where((anchor == "end") != minus, s + length, s)
    lo = a - np.where(minus, np.int64(downstream), np.int64(upstream))
    hi = a + np.where(minus, np.int64(upstream), np.int64(downstream))
    return lo, hi - w


def profile_bin_lengths(w_start, w_end, zero_based: bool, n_bins: int, reverse=None) -> np.ndarray:
    """Positions of every bin of every window, int64 (n, n_bins): bin j of a window of L positions is
    [floor(j L / n_bins), floor((j + 1) L / n_bins)) from its first position (L <= 0: every bin is empty); the rows flagged in
    ``reverse`` right to left."""
    length = np.maximum(np.asarray(w_end, np.int64) - np.asarray(w_start, np.int64) + (0 if zero_based else 1), 0)
    edges = length[:, None] * np.arange(n_bins + 1, dtype=np.int64)[None, :] // np.int64(n_bins)      # j L < 2^13 x 2^32
    lens = np.diff(edges, axis=1)
    if reverse is not None:
        rev = np.asarray(reverse, bool)
        lens[rev] = lens[rev, ::-1]
    return lens


def _profile_setup(df1, df2, n_bins, anchor, upstream, downstream, direction_col, on_cols, cols1, cols2, output, outputs, output_type):
    """What ``depth_profile`` and ``signal_profile`` share: the argument checks in the order their messages have always come, the
    encoded frames and the int32 window of every df1 row.
    -> (n_bins, zero_based, t1, t2, build, n_contigs, on_cols, is_minus, w_start, w_end, windows)."""
    on_cols = _validate_overlap_input(cols1, cols2, on_cols, ("_1", "_2"), "pyarrow.Table" if output_type == "numpy.ndarray" else output_type)
    if isinstance(n_bins, (bool, np.bool_)) or not isinstance(n_bins, (int, np.integer)) or not 1 <= int(n_bins) <= DEPTH_PROFILE_MAX_BINS:
        raise ValueError(f"n_bins must be an int in 1 .. {DEPTH_PROFILE_MAX_BINS}, got {n_bins!r}")
    n_bins = int(n_bins)
    if output not in outputs:
        raise ValueError(f"output must be {' or '.join(repr(o) for o in outputs) if len(outputs) == 2 else 'one of ' + str(outputs)}, got {output!r}")
    if anchor is not None and anchor not in _PROFILE_ANCHORS:
        raise ValueError(f"anchor must be None or one of {_PROFILE_ANCHORS}, got {anchor!r}")
    for name, v in (("upstream", upstream), ("downstream", downstream)):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 0 <= int(v) <= 0xffffffff:
            raise ValueError(f"{name} must be an int in 0 .. 2^32 - 1, got {v!r}")
    upstream, downstream = int(upstream), int(downstream)
    if anchor is None and (upstream or downstream):
        raise ValueError(f"upstream / downstream need an anchor ('start', 'end' or 'center'), got upstream={upstream}, downstream={downstream} with anchor=None")
    if anchor is not None and upstream + downstream < 1:
        raise ValueError(f"anchor={anchor!r} needs upstream + downstream >= 1, got {upstream} + {downstream}")
    if direction_col is not None:
        if not isinstance(direction_col, str):
            raise ValueError("direction_col must be the name of a df1 column")
        names = _schema_names(df1)
        if names is not None and direction_col not in names:
            raise ValueError(f"direction_col '{direction_col}' not found in {names}")
    _check_on_cols_present(on_cols, df1, df2)
    zero_based = validate_coordinate_systems(df1, df2)
    t1, t2, probe, build, n_contigs, _keys = _prepare(df1, df2, cols1, cols2, on_cols)
    if direction_col is not None and direction_col not in t1.column_names:
        raise ValueError(f"direction_col '{direction_col}' not found in {t1.column_names}")
    is_minus = A.minus_rows(t1.column(direction_col)) if direction_col is not None else None
    w_start, w_end = profile_windows(probe[1], probe[2], zero_based, anchor, upstream, downstream, is_minus)
    bad = np.flatnonzero((w_start < -0x80000000) | (w_start > 0x7fffffff) | (w_end < -0x80000000) | (w_end > 0x7fffffff))
    if bad.size:
        r = int(bad[0])
        raise ValueError(f"the window of df1 row {r} leaves the int32 range: [{int(w_start[r])}, {int(w_end[r])}] "
                         f"(row {int(probe[1][r])} .. {int(probe[2][r])}, anchor={anchor!r}, upstream={upstream}, downstream={downstream})")
    windows = (probe[0], w_start.astype(np.int32), w_end.astype(np.int32))
    return n_bins, zero_based, t1, t2, build, n_contigs, on_cols, is_minus, w_start, w_end, windows


def depth_profile(
    df1,
    df2,
    n_bins: int = 100,
    anchor: Union[str, None] = None,
    upstream: int = 0,
    downstream: int = 0,
    direction_col: Union[str, None] = None,
    on_cols: Union[list, None] = None,
    cols1: Union[list, None] = ["chrom", "start", "end"],
    cols2: Union[list, None] = ["chrom", "start", "end"],
    output: str = "mean",
    output_type: str = "polars.LazyFrame",
):
    """Binned depth of df2 across every df1 row: a rows x ``n_bins`` matrix for a heat map or an average profile (deepTools
    ``computeMatrix``, ngs.plot, ``bedtools makewindows -n`` + ``coverage -mean``), made on the device from the window of each row.

    The window of a df1 row of L positions from S is cut at S + floor(j L / n_bins), j = 0 .. n_bins: bin lengths differ by at
    most one and sum to L.  Per bin, ``bases`` = the positions it shares with each df2 interval of the row's contig, summed over
    the df2 intervals -- what ``mean_depth`` gives for the bin as a df1 row, so a row of the matrix sums to the window's
    ``mean_depth`` ``bases``.  A window with L < n_bins has empty bins, one with L <= 0 only empty bins: ``bases`` 0, mean null.

    ``anchor=None`` (scale-regions): the window is the df1 row itself; ``upstream`` / ``downstream`` must be 0.
    ``anchor`` = ``"start"`` | ``"end"`` | ``"center"`` (reference-point): the window is [a - upstream, a + downstream) in
    half-open position space, a = the row's first position, one past its last position, or S + L // 2 (a row that covers no
    position reads as L = 0: a = S for every anchor); ``upstream`` and
    ``downstream`` are ints >= 0 with ``upstream + downstream >= 1``.  Windows are computed in int64; one that leaves the int32
    range is a ValueError naming the first such row.  Negative coordinates are legal, the depth there is 0.
    ``direction_col`` names a df1 column of "+" / "-" (any other value or a null reads as "+"): a "-" row is read along its
    strand, i.e. its profile comes back right to left, and in reference-point mode "start" / "end" and ``upstream`` /
    ``downstream`` swap for it -- a minus gene's TSS is its end.

    ``output="mean"``: Float64 bases / bin length, null for an empty bin; ``output="bases"``: Int64.  The result is df1's columns
    plus one column ``profile`` of Arrow ``fixed_size_list<...>[n_bins]`` laid over the matrix, df1 row order kept;
    ``output_type="numpy.ndarray"`` returns the bare (n, n_bins) matrix (NaN for null in the mean form).  0-based frames are
    half-open, 1-based frames closed.  Rows of df2 that cover no position and rows with a null chrom share nothing.
    ``on_cols``: only df2 intervals of the df1 row's group of equal (chrom, on values) count; a null on-value matches nothing.

    Eager.  A value / weight column on df2 (bedGraph signal) is ``signal_profile``'s.  Not covered: streaming inputs or outputs,
    several devices, per-bin statistics other than the sum / mean."""
    n_bins, zero_based, t1, t2, build, n_contigs, on_cols, is_minus, w_start, w_end, windows = _profile_setup(
        df1, df2, n_bins, anchor, upstream, downstream, direction_col, on_cols, cols1, cols2, output, ("mean", "bases"), output_type)
    bases = default_engine().depth_profile(windows, is_minus, n_bins, build, strict=zero_based, n_contigs=n_contigs)
    if output == "bases":
        if output_type == "numpy.ndarray":
            return bases
        values = pa.array(bases.reshape(-1), type=pa.int64())
    else:
        lens = profile_bin_lengths(w_start, w_end, zero_based, n_bins, is_minus)
        empty = lens <= 0
        mean = np.divide(bases.astype(np.float64), lens.astype(np.float64), out=np.full(bases.shape, np.nan), where=~empty)
        if output_type == "numpy.ndarray":
            return mean
        values = pa.array(mean.reshape(-1), type=pa.float64(), mask=empty.reshape(-1))
    t = t1.append_column("profile", pa.FixedSizeListArray.from_arrays(values, n_bins))
    return _finish_eager(t, output_type, zero_based, None)


def _validate_thresholds(thresholds) -> list:
    """-> the thresholds as a list of ints: an iterable of at most 8 distinct ints >= 1 (empty: max_depth only)."""
    if isinstance(thresholds, (str, bytes)) or not hasattr(thresholds, "__iter__"):
        raise ValueError("thresholds must be an iterable of ints >= 1")
    out = []
    for t in thresholds:
        if isinstance(t, (bool, np.bool_)) or not isinstance(t, (int, np.integer)):
            raise ValueError(f"thresholds must be ints >= 1, got {t!r}")
        if int(t) < 1 or int(t) > 0x7fffffff:
            raise ValueError(f"thresholds must be ints in 1 .. 2^31 - 1, got {t!r}")
        out.append(int(t))
    if len(out) > 8:
        raise ValueError(f"at most 8 thresholds per call, got {len(out)}")
    if len(set(out)) != len(out):
        raise ValueError(f"thresholds must be distinct, got {out}")
    return out


def depth_summary(
    df1,
    df2,
    thresholds=(1,),
    suffixes: tuple = ("_1", "_2"),
    on_cols: Union[list, None] = None,
    cols1: Union[list, None] = ["chrom", "start", "end"],
    cols2: Union[list, None] = ["chrom", "start", "end"],
    output_type: str = "polars.LazyFrame",
    read_options=None,
    projection_pushdown: bool = True,
):
    """How deep df2 piles up over every df1 interval: ``max_depth`` = the largest number of df2 intervals of its contig that
    cover one position of the df1 row, and per threshold T ``bases_ge_<T>`` = the number of the row's positions that at least T
    df2 intervals cover.  The per-target columns of ``mosdepth --thresholds`` and of ``bedtools map -o max`` on a bedGraph of
    ``pb.depth(df2)``, for an interval frame of reads or fragments, in one call.

    Identities: ``bases_ge_1`` = ``pb.coverage``'s column; the sum of ``bases_ge_<T>`` over T = 1 .. max(max_depth) =
    ``pb.mean_depth``'s ``bases``; ``max_depth`` <= ``pb.count_overlaps``'s count; ``max_depth`` = 0 exactly where the coverage
    is 0; ``bases_ge_<T>`` does not grow with T and is positive exactly where T <= ``max_depth``.

    Output = df1 columns + ``max_depth`` (Int64) + one ``bases_ge_<T>`` (Int64) per threshold, in the given order, df1 row
    order kept.  ``thresholds``: an iterable of at most 8 distinct ints >= 1; empty gives ``max_depth`` only.  0-based frames
    are half-open (intervals that only touch share nothing), 1-based frames closed.  Rows of either frame that cover no
    position, and rows with a null chrom, share nothing (such df1 rows get 0 in every column).
    ``on_cols``: only df2 intervals of the df1 row's group of equal (chrom, on values) count; a null on-value matches nothing.
    More than 8 thresholds: ``pb.depth_histogram``; quantiles: ``pb.depth_quantiles``."""
    on_cols = _validate_overlap_input(cols1, cols2, on_cols, suffixes, output_type)
    thresholds = _validate_thresholds(thresholds)
    _check_on_cols_present(on_cols, df1, df2)
    zero_based = validate_coordinate_systems(df1, df2)
    t1, t2, probe, build, n_contigs, _keys = _prepare(df1, df2, cols1, cols2, on_cols)
    max_depth, bases_ge = default_engine().depth_summary(probe, build, strict=zero_based, n_contigs=n_contigs, thresholds=thresholds)
    t = t1.append_column("max_depth", pa.array(max_depth.astype(np.int64), type=pa.int64()))
    for k, thr in enumerate(thresholds):
        t = t.append_column(f"bases_ge_{thr}", pa.array(bases_ge[k], type=pa.int64()))
    return A.from_arrow(t, output_type, zero_based)


def _validate_max_depth(max_depth) -> int:
    from ._engine import MAX_HIST_DEPTH
    if isinstance(max_depth, (bool, np.bool_)) or not isinstance(max_depth, (int, np.integer)) or not 1 <= int(max_depth) <= MAX_HIST_DEPTH:
        raise ValueError(f"max_depth must be an int in 1 .. {MAX_HIST_DEPTH}, got {max_depth!r}")
    return int(max_depth)


def _histogram_engine(what: str):
    eng = default_engine()
    if not hasattr(eng, "depth_hist") or not hasattr(eng, "depth_hist_contigs"):
        raise NotImplementedError(f"{what} needs a single-device engine; the default engine is a {type(eng).__name__} "
                                  "(several devices), which has no histogram kernel")
    return eng


def depth_histogram(
    df1,
    df2,
    max_depth: int = 100,
    output: str = "bases",
    cumulative: bool = False,
    suffixes: tuple = ("_1", "_2"),
    on_cols: Union[list, None] = None,
    cols1: Union[list, None] = ["chrom", "start", "end"],
    cols2: Union[list, None] = ["chrom", "start", "end"],
    output_type: str = "polars.LazyFrame",
):
    """The distribution of df2's depth over every df1 interval: bin d of a row = the number of its positions that exactly d df2
    intervals of its contig cover, d = 0 .. ``max_depth`` - 1, and the last bin = the positions covered ``max_depth`` deep or
    deeper.  ``bedtools coverage -hist`` per target region and mosdepth's per-region distribution, in one call, with as many bins
    as wanted (``max_depth`` in 1 .. 1023) where ``depth_summary`` takes 8 thresholds.

    A row sums to its number of positions; bin 0 holds the uncovered ones.  Identities: the sum of the bins d >= T =
    ``depth_summary``'s ``bases_ge_<T>`` (T = 1: ``pb.coverage``); when ``max_depth`` exceeds every depth, the sum of d * bin d =
    ``pb.mean_depth``'s ``bases``.

    Output = df1 columns + ``histogram``, an Arrow ``fixed_size_list<...>[max_depth + 1]``, df1 row order kept.
    ``output="bases"``: Int64; ``output="fraction"``: Float64, each bin divided by the row's positions, null for a row without
    a position.  ``cumulative=True`` turns bin d into "depth >= d" (mosdepth's distribution: bin 0 = all positions of the row, resp.
    1.0).  ``output_type="numpy.ndarray"`` returns the bare (n, max_depth + 1) matrix (NaN for null in the fraction form).
    0-based frames are half-open, 1-based frames closed.  Rows of either frame that cover no position, and rows with a null
    chrom, share nothing (such df1 rows get zeros).  ``on_cols``: only df2 intervals of the df1 row's group of equal (chrom, on
    values) count; a null on-value matches nothing.

    Eager, one device.  Quantiles: ``pb.depth_quantiles``.  Not covered: streaming inputs or outputs, a weighted (signal)
    histogram."""
    on_cols = _validate_overlap_input(cols1, cols2, on_cols, suffixes, "pyarrow.Table" if output_type == "numpy.ndarray" else output_type)
    max_depth = _validate_max_depth(max_depth)
    if output not in ("bases", "fraction"):
        raise ValueError(f"output must be 'bases' or 'fraction', got {output!r}")
    _check_on_cols_present(on_cols, df1, df2)
    zero_based = validate_coordinate_systems(df1, df2)
    t1, t2, probe, build, n_contigs, _keys = _prepare(df1, df2, cols1, cols2, on_cols)
    hist = _histogram_engine("depth_histogram").depth_hist(probe, build, strict=zero_based, n_contigs=n_contigs, max_depth=max_depth)
    positions = hist.sum(axis=1)
    if cumulative:
        hist = np.ascontiguousarray(np.cumsum(hist[:, ::-1], axis=1)[:, ::-1])
    if output == "bases":
        if output_type == "numpy.ndarray":
            return hist
        values = pa.array(hist.reshape(-1), type=pa.int64())
    else:
        none = positions <= 0
        frac = np.divide(hist.astype(np.float64), positions.astype(np.float64)[:, None], out=np.full(hist.shape, np.nan), where=~none[:, None])
        if output_type == "numpy.ndarray":
            return frac
        values = pa.array(frac.reshape(-1), type=pa.float64(), mask=np.repeat(none, max_depth + 1))
    t = t1.append_column("histogram", pa.FixedSizeListArray.from_arrays(values, max_depth + 1))
    return _finish_eager(t, output_type, zero_based, None)


def quantile_ranks(length, q):
    """The order statistics a quantile of a list of ``length`` sorted values rests on, with numpy's convention: h = q (L - 1)
    evaluated in IEEE float64 -> (lo = floor(h), hi = ceil(h), both int64, g = h - lo float64).  ``length``: int64 lengths (any
    shape), ``q``: a float in [0, 1] or an array that broadcasts against the lengths.  A length <= 0 has no order statistic: lo =
    hi = -1, g = 0.  Pure host arithmetic, vectorised; L - 1 < 2^53 is exact in float64, so h is the correctly rounded product."""
    length = np.asarray(length, dtype=np.int64)
    qf = np.asarray(q, dtype=np.float64)
    if qf.size and not ((qf >= 0.0) & (qf <= 1.0)).all():
        raise ValueError(f"a quantile must lie in [0, 1], got {q!r}")
    length, qf = np.broadcast_arrays(length, qf)
    ok = length > 0
    h = qf * np.where(ok, length - 1, 0).astype(np.float64)
    lo_f = np.floor(h)
    lo = np.where(ok, lo_f.astype(np.int64), -1)
    hi = np.where(ok, np.ceil(h).astype(np.int64), -1)
    g = np.where(ok, h - lo_f, 0.0)
    assert (hi[ok] < length[ok]).all() and (lo[ok] >= 0).all() and (hi - lo <= 1).all()
    return lo, hi, g


QUANTILE_METHODS = ("lower", "higher", "midpoint", "linear")
MAX_QUANTILES = 8


def _validate_quantiles(q, method) -> list:
    if method not in QUANTILE_METHODS:
        raise ValueError(f"method must be one of {', '.join(map(repr, QUANTILE_METHODS))}, got {method!r}")
    if isinstance(q, (int, float, np.integer, np.floating)) and not isinstance(q, (bool, np.bool_)):
        q = (q,)
    try:
        qs = [float(x) for x in q]
    except (TypeError, ValueError):
        raise ValueError(f"q must be a float or an iterable of floats in [0, 1], got {q!r}") from None
    if not 1 <= len(qs) <= MAX_QUANTILES:
        raise ValueError(f"between 1 and {MAX_QUANTILES} quantiles per call, got {len(qs)}")
    for x in qs:
        if not 0.0 <= x <= 1.0:                            # (a NaN fails both comparisons)
            raise ValueError(f"a quantile must lie in [0, 1], got {x!r}")
    if len(set(qs)) != len(qs):
        raise ValueError(f"the quantiles must be distinct, got {qs!r}")
    return qs


def _quantile_engine(what: str):
    eng = default_engine()
    if not hasattr(eng, "depth_quantiles"):
        raise NotImplementedError(f"{what} needs a single-device engine; the default engine is a {type(eng).__name__} "
                                  "(several devices), which has no quantile kernel")
    return eng


def _depth_quantile_matrix(what, df1, df2, qs, method, suffixes, on_cols, cols1, cols2, output_type):
    """-> (t1, zero_based, values (n, len(qs)) int64 or float64, null bool[n])"""
    on_cols = _validate_overlap_input(cols1, cols2, on_cols, suffixes, "pyarrow.Table" if output_type == "numpy.ndarray" else output_type)
    _check_on_cols_present(on_cols, df1, df2)
    zero_based = validate_coordinate_systems(df1, df2)
    t1, t2, probe, build, n_contigs, _keys = _prepare(df1, df2, cols1, cols2, on_cols)
    lo, hi, g = quantile_ranks(_side_lengths(probe, zero_based)[:, None], np.asarray(qs, np.float64)[None, :])
    if method in ("lower", "higher"):
        ranks = lo if method == "lower" else hi
    else:                                                  # lo and hi of each quantile side by side
        ranks = np.stack([lo, hi], axis=2).reshape(len(lo), 2 * len(qs))
    v = _quantile_engine(what).depth_quantiles(probe, build, strict=zero_based, n_contigs=n_contigs, ranks=ranks).astype(np.int64)
    null = (v < 0).any(axis=1)                             # a row without a position, or outside the dictionary (null chrom)
    if method in ("lower", "higher"):
        return t1, zero_based, v, null
    vlo, vhi = v[:, 0::2].astype(np.float64), v[:, 1::2].astype(np.float64)
    val = (vlo + vhi) / 2.0 if method == "midpoint" else vlo + (vhi - vlo) * g
    return t1, zero_based, np.where(null[:, None], np.nan, val), null


def depth_quantiles(
    df1,
    df2,
    q=(0.25, 0.5, 0.75),
    method: str = "lower",
    suffixes: tuple = ("_1", "_2"),
    on_cols: Union[list, None] = None,
    cols1: Union[list, None] = ["chrom", "start", "end"],
    cols2: Union[list, None] = ["chrom", "start", "end"],
    output_type: str = "polars.LazyFrame",
):
    """Exact quantiles of df2's depth over the positions of every df1 interval: the median depth of a region and its quartiles
    (mosdepth ``--use-median``; what a CNV / target-QC normaliser divides by), without a histogram leaving the device and for any
    depth up to 2^31 - 1.

    For a df1 row with L >= 1 positions let v[0] <= ... <= v[L - 1] be the depths of its positions, sorted: the number of df2
    intervals of its contig that cover the position, 0 for an uncovered one.  For a quantile q in [0, 1]: h = q (L - 1) in float64,
    lo = floor(h), hi = ceil(h), g = h - lo (``quantile_ranks``), and ``method``, with numpy's names, selects
    ``"lower"`` (default) v[lo] | ``"higher"`` v[hi] (both Int64) | ``"midpoint"`` (v[lo] + v[hi]) / 2 | ``"linear"``
    v[lo] + (v[hi] - v[lo]) g (both Float64).  The device answers the order statistics; the quantile is host arithmetic on them.

    Output = df1 columns + one column per quantile, ``depth_q<q>`` with q as ``repr(float(q))`` (``depth_q0.5``), in the given
    order, df1 row order kept.  ``q``: 1 .. 8 distinct values in [0, 1], else ``ValueError``.  Rows without a position (empty,
    inverted, null chrom or null on-value) get null.  ``output_type="numpy.ndarray"`` returns the bare (n, len(q)) matrix: int64
    with -1 for null (``"lower"``, ``"higher"``), float64 with NaN for null (``"midpoint"``, ``"linear"``).
    0-based frames are half-open, 1-based frames closed.  ``on_cols``: only df2 intervals of the df1 row's group of equal
    (chrom, on values) count.  Identities: q = 1 gives ``depth_summary``'s ``max_depth``; q = 0 is positive exactly where
    ``pb.coverage`` equals the row's length.

    Eager, one device (a several-device engine raises ``NotImplementedError``).  Not covered: streaming inputs or outputs,
    several devices, a weighted (signal) quantile, per-contig / genome-wide quantiles, more than 8 quantiles per call."""
    qs = _validate_quantiles(q, method)
    t1, zero_based, val, null = _depth_quantile_matrix("depth_quantiles", df1, df2, qs, method, suffixes, on_cols, cols1, cols2, output_type)
    if output_type == "numpy.ndarray":
        return np.where(null[:, None], -1, val) if val.dtype == np.int64 else val
    typ = pa.int64() if val.dtype == np.int64 else pa.float64()
    for k, x in enumerate(qs):
        t1 = t1.append_column(f"depth_q{x!r}", pa.array(np.ascontiguousarray(val[:, k]), type=typ, mask=null))
    return _finish_eager(t1, output_type, zero_based, None)


def median_depth(
    df1,
    df2,
    suffixes: tuple = ("_1", "_2"),
    on_cols: Union[list, None] = None,
    cols1: Union[list, None] = ["chrom", "start", "end"],
    cols2: Union[list, None] = ["chrom", "start", "end"],
    output_type: str = "polars.LazyFrame",
):
    """The median depth of df2 over every df1 interval: ``depth_quantiles`` with ``q = 0.5`` and ``method="lower"`` (the value at
    rank floor((L - 1) / 2) of the row's L sorted per-position depths, uncovered positions at 0), as one Int64 column
    ``median_depth``; null for a row without a position.  The robust counterpart of ``pb.mean_depth``, which one PCR pile-up
    ruins.  ``output_type="numpy.ndarray"``: the bare (n, 1) int64 matrix, -1 for null.

    Eager, one device.  Not covered: streaming inputs or outputs, several devices, a weighted (signal) median, a per-contig /
    genome-wide median."""
    t1, zero_based, val, null = _depth_quantile_matrix("median_depth", df1, df2, [0.5], "lower", suffixes, on_cols, cols1, cols2, output_type)
    if output_type == "numpy.ndarray":
        return np.where(null[:, None], -1, val)
    t1 = t1.append_column("median_depth", pa.array(np.ascontiguousarray(val[:, 0]), type=pa.int64(), mask=null))
    return _finish_eager(t1, output_type, zero_based, None)


def genome_depth_histogram(
    df,
    genome=None,
    max_depth: int = 100,
    on_cols: Union[list, None] = None,
    cols: Union[list, None] = ["chrom", "start", "end"],
    output_type: str = "polars.LazyFrame",
):
    """The distribution of the frame's depth per contig and over the whole genome: ``bedtools genomecov``'s default table.

    Rows (chrom, <on_cols...>, depth, bases, size, fraction): ``bases`` = the positions of the contig that exactly ``depth`` rows of
    ``df`` cover, ``size`` = the contig's length, ``fraction`` = bases / size; per contig in sorted-name order, depth ascending, only
    rows with ``bases`` > 0.  The last bin is labelled ``max_depth`` and means "``max_depth`` or deeper" (``genomecov -max``).  After the
    contigs a block with chrom = "genome" sums all contigs of ``genome``.

    ``genome``: a {contig: length} dict or a two-column (name, length) frame.  The depth-0 row of a contig is its length minus
    its covered positions; a contig of ``genome`` that ``df`` never touches gets its single depth-0 row.  A contig of ``df`` that
    ``genome`` lacks is a ValueError, and so is a row that covers a position outside [0, length) (0-based frames) or
    [1, length] (1-based frames); the message names the first such row.
    ``genome=None``: contig lengths are unknown, so there are no depth-0 rows and no ``size`` / ``fraction`` columns, and the final
    block, the totals over all contigs, is named "all".

    ``on_cols``: the depth per group of equal (chrom, on values), e.g. per strand: rows in (chrom, on values, depth) order, and one
    "genome" / "all" block per combination of on values that occurs in ``df``; rows with a null on-value are dropped, as rows
    with a null chrom are.  Rows that cover no position contribute nothing.

    Eager, one device."""
    on_cols = _validate_overlap_input(cols, cols, on_cols, ("_1", "_2"), output_type)
    max_depth = _validate_max_depth(max_depth)
    _check_on_cols_present(on_cols, df)
    zero_based = validate_coordinate_system_single(df)
    cols = list(DEFAULT_INTERVAL_COLUMNS if cols is None else cols)
    t = A.to_arrow(df)
    side, n_contigs, dictionary = A.encode_frame(t, cols)
    names = [str(x) for x in pc.cast(dictionary, pa.string()).to_pylist()]            # chrom id -> name, sorted
    lengths = None
    if genome is not None:
        gnames, lengths = _genome_lengths(genome)
        where = {k: j for j, k in enumerate(gnames)}
        unknown = [k for k in names if k not in where]
        if unknown:
            raise ValueError(f"genome lacks contig {unknown[0]!r} of df" + (f" (and {len(unknown) - 1} more)" if len(unknown) > 1 else ""))
        to_out = np.array([where[k] for k in names], np.int64)                          # chrom id -> row of the genome
        c, s, e = (np.asarray(a).astype(np.int64) for a in side)
        known = c >= 0
        ln = lengths[to_out[np.where(known, c, 0)]] if len(names) else np.zeros(len(c), np.int64)
        if zero_based:
            out_of = known & (s < e) & ((s < 0) | (e > ln))
        else:
            out_of = known & (s <= e) & ((s < 1) | (e > ln))
        bad = np.flatnonzero(out_of)
        if bad.size:
            r = int(bad[0])
            raise ValueError(f"df row {r} ({names[int(c[r])]}: {int(s[r])} .. {int(e[r])}) reaches outside the contig, whose length is {int(ln[r])}"
                             + (" ([0, length), 0-based)" if zero_based else " ([1, length], 1-based)"))
        out_names = gnames
    else:
        to_out = np.arange(len(names), dtype=np.int64)
        out_names = names
    gchrom = dicts = None
    if on_cols:
        (codes,), cards, dicts, _ = A.encode_on_cols([t], on_cols)
        empty = (np.empty(0, np.int32),) * 3
        _, side, groups, table = A.group_sides(empty, side, n_contigs, [np.empty(0, np.int32)] * len(on_cols), codes, cards, on_cols)
        n_contigs, gchrom = max(groups, 1), np.asarray(table)[:groups]
    keep = side[0] >= 0                                   # rows with a null chrom (or on-value) belong to no contig
    side = tuple(a[keep] for a in side) if not keep.all() else side
    bins = max_depth + 1
    hist = _histogram_engine("genome_depth_histogram").depth_hist_contigs(side, strict=zero_based, n_contigs=n_contigs, max_depth=max_depth) if n_contigs > 0 else np.zeros((0, bins), np.int64)
    # H[contig of the output, combination of on values, depth]
    if gchrom is None:
        combos = np.zeros((1, 0), np.int64)
        H = np.zeros((len(out_names), 1, bins), np.int64)
        H[to_out, 0, :] = hist[:len(names)]
    else:
        combos, which = np.unique(gchrom[:, 1:].astype(np.int64), axis=0, return_inverse=True) if len(gchrom) else (np.zeros((0, len(on_cols)), np.int64), np.zeros(0, np.int64))
        H = np.zeros((len(out_names), len(combos), bins), np.int64)
        if len(gchrom):
            H[to_out[gchrom[:, 0].astype(np.int64)], np.asarray(which).reshape(-1), :] = hist[:len(gchrom)]
    size = None
    if lengths is not None:
        H[:, :, 0] = lengths[:, None] - H[:, :, 1:].sum(axis=2)
        size = np.broadcast_to(lengths[:, None, None], H.shape)
    total = H.sum(axis=0, keepdims=True)
    ci, ki, di = np.nonzero(H)
    _tc, tk, td = np.nonzero(total)
    chrom = pa.array([out_names[j] for j in ci] + ["genome" if lengths is not None else "all"] * len(tk), type=pa.string())
    data = {cols[0]: chrom}
    for j, name in enumerate(on_cols or ()):
        code = np.concatenate([combos[ki, j], combos[tk, j]]).astype(np.int32)
        data[name] = A.cast_on_values(pc.take(dicts[j], pa.array(code, type=pa.int32())), t.schema.field(name).type)
    bases = np.concatenate([H[ci, ki, di], total[0, tk, td]])
    data["depth"] = pa.array(np.concatenate([di, td]).astype(np.int64))
    data["bases"] = pa.array(bases)
    if lengths is not None:
        sz = np.concatenate([size[ci, ki, di], np.full(len(tk), int(lengths.sum()), np.int64)])
        data["size"] = pa.array(sz)
        data["fraction"] = pa.array(bases.astype(np.float64) / sz.astype(np.float64))
    return A.from_arrow(pa.table(data), output_type, zero_based)


_AGG_OP_NAMES = ("sum", "min", "max", "mean", "count")
_MAX_AGG_COLS = 16          # include/ivjoin.h: IVJ_MAX_AGG_COLS


def _validate_agg(agg, t: pa.Table, cols, on_cols) -> list:
    """pb.merge's ``agg`` -> [(column, [operations])] in the order given; ValueError (naming the column) on anything the engine
    cannot aggregate."""
    if not isinstance(agg, dict) or not agg:
        raise ValueError("agg must be a non-empty dict of column -> operation or list of operations, "
                         'e.g. {"score": ["sum", "max"], "qual": "mean"}')
    if len(agg) > _MAX_AGG_COLS:
        raise ValueError(f"agg: at most {_MAX_AGG_COLS} value columns per call, got {len(agg)}")
    spec, taken = [], set(cols) | set(on_cols or ()) | {"n_intervals"}
    for name, ops in agg.items():
        if name not in t.column_names:
            raise ValueError(f"agg: column '{name}' not found in {t.column_names}")
        if name in cols or name in (on_cols or ()):
            raise ValueError(f"agg: column '{name}' is an interval or on_cols column and cannot be aggregated")
        typ = t.schema.field(name).type
        if not (pa.types.is_floating(typ) and typ.bit_width in (32, 64)) and not pa.types.is_signed_integer(typ) and not (
                pa.types.is_unsigned_integer(typ) and typ.bit_width <= 32):
            raise ValueError(f"agg: column '{name}' has type {typ}; signed integers, unsigned integers up to 32 bits, float32 and "
                             "float64 can be aggregated")
        ops = [ops] if isinstance(ops, str) else list(ops) if isinstance(ops, (list, tuple)) else None
        if not ops:
            raise ValueError(f"agg: column '{name}' needs an operation or a non-empty list of operations out of {list(_AGG_OP_NAMES)}")
        for op in ops:
            if op not in _AGG_OP_NAMES:
                raise ValueError(f"agg: unknown operation {op!r} for column '{name}': expected one of {list(_AGG_OP_NAMES)}")
            out = f"{name}_{op}"
            if out in taken:
                raise ValueError(f"agg: the output column '{out}' of column '{name}' collides with another output column")
            taken.add(out)
        spec.append((name, ops))
    return spec


def _agg_input(t: pa.Table, name: str, keep):
    """One value column as the engine reads it: (int64 / float64 values with 0 at the nulls, validity or None, ops are the
    caller's), rows outside ``keep`` dropped."""
    col = t.column(name)
    col = col.combine_chunks() if isinstance(col, pa.ChunkedArray) else col
    wide = pa.float64() if pa.types.is_floating(col.type) else pa.int64()
    valid = None
    if col.null_count:
        valid = pc.is_valid(col).to_numpy(zero_copy_only=False)
        col = pc.fill_null(col, pa.scalar(0, type=col.type))
    values = pc.cast(col, wide).to_numpy(zero_copy_only=False)
    if keep is not None:
        values, valid = values[keep], (valid[keep] if valid is not None else None)
    return np.ascontiguousarray(values), valid


def _agg_outputs(name: str, ops, typ: pa.DataType, res: dict) -> dict:
    """The result columns <name>_<op> of one value column: sum Int64 / Float64, min / max the column's own type, mean Float64,
    count Int64; min / max / mean are null where no valid value was merged."""
    empty = res["count"] == 0
    mask = empty if empty.any() else None
    out = {}
    for op in ops:
        a = res[op]
        if op in ("min", "max"):
            if mask is not None:
                a = np.where(mask, 0, a)
            out[f"{name}_{op}"] = pc.cast(pa.array(a, mask=mask), typ)
        elif op == "mean":
            out[f"{name}_{op}"] = pa.array(a, type=pa.float64(), mask=mask)
        else:
            out[f"{name}_{op}"] = pa.array(a)
    return out


def merge(
    df,
    min_dist: int = 0,
    cols: Union[list, None] = ["chrom", "start", "end"],
    on_cols: Union[list, None] = None,
    output_type: str = "polars.LazyFrame",
    projection_pushdown: bool = True,
    *,
    agg: Union[dict, None] = None,
):
    """Merge overlapping intervals (reference: range_op.py:599-657; MergeProvider, src/operation.rs:352-381).
    Output: (chrom, start: Int64, end: Int64, n_intervals: Int64) in (chrom, start) order
    (range_op_helpers.py:78-90).  ``min_dist=0`` merges overlapping intervals only: bookended half-open
    intervals stay apart (tests/_expected.py:174-181).

    ``on_cols``: intervals merge only within groups of equal (chrom, on values); output (chrom, start, end, <on_cols...>,
    n_intervals) in (chrom, on values, start) order; rows with a null on-value are dropped, as rows with a null chrom are.

    ``agg``: value columns summarised per merged interval, as ``bedtools merge -c/-o`` does:
    ``agg={"score": ["sum", "max"], "qual": "mean"}`` appends ``score_sum``, ``score_max`` and ``qual_mean`` after
    ``n_intervals``, in the order of the dict and of each list.  Operations: ``sum`` (Int64 for integer columns, wrapping
    modulo 2^64; Float64 for float columns), ``min`` / ``max`` (the column's own type), ``mean`` (Float64), ``count`` (Int64,
    the non-null values).  Columns may be signed integers, unsigned integers up to 32 bits, float32 or float64.  Null values
    are skipped: ``sum`` over no value is 0, ``min`` / ``max`` / ``mean`` over none are null.  Rows that ``merge`` drops take
    their values with them."""
    on_cols = _validate_overlap_input(cols, cols, on_cols, ("_1", "_2"), output_type)
    _check_on_cols_present(on_cols, df)
    zero_based = validate_coordinate_system_single(df)
    cols = list(DEFAULT_INTERVAL_COLUMNS if cols is None else cols)
    t = A.to_arrow(df)
    spec = _validate_agg(agg, t, cols, on_cols) if agg is not None else None
    side, n_contigs, dictionary = A.encode_frame(t, cols)
    gchrom = None
    if on_cols:
        # group ids over (chrom, on values) with the frame as the build side: sorted dictionaries make them ascend in that order
        (codes,), cards, dicts, _ = A.encode_on_cols([t], on_cols)
        empty = (np.empty(0, np.int32),) * 3
        _, side, groups, table = A.group_sides(empty, side, n_contigs, [np.empty(0, np.int32)] * len(on_cols), codes, cards, on_cols)
        n_contigs, gchrom = max(groups, 1), table
    keep = side[0] >= 0                                   # rows with a null chrom (or on-value) belong to no contig
    dropped = not keep.all()
    side = tuple(a[keep] for a in side) if dropped else side
    if spec is None:
        c, s, e, n = default_engine().merge(side, strict=zero_based, n_contigs=n_contigs, min_dist=int(min_dist))
    else:
        # count always travels along: it tells where min / max / mean are null
        inputs = [(*_agg_input(t, name, keep if dropped else None), list(ops) + ["count"]) for name, ops in spec]
        c, s, e, n, results = default_engine().merge_agg(side, strict=zero_based, n_contigs=n_contigs, agg=inputs, min_dist=int(min_dist))
    c = np.ascontiguousarray(c, np.int32)
    chrom_ids = c if gchrom is None else A.H.take(np.ascontiguousarray(gchrom[:, 0]), c)
    data = {cols[0]: pc.cast(pc.take(dictionary, pa.array(chrom_ids, type=pa.int32())), pa.string()),
            cols[1]: pa.array(s.astype(np.int64)), cols[2]: pa.array(e.astype(np.int64))}
    for j, name in enumerate(on_cols or ()):
        values = pc.take(dicts[j], pa.array(A.H.take(np.ascontiguousarray(gchrom[:, 1 + j]), c), type=pa.int32()))
        data[name] = A.cast_on_values(values, t.schema.field(name).type)
    data["n_intervals"] = pa.array(n, type=pa.int64())
    if spec is not None:
        for (name, ops), res in zip(spec, results):
            data.update(_agg_outputs(name, ops, t.schema.field(name).type, res))
    return A.from_arrow(pa.table(data), output_type, zero_based)


def _map_engine(what: str = "map_overlaps", entry: str = "overlap_agg"):
    eng = default_engine()
    if not hasattr(eng, entry):
        raise NotImplementedError(f"{what} needs a single-device engine; the default engine is a {type(eng).__name__} "
                                  "(several devices), which has no overlap aggregates")
    return eng


def map_overlaps(
    df1,
    df2,
    agg: Union[dict, None] = None,
    on_cols: Union[list, None] = None,
    cols1: Union[list, None] = ["chrom", "start", "end"],
    cols2: Union[list, None] = ["chrom", "start", "end"],
    output_type: str = "polars.LazyFrame",
    limit: Union[int, None] = None,
    *,
    min_overlap: Union[int, None] = None,
    min_frac1: Union[float, None] = None,
    min_frac2: Union[float, None] = None,
):
    """Summarise df2 value columns over the df2 intervals that overlap every df1 interval, as ``bedtools map -c/-o`` does:
    ``pb.map_overlaps(genes, peaks, agg={"score": ["mean", "max"], "weight": "sum"})`` returns the df1 columns plus
    ``score_mean``, ``score_max`` and ``weight_sum``, in the order of the dict and of each list, one row per df1 row in df1 row
    order.  The pairs are reduced on the device: none is enumerated, none leaves it.

    ``agg`` names df2 columns (signed integers, unsigned integers up to 32 bits, float32 or float64; not the interval or
    ``on_cols`` columns).  Operations: ``sum`` (Int64 for integer columns, wrapping modulo 2^64; Float64 for float columns),
    ``min`` / ``max`` (the column's own type), ``mean`` (Float64), ``count`` (Int64, the non-null values).  Null values are
    skipped: ``sum`` and ``count`` over no value are 0, ``min`` / ``max`` / ``mean`` over none are null.  A NaN value makes the
    ``sum`` and ``mean`` of its df1 row NaN; ``min`` / ``max`` skip NaNs unless every value is NaN.  Integer results are identical
    from run to run; a float ``sum`` is evaluated in a fixed order and repeats bit for bit for the same rows in the same order.
    An output name that is already a df1 column is a ValueError.

    Which df2 rows count is what ``count_overlaps`` counts for the same call: the ``count`` of a column without nulls equals it.
    ``on_cols``: only df2 rows of the df1 row's group of equal (chrom, on values) are reduced.  ``min_overlap`` / ``min_frac1`` /
    ``min_frac2`` (keyword-only): only the df2 rows that pass the overlap thresholds of ``overlap`` (which see).  df1 rows with a
    null chrom or on-value match nothing.

    The call is eager whatever the ``output_type`` (``limit`` takes the head of the finished table, ``pyarrow.RecordBatchReader``
    reads it).  ``median`` and other quantiles are ``pb.map_quantiles`` / ``pb.map_median``, not an ``agg`` operation.  Not offered:
    ``first`` / ``last`` / ``collapse`` / ``distinct``, string columns, the streaming and Arrow-stream entries, several devices."""
    mo, f1, f2 = _validate_overlap_thresholds(min_overlap, min_frac1, min_frac2)
    on_cols = _validate_overlap_input(cols1, cols2, on_cols, ("_1", "_2"), output_type)
    _check_on_cols_present(on_cols, df1, df2)
    zero_based = validate_coordinate_systems(df1, df2)
    c2 = list(DEFAULT_INTERVAL_COLUMNS if cols2 is None else cols2)
    t1, t2, probe, build, n_contigs, _keys = _prepare(df1, df2, cols1, cols2, on_cols)
    spec = _validate_agg(agg, t2, c2, on_cols)
    for name, ops in spec:
        for op in ops:
            if f"{name}_{op}" in t1.column_names:
                raise ValueError(f"agg: the output column '{name}_{op}' of column '{name}' collides with a column of df1")
    eng = _map_engine()
    pm, bm = _threshold_minima(probe, build, zero_based, f1, f2)
    # count always travels along: it tells where min / max / mean are null
    inputs = [(*_agg_input(t2, name, None), list(ops) + ["count"]) for name, ops in spec]
    results = eng.overlap_agg(probe, build, strict=zero_based, n_contigs=n_contigs, agg=inputs, min_overlap=mo, probe_min=pm, build_min=bm)
    table = t1
    for (name, ops), res in zip(spec, results):
        for out, column in _agg_outputs(name, ops, t2.schema.field(name).type, res).items():
            table = table.append_column(out, column)
    return _finish_eager(table, output_type, zero_based, limit)


def _map_quantile_matrix(what, df1, df2, value, qs, method, on_cols, cols1, cols2, output_type, min_overlap, min_frac1, min_frac2, names):
    """-> (t1, zero_based, values (n, len(qs)) in the engine's dtype or float64, null bool[n], the value column's arrow type);
    ``names(value)`` = the output column names, checked against df1's before the engine is touched."""
    mo, f1, f2 = _validate_overlap_thresholds(min_overlap, min_frac1, min_frac2)
    on_cols = _validate_overlap_input(cols1, cols2, on_cols, ("_1", "_2"), "pyarrow.Table" if output_type == "numpy.ndarray" else output_type)
    _check_on_cols_present(on_cols, df1, df2)
    zero_based = validate_coordinate_systems(df1, df2)
    c2 = list(DEFAULT_INTERVAL_COLUMNS if cols2 is None else cols2)
    t1, t2, probe, build, n_contigs, _keys = _prepare(df1, df2, cols1, cols2, on_cols)
    _signal_values(value, t2, c2, on_cols, True)
    for out in names(value):
        if out in t1.column_names:
            raise ValueError(f"{what}: the output column '{out}' of column '{value}' collides with a column of df1")
    eng = _map_engine(what, "overlap_quantiles")
    pm, bm = _threshold_minima(probe, build, zero_based, f1, f2)
    values, valid = _agg_input(t2, value, None)
    exact = method in ("lower", "higher")
    if exact:
        q, upper = qs, [method == "higher"] * len(qs)
    else:                                                  # lo and hi of each quantile side by side, on float64 values
        values = values.astype(np.float64)
        q, upper = [x for x in qs for _ in (0, 1)], [False, True] * len(qs)
    v, count = eng.overlap_quantiles(probe, build, strict=zero_based, n_contigs=n_contigs, values=values, valid=valid, q=q, upper=upper,
                                     min_overlap=mo, probe_min=pm, build_min=bm)
    null = count == 0
    typ = t2.schema.field(value).type
    if exact:
        return t1, zero_based, v, null, typ
    _lo, _hi, g = quantile_ranks(count[:, None], np.asarray(qs, np.float64)[None, :])
    vlo, vhi = v[:, 0::2], v[:, 1::2]
    with np.errstate(invalid="ignore", over="ignore"):
        val = (vlo + vhi) / 2.0 if method == "midpoint" else vlo + (vhi - vlo) * g
    val = np.where((vlo == vhi) | (g == 0.0), vlo, val)
    return t1, zero_based, np.where(null[:, None], np.nan, val), null, typ


def map_quantiles(
    df1,
    df2,
    value,
    q=(0.25, 0.5, 0.75),
    method: str = "linear",
    on_cols: Union[list, None] = None,
    cols1: Union[list, None] = ["chrom", "start", "end"],
    cols2: Union[list, None] = ["chrom", "start", "end"],
    output_type: str = "polars.LazyFrame",
    limit: Union[int, None] = None,
    *,
    min_overlap: Union[int, None] = None,
    min_frac1: Union[float, None] = None,
    min_frac2: Union[float, None] = None,
):
    """Exact quantiles of a df2 value column over the df2 intervals that overlap every df1 interval (``bedtools map -o median``
    and its quartiles): ``pb.map_quantiles(genes, peaks, "score", q=[0.25, 0.5, 0.75])`` returns the df1 columns plus
    ``score_q0.25``, ``score_q0.5`` and ``score_q0.75``, one row per df1 row in df1 row order.  Selected on the device: no pair
    is enumerated, none leaves it, nothing is sorted.

    ``value`` names ONE df2 column (signed integers, unsigned integers up to 32 bits, float32 or float64; not an interval or
    ``on_cols`` column).  For a df1 row let v[0] <= ... <= v[m - 1] be the non-null values of the df2 rows it matches, sorted;
    NaN values sort last, as in ``np.sort``.  For a quantile q in [0, 1]: h = q (m - 1) in float64, lo = floor(h), hi = ceil(h),
    g = h - lo (``quantile_ranks``), and ``method``, with numpy's names, selects ``"lower"`` v[lo] | ``"higher"`` v[hi] (both
    the column's own type) | ``"midpoint"`` (v[lo] + v[hi]) / 2 | ``"linear"`` (default) v[lo] + (v[hi] - v[lo]) g (both
    Float64; v[lo] itself where v[lo] == v[hi] or g == 0, so that infinities give no NaN).  For ``"midpoint"`` and ``"linear"``
    the values are converted to float64 first: the result is exact for integers below 2^53 in magnitude.  The device answers
    the order statistics; the interpolation is host arithmetic on them.

    Output columns are ``<value>_q<q>`` with q as ``repr(float(q))``, in the given order; ``q``: 1 .. 8 distinct values in
    [0, 1], else ``ValueError``; a name that is already a df1 column is a ``ValueError``.  df1 rows that match no non-null
    value get null.  ``output_type="numpy.ndarray"`` returns the bare (n, len(q)) float64 matrix with NaN for null.

    Which df2 rows count, ``on_cols`` and ``min_overlap`` / ``min_frac1`` / ``min_frac2`` (keyword-only) are as in
    ``map_overlaps``: the number of values under a row is its ``count`` there.  Identities: q = 0 / q = 1 with ``"lower"`` are
    ``map_overlaps``' ``min`` / ``max`` for columns without NaN.

    The call is eager whatever the ``output_type`` (``limit`` takes the head of the finished table,
    ``pyarrow.RecordBatchReader`` reads it).  Not offered: quantiles per merged interval (``pb.merge``), a weighted (signal)
    median, ``first`` / ``last`` / ``collapse`` / ``distinct`` / ``mode``, string columns, the streaming and Arrow-stream entries,
    several devices (``NotImplementedError``), more than 8 quantiles per call."""
    qs = _validate_quantiles(q, method)
    t1, zero_based, val, null, typ = _map_quantile_matrix("map_quantiles", df1, df2, value, qs, method, on_cols, cols1, cols2, output_type,
                                                          min_overlap, min_frac1, min_frac2, lambda name: [f"{name}_q{x!r}" for x in qs])
    if output_type == "numpy.ndarray":
        return np.where(null[:, None], np.nan, val.astype(np.float64))
    mask = null if null.any() else None
    for k, x in enumerate(qs):
        a = np.ascontiguousarray(val[:, k])
        if method in ("lower", "higher"):
            column = pc.cast(pa.array(np.where(null, 0, a) if mask is not None else a, mask=mask), typ)
        else:
            column = pa.array(a, type=pa.float64(), mask=mask)
        t1 = t1.append_column(f"{value}_q{x!r}", column)
    return _finish_eager(t1, output_type, zero_based, limit)


def map_median(
    df1,
    df2,
    value,
    on_cols: Union[list, None] = None,
    cols1: Union[list, None] = ["chrom", "start", "end"],
    cols2: Union[list, None] = ["chrom", "start", "end"],
    output_type: str = "polars.LazyFrame",
    limit: Union[int, None] = None,
    *,
    min_overlap: Union[int, None] = None,
    min_frac1: Union[float, None] = None,
    min_frac2: Union[float, None] = None,
):
    """The median of a df2 value column over the df2 intervals that overlap every df1 interval, as ``bedtools map -o median``
    gives it: ``map_quantiles`` with ``q = 0.5`` and ``method="linear"`` -- the middle value of an odd count, the mean of the two
    middle values of an even one -- as the one Float64 column ``<value>_median``; null where no non-null value matches.  Exact
    for integers below 2^53 in magnitude.  ``output_type="numpy.ndarray"``: the bare (n, 1) float64 matrix, NaN for null.

    Arguments, what is matched and what is not offered: as ``map_quantiles``."""
    t1, zero_based, val, null, _typ = _map_quantile_matrix("map_median", df1, df2, value, [0.5], "linear", on_cols, cols1, cols2, output_type,
                                                           min_overlap, min_frac1, min_frac2, lambda name: [f"{name}_median"])
    if output_type == "numpy.ndarray":
        return val
    t1 = t1.append_column(f"{value}_median", pa.array(np.ascontiguousarray(val[:, 0]), type=pa.float64(), mask=null if null.any() else None))
    return _finish_eager(t1, output_type, zero_based, limit)


_SIGNAL_STATS = ("size", "bases", "sum", "mean0", "mean", "min", "max")
_SIGNAL_PROFILE_OUTPUTS = ("mean", "mean0", "sum", "bases", "min", "max")


def _signal_values(value, t2: pa.Table, cols2, on_cols, single_only: bool):
    """``value`` -> (names, single): a df2 column name, or (``signal_summary``) a non-empty list of distinct names; the columns
    are checked as ``map_overlaps`` checks its ``agg`` columns."""
    single = isinstance(value, str)
    if single_only and not single:
        raise ValueError(f"value must be the name of one df2 column, got {value!r}")
    names = [value] if single else list(value) if isinstance(value, (list, tuple)) else None
    if not names or not all(isinstance(n, str) for n in names):
        raise ValueError(f"value must be the name of a df2 column or a non-empty list of names, got {value!r}")
    if len(set(names)) != len(names):
        raise ValueError(f"value names a column twice: {names}")
    _validate_agg({name: "sum" for name in names}, t2, cols2, on_cols)
    return names, single


def signal_summary(
    df1,
    df2,
    value,
    on_cols: Union[list, None] = None,
    cols1: Union[list, None] = ["chrom", "start", "end"],
    cols2: Union[list, None] = ["chrom", "start", "end"],
    output_type: str = "polars.LazyFrame",
    limit: Union[int, None] = None,
    *,
    min_overlap: Union[int, None] = None,
    min_frac1: Union[float, None] = None,
    min_frac2: Union[float, None] = None,
):
    """Summarise a signal track over every df1 interval: df2 holds (chrom, start, end, ``value``) rows as a bedGraph does, and a
    df2 row weighs its value on every position it shares with the df1 row -- ``bigWigAverageOverBed`` (with ``-minMax``),
    ``multiBigwigSummary BED-file``, ``bedtools map`` on a bedGraph done right.  Reduced on the device: no pair is enumerated.

    With ov = the positions a df2 row shares with the df1 row (0-based frames half-open, 1-based closed), a df2 row contributes
    iff ov >= 1 and its value is not null -- rows of either side that cover no position share nothing, as in ``mean_depth``;
    this is NOT what the unthresholded ``map_overlaps`` counts.  Output: df1's columns, one row per df1 row in df1 order, plus

      ``size``   Int64, the positions of the df1 row (0 if it has none)
      ``bases``  Int64, the sum of ov over the contributing df2 rows.  df2 rows that overlap each other count with their
                 multiplicity: ``bases`` can exceed ``size`` then (a proper bedGraph has no such rows, and there it is ``covered``)
      ``sum``    the sum of value * ov: Int64 for integer columns, wrapping modulo 2^64; Float64 for float columns
      ``mean0``  Float64 sum / size, null where size is 0 (positions without signal count as 0)
      ``mean``   Float64 sum / bases, null where bases is 0 (positions without signal are left out)
      ``min`` / ``max``  the column's own type, over the contributing values (unweighted), null where bases is 0

    ``value`` is a df2 column name, or a list of names: with a list every output is suffixed ``_<name>`` (``size_score``,
    ``sum_score``, ...), a single string gives the bare names.  Columns may be signed integers, unsigned integers up to 32
    bits, float32 or float64, not the interval or ``on_cols`` columns.  A NaN value makes ``sum`` / ``mean0`` / ``mean`` of its
    df1 row NaN; ``min`` / ``max`` skip NaNs unless every value is NaN.  Integer results are identical from run to run; a float
    ``sum`` is evaluated in a fixed order and repeats bit for bit for the same rows in the same order.  An output name that is
    already a df1 column is a ValueError.

    ``on_cols`` and ``min_overlap`` / ``min_frac1`` / ``min_frac2`` (keyword-only) as in ``map_overlaps``: only df2 rows of the
    df1 row's group, and only those that pass the overlap thresholds, contribute.  The cost is one test per candidate df2 row of
    each df1 row and value column.

    Eager whatever the ``output_type``; ``limit`` takes the head of the finished table.  Not offered: the streaming and
    Arrow-stream entries, several devices, a weighted ``median`` and other weighted order statistics (the unweighted ones are
    ``pb.map_quantiles``)."""
    mo, f1, f2 = _validate_overlap_thresholds(min_overlap, min_frac1, min_frac2)
    on_cols = _validate_overlap_input(cols1, cols2, on_cols, ("_1", "_2"), output_type)
    _check_on_cols_present(on_cols, df1, df2)
    zero_based = validate_coordinate_systems(df1, df2)
    c2 = list(DEFAULT_INTERVAL_COLUMNS if cols2 is None else cols2)
    t1, t2, probe, build, n_contigs, _keys = _prepare(df1, df2, cols1, cols2, on_cols)
    names, single = _signal_values(value, t2, c2, on_cols, False)
    taken = set(t1.column_names)
    for name in names:
        for stat in _SIGNAL_STATS:
            out = stat if single else f"{stat}_{name}"
            if out in taken:
                raise ValueError(f"value: the output column '{out}' of column '{name}' collides with a column of df1 or another output column")
            taken.add(out)
    eng = _map_engine("signal_summary", "overlap_wagg")
    pm, bm = _threshold_minima(probe, build, zero_based, f1, f2)
    ops = ["sum", "min", "max", "mean", "count"]
    inputs = [(*_agg_input(t2, name, None), ops) for name in names]
    results = eng.overlap_wagg(probe, build, strict=zero_based, n_contigs=n_contigs, agg=inputs, min_overlap=mo, probe_min=pm, build_min=bm)
    size = np.maximum(np.asarray(probe[2], np.int64) - np.asarray(probe[1], np.int64) + (0 if zero_based else 1), 0)
    no_size = size == 0
    table = t1
    for name, res in zip(names, results):
        rest = _agg_outputs(name, ["mean", "min", "max"], t2.schema.field(name).type, res)
        total = res["sum"]
        mean0 = np.divide(total.astype(np.float64), size.astype(np.float64), out=np.zeros(len(size), np.float64), where=~no_size)
        columns = {"size": pa.array(size, type=pa.int64()), "bases": pa.array(res["count"], type=pa.int64()), "sum": pa.array(total),
                   "mean0": pa.array(mean0, type=pa.float64(), mask=no_size if no_size.any() else None),
                   "mean": rest[f"{name}_mean"], "min": rest[f"{name}_min"], "max": rest[f"{name}_max"]}
        for stat in _SIGNAL_STATS:
            table = table.append_column(stat if single else f"{stat}_{name}", columns[stat])
    return _finish_eager(table, output_type, zero_based, limit)


def signal_profile(
    df1,
    df2,
    value,
    n_bins: int = 100,
    anchor: Union[str, None] = None,
    upstream: int = 0,
    downstream: int = 0,
    direction_col: Union[str, None] = None,
    on_cols: Union[list, None] = None,
    cols1: Union[list, None] = ["chrom", "start", "end"],
    cols2: Union[list, None] = ["chrom", "start", "end"],
    output: str = "mean",
    output_type: str = "polars.LazyFrame",
):
    """Binned signal of a track across every df1 row: the rows x ``n_bins`` matrix of deepTools ``computeMatrix`` over a
    bedGraph-like df2 of (chrom, start, end, ``value``) rows, made on the device from the window of each df1 row -- no frame of
    bins is built.

    Windows, bins, ``anchor`` / ``upstream`` / ``downstream``, ``direction_col``, ``on_cols``, the int32-range check and the
    shape of the result (df1's columns plus ``profile``: ``fixed_size_list[n_bins]``, or the bare matrix with
    ``output_type="numpy.ndarray"``) are ``depth_profile``'s.  Every bin is summarised as ``signal_summary`` summarises a df1
    row: a df2 row contributes to a bin iff it shares ov >= 1 positions with it and its value is not null.  ``output``:

      ``"mean"``   Float64 sum of value * ov / sum of ov; null (NaN in the matrix) where no signal reaches the bin -- deepTools'
                   default
      ``"mean0"``  Float64 sum of value * ov / bin length; null for an empty bin -- ``--missingDataAsZero``
      ``"sum"``    the sum of value * ov: Int64 (wrapping) for integer columns, Float64 for float columns
      ``"bases"``  Int64 sum of ov (df2 rows that overlap each other count with their multiplicity)
      ``"min"`` / ``"max"``  the column's own type over the contributing values; null where there is none (the bare matrix is
                   Float64 with NaN there)

    One ``value`` column per call (types as in ``signal_summary``).  A row of the ``sum`` / ``bases`` matrix adds up to the
    window's ``signal_summary``.  The cost is one test per candidate df2 row of every BIN: a df2 row that spans k bins is visited
    k times, which suits tracks of short rows (bedGraph steps, per-base signal runs), not contig-wide rows.

    Eager.  Not covered: thresholds per bin, streaming inputs or outputs, several devices, ``median``."""
    n_bins, zero_based, t1, t2, build, n_contigs, on_cols, is_minus, w_start, w_end, windows = _profile_setup(
        df1, df2, n_bins, anchor, upstream, downstream, direction_col, on_cols, cols1, cols2, output, _SIGNAL_PROFILE_OUTPUTS, output_type)
    c2 = list(DEFAULT_INTERVAL_COLUMNS if cols2 is None else cols2)
    (name,), _single = _signal_values(value, t2, c2, on_cols, True)
    eng = _map_engine("signal_profile", "signal_profile")
    ops = {"mean": ["mean", "count"], "mean0": ["sum"], "sum": ["sum"], "bases": ["count"], "min": ["min", "count"], "max": ["max", "count"]}[output]
    (res,) = eng.signal_profile(windows, is_minus, n_bins, build, strict=zero_based, n_contigs=n_contigs,
                                agg=[(*_agg_input(t2, name, None), ops)])
    as_matrix = output_type == "numpy.ndarray"
    if output in ("sum", "bases"):
        m = res["sum" if output == "sum" else "count"]
        if as_matrix:
            return m
        values = pa.array(m.reshape(-1))
    elif output == "mean0":
        lens = profile_bin_lengths(w_start, w_end, zero_based, n_bins, is_minus)
        null = lens <= 0
        m = np.divide(res["sum"].astype(np.float64), lens.astype(np.float64), out=np.full(null.shape, np.nan), where=~null)
        if as_matrix:
            return m
        values = pa.array(m.reshape(-1), type=pa.float64(), mask=null.reshape(-1))
    else:
        null = res["count"] == 0
        if as_matrix:
            return np.where(null, np.nan, res[output].astype(np.float64))
        if output == "mean":
            values = pa.array(res["mean"].reshape(-1), type=pa.float64(), mask=null.reshape(-1))
        else:
            values = pc.cast(pa.array(np.where(null, 0, res[output]).reshape(-1), mask=null.reshape(-1)), t2.schema.field(name).type)
    t = t1.append_column("profile", pa.FixedSizeListArray.from_arrays(values, n_bins))
    return _finish_eager(t, output_type, zero_based, None)


PERMUTATION_MAX = (1 << 20) - 1          # the engine takes 2^20 offset rows per call, one of them the observed (all-zero) row


def _permutation_engine():
    eng = default_engine()
    if not hasattr(eng, "permute_overlaps"):
        raise NotImplementedError(f"permutation_test needs a single-device engine; the default engine is a {type(eng).__name__} "
                                  "(several devices), which has no permutation kernel")
    return eng


def _genome_lengths(genome):
    """-> (names sorted, int64 lengths in that order) of a {contig: length} dict or a two-column (name, length) frame."""
    if not isinstance(genome, dict):
        t = A.to_arrow(genome)
        if t.num_columns != 2:
            raise ValueError(f"genome must be a dict or a frame of two columns (contig, length), got {t.num_columns} columns")
        names, lens = t.column(0).to_pylist(), t.column(1).to_pylist()
        if len(set(names)) != len(names):
            raise ValueError("genome names a contig twice")
        genome = dict(zip(names, lens))
    if not genome:
        raise ValueError("genome is empty")
    for k, v in genome.items():
        if k is None or v is None or isinstance(v, bool) or int(v) != v or not 1 <= int(v) <= 2 ** 31 - 1:
            raise ValueError(f"genome: the length of contig {k!r} must be an integer in [1, 2^31 - 1], got {v!r}")
    genome = {str(k): int(v) for k, v in genome.items()}
    names = sorted(genome)
    return names, np.array([genome[k] for k in names], np.int64)


def permutation_offsets(genome, n_perm: int, seed: int = 0):
    """The offset table ``permutation_test`` draws for (genome, n_perm, seed): -> (names, offsets int64 [n_perm, len(names)]);
    column j belongs to names[j] = sorted(genome)[j]."""
    names, lengths = _genome_lengths(genome)
    rng = np.random.default_rng(seed)
    return names, rng.integers(0, lengths[None, :], size=(n_perm, len(names)))


def permutation_test(
    df1,
    df2,
    genome,
    n_perm: int = 1000,
    seed: int = 0,
    on_cols: Union[list, None] = None,
    cols1: Union[list, None] = ["chrom", "start", "end"],
    cols2: Union[list, None] = ["chrom", "start", "end"],
    output: str = "summary",
    output_type: str = "polars.LazyFrame",
    offsets=None,
):
    """Is the overlap of df1 with df2 more than chance?  A circular-shift permutation test (regioneR's
    ``circularRandomizeRegions``, a loop over ``bedtools shuffle | bedtools intersect``): in every permutation all df1 intervals of
    a contig move by one random offset along it, wrapping at its end; df2 stays.  Two statistics are recounted per permutation on
    the device, where df1 stays in registers and nothing per row or per pair exists in memory:

    * ``n_pairs``: the overlapping (df1, df2) pairs.  A df1 interval that wraps is two pieces, [s', L) and [0, e' - L); a df2
      interval that reaches both pieces counts TWICE;
    * ``n_rows``: the df1 intervals that overlap at least one df2 interval.

    "Overlap" means sharing at least one position (``min_overlap = 1``); intervals that cover no position match nothing.  The
    observed values are the same computation with every offset 0.

    ``genome``: {contig: length} or a two-column frame (contig, length); contig c covers [0, length) in half-open coordinates.
    Every contig of df1 must be in it, and every df1 interval with a chrom must lie inside its contig and cover a position
    (ValueError otherwise, naming the first row that does not).  df1 rows with a null chrom or a null on-value take no part.

    Offsets, so that a result can be reproduced outside the library::

        names = sorted(genome); rng = np.random.default_rng(seed)
        off = rng.integers(0, lengths[None, :], size=(n_perm, len(names)))       # column j belongs to names[j]

    ``offsets=`` gives that table explicitly ([n_perm, len(genome)], 0 <= offset < length) and overrides ``seed`` and ``n_perm``.
    ``on_cols``: only df2 rows of the df1 row's group of equal (chrom, on values) count; every group of a chrom moves by that
    chrom's offset.

    ``output="null"``: the table (permutation, n_pairs, n_rows), one row per permutation.  ``output="summary"``: one row per
    statistic with ``statistic, observed, n_perm, null_mean, null_sd`` (ddof = 1, null when n_perm < 2), ``z_score`` (null when
    the sd is 0 or null), ``p_greater = (1 + #{null >= observed}) / (n_perm + 1)`` and ``p_less`` likewise with <=.

    The call is eager.  Not offered: a bases or jaccard statistic, thresholds other than the implied ``min_overlap = 1``,
    non-circular randomisation (``shuffle`` with exclusion masks), per-group offsets, the streaming and Arrow-stream entries,
    several devices."""
    if output not in ("summary", "null"):
        raise ValueError(f"output must be 'summary' or 'null', got {output!r}")
    on_cols = _validate_overlap_input(cols1, cols2, on_cols, ("_1", "_2"), output_type)
    _check_on_cols_present(on_cols, df1, df2)
    names, lengths = _genome_lengths(genome)
    if offsets is None:
        if isinstance(n_perm, bool) or int(n_perm) != n_perm or not 1 <= int(n_perm) <= PERMUTATION_MAX:
            raise ValueError(f"n_perm must be an integer in [1, {PERMUTATION_MAX}], got {n_perm!r}")
        off = np.random.default_rng(seed).integers(0, lengths[None, :], size=(int(n_perm), len(names)))
    else:
        off = np.asarray(offsets)
        if off.ndim != 2 or off.shape[1] != len(names) or not 1 <= off.shape[0] <= PERMUTATION_MAX or off.dtype.kind not in "iu":
            raise ValueError(f"offsets must be an integer array of shape [1 .. {PERMUTATION_MAX}, {len(names)}], got {off.dtype} {off.shape}")
        off = off.astype(np.int64)
        if (off < 0).any() or (off >= lengths[None, :]).any():
            raise ValueError("offsets must satisfy 0 <= offsets[p, j] < length of sorted(genome)[j]")
    n_perm = int(off.shape[0])
    zero_based = validate_coordinate_systems(df1, df2)
    c1 = list(DEFAULT_INTERVAL_COLUMNS if cols1 is None else cols1)
    t1, _t2, probe, build, n_contigs, keys = _prepare(df1, df2, cols1, cols2, on_cols)
    # genome column of every chrom id of the shared dictionary (-1: the genome does not name it)
    chroms = [None if x is None else str(x) for x in keys[4].to_pylist()]
    col_of = {k: j for j, k in enumerate(names)}
    chrom_col = np.array([col_of.get(k, -1) for k in chroms] + [-1], np.int64)              # (the last entry answers id -1)
    ch1 = keys[1]
    if len(ch1):
        absent = (ch1 >= 0) & (chrom_col[ch1] < 0)
        if absent.any():
            i = int(np.flatnonzero(absent)[0])
            raise ValueError(f"df1 row {i}: contig {chroms[ch1[i]]!r} is not in genome")
        hs = probe[1].astype(np.int64) - (0 if zero_based else 1)
        he = probe[2].astype(np.int64)
        bad = (ch1 >= 0) & ~((0 <= hs) & (hs < he) & (he <= lengths[np.maximum(chrom_col[ch1], 0)]))
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise ValueError(f"df1 row {i}: {c1[1]}={int(probe[1][i])}, {c1[2]}={int(probe[2][i])} does not lie inside contig "
                             f"{chroms[ch1[i]]!r} of length {int(lengths[chrom_col[ch1[i]]])} or covers no position")
    eng = _permutation_engine()
    # the engine's contigs are chrom ids, or with on_cols group ids, each with its chrom's column; contigs the genome does not name
    # hold no df1 row: any length does
    group_chrom = np.arange(n_contigs, dtype=np.int64) if keys[5] is None else np.asarray(keys[5], np.int64)[:n_contigs]
    gcol = chrom_col[group_chrom] if len(chroms) else np.full(n_contigs, -1, np.int64)
    have = gcol >= 0
    lens = np.where(have, lengths[np.maximum(gcol, 0)], 1).astype(np.int32)
    table = np.zeros((n_perm + 1, n_contigs), np.int32)                                      # row 0: the observed statistics
    table[1:, have] = off[:, gcol[have]]
    pairs, rows = eng.permute_overlaps(probe, build, strict=zero_based, n_contigs=n_contigs, contig_len=lens, offsets=table)
    pairs, rows = np.asarray(pairs, np.int64), np.asarray(rows, np.int64)
    if output == "null":
        out = pa.table({"permutation": pa.array(np.arange(n_perm, dtype=np.int64)), "n_pairs": pa.array(pairs[1:]), "n_rows": pa.array(rows[1:])})
        return _finish_eager(out, output_type, zero_based, None)
    data = {k: [] for k in ("statistic", "observed", "n_perm", "null_mean", "null_sd", "z_score", "p_greater", "p_less")}
    for name, v in (("n_pairs", pairs), ("n_rows", rows)):
        obs, null = int(v[0]), v[1:].astype(np.float64)
        mean = float(null.mean())
        sd = float(null.std(ddof=1)) if n_perm >= 2 else None
        for k, x in (("statistic", name), ("observed", obs), ("n_perm", n_perm), ("null_mean", mean), ("null_sd", sd),
                     ("z_score", (obs - mean) / sd if sd else None),
                     ("p_greater", (1 + int((v[1:] >= obs).sum())) / (n_perm + 1)), ("p_less", (1 + int((v[1:] <= obs).sum())) / (n_perm + 1))):
            data[k].append(x)
    types = {"statistic": pa.large_string(), "observed": pa.int64(), "n_perm": pa.int64()}
    out = pa.table({k: pa.array(x, type=types.get(k, pa.float64())) for k, x in data.items()})
    return _finish_eager(out, output_type, zero_based, None)


def depth(
    df,
    cols: Union[list, None] = ["chrom", "start", "end"],
    on_cols: Union[list, None] = None,
    output_type: str = "polars.LazyFrame",
    projection_pushdown: bool = True,
):
    """Run-length coverage blocks of one interval frame: the disjoint maximal runs of positions covered by the same number
    (>= 1) of rows, the bedGraph / mosdepth block form.  The reference computes these blocks from alignment files only
    (``pb.depth``, pileup_op.py:50-118); here the reads, peaks or fragments are an interval frame.

    Output: (chrom, start: Int64, end: Int64, <on_cols...>, coverage: Int64) in (chrom, start) order, block bounds in the
    frame's own coordinate system (0-based: half-open, 1-based: closed), which is set on the result: the blocks feed straight
    back into ``overlap`` / ``coverage``.  Zero-depth gaps are not reported (``complement`` gives them); intervals that only
    touch do not split a block; rows that cover no position and rows with a null chrom contribute nothing.

    ``on_cols``: depth per group of equal (chrom, on values), e.g. per strand; output in (chrom, on values, start) order; rows
    with a null on-value are dropped, as rows with a null chrom are.

    Two deliberate differences from the reference's file-based ``pb.depth``: the column names come from ``cols`` (there:
    contig / pos_start / pos_end), and ``coverage`` is Int64 (there: Int16)."""
    if isinstance(df, (str, bytes, os.PathLike)):
        raise ValueError("depth: alignment files (BAM / SAM / CRAM) are outside this engine; an interval frame "
                         "(polars / pandas / pyarrow, one row per aligned block) is expected")
    on_cols = _validate_overlap_input(cols, cols, on_cols, ("_1", "_2"), output_type)
    _check_on_cols_present(on_cols, df)
    zero_based = validate_coordinate_system_single(df)
    cols = list(DEFAULT_INTERVAL_COLUMNS if cols is None else cols)
    t = A.to_arrow(df)
    side, n_contigs, dictionary = A.encode_frame(t, cols)
    gchrom = None
    if on_cols:
        # group ids over (chrom, on values) with the frame as the build side: sorted dictionaries make them ascend in that order
        (codes,), cards, dicts, _ = A.encode_on_cols([t], on_cols)
        empty = (np.empty(0, np.int32),) * 3
        _, side, groups, table = A.group_sides(empty, side, n_contigs, [np.empty(0, np.int32)] * len(on_cols), codes, cards, on_cols)
        n_contigs, gchrom = max(groups, 1), table
    keep = side[0] >= 0                                   # rows with a null chrom (or on-value) belong to no contig
    side = tuple(a[keep] for a in side) if not keep.all() else side
    c, s, e, d = default_engine().depth(side, strict=zero_based, n_contigs=n_contigs)
    c = np.ascontiguousarray(c, np.int32)
    chrom_ids = c if gchrom is None else A.H.take(np.ascontiguousarray(gchrom[:, 0]), c)
    data = {cols[0]: pc.cast(pc.take(dictionary, pa.array(chrom_ids, type=pa.int32())), pa.string()),
            cols[1]: pa.array(s.astype(np.int64)), cols[2]: pa.array(e.astype(np.int64))}
    for j, name in enumerate(on_cols or ()):
        values = pc.take(dicts[j], pa.array(A.H.take(np.ascontiguousarray(gchrom[:, 1 + j]), c), type=pa.int32()))
        data[name] = A.cast_on_values(values, t.schema.field(name).type)
    data["coverage"] = pa.array(d.astype(np.int64))
    return A.from_arrow(pa.table(data), output_type, zero_based)


# ---- set operations on two frames (setop.hip.h) -------------------------------------------------------

def _set_frames(dfs, cols_list, on_cols):
    """Frames as position sets -> (tables, sides, n_contigs, dictionary, group table, on_col dictionaries); sides[f] =
    (contig, start, end) int32 of frame f without its rows of a null chrom (or on-value).
    One chrom dictionary over all frames, numbered in sorted-name order: the result is in (chrom, start) order, as
    encode_frame numbers the one frame of merge / depth.  _prepare's on_cols groups are ranks among the keys of df2 alone (a
    df1 row whose key df2 lacks gets -1, which is right for a join and wrong for a union), so the groups are numbered here
    over the rows of ALL frames, the way merge / depth number the groups of their one frame."""
    tables = [A.to_arrow(df) for df in dfs]
    cols_list = [list(DEFAULT_INTERVAL_COLUMNS if cols is None else cols) for cols in cols_list]
    for t, cols in zip(tables, cols_list):
        for c in cols:
            if c not in t.column_names:
                raise ValueError(f"column '{c}' not found in {t.column_names}")
    encoded = [A._encode_chrom(t.column(cols[0])) for t, cols in zip(tables, cols_list)]
    dictionary = pc.unique(pa.concat_arrays([d for d, _ in encoded]))
    dictionary = dictionary.combine_chunks() if isinstance(dictionary, pa.ChunkedArray) else dictionary
    dictionary = pc.take(dictionary, pc.sort_indices(dictionary))
    n_contigs = len(dictionary)
    sides = []
    for (d, ids), t, cols in zip(encoded, tables, cols_list):
        if len(ids):
            remap = pc.index_in(d, value_set=dictionary).to_numpy(zero_copy_only=False).astype(np.int32)
            ids = np.where(ids >= 0, remap[np.maximum(ids, 0)], -1).astype(np.int32)
        sides.append((ids, A._coord_to_i32(t.column(cols[1]), cols[1]), A._coord_to_i32(t.column(cols[2]), cols[2])))
    gchrom = dicts = None
    if on_cols:
        for t in tables:
            missing = [c for c in on_cols if c not in t.column_names]
            assert not missing, f"on_cols {missing} not found in {t.column_names}"
        codes_by_frame, cards, dicts, _ = A.encode_on_cols(tables, on_cols)
        bounds = np.concatenate([[0], np.cumsum([len(x[0]) for x in sides])])
        every = tuple(np.concatenate([x[k] for x in sides]) for k in range(3))
        codes = [np.concatenate([cf[j] for cf in codes_by_frame]) for j in range(len(on_cols))]
        empty = (np.empty(0, np.int32),) * 3
        _, every, groups, table = A.group_sides(empty, every, n_contigs, [np.empty(0, np.int32)] * len(on_cols), codes, cards, on_cols)
        sides = [(every[0][bounds[f]:bounds[f + 1]], x[1], x[2]) for f, x in enumerate(sides)]
        n_contigs, gchrom = max(groups, 1), table

    def known(side):                                      # rows with a null chrom (or on-value) belong to no contig
        keep = side[0] >= 0
        return side if keep.all() else tuple(np.ascontiguousarray(x[keep]) for x in side)
    return tables, [known(x) for x in sides], n_contigs, dictionary, gchrom, dicts


def _set_sides(df1, df2, cols1, cols2, on_cols):
    """Both frames as sides of a set operation -> (t1, a, b, n_contigs, dictionary, group table, on_col dictionaries)."""
    tables, (a, b), n_contigs, dictionary, gchrom, dicts = _set_frames([df1, df2], [cols1, cols2], on_cols)
    return tables[0], a, b, n_contigs, dictionary, gchrom, dicts


def _regions_table(t1, cols, c, s, e, dictionary, gchrom, dicts, on_cols):
    """(contig id, start, end) of a position-set result -> the columns (chrom, start, end, <on_cols...>) named from ``cols``"""
    c = np.ascontiguousarray(c, np.int32)
    chrom_ids = c if gchrom is None else A.H.take(np.ascontiguousarray(gchrom[:, 0]), c)
    data = {cols[0]: pc.cast(pc.take(dictionary, pa.array(chrom_ids, type=pa.int32())), pa.string()),
            cols[1]: pa.array(s.astype(np.int64)), cols[2]: pa.array(e.astype(np.int64))}
    for j, name in enumerate(on_cols or ()):
        values = pc.take(dicts[j], pa.array(A.H.take(np.ascontiguousarray(gchrom[:, 1 + j]), c), type=pa.int32()))
        data[name] = A.cast_on_values(values, t1.schema.field(name).type)
    return data


def _set_operation(op, df1, df2, on_cols, cols1, cols2, output_type):
    on_cols = _validate_overlap_input(cols1, cols2, on_cols, ("_1", "_2"), output_type)
    _check_on_cols_present(on_cols, df1, df2)
    zero_based = validate_coordinate_systems(df1, df2)
    t1, a, b, n_contigs, dictionary, gchrom, dicts = _set_sides(df1, df2, cols1, cols2, on_cols)
    cols = list(DEFAULT_INTERVAL_COLUMNS if cols1 is None else cols1)
    c, s, e = default_engine().setop(a, b, op, strict=zero_based, n_contigs=n_contigs)
    return A.from_arrow(pa.table(_regions_table(t1, cols, c, s, e, dictionary, gchrom, dicts, on_cols)), output_type, zero_based)


_SET_DOC = """{what}

    A frame is read as the SET of (chrom, position) its rows cover: 0-based frames are half-open (a row covers [start, end)),
    1-based frames closed ([start, end]); rows that cover no position and rows with a null chrom contribute nothing.  The
    result is that set's maximal runs -- regions that touch are one region ([0,5) and [5,9) give [0,9); closed [1,5] and [6,9]
    give [1,9]), no two output rows are adjacent or overlap.  (GenomicRanges intersect / union / setdiff, bioframe setdiff.)

    Output: (chrom, start: Int64, end: Int64, <on_cols...>), named from ``cols1``, in (chrom, on values, start) order, bounds in
    the frames' own coordinate system, which both frames must share and which is set on the result: it feeds straight back
    into ``overlap``, ``coverage`` or another set operation.

    ``on_cols``: positions match within groups of equal (chrom, on values) only, e.g. per strand; rows with a null on-value are
    dropped, as rows with a null chrom are."""


def set_intersect(df1, df2, on_cols: Union[list, None] = None, cols1: Union[list, None] = ["chrom", "start", "end"],
                  cols2: Union[list, None] = ["chrom", "start", "end"], output_type: str = "polars.LazyFrame"):
    return _set_operation("intersection", df1, df2, on_cols, cols1, cols2, output_type)


def set_union(df1, df2, on_cols: Union[list, None] = None, cols1: Union[list, None] = ["chrom", "start", "end"],
              cols2: Union[list, None] = ["chrom", "start", "end"], output_type: str = "polars.LazyFrame"):
    return _set_operation("union", df1, df2, on_cols, cols1, cols2, output_type)


def set_difference(df1, df2, on_cols: Union[list, None] = None, cols1: Union[list, None] = ["chrom", "start", "end"],
                   cols2: Union[list, None] = ["chrom", "start", "end"], output_type: str = "polars.LazyFrame"):
    return _set_operation("difference", df1, df2, on_cols, cols1, cols2, output_type)


def set_symmetric_difference(df1, df2, on_cols: Union[list, None] = None, cols1: Union[list, None] = ["chrom", "start", "end"],
                             cols2: Union[list, None] = ["chrom", "start", "end"], output_type: str = "polars.LazyFrame"):
    return _set_operation("symmetric_difference", df1, df2, on_cols, cols1, cols2, output_type)


set_intersect.__doc__ = _SET_DOC.format(what="The regions both frames cover: U(df1) & U(df2).")
set_union.__doc__ = _SET_DOC.format(what="The regions at least one of the frames covers: U(df1) | U(df2).")
set_difference.__doc__ = _SET_DOC.format(what="What df1 covers and df2 does not, as regions (``subtract`` gives fragments of df1's rows): U(df1) \\ U(df2).")
set_symmetric_difference.__doc__ = _SET_DOC.format(what="The regions exactly one of the two frames covers.")


def jaccard(df1, df2, on_cols: Union[list, None] = None, cols1: Union[list, None] = ["chrom", "start", "end"],
            cols2: Union[list, None] = ["chrom", "start", "end"], output_type: str = "polars.LazyFrame"):
    """Similarity of two interval frames as position sets, the columns of ``bedtools jaccard``: one row with ``intersection``
    (Int64, positions both frames cover), ``union`` (Int64, positions at least one covers), ``jaccard`` (Float64,
    intersection / union computed on the host from the two exact integers; null when the union is empty) and
    ``n_intersections`` (Int64, the regions ``set_intersect`` would return).  One walk over both frames, no regions written.
    Positions and conventions are those of the set operations; with ``on_cols`` positions match within groups of equal
    (chrom, on values) only and the totals are summed over the groups."""
    on_cols = _validate_overlap_input(cols1, cols2, on_cols, ("_1", "_2"), output_type)
    _check_on_cols_present(on_cols, df1, df2)
    zero_based = validate_coordinate_systems(df1, df2)
    _t1, a, b, n_contigs, _dictionary, _gchrom, _dicts = _set_sides(df1, df2, cols1, cols2, on_cols)
    only_a, only_b, both, n_int = default_engine().set_stats(a, b, strict=zero_based, n_contigs=n_contigs)
    union = only_a + only_b + both
    res = pa.table({"intersection": pa.array([both], type=pa.int64()), "union": pa.array([union], type=pa.int64()),
                    "jaccard": pa.array([both / union if union else None], type=pa.float64()),
                    "n_intersections": pa.array([n_int], type=pa.int64())})
    return A.from_arrow(res, output_type, zero_based)


# ---- N frames as position sets (multi.hip.h) ------------------------------------------------------------

_MULTI_DOC = """

    Every frame is read as the set operations read it: the SET of (chrom, position) its rows cover, 0-based frames half-open,
    1-based frames closed; rows that cover no position and rows with a null chrom (or a null on-value) contribute nothing.  All
    frames must share one coordinate system, which is set on the result.  ``frames``: a list of 1 .. 64 frames; ``cols`` names
    the interval columns of every frame; ``on_cols``: positions match within groups of equal (chrom, on values) only."""


def _multi_frames(frames, min_frames, on_cols, cols, output_type):
    """the shared front of multi_intersect / consensus: every argument check (ValueError, before the engine is touched), then
    the frames as sides -> (min_frames, on_cols, cols, zero_based, t1, sides, n_contigs, dictionary, group table, dictionaries)"""
    from ._engine import check_multi
    if isinstance(frames, (str, bytes)) or not isinstance(frames, (list, tuple)):
        raise ValueError("frames must be a list of interval frames")
    frames = list(frames)
    min_frames = check_multi(len(frames), min_frames)
    on_cols = _validate_overlap_input(cols, cols, on_cols, ("_1", "_2"), output_type)
    _check_on_cols_present(on_cols, *frames)
    zero_based = validate_coordinate_system_single(frames[0]) if len(frames) == 1 else None
    for other in frames[1:]:
        zero_based = validate_coordinate_systems(frames[0], other)
    cols = list(DEFAULT_INTERVAL_COLUMNS if cols is None else cols)
    tables, sides, n_contigs, dictionary, gchrom, dicts = _set_frames(frames, [cols] * len(frames), on_cols)
    return min_frames, on_cols, cols, zero_based, tables[0], sides, n_contigs, dictionary, gchrom, dicts


def multi_intersect(frames, min_frames: int = 1, names: Union[list, None] = None, on_cols: Union[list, None] = None,
                    cols: Union[list, None] = ["chrom", "start", "end"], output_type: str = "polars.LazyFrame"):
    if names is not None:
        names = _check_names(names, frames, on_cols, cols)
    min_frames, on_cols, cols, zero_based, t1, sides, n_contigs, dictionary, gchrom, dicts = _multi_frames(frames, min_frames, on_cols, cols, output_type)
    from ._engine import MULTI_SEGMENTS
    c, s, e, mask = default_engine().multi_inter(sides, min_frames, MULTI_SEGMENTS, strict=zero_based, n_contigs=n_contigs)
    data = _regions_table(t1, cols, c, s, e, dictionary, gchrom, dicts, on_cols)
    mask = np.ascontiguousarray(mask, np.uint64)
    bits = np.unpackbits(mask.view(np.uint8).reshape(-1, 8), axis=1, bitorder="little") if mask.size else np.zeros((0, 64), np.uint8)
    data["n_frames"] = pa.array(bits.sum(axis=1, dtype=np.int64), type=pa.int64())
    data["mask"] = pa.array(mask, type=pa.uint64())
    for f, name in enumerate(names or ()):
        data[name] = pa.array(bits[:, f].astype(bool), type=pa.bool_())
    return A.from_arrow(pa.table(data), output_type, zero_based)


def _check_names(names, frames, on_cols, cols) -> list:
    """names: one distinct string per frame, none colliding with the other output columns (ValueError) -> names as a list"""
    if isinstance(names, (str, bytes)) or not isinstance(names, (list, tuple)) or not all(isinstance(x, str) for x in names):
        raise ValueError("names must be a list of strings, one per frame")
    names = list(names)
    if isinstance(frames, (list, tuple)) and len(names) != len(frames):
        raise ValueError(f"names must hold one string per frame: {len(frames)} frames, {len(names)} names")
    if len(set(names)) != len(names):
        raise ValueError("names holds a name twice")
    on = [on_cols] if isinstance(on_cols, str) else list(on_cols or ())
    taken = set(DEFAULT_INTERVAL_COLUMNS if cols is None else cols) | set(on) | {"n_frames", "mask"}
    bad = [x for x in names if x in taken]
    if bad:
        raise ValueError(f"names collide with other output columns: {bad}")
    return names


multi_intersect.__doc__ = """For each stretch of the genome, which of the N frames cover it (``bedtools multiinter``): the maximal
    runs of positions covered by the same non-empty set of frames, in (chrom, on values, start) order.

    Output: (chrom, start: Int64, end: Int64, <on_cols...>, n_frames: Int64, mask: UInt64), named from ``cols``; bit f of
    ``mask`` is set where ``frames[f]`` covers the segment and ``n_frames`` is its popcount.  With ``names`` (one distinct string
    per frame, none of them another output column) one Boolean column per frame follows.  Two adjacent segments always differ in
    ``mask``: where a row of frame 0 ends and a row of frame 1 starts is a segment boundary, two touching rows of the same frame
    are not.  Segments covered by fewer than ``min_frames`` frames are dropped; the remaining ones are not merged
    (``consensus`` merges them).""" + _MULTI_DOC


def consensus(frames, min_frames: int, on_cols: Union[list, None] = None, cols: Union[list, None] = ["chrom", "start", "end"],
              output_type: str = "polars.LazyFrame"):
    min_frames, on_cols, cols, zero_based, t1, sides, n_contigs, dictionary, gchrom, dicts = _multi_frames(frames, min_frames, on_cols, cols, output_type)
    from ._engine import MULTI_CONSENSUS
    c, s, e, _ = default_engine().multi_inter(sides, min_frames, MULTI_CONSENSUS, strict=zero_based, n_contigs=n_contigs)
    return A.from_arrow(pa.table(_regions_table(t1, cols, c, s, e, dictionary, gchrom, dicts, on_cols)), output_type, zero_based)


consensus.__doc__ = """Consensus regions of N frames (DiffBind / GenomicRanges "consensus peaks"): the maximal runs of positions
    covered by at least ``min_frames`` of the frames; runs that touch are one region.  ``min_frames=1`` is the N-way union,
    ``min_frames=len(frames)`` the N-way intersection.

    Output: (chrom, start: Int64, end: Int64, <on_cols...>), named from ``cols``, in (chrom, on values, start) order -- the
    columns and order of the set operations.""" + _MULTI_DOC


PAIRWISE_STATISTICS = ("jaccard", "intersection", "union", "n_intersections", "fraction")


def pairwise_jaccard(frames, names: Union[list, None] = None, statistic: str = "jaccard", on_cols: Union[list, None] = None,
                     cols: Union[list, None] = ["chrom", "start", "end"], output_type: str = "polars.LazyFrame"):
    if statistic not in PAIRWISE_STATISTICS:
        raise ValueError(f"unknown statistic {statistic!r}: one of {list(PAIRWISE_STATISTICS)}")
    if names is not None:
        names = _check_names(names, frames, on_cols, cols)
    as_matrix = output_type == "numpy.ndarray"
    _k, on_cols, cols, zero_based, _t1, sides, n_contigs, _dictionary, _gchrom, _dicts = _multi_frames(
        frames, 1, on_cols, cols, "pyarrow.Table" if as_matrix else output_type)
    bases, runs = default_engine().multi_pairwise(sides, strict=zero_based, n_contigs=n_contigs)
    n = len(sides)
    own = np.diagonal(bases)
    union = own[:, None] + own[None, :] - bases
    if as_matrix:
        if statistic == "intersection":
            return bases
        if statistic == "union":
            return union
        if statistic == "n_intersections":
            return runs
        den = union if statistic == "jaccard" else np.broadcast_to(own[:, None], bases.shape)
        res = np.full(bases.shape, np.nan)
        np.divide(bases, den, out=res, where=den != 0)
        return res
    labels = pa.array(names, type=pa.string()) if names is not None else pa.array(np.arange(n, dtype=np.int64))
    first, second = np.repeat(np.arange(n), n), np.tile(np.arange(n), n)
    inter, uni = bases.reshape(-1), union.reshape(-1)
    res = pa.table({"frame_1": labels.take(pa.array(first)), "frame_2": labels.take(pa.array(second)),
                    "intersection": pa.array(inter, type=pa.int64()), "union": pa.array(uni, type=pa.int64()),
                    "jaccard": pa.array([int(i) / int(u) if u else None for i, u in zip(inter, uni)], type=pa.float64()),
                    "n_intersections": pa.array(runs.reshape(-1), type=pa.int64())})
    return A.from_arrow(res, output_type, zero_based)


pairwise_jaccard.__doc__ = """How similar is every frame to every other: ``jaccard`` for all F^2 ordered pairs of the F frames from
    ONE walk over all of them (the "Jaccard statistic for all pairwise comparisons" heat map of bedtools, ``intervene pairwise``,
    DiffBind's overlap correlation) instead of F (F - 1) / 2 ``jaccard`` calls.

    Output, the long form, pivot-ready: one row per ordered pair in row-major order -- ``frame_1``, ``frame_2`` (the ``names``, one
    distinct string per frame, or the frames' Int64 positions in the list without them), ``intersection`` (Int64, positions both
    frames cover), ``union`` (Int64), ``jaccard`` (Float64, intersection / union computed on the host from the two exact integers;
    null where the union is empty) and ``n_intersections`` (Int64, the regions ``set_intersect`` of the pair would return).  The
    pair of a frame with itself holds what the frame covers and its merged regions.

    ``output_type="numpy.ndarray"`` returns the bare (F, F) matrix of ``statistic`` instead: "jaccard" (Float64, NaN where the union
    is empty), "intersection", "union", "n_intersections" (Int64) or "fraction" (Float64, intersection[i, j] / intersection[i, i]:
    the share of frame i that frame j covers -- not symmetric; NaN for an empty frame i).  With ``on_cols`` the totals are summed
    over the groups.""" + _MULTI_DOC


def cluster(
    df,
    min_dist: int = 0,
    cols: Union[list, None] = ["chrom", "start", "end"],
    output_type: str = "polars.LazyFrame",
    projection_pushdown: bool = True,
):
    """Cluster ids for overlapping / nearby intervals (reference: range_op.py:660-715; ClusterProvider,
    src/operation.rs:383-418).  Output: every input column + ``cluster``, ``cluster_start``, ``cluster_end``
    (Int64), input row order; clusters are numbered in (chrom, start) order (range_op_helpers.py:93-121)."""
    _validate_overlap_input(cols, cols, None, ("_1", "_2"), output_type)
    zero_based = validate_coordinate_system_single(df)
    cols = list(DEFAULT_INTERVAL_COLUMNS if cols is None else cols)
    t = A.to_arrow(df)
    side, n_contigs, _ = A.encode_frame(t, cols)
    keep = side[0] >= 0                                   # rows with a null chrom belong to no contig: null cluster columns
    null_mask = None
    if keep.all():
        cid, cs, ce, _ = default_engine().cluster(side, strict=zero_based, n_contigs=n_contigs, min_dist=int(min_dist))
    else:
        kc, ks, ke, _ = default_engine().cluster(tuple(a[keep] for a in side), strict=zero_based, n_contigs=n_contigs,
                                                 min_dist=int(min_dist))
        n_all = len(keep)
        cid, cs, ce = np.zeros(n_all, np.int64), np.zeros(n_all, np.int32), np.zeros(n_all, np.int32)
        cid[keep], cs[keep], ce[keep] = kc, ks, ke
        null_mask = ~keep
    res = t
    if t.num_columns == 3:                                # the classic triplet comes back with Int64 coordinates
        res = pa.table({cols[0]: t.column(cols[0]), cols[1]: pc.cast(t.column(cols[1]), pa.int64()),
                        cols[2]: pc.cast(t.column(cols[2]), pa.int64())})
    res = res.append_column("cluster", pa.array(cid, type=pa.int64(), mask=null_mask))
    res = res.append_column("cluster_start", pa.array(cs.astype(np.int64), mask=null_mask))
    res = res.append_column("cluster_end", pa.array(ce.astype(np.int64), mask=null_mask))
    return A.from_arrow(res, output_type, zero_based)


_I32_MAX = np.iinfo(np.int32).max
_I64_MAX = np.iinfo(np.int64).max


def complement(
    df,
    view_df=None,
    cols: Union[list, None] = ["chrom", "start", "end"],
    view_cols: Union[list, None] = None,
    output_type: str = "polars.LazyFrame",
    projection_pushdown: bool = True,
):
    """Gaps between the intervals of ``df`` (reference: range_op.py:717-790; ComplementProvider,
    src/operation.rs:420-455).  With ``view_df`` the gaps are taken inside its intervals (e.g. one row per
    chromosome); without it every contig of ``df`` spans [0, i64::MAX) and a warning says so.
    Output: (chrom, start: Int64, end: Int64) (range_op_helpers.py:124-137)."""
    _validate_overlap_input(cols, cols, None, ("_1", "_2"), output_type)
    zero_based = validate_coordinate_system_single(df)
    cols = list(DEFAULT_INTERVAL_COLUMNS if cols is None else cols)
    view_cols = cols if view_cols is None else list(view_cols)
    t = A.to_arrow(df)
    open_ended = view_df is None
    if open_ended:
        logger.warning("No view_df provided -- complement will span [0, i64::MAX) per contig. "
                       "Pass a view_df with contig boundaries (e.g., chromosome sizes).")
        chroms = pc.drop_null(pc.unique(A._as_string(t.column(cols[0]))))
        chroms = chroms.combine_chunks() if isinstance(chroms, pa.ChunkedArray) else chroms
        # the device works on int32 coordinates: the open end is carried as INT32_MAX and restored below
        tv = pa.table({view_cols[0]: chroms, view_cols[1]: pa.array(np.zeros(len(chroms), np.int32)),
                       view_cols[2]: pa.array(np.full(len(chroms), _I32_MAX, np.int32))})
    else:
        tv = A.to_arrow(view_df)
    frame, view, n_contigs, dictionary = A.encode_keys(t, cols, tv, view_cols, with_dictionary=True)
    vkeep = view[0] >= 0                                  # view rows with a null chrom name no contig: dropped (as merge does)
    if not vkeep.all():
        view = tuple(a[vkeep] for a in view)
    row, s, e = default_engine().complement(frame, view, strict=zero_based, n_contigs=n_contigs)
    e64 = e.astype(np.int64)
    if open_ended:
        e64[e == (_I32_MAX if zero_based else _I32_MAX)] = _I64_MAX
    chrom = pc.take(dictionary, pa.array(view[0][row], type=pa.int32()))
    res = pa.table({cols[0]: pc.cast(chrom, pa.string()), cols[1]: pa.array(s.astype(np.int64)), cols[2]: pa.array(e64)})
    return A.from_arrow(res, output_type, zero_based)


def subtract(
    df1,
    df2,
    cols1: Union[list, None] = ["chrom", "start", "end"],
    cols2: Union[list, None] = ["chrom", "start", "end"],
    output_type: str = "polars.LazyFrame",
    projection_pushdown: bool = True,
):
    """Every df1 interval minus the parts covered by df2 intervals (reference: range_op.py:792-857;
    SubtractProvider, src/operation.rs:457-510).  Output: the df1 columns, one row per remaining fragment,
    start / end replaced by the fragment's; the classic triplet comes back with Int64 coordinates
    (range_op_helpers.py:140-158)."""
    _validate_overlap_input(cols1, cols2, None, ("_1", "_2"), output_type)
    zero_based = validate_coordinate_systems(df1, df2)
    t1, t2, left, right, n_contigs, _keys = _prepare(df1, df2, cols1, cols2)
    c1 = list(DEFAULT_INTERVAL_COLUMNS if cols1 is None else cols1)
    row, s, e = default_engine().subtract(left, right, strict=zero_based, n_contigs=n_contigs)
    res = A.take_rows(t1, row)
    triplet = t1.num_columns == 3
    for name, arr in ((c1[1], s), (c1[2], e)):
        typ = pa.int64() if triplet else t1.schema.field(name).type
        res = res.set_column(res.column_names.index(name), pa.field(name, typ), pc.cast(pa.array(arr, type=pa.int32()), typ))
    return A.from_arrow(res, output_type, zero_based)
