"""The yardstick of pb.merge(agg=...) (test helper; numpy only): the cluster id of every row from the oracle's sweep
(oracle.np_cluster, a plain loop over the sorted rows), then a LITERAL group-by -- per cluster id the valid values of its rows,

    count = how many,      sum = np.add.reduce in the column's dtype (int64 wraps as numpy does),
    min / max = np.fmin / np.fmax reductions (NaN only where every value is NaN),      mean = float64(sum) / count

-- and no knowledge of tiles, scans or the sorted order.  A cluster without a valid value has count 0 and sum 0; its min, max
and mean are reported as None."""
import os
import re

import numpy as np

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ("sum", "min", "max", "mean", "count")


def kernel_tile():
    """Sorted positions per workgroup of the aggregate kernel, from its header."""
    src = open(os.path.join(ROOT, "polars-bio_amd", "csrc", "merge_agg.hip.h")).read()
    threads = int(re.search(r"MAGG_THREADS\s*=\s*(\d+)", src).group(1))
    items = int(re.search(r"MAGG_ITEMS\s*=\s*(\d+)", src).group(1))
    return threads * items


def clusters(side, n_contigs, strict, min_dist=0):
    """-> (cluster id per input row in the ENGINE's numbering, merged table (contig, start, end, n_intervals) in the engine's
    order): (contig id, start) order with the rows outside the dictionary as the pseudo-contig -1 after every real contig."""
    c = np.asarray(side[0])
    c = np.where((c >= 0) & (c < n_contigs), c, -1).astype(np.int32)
    cid, _, _, (mc, ms, me, mn) = O.np_cluster(O.Side(c, side[1], side[2]), strict, min_dist)
    order = np.lexsort((ms, np.where(mc < 0, n_contigs, mc)))
    rank = np.empty(len(order), np.int64)
    rank[order] = np.arange(len(order))
    table = (np.asarray(mc, np.int32)[order], np.asarray(ms, np.int32)[order], np.asarray(me, np.int32)[order], np.asarray(mn, np.int64)[order])
    return (rank[cid] if len(cid) else np.empty(0, np.int64)), table


def group_by(cid, n_clusters, values, valid=None):
    """The literal group-by -> dict op -> list with one entry per cluster (None where the op has no value)."""
    values = np.asarray(values)
    assert values.dtype in (np.int64, np.float64)
    use = np.ones(len(values), bool) if valid is None else np.asarray(valid).astype(bool)
    out = {op: [] for op in OPS}
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(n_clusters):
            v = values[(cid == k) & use]
            out["count"].append(len(v))
            if len(v) == 0:
                out["sum"].append(values.dtype.type(0))
                for op in ("min", "max", "mean"):
                    out[op].append(None)
                continue
            s = np.add.reduce(v, dtype=values.dtype)
            out["sum"].append(s)
            out["min"].append(np.fmin.reduce(v))
            out["max"].append(np.fmax.reduce(v))
            out["mean"].append(np.float64(s) / np.float64(len(v)))
    return out


def bits(x, dtype):
    """One value as its 64 bits, for bit-exact comparison (NaN payloads and signed zeros included)."""
    return int(np.asarray(x, dtype=dtype).reshape(1).view(np.uint64)[0])


def assert_column(got, exp, dtype, what=""):
    """got: dict op -> array of the engine for one value column; exp: group_by's dict.  Every op present in got is compared bit for
    bit with the yardstick; entries the yardstick reports as None are unspecified and skipped.  A NaN expected compares as NaN."""
    for op, arr in got.items():
        want = exp[op]
        assert len(arr) == len(want), f"{what} {op}: {len(arr)} clusters, expected {len(want)}"
        kind = np.int64 if op == "count" else np.float64 if op == "mean" else dtype
        assert np.asarray(arr).dtype == kind, f"{what} {op}: dtype {np.asarray(arr).dtype}, expected {np.dtype(kind)}"
        for k, w in enumerate(want):
            if w is None:
                continue
            g = arr[k]
            if kind == np.float64 and np.isnan(w):
                assert np.isnan(g), f"{what} {op}[{k}]: got {g!r}, expected NaN"
            else:
                assert bits(g, kind) == bits(w, kind), f"{what} {op}[{k}]: got {g!r}, expected {w!r}"
