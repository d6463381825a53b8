"""The yardstick of pb.map_overlaps (test helper; numpy only): the matching (probe row, build row) pairs from a brute force --
oracle.overlap_brute for the plain predicate, _thresholds_util.brute under thresholds -- then a LITERAL per-probe group-by over
the valid values of the matched build rows,

    count = how many,      sum = np.add.reduce in the column's dtype (int64 wraps as numpy does),
    min / max = np.fmin / np.fmax reductions (NaN only where every value is NaN),      mean = float64(sum) / count

-- and no knowledge of tiles, chunks, wavefronts or the sorted order.  A probe without a valid matched value has count 0 and
sum 0; its min, max and mean are reported as None.  Build rows at or beyond ``n_values`` carry no value."""
import os
import re

import numpy as np

from oracle import oracle as O
import _thresholds_util as T
from _merge_agg_util import OPS, assert_column, bits  # noqa: F401  (re-exported for the tests)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_geometry():
    """(probes per workgroup, candidates per chunk, threads per workgroup, wavefront width) of the reduce kernel, read from the
    headers it takes them from."""
    src = open(os.path.join(ROOT, "polars-bio_amd", "csrc", "thresh.hip.h")).read()
    threads = int(re.search(r"THRESH_THREADS\s*=\s*(\d+)", src).group(1))
    items = int(re.search(r"THRESH_ITEMS\s*=\s*(\d+)", src).group(1))
    chunk = int(re.search(r"THRESH_CH\s*=\s*(\d+)", src).group(1))
    agg = open(os.path.join(ROOT, "polars-bio_amd", "csrc", "overlap_agg.hip.h")).read()
    assert "THRESH_CH" in agg and "THRESH_TILE" in agg, "the reduce kernel no longer takes its geometry from thresh.hip.h"
    return threads * items, chunk, threads, 64


def per_wave(n_chunk):
    """Candidates of one wavefront's sub-range in a chunk of n_chunk candidates (the `per` of the kernels)."""
    _, _, threads, wave = kernel_geometry()
    return ((n_chunk + threads - 1) // threads) * wave


def pairs(probe, build, n_contigs, strict, **thr):
    """-> (probe_idx, build_idx) of the matching pairs.  Rows outside the dictionary match nothing."""
    if thr:
        p, b, _ = T.brute(probe, build, n_contigs, strict, **thr)
        return np.asarray(p, np.int64), np.asarray(b, np.int64)
    # the brute force contig by contig (it compares every probe row with every build row it is given)
    pc, bc = np.asarray(probe[0]), np.asarray(build[0])
    outp, outb = [np.empty(0, np.int64)], [np.empty(0, np.int64)]
    for c in np.unique(pc):
        if c < 0 or c >= n_contigs:
            continue
        P, B = np.nonzero(pc == c)[0], np.nonzero(bc == c)[0]
        if len(B) == 0:
            continue
        p, b = O.overlap_brute(O.Side(*(np.asarray(a)[P] for a in probe)), O.Side(*(np.asarray(a)[B] for a in build)), strict)
        outp.append(P[np.asarray(p, np.int64)])
        outb.append(B[np.asarray(b, np.int64)])
    return np.concatenate(outp), np.concatenate(outb)


def group_by(p, b, n_probe, values, valid=None, n_values=None):
    """The literal group-by -> dict op -> list with one entry per probe row (None where the op has no value)."""
    values = np.asarray(values)
    assert values.dtype in (np.int64, np.float64)
    n_values = len(values) if n_values is None else n_values
    use = np.ones(len(values), bool) if valid is None else np.asarray(valid).astype(bool)
    inside = b < n_values
    p, b = p[inside], b[inside]
    ok = use[b]
    p, b = p[ok], b[ok]
    order = np.argsort(p, kind="stable")
    p, b = p[order], b[order]
    first = np.searchsorted(p, np.arange(n_probe), "left")
    last = np.searchsorted(p, np.arange(n_probe), "right")
    out = {op: [] for op in OPS}
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(n_probe):
            v = values[b[first[k]:last[k]]]
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


def expected(probe, build, n_contigs, strict, values, valid=None, n_values=None, **thr):
    p, b = pairs(probe, build, n_contigs, strict, **thr)
    return group_by(p, b, len(probe[0]), values, valid, n_values)
