"""The yardstick of pb.signal_summary / pb.signal_profile (test helper; numpy and Python ints only): ALL (probe row, build row)
pairs of a contig, the shared positions by the formula

    ov = min(q.end, b.end) - max(q.start, b.start) (+ 1 for closed frames)          int64

a build row CONTRIBUTES iff ov >= max(1, min_overlap, probe_min[q], build_min[b]) (0xffffffff = never), its value is valid and it
lies inside n_values; then per probe, literally,

    count (= bases) = sum of ov            Python ints, wrapped to int64 at the end
    sum             = sum of value * ov    int64 columns: Python ints, wrapped to int64 at the end
                                           double columns: math.fsum of the float products value * float(ov)
    min / max       = np.fmin / np.fmax over the contributing values
    mean            = float64(sum) / float64(bases)

-- no knowledge of tiles, chunks, wavefronts or the sorted order.  "n" holds the number of contributing rows (for vacuity guards).
A probe without a contributing row has count 0 and sum 0; its min, max and mean are None.  The bins of a window come from
range_op.profile_windows / profile_bin_lengths plus cumulative sums."""
import math

import numpy as np

from polars_bio_amd import range_op
import _overlap_agg_util as OU
from _overlap_agg_util import OPS, assert_column, bits, kernel_geometry, per_wave  # noqa: F401  (re-exported for the tests)

NEVER = 0xFFFFFFFF


def wrap64(x: int) -> int:
    """A Python int as the int64 with the same low 64 bits."""
    return ((int(x) + (1 << 63)) % (1 << 64)) - (1 << 63)


def summary(probe, build, n_contigs, strict, values, valid=None, n_values=None, min_overlap=0, probe_min=None, build_min=None):
    """-> dict op -> list with one entry per probe row, plus "n"."""
    values = np.asarray(values)
    assert values.dtype in (np.int64, np.float64)
    is_int = values.dtype == np.int64
    pc, ps, pe = (np.asarray(a).astype(np.int64) for a in probe)
    bc, bs, be = (np.asarray(a).astype(np.int64) for a in build)
    n, nb = len(pc), len(bc)
    n_values = len(values) if n_values is None else n_values
    use = np.ones(nb, bool) if valid is None else np.concatenate([np.asarray(valid).astype(bool), np.zeros(nb, bool)])[:nb]
    use = use & (np.arange(nb) < n_values)
    pm = np.zeros(n, np.int64) if probe_min is None else np.asarray(probe_min).astype(np.int64)
    bm = np.zeros(nb, np.int64) if build_min is None else np.asarray(build_min).astype(np.int64)
    w = 0 if strict else 1
    out = {op: [None] * n for op in OPS}
    out["n"] = [0] * n
    out["count"] = [0] * n
    out["sum"] = [values.dtype.type(0)] * n
    for c in np.unique(pc):
        if c < 0 or c >= n_contigs:
            continue
        B = np.nonzero((bc == c) & use)[0]
        if len(B) == 0:
            continue
        for k in np.nonzero(pc == c)[0]:
            ov = np.minimum(pe[k], be[B]) - np.maximum(ps[k], bs[B]) + w
            need = np.maximum(np.maximum(1, int(min_overlap)), np.maximum(pm[k], bm[B]))
            hit = (ov >= need) & (bm[B] != NEVER) & (pm[k] != NEVER)
            rows, o = B[hit], ov[hit]
            if len(rows) == 0:
                continue
            v = values[rows]
            bases = sum(int(x) for x in o)
            out["n"][k] = len(rows)
            out["count"][k] = np.int64(wrap64(bases))
            if is_int:
                total = np.int64(wrap64(sum(int(a) * int(x) for a, x in zip(v, o))))
            else:
                prods = [float(a) * float(x) for a, x in zip(v, o)]
                total = np.float64(math.nan) if any(math.isnan(p) for p in prods) else np.float64(math.fsum(prods))
            out["sum"][k] = total
            out["min"][k] = np.fmin.reduce(v)
            out["max"][k] = np.fmax.reduce(v)
            with np.errstate(invalid="ignore", divide="ignore"):
                out["mean"][k] = np.float64(float(total)) / np.float64(float(wrap64(bases)))
    return out


def bin_frame(windows, strict, n_bins, reverse=None):
    """The explicit bin frame of the windows, row-major in OUTPUT order (a reversed row's bins right to left): (contig, start, end)
    int64 in the frame's own convention, and the bin lengths.  An empty bin is a row that covers no position and is always
    representable in int32: (0, 0) half-open, (0, -1) closed."""
    c, s, e = (np.asarray(a).astype(np.int64) for a in windows)
    lens = range_op.profile_bin_lengths(s, e, strict, n_bins)                 # left to right
    edges = s[:, None] + np.concatenate([np.zeros((len(s), 1), np.int64), np.cumsum(lens, axis=1)], axis=1)
    bs, be = edges[:, :-1].copy(), edges[:, 1:] - (0 if strict else 1)
    bs[lens <= 0], be[lens <= 0] = 0, (0 if strict else -1)
    if reverse is not None:
        rev = np.asarray(reverse).astype(bool)
        bs[rev], be[rev], lens[rev] = bs[rev, ::-1], be[rev, ::-1], lens[rev, ::-1]
    bc = np.repeat(c, n_bins)
    return (bc, bs.reshape(-1), be.reshape(-1)), lens


def profile(windows, build, n_contigs, strict, n_bins, values, valid=None, reverse=None):
    """The yardstick of the profile: summary() of the explicit bin frame -> dict op -> list of n * n_bins entries, row-major."""
    frame, _ = bin_frame(windows, strict, n_bins, reverse)
    return summary(frame, build, n_contigs, strict, values, valid)


def mean_depth_bases(probe, build, n_contigs, strict):
    """The yardstick of mean_depth's bases, independent of summary(): per probe the shared positions summed over the build rows."""
    pc, ps, pe = (np.asarray(a).astype(np.int64) for a in probe)
    bc, bs, be = (np.asarray(a).astype(np.int64) for a in build)
    w = 0 if strict else 1
    out = np.zeros(len(pc), np.int64)
    for k in range(len(pc)):
        if 0 <= pc[k] < n_contigs:
            m = bc == pc[k]
            out[k] = np.clip(np.minimum(pe[k], be[m]) - np.maximum(ps[k], bs[m]) + w, 0, None).sum()
    return out
