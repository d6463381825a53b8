"""The yardstick of pb.map_quantiles / pb.map_median (test helper; numpy only): the matching (probe row, build row) pairs from the
brute force of tests/_overlap_agg_util.py (oracle.overlap_brute, _thresholds_util.brute under thresholds), then per probe row a
LITERAL np.sort of the valid matched values, indexed with range_op.quantile_ranks(m, q) -- no knowledge of tiles, chunks, digits
or keys.  Comparison is exact: int64 bit for bit; doubles bit for bit except that zeros compare with == and NaN matches NaN."""
import numpy as np

from polars_bio_amd import _engine
from polars_bio_amd.range_op import quantile_ranks
import _overlap_agg_util as A

ROOT = A.ROOT
pairs = A.pairs
kernel_geometry = A.kernel_geometry
per_wave = A.per_wave


def rows_per_workgroup(n_q):
    """Probe rows one workgroup of the select kernel owns for n_q requests, from the constants of include/ivjoin.h."""
    import re
    hdr = open(f"{ROOT}/include/ivjoin.h").read()
    bits = int(re.search(r"#define IVJ_OVQ_BITS (\d+)", hdr).group(1))
    lds = int(re.search(r"#define IVJ_OVQ_LDS_BYTES (\d+)", hdr).group(1))
    tile = int(re.search(r"#define IVJ_OVQ_MAX_TILE (\d+)", hdr).group(1))
    p = min(max(lds // (n_q * (1 << bits) * 4), 1), tile)
    assert p == _engine.overlap_quant_tile(n_q)
    return p


def matched_values(p, b, n_probe, values, valid=None, n_values=None):
    """-> per probe row the array of its valid matched values, in no particular order."""
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
    return [values[b[first[k]:last[k]]] for k in range(n_probe)]


def select(lists, dtype, q, upper):
    """np.sort of every list, indexed with quantile_ranks -> (out (n, n_q) of dtype, zeros where the list is empty; count int64)."""
    q = np.atleast_1d(np.asarray(q, np.float64))
    upper = np.atleast_1d(np.asarray(upper)).astype(bool)
    out = np.zeros((len(lists), len(q)), dtype)
    count = np.array([len(v) for v in lists], np.int64)
    for k, v in enumerate(lists):
        if len(v) == 0:
            continue
        s = np.sort(v)
        lo, hi, _ = quantile_ranks(len(v), q)
        out[k] = s[np.where(upper, hi, lo)]
    return out, count


def expected(probe, build, n_contigs, strict, values, valid, q, upper, n_values=None, **thr):
    p, b = pairs(probe, build, n_contigs, strict, **thr)
    return select(matched_values(p, b, len(probe[0]), values, valid, n_values), np.asarray(values).dtype, q, upper)


def assert_same(got, exp, what=""):
    """Exact comparison of two arrays of one 8-byte dtype."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, f"{what}: {got.dtype}{got.shape} vs {exp.dtype}{exp.shape}"
    if got.dtype == np.float64:
        same = (got.view(np.uint64) == exp.view(np.uint64)) | ((got == 0.0) & (exp == 0.0)) | (np.isnan(got) & np.isnan(exp))
    else:
        same = got == exp
    if not same.all():
        at = np.argwhere(~same)[0]
        raise AssertionError(f"{what}: {int((~same).sum())} cells differ, first at {tuple(at)}: got {got[tuple(at)]!r}, expected {exp[tuple(at)]!r}")
