"""pb.depth_quantiles and pb.median_depth, the front door: export, accessor entries, argument validation, the refusal of a
several-device engine (CPU); column names and dtypes per method, nulls, all four methods against the per-base form, on_cols, both
coordinate systems, the bare matrix (GPU)."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
from polars_bio_amd import namespace, range_op
import _depth_quant_util as Q
from test_depth_sum_frontend import _frame
from test_depth_summary_frontend import _ids

gpu = pytest.mark.gpu
QS = (0.25, 0.5, 0.75)
METHODS = list(range_op.QUANTILE_METHODS)


def _expected(df1, df2, zero_based, qs, method, on=None):
    """-> (values (n, len(qs)) by the per-base form and the issue's formula, null bool[n])"""
    c1, c2, nc = _ids(df1, df2, on)
    probe = (c1, df1["start"].to_numpy(), df1["end"].to_numpy())
    build = (c2, df2["start"].to_numpy(), df2["end"].to_numpy())
    L = Q.positions(probe, zero_based, nc)
    lo, hi, g = range_op.quantile_ranks(L[:, None], np.asarray(qs, np.float64)[None, :])
    vlo = Q.dense_form(probe, build, zero_based, nc, lo)
    vhi = Q.dense_form(probe, build, zero_based, nc, hi)
    return Q.quantiles(vlo, vhi, g, method), L <= 0


def _columns(res, qs):
    return np.stack([res[f"depth_q{float(x)!r}"].to_numpy(dtype=np.float64, na_value=np.nan) for x in qs], axis=1)


def test_both_are_exported():
    for name in ("depth_quantiles", "median_depth"):
        assert name in pb.__all__ and callable(getattr(pb, name)) and name in range_op.__all__
        assert namespace._ALIASES[name] == (getattr(range_op, name), True)
    assert "quantile_ranks" in range_op.__all__


def test_argument_validation():
    df = _frame(True, 1, 10, 20, strand=True)
    kw = dict(output_type="pandas.DataFrame")
    for bad in ((-0.1,), (1.5,), (0.5, float("nan")), 2):
        with pytest.raises(ValueError, match=r"must lie in \[0, 1\]"):
            pb.depth_quantiles(df, df, q=bad, **kw)
    with pytest.raises(ValueError, match="distinct"):
        pb.depth_quantiles(df, df, q=(0.5, 0.25, 0.5), **kw)
    with pytest.raises(ValueError, match="between 1 and 8 quantiles"):
        pb.depth_quantiles(df, df, q=tuple(np.linspace(0, 1, 9)), **kw)
    with pytest.raises(ValueError, match="between 1 and 8 quantiles"):
        pb.depth_quantiles(df, df, q=(), **kw)
    with pytest.raises(ValueError, match="q must be a float or an iterable"):
        pb.depth_quantiles(df, df, q=("half",), **kw)
    for bad in ("nearest", "median", None):
        with pytest.raises(ValueError, match="method must be one of 'lower', 'higher', 'midpoint', 'linear'"):
            pb.depth_quantiles(df, df, method=bad, **kw)
    with pytest.raises(AssertionError):
        pb.depth_quantiles(df, df, output_type="numpy")
    with pytest.raises(AssertionError, match="not found"):
        pb.median_depth(df, _frame(True, 2, 10, 20), on_cols=["strand"], **kw)
    with pytest.raises(pb.CoordinateSystemMismatchError):
        pb.median_depth(_frame(True, 1, 10, 20), _frame(False, 2, 10, 20), **kw)


def test_a_several_device_engine_is_refused(monkeypatch):
    class Several:                                         # what an engine over several devices looks like to the front door
        pass
    monkeypatch.setattr(range_op, "default_engine", lambda: Several())
    df = _frame(True, 1, 10, 20)
    with pytest.raises(NotImplementedError, match="depth_quantiles needs a single-device engine.*Several"):
        pb.depth_quantiles(df, df, output_type="pandas.DataFrame")
    with pytest.raises(NotImplementedError, match="median_depth needs a single-device engine"):
        pb.median_depth(df, df, output_type="pandas.DataFrame")


@gpu
@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("zero_based", [True, False])
def test_columns_types_nulls_and_values(zero_based, method):
    df1 = _frame(zero_based, 3, 1500, 400, empty_rows=True)
    df2 = _frame(zero_based, 4, 4000, 90, empty_rows=True)
    exp, null = _expected(df1, df2, zero_based, QS, method)
    assert null.any() and not null.all() and (exp[~null] > 0).any()
    tab = pb.depth_quantiles(df1, df2, q=QS, method=method, output_type="pyarrow.Table")
    assert tab.column_names == ["chrom", "start", "end", "depth_q0.25", "depth_q0.5", "depth_q0.75"]
    typ = pa.int64() if method in ("lower", "higher") else pa.float64()
    for name in tab.column_names[3:]:
        assert tab.schema.field(name).type == typ
        assert (np.asarray(tab.column(name).is_null()) == null).all()
    res = pb.depth_quantiles(df1, df2, q=QS, method=method, output_type="pandas.DataFrame")
    assert res.attrs["coordinate_system_zero_based"] == zero_based
    assert (res["start"].to_numpy() == df1["start"].to_numpy()).all() and (res["end"].to_numpy() == df1["end"].to_numpy()).all()
    got = _columns(res, QS)
    assert np.isnan(got[null]).all() and (got[~null] == exp[~null]).all()
    # the default: the three quartiles, "lower"
    default = pb.depth_quantiles(df1, df2, output_type="pyarrow.Table")
    assert default.column_names == tab.column_names and default.schema.field("depth_q0.5").type == pa.int64()


@gpu
def test_column_names_follow_repr_of_the_float():
    df1, df2 = _frame(True, 5, 200, 300), _frame(True, 6, 600, 80)
    tab = pb.depth_quantiles(df1, df2, q=(0, 1, 1 / 3, 0.9), output_type="pyarrow.Table")
    assert tab.column_names[3:] == ["depth_q0.0", "depth_q1.0", "depth_q0.3333333333333333", "depth_q0.9"]
    one = pb.depth_quantiles(df1, df2, q=0.5, output_type="pyarrow.Table")
    assert one.column_names[3:] == ["depth_q0.5"]
    s = pb.depth_summary(df1, df2, thresholds=(), output_type="pandas.DataFrame")
    assert (tab.column("depth_q1.0").to_numpy() == s["max_depth"].to_numpy()).all()
    cov = pb.coverage(df1, df2, output_type="pandas.DataFrame")["coverage"].to_numpy()
    assert ((tab.column("depth_q0.0").to_numpy() > 0) == (cov == (df1["end"] - df1["start"]).to_numpy())).all()


@gpu
def test_median_depth_is_the_lower_half_quantile():
    df1 = _frame(True, 7, 1200, 400, empty_rows=True)
    df2 = _frame(True, 8, 3000, 90)
    med = pb.median_depth(df1, df2, output_type="pyarrow.Table")
    assert med.column_names == ["chrom", "start", "end", "median_depth"] and med.schema.field("median_depth").type == pa.int64()
    q = pb.depth_quantiles(df1, df2, q=(0.5,), output_type="pyarrow.Table")
    assert med.column("median_depth").equals(q.column("depth_q0.5")) and med.column("median_depth").null_count > 0
    m = pb.median_depth(df1, df2, output_type="numpy.ndarray")
    assert m.dtype == np.int64 and m.shape == (len(df1), 1)
    assert (m == pb.depth_quantiles(df1, df2, q=(0.5,), output_type="numpy.ndarray")).all()


@gpu
@pytest.mark.parametrize("method", METHODS)
def test_the_bare_matrix(method):
    df1, df2 = _frame(True, 13, 900, 400, empty_rows=True), _frame(True, 14, 2500, 90, empty_rows=True)
    qs = (0.0, 0.1, 0.5, 0.9, 1.0)
    exp, null = _expected(df1, df2, True, qs, method)
    m = pb.depth_quantiles(df1, df2, q=qs, method=method, output_type="numpy.ndarray")
    assert isinstance(m, np.ndarray) and m.shape == (len(df1), len(qs))
    if method in ("lower", "higher"):
        assert m.dtype == np.int64 and (m[null] == -1).all() and (m[~null] == exp[~null]).all()
    else:
        assert m.dtype == np.float64 and np.isnan(m[null]).all() and (m[~null] == exp[~null]).all()
    assert null.any() and (np.diff(m[~null], axis=1) >= 0).all()


@gpu
@pytest.mark.parametrize("zero_based", [True, False])
def test_on_cols_restricts_to_the_group(zero_based):
    df1 = _frame(zero_based, 9, 1500, 300, strand=True, null_chrom=True, null_strand=True)
    df2 = _frame(zero_based, 10, 4000, 90, strand=True, null_chrom=True, null_strand=True)
    res = pb.depth_quantiles(df1, df2, q=QS, method="linear", on_cols=["strand"], output_type="pandas.DataFrame")
    assert list(res.columns) == ["chrom", "start", "end", "strand", "depth_q0.25", "depth_q0.5", "depth_q0.75"]
    exp, null = _expected(df1, df2, zero_based, QS, "linear", on="strand")
    assert ((df1["chrom"].isna() | df1["strand"].isna()).to_numpy() == null).all() and null.any()
    got = _columns(res, QS)
    assert np.isnan(got[null]).all() and (got[~null] == exp[~null]).all()
    both = pb.depth_quantiles(df1, df2, q=QS, method="linear", output_type="numpy.ndarray")
    keep = ~null
    assert (got[keep] <= both[keep]).all() and (got[keep] < both[keep]).any()


@gpu
def test_pb_accessor():
    df1, df2 = _frame(True, 11, 500, 300), _frame(True, 12, 1500, 80)
    res = df1.pb.depth_quantiles(df2, q=(0.5, 0.9), method="midpoint")
    assert isinstance(res, pd.DataFrame) and list(res.columns)[3:] == ["depth_q0.5", "depth_q0.9"]
    assert (_columns(res, (0.5, 0.9)) == pb.depth_quantiles(df1, df2, q=(0.5, 0.9), method="midpoint", output_type="numpy.ndarray")).all()
    med = df1.pb.median_depth(df2)
    assert isinstance(med, pd.DataFrame) and (med["median_depth"].to_numpy() == pb.median_depth(df1, df2, output_type="numpy.ndarray")[:, 0]).all()
