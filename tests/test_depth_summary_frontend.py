"""pb.depth_summary, the front door: export, accessor entry, argument validation (CPU); input kinds, output schema and order, both
coordinate systems, on_cols, nulls, and the identities with pb.coverage, pb.mean_depth and pb.depth (GPU)."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
from polars_bio_amd import namespace, range_op
import _depth_summary_util as D
from test_depth_sum_frontend import _frame

gpu = pytest.mark.gpu
THR = (1, 3, 2)


def _ids(df1, df2, on=None):
    """contig ids of both frames' rows over their shared names; rows with a null key get -1, which matches nothing"""
    def keys(df):
        key = df["chrom"].astype(object)
        ok = key.notna()
        if on:
            ok &= df[on].notna()
            key = key.astype(str) + "\t" + df[on].astype(str)
        return key, ok
    k1, ok1 = keys(df1)
    k2, ok2 = keys(df2)
    names = np.array(sorted(set(k1[ok1]) | set(k2[ok2])))
    c1 = np.where(ok1, np.searchsorted(names, k1.astype(str).to_numpy()), -1)
    c2 = np.where(ok2, np.searchsorted(names, k2.astype(str).to_numpy()), -1)
    return c1, c2, len(names)


def _expected(df1, df2, zero_based, thresholds, on=None):
    c1, c2, nc = _ids(df1, df2, on)
    probe = (c1, df1["start"].to_numpy(), df1["end"].to_numpy())
    build = (c2, df2["start"].to_numpy(), df2["end"].to_numpy())
    return D.block_form(probe, build, zero_based, nc, thresholds)


def _check_result(res, df1, exp, zero_based, thresholds, extra=()):
    md, bg = exp
    assert list(res.columns) == ["chrom", "start", "end", *extra, "max_depth", *(f"bases_ge_{t}" for t in thresholds)]
    assert all(str(res[c].dtype) == "int64" for c in res.columns[3 + len(extra):])
    assert res.attrs["coordinate_system_zero_based"] == zero_based
    assert (res["start"].to_numpy() == df1["start"].to_numpy()).all() and (res["end"].to_numpy() == df1["end"].to_numpy()).all()
    assert (res["max_depth"].to_numpy() == md).all()
    for k, t in enumerate(thresholds):
        assert (res[f"bases_ge_{t}"].to_numpy() == bg[k]).all(), t


def test_depth_summary_is_exported():
    assert "depth_summary" in pb.__all__ and callable(pb.depth_summary) and "depth_summary" in range_op.__all__


def test_the_accessor_table_holds_it():
    assert namespace._ALIASES["depth_summary"] == (range_op.depth_summary, True)
    assert list(namespace._ALIASES).index("depth_summary") == list(namespace._ALIASES).index("mean_depth") + 1


def test_argument_validation():
    df = _frame(True, 1, 10, 20, strand=True)
    with pytest.raises(AssertionError):
        pb.depth_summary(df, df, output_type="numpy")
    with pytest.raises(AssertionError, match="interval columns"):
        pb.depth_summary(df, df, on_cols=["start"], output_type="pandas.DataFrame")
    for bad in [(0,), (1, -2), (1.5,), ("1",), (True,), 3, "12", None, (1, 2, 2), (2 ** 31,), tuple(range(1, 10))]:
        with pytest.raises(ValueError, match="threshold"):
            pb.depth_summary(df, df, thresholds=bad, output_type="pandas.DataFrame")
    with pytest.raises(ValueError, match="at most 8"):
        pb.depth_summary(df, df, thresholds=range(1, 10), output_type="pandas.DataFrame")
    with pytest.raises(ValueError, match="distinct"):
        pb.depth_summary(df, df, thresholds=[4, 1, 4], output_type="pandas.DataFrame")


def test_a_missing_on_cols_column_raises():
    df1 = _frame(True, 1, 10, 20, strand=True)
    df2 = _frame(True, 2, 10, 20)
    with pytest.raises(AssertionError, match="not found"):
        pb.depth_summary(df1, df2, on_cols=["strand"], output_type="pandas.DataFrame")


def test_mismatched_coordinate_systems_raise():
    with pytest.raises(pb.CoordinateSystemMismatchError):
        pb.depth_summary(_frame(True, 1, 10, 20), _frame(False, 2, 10, 20), output_type="pandas.DataFrame")


@gpu
@pytest.mark.parametrize("zero_based", [True, False])
def test_pandas_frames(zero_based):
    df1 = _frame(zero_based, 3, 3000, 400, empty_rows=True)
    df2 = _frame(zero_based, 4, 4000, 90, empty_rows=True)
    res = pb.depth_summary(df1, df2, thresholds=THR, output_type="pandas.DataFrame")
    exp = _expected(df1, df2, zero_based, THR)
    assert (exp[0] >= 3).any() and ((df1["end"] - df1["start"]) < 0).any()
    _check_result(res, df1, exp, zero_based, THR)


@gpu
@pytest.mark.parametrize("zero_based", [True, False])
def test_pyarrow_tables(zero_based):
    df1, df2 = _frame(zero_based, 5, 2000, 300), _frame(zero_based, 6, 2500, 80)
    meta = {"coordinate_system_zero_based": "true" if zero_based else "false"}
    t1, t2 = (pa.Table.from_pandas(d, preserve_index=False).replace_schema_metadata(meta) for d in (df1, df2))
    res = pb.depth_summary(t1, t2, thresholds=THR, output_type="pandas.DataFrame")
    _check_result(res, df1, _expected(df1, df2, zero_based, THR), zero_based, THR)
    tab = pb.depth_summary(t1, t2, thresholds=THR, output_type="pyarrow.Table")
    assert isinstance(tab, pa.Table) and tab.column_names[-4:] == ["max_depth", "bases_ge_1", "bases_ge_3", "bases_ge_2"]
    assert all(tab.schema.field(c).type == pa.int64() for c in tab.column_names[-4:])
    assert tab.column("bases_ge_3").to_numpy().tolist() == res["bases_ge_3"].tolist()


@gpu
def test_no_thresholds_gives_max_depth_only():
    df1, df2 = _frame(True, 15, 800, 300), _frame(True, 16, 900, 80)
    res = pb.depth_summary(df1, df2, thresholds=(), output_type="pandas.DataFrame")
    _check_result(res, df1, _expected(df1, df2, True, ()), True, ())
    one = pb.depth_summary(df1, df2, output_type="pandas.DataFrame")                  # the default: (1,)
    assert list(one.columns)[-2:] == ["max_depth", "bases_ge_1"]


@gpu
@pytest.mark.parametrize("zero_based", [True, False])
def test_on_cols_restricts_to_the_group(zero_based):
    df1 = _frame(zero_based, 7, 2500, 300, strand=True)
    df2 = _frame(zero_based, 8, 3000, 90, strand=True)
    res = pb.depth_summary(df1, df2, thresholds=THR, on_cols=["strand"], output_type="pandas.DataFrame")
    exp = _expected(df1, df2, zero_based, THR, on="strand")
    _check_result(res, df1, exp, zero_based, THR, extra=("strand",))
    both = pb.depth_summary(df1, df2, thresholds=THR, output_type="pandas.DataFrame")
    assert (res["max_depth"] <= both["max_depth"]).all() and (res["max_depth"] < both["max_depth"]).any()


@gpu
def test_null_chrom_and_null_on_value_rows_receive_zero():
    df1 = _frame(True, 9, 2000, 300, strand=True, null_chrom=True, null_strand=True)
    df2 = _frame(True, 10, 2500, 90, strand=True, null_chrom=True, null_strand=True)
    res = pb.depth_summary(df1, df2, thresholds=THR, on_cols=["strand"], output_type="pandas.DataFrame")
    null = (df1["chrom"].isna() | df1["strand"].isna()).to_numpy()
    assert null.any()
    for col in ["max_depth", *(f"bases_ge_{t}" for t in THR)]:
        assert (res[col].to_numpy()[null] == 0).all()
    md, bg = _expected(df1, df2, True, THR, on="strand")
    assert (res["max_depth"].to_numpy() == md).all() and (res["bases_ge_3"].to_numpy() == bg[1]).all()


@gpu
def test_pb_accessor():
    df1, df2 = _frame(True, 11, 500, 300), _frame(True, 12, 600, 80)
    res = df1.pb.depth_summary(df2, thresholds=(2,))
    assert isinstance(res, pd.DataFrame)
    pd.testing.assert_frame_equal(res, pb.depth_summary(df1, df2, thresholds=(2,), output_type="pandas.DataFrame"))


@gpu
@pytest.mark.parametrize("zero_based", [True, False])
def test_identities_with_coverage_and_mean_depth(zero_based):
    df1, df2 = _frame(zero_based, 13, 1500, 400, empty_rows=True), _frame(zero_based, 14, 2000, 90, empty_rows=True)
    first = pb.depth_summary(df1, df2, thresholds=(1,), output_type="pandas.DataFrame")
    assert (first["bases_ge_1"].to_numpy() == pb.coverage(df1, df2, output_type="pandas.DataFrame")["coverage"].to_numpy()).all()
    top = int(first["max_depth"].max())
    assert top > 1
    total = np.zeros(len(df1), np.int64)
    for lo in range(1, top + 1, 8):
        ts = tuple(range(lo, min(lo + 8, top + 1)))
        part = pb.depth_summary(df1, df2, thresholds=ts, output_type="pandas.DataFrame")
        total += sum(part[f"bases_ge_{t}"].to_numpy() for t in ts)
    assert (total == pb.mean_depth(df1, df2, output_type="pandas.DataFrame")["bases"].to_numpy()).all()
    cnt = pb.count_overlaps(df1, df2, output_type="pandas.DataFrame")["count"].to_numpy()
    assert (first["max_depth"].to_numpy() <= cnt).all()


@gpu
@pytest.mark.parametrize("zero_based", [True, False])
def test_depth_blocks_filtered_and_fed_to_coverage_give_the_same_bases(zero_based):
    df1, df2 = _frame(zero_based, 17, 1500, 400), _frame(zero_based, 18, 2000, 90)
    res = pb.depth_summary(df1, df2, thresholds=(1, 2, 4), output_type="pandas.DataFrame")
    blocks = pb.depth(df2, output_type="pandas.DataFrame")
    for t in (1, 2, 4):
        deep = blocks[blocks["coverage"] >= t][["chrom", "start", "end"]].reset_index(drop=True)
        deep.attrs["coordinate_system_zero_based"] = zero_based
        assert len(deep) > 0
        cov = pb.coverage(df1, deep, output_type="pandas.DataFrame")["coverage"].to_numpy()
        assert (res[f"bases_ge_{t}"].to_numpy() == cov).all(), t
