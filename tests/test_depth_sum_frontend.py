"""pb.mean_depth, the front door: export, argument validation (CPU); input kinds, output schema and order, both coordinate
systems, on_cols, nulls, the mean's exact definition, the .pb accessor and the round trip through pb.depth (GPU)."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
import _depth_sum_util as S

gpu = pytest.mark.gpu
NAMES = np.array(["chr10", "chr2", "chrX", "chr1"])


def _frame(zero_based, seed, n, max_len, strand=False, null_chrom=False, null_strand=False, empty_rows=False):
    rng = np.random.default_rng(seed)
    c, s, e = S.U.random_rows(rng, n, len(NAMES), 1500, max_len=max_len)
    s, e = s.astype(np.int64), e.astype(np.int64)
    if empty_rows:
        kind = rng.integers(0, 6, n)
        e = np.where(kind == 0, s - (0 if zero_based else 1), e)       # no position
        e = np.where(kind == 1, s - 5, e)                              # inverted
    d = {"chrom": NAMES[c].astype(object), "start": s, "end": e}
    if strand:
        d["strand"] = np.array(["+", "-"])[rng.integers(0, 2, n)].astype(object)
        if null_strand:
            d["strand"][rng.integers(0, n, n // 10)] = None
    if null_chrom:
        d["chrom"][rng.integers(0, n, n // 10)] = None
    df = pd.DataFrame(d)
    df.attrs["coordinate_system_zero_based"] = zero_based
    return df


def _expected_bases(df1, df2, zero_based, on=None):
    """the pair form on the frames' rows; rows with a null key get the id -1, which matches nothing"""
    def ids(df):
        key = df["chrom"].astype(object)
        ok = key.notna()
        if on:
            ok &= df[on].notna()
            key = key.astype(str) + "\t" + df[on].astype(str)
        return key, ok
    k1, ok1 = ids(df1)
    k2, ok2 = ids(df2)
    names = np.array(sorted(set(k1[ok1]) | set(k2[ok2])))
    c1 = np.where(ok1, np.searchsorted(names, k1.astype(str).to_numpy()), -1)
    c2 = np.where(ok2, np.searchsorted(names, k2.astype(str).to_numpy()), -1)
    probe = (c1, df1["start"].to_numpy(), df1["end"].to_numpy())
    build = (c2, df2["start"].to_numpy(), df2["end"].to_numpy())
    return S.pair_form(probe, build, zero_based, len(names))


def test_mean_depth_is_exported():
    assert "mean_depth" in pb.__all__ and callable(pb.mean_depth)


def test_argument_validation():
    df = _frame(True, 1, 10, 20, strand=True)
    with pytest.raises(AssertionError):
        pb.mean_depth(df, df, output_type="numpy")
    with pytest.raises(AssertionError, match="interval columns"):
        pb.mean_depth(df, df, on_cols=["start"], output_type="pandas.DataFrame")
    with pytest.raises(AssertionError, match="twice"):
        pb.mean_depth(df, df, on_cols=["strand", "strand"], output_type="pandas.DataFrame")


def test_a_missing_on_cols_column_raises():
    df1 = _frame(True, 1, 10, 20, strand=True)
    df2 = _frame(True, 2, 10, 20)
    with pytest.raises(AssertionError, match="not found"):
        pb.mean_depth(df1, df2, on_cols=["strand"], output_type="pandas.DataFrame")


def _check_result(res, df1, bases, zero_based, extra=()):
    assert list(res.columns) == ["chrom", "start", "end", *extra, "bases", "mean_depth"]
    assert str(res["bases"].dtype) == "int64" and str(res["mean_depth"].dtype) == "float64"
    assert res.attrs["coordinate_system_zero_based"] == zero_based
    assert (res["start"].to_numpy() == df1["start"].to_numpy()).all() and (res["end"].to_numpy() == df1["end"].to_numpy()).all()
    assert (res["bases"].to_numpy() == bases).all()
    L = (df1["end"] - df1["start"]).to_numpy().astype(np.int64) + (0 if zero_based else 1)
    mean = res["mean_depth"].to_numpy()
    assert (np.isnan(mean) == (L <= 0)).all()
    ok = L > 0
    assert (mean[ok] == bases[ok].astype(np.float64) / L[ok].astype(np.float64)).all()          # exactly this quotient


@gpu
@pytest.mark.parametrize("zero_based", [True, False])
def test_pandas_frames(zero_based):
    df1 = _frame(zero_based, 3, 3000, 400, empty_rows=True)
    df2 = _frame(zero_based, 4, 4000, 90, empty_rows=True)
    res = pb.mean_depth(df1, df2, output_type="pandas.DataFrame")
    bases = _expected_bases(df1, df2, zero_based)
    assert (bases > 0).any() and ((df1["end"] - df1["start"]) < 0).any()
    _check_result(res, df1, bases, zero_based)


@gpu
@pytest.mark.parametrize("zero_based", [True, False])
def test_pyarrow_tables(zero_based):
    df1, df2 = _frame(zero_based, 5, 2000, 300), _frame(zero_based, 6, 2500, 80)
    meta = {"coordinate_system_zero_based": "true" if zero_based else "false"}
    t1, t2 = (pa.Table.from_pandas(d, preserve_index=False).replace_schema_metadata(meta) for d in (df1, df2))
    res = pb.mean_depth(t1, t2, output_type="pandas.DataFrame")
    _check_result(res, df1, _expected_bases(df1, df2, zero_based), zero_based)


@gpu
@pytest.mark.parametrize("zero_based", [True, False])
def test_on_cols_equals_the_pair_form_per_group(zero_based):
    df1 = _frame(zero_based, 7, 2500, 300, strand=True)
    df2 = _frame(zero_based, 8, 3000, 90, strand=True)
    res = pb.mean_depth(df1, df2, on_cols=["strand"], output_type="pandas.DataFrame")
    bases = np.zeros(len(df1), np.int64)
    for strand in ("+", "-"):
        m = (df1["strand"] == strand).to_numpy()
        bases[m] = _expected_bases(df1[m], df2[df2["strand"] == strand], zero_based)
    _check_result(res, df1, bases, zero_based, extra=("strand",))
    both = pb.mean_depth(df1, df2, output_type="pandas.DataFrame")["bases"].to_numpy()
    assert (bases <= both).all() and (bases < both).any()


@gpu
def test_null_chrom_and_null_on_value_rows_share_nothing():
    df1 = _frame(True, 9, 2000, 300, strand=True, null_chrom=True, null_strand=True)
    df2 = _frame(True, 10, 2500, 90, strand=True, null_chrom=True, null_strand=True)
    res = pb.mean_depth(df1, df2, on_cols=["strand"], output_type="pandas.DataFrame")
    null = (df1["chrom"].isna() | df1["strand"].isna()).to_numpy()
    assert null.any() and (res["bases"].to_numpy()[null] == 0).all()
    assert (res["bases"].to_numpy() == _expected_bases(df1, df2, True, on="strand")).all()
    plain = pb.mean_depth(df1.drop(columns=["strand"]), df2.drop(columns=["strand"]), output_type="pandas.DataFrame")
    assert (plain["bases"].to_numpy()[df1["chrom"].isna().to_numpy()] == 0).all()


@gpu
def test_pb_accessor():
    df1, df2 = _frame(True, 11, 500, 300), _frame(True, 12, 600, 80)
    res = df1.pb.mean_depth(df2)
    assert isinstance(res, pd.DataFrame)
    pd.testing.assert_frame_equal(res, pb.mean_depth(df1, df2, output_type="pandas.DataFrame"))


@gpu
@pytest.mark.parametrize("zero_based", [True, False])
def test_depth_blocks_fed_back_give_the_same_bases(zero_based):
    df1, df2 = _frame(zero_based, 13, 1500, 400), _frame(zero_based, 14, 2000, 90)
    bases = pb.mean_depth(df1, df2, output_type="pandas.DataFrame")["bases"].to_numpy()
    blocks = pb.depth(df2, output_type="pandas.DataFrame")
    w = 0 if zero_based else 1
    exp = np.zeros(len(df1), np.int64)
    for i, (c, s, e) in enumerate(zip(df1["chrom"], df1["start"], df1["end"])):
        b = blocks[blocks["chrom"] == c]
        clipped = np.maximum(np.minimum(b["end"].to_numpy(), e) - np.maximum(b["start"].to_numpy(), s) + w, 0)
        exp[i] = int((clipped * b["coverage"].to_numpy()).sum())
    assert (bases == exp).all()
