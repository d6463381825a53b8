"""pb.signal_summary / pb.signal_profile, the front door on the GPU: pandas in, pandas out.  signal_summary against pb.overlap on
the same frames followed by clipping, multiplying and a pandas group-by; signal_profile against signal_summary over a bin frame
built with numpy.  Values are multiples of 1/8 with small magnitudes, so every sum is exact and the comparisons are exact."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
from polars_bio_amd import range_op
import _fake_polars

pytestmark = pytest.mark.gpu
NAMES = np.array(["chr10", "chr2", "chrX", "chr1"])
ZB = [pytest.param(True, id="zero_based"), pytest.param(False, id="one_based")]
STATS = ["size", "bases", "sum", "mean0", "mean", "min", "max"]
PD = dict(output_type="pandas.DataFrame")


def _frame(zero_based, seed, n, max_len, span=3000, values=False, nulls=False):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, span, n).astype(np.int64)
    ln = rng.integers(0, max_len + 1, n)
    ln[rng.random(n) < 0.05] = 0                                     # rows that cover no position
    d = {"chrom": NAMES[rng.integers(0, len(NAMES), n)].astype(object), "start": s, "end": s + ln - (0 if zero_based else 1),
         "strand": np.array(["+", "-"])[rng.integers(0, 2, n)].astype(object), "rid": np.arange(n)}
    if values:
        d["score"] = rng.integers(-400, 400, n) / 8.0                # float64, multiples of 1/8
        d["hits"] = rng.integers(-50, 50, n).astype(np.int32)
        d["f32"] = (rng.integers(-400, 400, n) / 8.0).astype(np.float32)
        d["u32"] = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    df = pd.DataFrame(d)
    if nulls:
        df["score"] = df["score"].where(rng.random(n) > 0.2)
        df["hits"] = df["hits"].astype("Int32").where(rng.random(n) > 0.2)
        df.loc[rng.random(n) < 0.05, "chrom"] = None
    df.attrs["coordinate_system_zero_based"] = zero_based
    return df


def _reference(df1, df2, zero_based, name, **kw):
    """pb.overlap -> clip, multiply, group by df1 row; one row per df1 row with the seven statistics (NaN = null)."""
    w = 0 if zero_based else 1
    pairs = pb.overlap(df1, df2, **PD, **kw)
    ov = np.minimum(pairs["end_1"], pairs["end_2"]) - np.maximum(pairs["start_1"], pairs["start_2"]) + w
    v = pairs[f"{name}_2"]
    keep = (ov >= 1) & v.notna()
    pairs, ov, v = pairs[keep], ov[keep].astype(np.int64), v[keep]
    integer = pd.api.types.is_integer_dtype(df2[name].dtype)
    v = v.astype(np.int64 if integer else np.float64)
    g = pd.DataFrame({"rid": pairs["rid_1"].to_numpy(), "ov": ov.to_numpy(), "prod": (v * ov).to_numpy(), "v": v.to_numpy()}).groupby("rid")
    out = pd.DataFrame({"size": np.maximum(df1["end"] - df1["start"] + w, 0).to_numpy()}, index=df1["rid"])
    out["bases"] = g["ov"].sum().reindex(out.index, fill_value=0)
    out["sum"] = g["prod"].sum().reindex(out.index, fill_value=0)
    out["min"], out["max"] = g["v"].min().reindex(out.index), g["v"].max().reindex(out.index)
    out["mean0"] = np.where(out["size"] > 0, out["sum"] / out["size"].where(out["size"] > 0, 1), np.nan)
    out["mean"] = np.where(out["bases"] > 0, out["sum"] / out["bases"].where(out["bases"] > 0, 1), np.nan)
    return out, int(keep.sum()), len(keep)


def _same(got, want, what):
    g, w = np.asarray(got.astype("float64")), np.asarray(want.astype("float64"))
    assert (np.isnan(g) == np.isnan(w)).all(), f"{what}: nulls differ"
    assert (g[~np.isnan(g)] == w[~np.isnan(w)]).all(), f"{what}: values differ"


def _check_summary(res, ref, suffix=""):
    for stat in STATS:
        _same(res[stat + suffix], ref[stat].reset_index(drop=True), stat + suffix)


@pytest.mark.parametrize("zero_based", ZB)
def test_summary_against_overlap_and_a_pandas_group_by(zero_based):
    df1, df2 = _frame(zero_based, 1, 700, 400), _frame(zero_based, 2, 3000, 60, values=True, nulls=True)
    res = pb.signal_summary(df1, df2, "score", **PD)
    assert list(res.columns) == list(df1.columns) + STATS and len(res) == len(df1) and (res["rid"] == df1["rid"]).all()
    assert res["size"].dtype == np.int64 and res["bases"].dtype == np.int64 and res["sum"].dtype == np.float64
    ref, kept, seen = _reference(df1, df2, zero_based, "score")
    assert 2000 < kept < seen, "no pair of the plain predicate shares nothing or holds a null"
    _check_summary(res, ref)
    assert res["mean"].isna().any() and res["mean0"].isna().any() and (res["bases"] > res["size"]).any()


def test_summary_value_list_integer_and_narrow_columns():
    df1, df2 = _frame(True, 3, 500, 300), _frame(True, 4, 2000, 50, values=True, nulls=True)
    names = ["hits", "f32", "u32", "score"]
    res = pb.signal_summary(df1, df2, names, **PD)
    assert list(res.columns) == list(df1.columns) + [f"{s}_{n}" for n in names for s in STATS]
    assert res["sum_hits"].dtype == np.int64 and res["sum_u32"].dtype == np.int64 and res["sum_f32"].dtype == np.float64
    t = pb.signal_summary(df1, df2, names, output_type="pyarrow.Table")
    assert t.schema.field("min_hits").type == pa.int32() and t.schema.field("max_u32").type == pa.uint32()
    assert t.schema.field("min_f32").type == pa.float32() and t.schema.field("mean_hits").type == pa.float64()
    for name in names:
        ref, kept, _ = _reference(df1, df2, True, name)
        assert kept > 1000
        _check_summary(res, ref, f"_{name}")


@pytest.mark.parametrize("zero_based", ZB)
def test_summary_on_cols_thresholds_and_limit(zero_based):
    df1, df2 = _frame(zero_based, 5, 600, 300), _frame(zero_based, 6, 2500, 80, values=True)
    plain, kept_plain, _ = _reference(df1, df2, zero_based, "score")
    for kw in (dict(on_cols=["strand"]), dict(min_overlap=20), dict(min_frac2=0.5, min_frac1=0.05), dict(on_cols=["strand"], min_overlap=10)):
        ref, kept, _ = _reference(df1, df2, zero_based, "score", **kw)
        assert 200 < kept < kept_plain, f"{kw} removed nothing, or everything"
        _check_summary(pb.signal_summary(df1, df2, "score", **PD, **kw), ref)
    head = pb.signal_summary(df1, df2, "score", limit=17, **PD)
    assert len(head) == 17
    _check_summary(head, plain.iloc[:17])


def test_summary_outputs_and_the_accessor(monkeypatch):
    df1, df2 = _frame(True, 7, 300, 300), _frame(True, 8, 1000, 50, values=True)
    want = pb.signal_summary(df1, df2, "score", **PD)
    assert want["bases"].sum() > 1000
    t = pb.signal_summary(df1, df2, "score", output_type="pyarrow.Table")
    assert t.column_names == list(want.columns) and t.column("sum").to_pylist() == want["sum"].tolist()
    assert df1.pb.signal_summary(df2, value="score").equals(want)
    pl = _fake_polars.install(monkeypatch)
    for kind, cls in (("polars.DataFrame", pl.DataFrame), ("polars.LazyFrame", pl.LazyFrame)):
        res = pb.signal_summary(df1, df2, "score", output_type=kind)
        assert isinstance(res, cls)
        res = res.collect() if kind.endswith("LazyFrame") else res
        assert res.to_arrow().column("bases").to_pylist() == want["bases"].tolist()


# ---- signal_profile -----------------------------------------------------------------------------------------------------------------

def _bin_frame(df1, zero_based, n_bins, w_start, w_end, reverse):
    """The explicit bin frame with numpy, row-major in output order; an empty bin is a row that covers no position."""
    w = 0 if zero_based else 1
    lens = range_op.profile_bin_lengths(w_start, w_end, zero_based, n_bins)
    edges = np.asarray(w_start, np.int64)[:, None] + np.concatenate([np.zeros((len(df1), 1), np.int64), np.cumsum(lens, axis=1)], axis=1)
    s, e = edges[:, :-1].copy(), edges[:, 1:] - w
    s[lens <= 0], e[lens <= 0] = 0, -w
    if reverse is not None:
        s[reverse], e[reverse] = s[reverse, ::-1], e[reverse, ::-1]
    bins = pd.DataFrame({"chrom": np.repeat(df1["chrom"].to_numpy(), n_bins), "start": s.reshape(-1), "end": e.reshape(-1),
                         "strand": np.repeat(df1["strand"].to_numpy(), n_bins)})
    bins.attrs["coordinate_system_zero_based"] = zero_based
    return bins


def _matrix(col):
    return np.array([np.array([np.nan if v is None else v for v in row], np.float64) for row in col])


@pytest.mark.parametrize("zero_based", ZB)
@pytest.mark.parametrize("mode", ["scale", "anchored"])
def test_profile_is_the_summary_of_the_bin_frame(zero_based, mode):
    df1, df2 = _frame(zero_based, 11, 150, 500), _frame(zero_based, 12, 3000, 40, values=True, nulls=True)
    n_bins = 13
    if mode == "scale":
        kw, minus = {}, None
        w_start, w_end = df1["start"].to_numpy(), df1["end"].to_numpy()
    else:
        kw, minus = dict(anchor="start", upstream=70, downstream=120, direction_col="strand"), (df1["strand"] == "-").to_numpy()
        w_start, w_end = range_op.profile_windows(df1["start"], df1["end"], zero_based, "start", 70, 120, minus)
    bins = _bin_frame(df1, zero_based, n_bins, w_start, w_end, minus)
    for name in ("score", "hits"):
        flat = pb.signal_summary(bins, df2, name, **PD)
        assert (flat["bases"] > 0).sum() > 300 and (flat["bases"] == 0).sum() > 50
        for output in ("mean", "mean0", "sum", "bases", "min", "max"):
            res = pb.signal_profile(df1, df2, name, n_bins=n_bins, output=output, **PD, **kw)
            assert list(res.columns) == list(df1.columns) + ["profile"] and (res["rid"] == df1["rid"]).all()
            want = flat[output].astype("float64").to_numpy().reshape(len(df1), n_bins)
            got = _matrix(res["profile"])
            assert (np.isnan(got) == np.isnan(want)).all() and (got[~np.isnan(got)] == want[~np.isnan(want)]).all(), (name, output)
            m = pb.signal_profile(df1, df2, name, n_bins=n_bins, output=output, output_type="numpy.ndarray", **kw)
            assert m.shape == (len(df1), n_bins) and m.dtype == (np.int64 if output == "bases" or (output == "sum" and name == "hits") else np.float64)
            assert (np.isnan(m.astype(np.float64)) == np.isnan(want)).all() and (m[~np.isnan(want)] == want[~np.isnan(want)]).all()
    t = pb.signal_profile(df1, df2, "hits", n_bins=n_bins, output="max", output_type="pyarrow.Table", **kw)
    assert t.schema.field("profile").type == pa.list_(pa.int32(), n_bins)
    via_accessor = _matrix(df1.pb.signal_profile(df2, value="score", n_bins=n_bins, **kw)["profile"])
    assert np.array_equal(via_accessor, _matrix(pb.signal_profile(df1, df2, "score", n_bins=n_bins, **PD, **kw)["profile"]), equal_nan=True)


@pytest.mark.parametrize("zero_based", ZB)
def test_a_constant_on_disjoint_rows_gives_the_constant_and_scales_depth_profile(zero_based):
    c = 4.0                                                          # a power of two: c * (bases / length) == (c * bases) / length exactly
    df1 = _frame(zero_based, 21, 200, 600)
    w = 0 if zero_based else 1
    s = np.arange(0, 3600, 12, dtype=np.int64)                       # disjoint rows of 7 positions every 12
    df2 = pd.DataFrame({"chrom": np.repeat(NAMES, len(s)).astype(object), "start": np.tile(s, len(NAMES)), "end": np.tile(s + 7 - w, len(NAMES))})
    df2["score"] = c
    df2.attrs["coordinate_system_zero_based"] = zero_based
    kw = dict(n_bins=20, output_type="numpy.ndarray")
    bases = pb.signal_profile(df1, df2, "score", output="bases", **kw)
    mean, mean0 = pb.signal_profile(df1, df2, "score", output="mean", **kw), pb.signal_profile(df1, df2, "score", output="mean0", **kw)
    depth = pb.depth_profile(df1, df2, output="mean", **kw)
    depth_bases = pb.depth_profile(df1, df2, output="bases", **kw)
    assert (depth_bases > 0).sum() > 1000 and (depth_bases == 0).sum() > 100
    assert (bases == depth_bases).all()
    assert (np.isnan(mean) == (depth_bases == 0)).all() and (mean[depth_bases > 0] == c).all()
    assert (np.isnan(mean0) == np.isnan(depth)).all() and (mean0[~np.isnan(depth)] == c * depth[~np.isnan(depth)]).all()
