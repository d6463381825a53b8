"""pb.map_overlaps end to end on the GPU: frames in, frames out, against what a user had before -- pb.overlap, then a pandas
group-by of the df2 values over the df1 row of every pair.  Values are multiples of 1/8 of moderate size, so every sum is exact
in any order and the comparison is exact."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb

pytestmark = pytest.mark.gpu


def _frames(n1=700, n2=1500, seed=0, zero_based=True):
    rng = np.random.default_rng(seed)
    chroms = np.array(["chr1", "chr2", "chrX"])

    def intervals(n, max_len):
        s = rng.integers(0, 200_000, n)
        return chroms[rng.integers(0, 3, n)], s, s + rng.integers(1, max_len, n)

    c1, s1, e1 = intervals(n1, 900)
    c2, s2, e2 = intervals(n2, 300)
    df1 = pd.DataFrame({"chrom": c1, "start": s1, "end": e1, "strand": rng.choice(["+", "-"], n1), "gene": [f"g{i}" for i in range(n1)]})
    df2 = pd.DataFrame({"chrom": c2, "start": s2, "end": e2, "strand": rng.choice(["+", "-"], n2),
                        "score": rng.integers(-500, 500, n2).astype(np.int32), "signal": rng.integers(-4000, 4000, n2) / 8.0,
                        "f32": (rng.integers(-4000, 4000, n2) / 8.0).astype(np.float32), "u32": rng.integers(0, 2 ** 32, n2, dtype=np.uint32)})
    df1.attrs["coordinate_system_zero_based"] = zero_based
    df2.attrs["coordinate_system_zero_based"] = zero_based
    return df1, df2


def _by_hand(df1, df2, agg, **kw):
    """pb.overlap + pandas group-by on the same frames -> the expected frame."""
    a = df1.assign(_row=np.arange(len(df1)))
    a.attrs = dict(df1.attrs)
    pairs = pb.overlap(a, df2, output_type="pandas.DataFrame", suffixes=("_1", "_2"), **kw)
    out = df1.copy()
    for name, ops in agg.items():
        ops = [ops] if isinstance(ops, str) else ops
        col = pairs[["_row_1", f"{name}_2"]].dropna()
        g = col.groupby("_row_1")[f"{name}_2"]
        for op in ops:
            if op == "sum":
                r = g.sum().reindex(range(len(df1)), fill_value=0)
                r = r.astype("int64" if np.issubdtype(df2[name].dtype, np.integer) else "float64")
            elif op == "count":
                r = g.count().reindex(range(len(df1)), fill_value=0).astype("int64")
            elif op == "mean":
                r = (g.sum().astype("float64") / g.count()).reindex(range(len(df1)))
            else:
                r = getattr(g, op)().reindex(range(len(df1)))
            out[f"{name}_{op}"] = r.to_numpy()
    return out


def _same(got, exp):
    assert list(got.columns) == list(exp.columns)
    for c in exp.columns:
        g, e = got[c], exp[c]
        assert g.isna().tolist() == e.isna().tolist(), c
        pd.testing.assert_series_equal(g.dropna().astype(e.dropna().dtype), e.dropna(), check_exact=True, check_names=False, obj=c)


AGG = {"score": ["sum", "min", "max", "mean", "count"], "signal": ["mean", "sum", "max"]}


@pytest.mark.parametrize("zero_based", [True, False])
def test_pandas_against_overlap_and_group_by(zero_based):
    df1, df2 = _frames(zero_based=zero_based)
    got = pb.map_overlaps(df1, df2, AGG, output_type="pandas.DataFrame")
    exp = _by_hand(df1, df2, AGG)
    assert (exp["score_count"] > 0).sum() > 400 and (exp["score_count"] == 0).sum() > 0
    _same(got, exp)
    assert got["score_sum"].dtype == np.int64 and got["score_count"].dtype == np.int64 and got["signal_sum"].dtype == np.float64
    assert (got["score_count"].to_numpy() == pb.count_overlaps(df1, df2, output_type="pandas.DataFrame")["count"].to_numpy()).all()


def test_pyarrow_in_and_out_column_order_and_types():
    df1, df2 = _frames(seed=1)
    meta = {b"coordinate_system_zero_based": b"true"}
    t1 = pa.Table.from_pandas(df1, preserve_index=False).replace_schema_metadata(meta)
    t2 = pa.Table.from_pandas(df2, preserve_index=False).replace_schema_metadata(meta)
    t = pb.map_overlaps(t1, t2, {"f32": ["min", "max", "sum"], "u32": ["max", "sum", "count"], "score": "min"}, output_type="pyarrow.Table")
    assert t.column_names == list(df1.columns) + ["f32_min", "f32_max", "f32_sum", "u32_max", "u32_sum", "u32_count", "score_min"]
    types = {f.name: f.type for f in t.schema}
    assert types["f32_min"] == pa.float32() and types["f32_max"] == pa.float32() and types["f32_sum"] == pa.float64()
    assert types["u32_max"] == pa.uint32() and types["u32_sum"] == pa.int64() and types["u32_count"] == pa.int64() and types["score_min"] == pa.int32()
    got = t.to_pandas()
    exp = _by_hand(df1, df2, {"f32": ["min", "max", "sum"], "u32": ["max", "sum", "count"], "score": "min"})
    _same(got, exp)
    assert t.column("gene").to_pylist() == df1["gene"].tolist()


def test_nulls_in_values_and_in_chrom():
    df1, df2 = _frames(seed=2)
    df2["signal"] = df2["signal"].where(np.arange(len(df2)) % 3 != 0)           # NaN in pandas = null in Arrow
    df2.loc[::11, "chrom"] = None
    df1.loc[::13, "chrom"] = None
    got = pb.map_overlaps(df1, df2, {"signal": ["count", "sum", "min", "mean"], "score": ["count"]}, output_type="pandas.DataFrame")
    known1, known2 = df1[df1["chrom"].notna()], df2[df2["chrom"].notna()]
    known1.attrs, known2.attrs = dict(df1.attrs), dict(df2.attrs)
    exp = _by_hand(known1.reset_index(drop=True), known2.reset_index(drop=True), {"signal": ["count", "sum", "min", "mean"], "score": ["count"]})
    sub = got[df1["chrom"].notna().to_numpy()].reset_index(drop=True)
    exp.attrs = {}
    _same(sub, exp)
    null_rows = got[df1["chrom"].isna().to_numpy()]
    assert (null_rows["signal_count"] == 0).all() and (null_rows["signal_sum"] == 0).all() and null_rows["signal_min"].isna().all()
    assert (got["signal_count"] <= got["score_count"]).all() and (got["signal_count"] < got["score_count"]).any()


def test_on_cols_thresholds_limit_and_accessor():
    df1, df2 = _frames(seed=3)
    agg = {"score": ["sum", "count"], "signal": "max"}
    _same(pb.map_overlaps(df1, df2, agg, on_cols=["strand"], output_type="pandas.DataFrame"), _by_hand(df1, df2, agg, on_cols=["strand"]))
    exp = _by_hand(df1, df2, agg, min_frac1=0.5)
    got = pb.map_overlaps(df1, df2, agg, output_type="pandas.DataFrame", min_frac1=0.5)
    _same(got, exp)
    assert 0 < got["score_count"].sum() < pb.map_overlaps(df1, df2, agg, output_type="pandas.DataFrame")["score_count"].sum()
    _same(pb.map_overlaps(df1, df2, agg, output_type="pandas.DataFrame", limit=17), _by_hand(df1, df2, agg).head(17))
    _same(df1.pb.map_overlaps(df2, agg=agg, min_overlap=20), _by_hand(df1, df2, agg, min_overlap=20))
    reader = pb.map_overlaps(df1, df2, agg, output_type="pyarrow.RecordBatchReader")
    assert isinstance(reader, pa.RecordBatchReader)
    _same(reader.read_all().to_pandas(), _by_hand(df1, df2, agg))
