"""pb.set_intersect / set_union / set_difference / set_symmetric_difference and pb.jaccard, the front door: input kinds, output
schema and order, null chroms, on_cols, both coordinate systems, feeding a result back in, the .pb accessor."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
import _setop_util as U

pytestmark = pytest.mark.gpu

NAMES = np.array(["chr10", "chr2", "chrX", "chr1"])
FUNCS = {"intersection": "set_intersect", "union": "set_union", "difference": "set_difference",
         "symmetric_difference": "set_symmetric_difference"}


def _frame(zero_based, seed, n=3000, nulls=False, strand=False, names=NAMES):
    rng = np.random.default_rng(seed)
    c, s, e = U.random_rows(rng, n, len(names), 4000, max_len=40)
    d = {"chrom": names[c].astype(object), "start": s.astype(np.int64), "end": e.astype(np.int64)}
    if strand:
        d["strand"] = np.array(["+", "-"])[rng.integers(0, 2, n)]
    if nulls:
        d["chrom"][rng.integers(0, n, n // 10)] = None
    df = pd.DataFrame(d)
    df.attrs["coordinate_system_zero_based"] = zero_based
    return df


def _sides(df1, df2, cols1=("chrom", "start", "end"), cols2=("chrom", "start", "end")):
    """chrom ids in sorted-name order over both frames, as the front door numbers them"""
    d1, d2 = df1[df1[cols1[0]].notna()], df2[df2[cols2[0]].notna()]
    names = np.array(sorted(set(d1[cols1[0]]) | set(d2[cols2[0]])))
    ids = lambda d, c: np.searchsorted(names, d[c[0]].to_numpy().astype(str)) if len(d) else np.empty(0, np.int64)
    a = U.as_i32(ids(d1, cols1), d1[cols1[1]].to_numpy(), d1[cols1[2]].to_numpy())
    b = U.as_i32(ids(d2, cols2), d2[cols2[1]].to_numpy(), d2[cols2[2]].to_numpy())
    return a, b, names


def _expected_frame(df1, df2, op, zero_based, cols=("chrom", "start", "end"), cols2=("chrom", "start", "end")):
    a, b, names = _sides(df1, df2, cols, cols2)
    (c, s, e), _ = U.setop_events(a, b, zero_based, max(len(names), 1), op)
    return pd.DataFrame({cols[0]: names[c].astype(object) if len(names) else np.empty(0, object), cols[1]: s, cols[2]: e})


def _same(res, exp, str_cols=("chrom",)):
    cast = {c: object for c in str_cols}
    pd.testing.assert_frame_equal(res.reset_index(drop=True).astype(cast), exp.reset_index(drop=True).astype(cast), check_dtype=False)


def test_functions_are_exported():
    for name in list(FUNCS.values()) + ["jaccard"]:
        assert name in pb.__all__ and callable(getattr(pb, name))


@pytest.mark.parametrize("zero_based", [True, False])
@pytest.mark.parametrize("op", list(FUNCS))
def test_pandas_frames_schema_order_and_values(op, zero_based):
    df1, df2 = _frame(zero_based, 11), _frame(zero_based, 12, names=NAMES[:3])
    res = getattr(pb, FUNCS[op])(df1, df2, output_type="pandas.DataFrame")
    assert list(res.columns) == ["chrom", "start", "end"]
    assert [str(t) for t in res.dtypes[1:]] == ["int64"] * 2
    assert res.attrs["coordinate_system_zero_based"] == zero_based
    _same(res, _expected_frame(df1, df2, op, zero_based))
    key = list(zip(res["chrom"], res["start"]))
    assert key == sorted(key) and len(key) > 0


def test_a_one_based_frame_gives_closed_bounds():
    mk = lambda rows: pd.DataFrame(rows, columns=["chrom", "start", "end"])
    a, b = mk([("chr1", 1, 5), ("chr1", 20, 29)]), mk([("chr1", 6, 9), ("chr1", 24, 26)])
    for d in (a, b):
        d.attrs["coordinate_system_zero_based"] = False
    _same(pb.set_union(a, b, output_type="pandas.DataFrame"), mk([("chr1", 1, 9), ("chr1", 20, 29)]))
    _same(pb.set_difference(a, b, output_type="pandas.DataFrame"), mk([("chr1", 1, 5), ("chr1", 20, 23), ("chr1", 27, 29)]))
    _same(pb.set_intersect(a, b, output_type="pandas.DataFrame"), mk([("chr1", 24, 26)]))
    a0, b0 = mk([("chr1", 0, 5)]), mk([("chr1", 5, 9)])
    for d in (a0, b0):
        d.attrs["coordinate_system_zero_based"] = True
    _same(pb.set_union(a0, b0, output_type="pandas.DataFrame"), mk([("chr1", 0, 9)]))
    _same(pb.set_symmetric_difference(a0, b0, output_type="pandas.DataFrame"), mk([("chr1", 0, 9)]))
    assert len(pb.set_intersect(a0, b0, output_type="pandas.DataFrame")) == 0


def test_pyarrow_tables_and_column_names_from_cols1():
    df1 = _frame(True, 13).rename(columns={"chrom": "contig", "start": "pos_start", "end": "pos_end"})
    df2 = _frame(True, 14).rename(columns={"chrom": "seq", "start": "lo", "end": "hi"})
    meta = {"coordinate_system_zero_based": "true"}
    t1 = pa.Table.from_pandas(df1, preserve_index=False).replace_schema_metadata(meta)
    t2 = pa.Table.from_pandas(df2, preserve_index=False).replace_schema_metadata(meta)
    cols1, cols2 = ["contig", "pos_start", "pos_end"], ["seq", "lo", "hi"]
    res = pb.set_difference(t1, t2, cols1=cols1, cols2=cols2, output_type="pandas.DataFrame")
    assert list(res.columns) == cols1
    _same(res, _expected_frame(df1, df2, "difference", True, cols1, cols2), str_cols=("contig",))


def test_rows_with_a_null_chrom_are_dropped():
    df1, df2 = _frame(True, 15, nulls=True), _frame(True, 16, nulls=True)
    assert df1["chrom"].isna().any() and df2["chrom"].isna().any()
    for op, fn in FUNCS.items():
        _same(getattr(pb, fn)(df1, df2, output_type="pandas.DataFrame"), _expected_frame(df1, df2, op, True))


def test_mismatching_coordinate_systems_raise():
    df1, df2 = _frame(True, 17, n=50), _frame(False, 18, n=50)
    for fn in list(FUNCS.values()) + ["jaccard"]:
        with pytest.raises(pb.CoordinateSystemMismatchError):
            getattr(pb, fn)(df1, df2, output_type="pandas.DataFrame")


@pytest.mark.parametrize("zero_based", [True, False])
@pytest.mark.parametrize("op", list(FUNCS))
def test_on_cols_equals_every_strand_on_its_own(op, zero_based):
    df1, df2 = _frame(zero_based, 19, strand=True), _frame(zero_based, 20, strand=True)
    df2 = df2[(df2["strand"] == "+") | (df2["chrom"] != "chr2")]          # a (chrom, strand) group that only df1 has
    df2.attrs["coordinate_system_zero_based"] = zero_based
    fn = getattr(pb, FUNCS[op])
    res = fn(df1, df2, on_cols=["strand"], output_type="pandas.DataFrame")
    assert list(res.columns) == ["chrom", "start", "end", "strand"]
    parts, totals = [], np.zeros(4, np.int64)
    for strand in ("+", "-"):
        subs = []
        for df in (df1, df2):
            sub = df[df["strand"] == strand].drop(columns=["strand"])
            sub.attrs["coordinate_system_zero_based"] = zero_based
            subs.append(sub)
        one = fn(*subs, output_type="pandas.DataFrame")
        _same(one, _expected_frame(subs[0], subs[1], op, zero_based))
        one.insert(3, "strand", strand)
        parts.append(one)
        j = pb.jaccard(*subs, output_type="pandas.DataFrame")
        totals += j[["intersection", "union", "n_intersections"]].to_numpy()[0].tolist() + [0]
    exp = pd.concat(parts).sort_values(["chrom", "strand", "start"], kind="stable")
    _same(res, exp, str_cols=("chrom", "strand"))
    j = pb.jaccard(df1, df2, on_cols=["strand"], output_type="pandas.DataFrame")
    assert (int(j["intersection"][0]), int(j["union"][0]), int(j["n_intersections"][0])) == tuple(int(x) for x in totals[:3])


def test_a_union_feeds_back_into_an_intersection():
    df1, df2, df3 = _frame(True, 21), _frame(True, 22), _frame(True, 23)
    u = pb.set_union(df1, df2, output_type="pandas.DataFrame")
    assert u.attrs["coordinate_system_zero_based"] is True
    res = pb.set_intersect(u, df3, output_type="pandas.DataFrame")
    both = pd.concat([df1, df2])
    _same(res, _expected_frame(both, df3, "intersection", True))


@pytest.mark.parametrize("zero_based", [True, False])
def test_jaccard_columns(zero_based):
    df1, df2 = _frame(zero_based, 24), _frame(zero_based, 25, nulls=True)
    res = pb.jaccard(df1, df2, output_type="pandas.DataFrame")
    assert list(res.columns) == ["intersection", "union", "jaccard", "n_intersections"] and len(res) == 1
    assert [str(t) for t in res.dtypes] == ["int64", "int64", "float64", "int64"]
    a, b, names = _sides(df1, df2)
    regions, (only_a, only_b, both) = U.setop_events(a, b, zero_based, len(names), "intersection")
    assert int(res["intersection"][0]) == both and int(res["union"][0]) == only_a + only_b + both
    assert int(res["n_intersections"][0]) == len(regions[0])
    assert res["jaccard"][0] == both / (only_a + only_b + both)


def test_jaccard_of_two_empty_frames_is_null():
    empty = pd.DataFrame({"chrom": pd.Series([], dtype=object), "start": pd.Series([], dtype=np.int64), "end": pd.Series([], dtype=np.int64)})
    empty.attrs["coordinate_system_zero_based"] = True
    res = pb.jaccard(empty, empty.copy(), output_type="pandas.DataFrame")
    assert int(res["intersection"][0]) == 0 and int(res["union"][0]) == 0 and int(res["n_intersections"][0]) == 0
    assert pd.isna(res["jaccard"][0])
    assert len(pb.set_union(empty, empty.copy(), output_type="pandas.DataFrame")) == 0


def test_pb_accessor():
    df1, df2 = _frame(True, 26, n=500), _frame(True, 27, n=500)
    res = df1.pb.set_intersect(df2)
    assert isinstance(res, pd.DataFrame) and list(res.columns) == ["chrom", "start", "end"]
    pd.testing.assert_frame_equal(res, pb.set_intersect(df1, df2, output_type="pandas.DataFrame"))
    assert list(df1.pb.jaccard(df2).columns) == ["intersection", "union", "jaccard", "n_intersections"]
