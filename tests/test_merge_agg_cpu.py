"""pb.merge(agg=...) without a GPU: the yardstick of tests/_merge_agg_util.py on hand-written cases whose answers are written
out here, the front door's validation, naming and typing against a stand-in engine that answers with the yardstick, and the
ABI symbol list."""
import math

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
from polars_bio_amd import _engine, range_op
import _merge_agg_util as M

I64, F64 = np.int64, np.float64


def _side(rows):
    c, s, e = zip(*rows)
    return np.array(c, np.int32), np.array(s, np.int32), np.array(e, np.int32)


# ---- the yardstick on cases answered by hand ---------------------------------------------------------------------------------

def test_yardstick_bookended_rows_and_min_dist():
    #             row 0        1          2          3          4
    side = _side([(0, 10, 20), (0, 20, 30), (0, 25, 40), (0, 41, 50), (1, 0, 5)])
    v = np.array([1, 2, 4, 8, 16], I64)
    # Strict, min_dist 0: [10,20) and [20,30) only touch -> {0}, {1,2}, {3}, {4}
    cid, table = M.clusters(side, 2, True, 0)
    assert cid.tolist() == [0, 1, 1, 2, 3] and table[1].tolist() == [10, 20, 41, 0] and table[3].tolist() == [1, 2, 1, 1]
    g = M.group_by(cid, 4, v)
    assert g["sum"] == [1, 6, 8, 16] and g["min"] == [1, 2, 8, 16] and g["max"] == [1, 4, 8, 16] and g["count"] == [1, 2, 1, 1]
    assert g["mean"] == [1.0, 3.0, 8.0, 16.0]
    # Strict, min_dist 1: the bookended pair merges, 41 < 40 + 1 does not hold -> {0,1,2}, {3}, {4}
    cid, table = M.clusters(side, 2, True, 1)
    assert cid.tolist() == [0, 0, 0, 1, 2]
    assert M.group_by(cid, 3, v)["sum"] == [7, 8, 16]
    # Weak (closed ends), min_dist 0: 20 <= 20 merges, 41 <= 40 does not; min_dist 1: 41 <= 41 merges
    assert M.clusters(side, 2, False, 0)[0].tolist() == [0, 0, 0, 1, 2]
    cid, _ = M.clusters(side, 2, False, 1)
    assert cid.tolist() == [0, 0, 0, 0, 1]
    g = M.group_by(cid, 2, v)
    assert g["sum"] == [15, 16] and g["mean"] == [3.75, 16.0]


def test_yardstick_nulls_and_an_all_null_cluster():
    side = _side([(0, 0, 10), (0, 5, 15), (0, 100, 110), (0, 105, 120), (0, 300, 310)])
    v = np.array([5.0, -2.0, 7.0, 9.0, 1.0], F64)
    valid = np.array([1, 0, 0, 0, 1], np.uint8)
    cid, _ = M.clusters(side, 1, True, 0)
    assert cid.tolist() == [0, 0, 1, 1, 2]
    g = M.group_by(cid, 3, v, valid)
    assert g["count"] == [1, 0, 1] and g["sum"] == [5.0, 0.0, 1.0]
    assert g["min"] == [5.0, None, 1.0] and g["max"] == [5.0, None, 1.0] and g["mean"] == [5.0, None, 1.0]


def test_yardstick_int64_wraps_and_nan_rules():
    cid = np.array([0, 0, 0, 1, 1, 2])
    big = np.array([2 ** 62, 2 ** 62, 2 ** 62, -5, 3, 0], I64)
    g = M.group_by(cid, 3, big)
    assert int(g["sum"][0]) == 3 * 2 ** 62 - 2 ** 64 and g["sum"][1] == -2 and g["min"][1] == -5 and g["max"][1] == 3
    assert g["mean"][0] == float(3 * 2 ** 62 - 2 ** 64) / 3.0
    x = np.array([1.0, np.nan, 3.0, np.nan, np.nan, 2.0], F64)
    g = M.group_by(cid, 3, x)
    assert g["min"][0] == 1.0 and g["max"][0] == 3.0 and math.isnan(g["sum"][0]) and math.isnan(g["mean"][0])
    assert math.isnan(g["min"][1]) and math.isnan(g["max"][1]) and g["count"][1] == 2
    assert g["sum"][2] == 2.0


def test_yardstick_pseudo_contig_comes_last():
    side = _side([(7, 0, 10), (1, 0, 10), (-3, 5, 15), (0, 0, 10)])       # contigs 7 and -3 are outside a dictionary of 2
    cid, table = M.clusters(side, 2, True, 0)
    assert table[0].tolist() == [0, 1, -1] and cid.tolist() == [2, 1, 2, 0] and table[3].tolist() == [1, 1, 2]


def test_kernel_tile_reads_the_header():
    t = M.kernel_tile()
    assert t >= 64 and t % 64 == 0


# ---- the ABI -----------------------------------------------------------------------------------------------------------------

def test_abi_symbols_and_constants():
    for s in ("ivj_merge_agg", "ivj_merge_agg_free", "ivj_merge_agg_dev"):
        assert s in _engine.ABI_SYMBOLS
    L = _engine.load_library()
    assert all(hasattr(L, s) for s in ("ivj_merge_agg", "ivj_merge_agg_free", "ivj_merge_agg_dev"))
    hdr = open(f"{M.ROOT}/include/ivjoin.h").read()
    for name, value in (("IVJ_AGG_SUM", _engine.AGG_SUM), ("IVJ_AGG_MIN", _engine.AGG_MIN), ("IVJ_AGG_MAX", _engine.AGG_MAX),
                        ("IVJ_AGG_MEAN", _engine.AGG_MEAN), ("IVJ_AGG_COUNT", _engine.AGG_COUNT), ("IVJ_AGG_I64", _engine.AGG_I64),
                        ("IVJ_AGG_F64", _engine.AGG_F64), ("IVJ_MAX_AGG_COLS", _engine.MAX_AGG_COLS), ("IVJ_ABI_VERSION", 6)):
        assert f"#define {name} {value}" in hdr.replace("u\n", "\n"), name
    assert _engine.agg_ops_mask(["sum", "count"]) == 17 and _engine.agg_ops_mask("mean") == 8 and _engine.agg_ops_mask(31) == 31
    for bad in ([], ["median"], [3]):
        with pytest.raises(ValueError):
            _engine.agg_ops_mask(bad)


# ---- the front door against a stand-in engine --------------------------------------------------------------------------------

class YardstickEngine:
    """Answers merge / merge_agg with the yardstick; records what the front door handed it."""
    calls = []

    def merge(self, frame, strict, n_contigs, min_dist=0):
        return M.clusters(frame, n_contigs, strict, min_dist)[1]

    def merge_agg(self, frame, strict, n_contigs, agg, min_dist=0):
        cid, table = M.clusters(frame, n_contigs, strict, min_dist)
        results = []
        for values, valid, ops in agg:
            assert values.dtype in (I64, F64) and values.shape == frame[0].shape and (valid is None or valid.shape == values.shape)
            YardstickEngine.calls.append((values.copy(), None if valid is None else valid.copy(), list(ops)))
            g = M.group_by(cid, len(table[0]), values, valid)
            kinds = {"sum": values.dtype, "min": values.dtype, "max": values.dtype, "mean": F64, "count": I64}
            results.append({op: np.array([0 if x is None else x for x in g[op]], kinds[op]) for op in ops})
        return (*table, results)


@pytest.fixture
def stand_in(monkeypatch):
    YardstickEngine.calls = []
    monkeypatch.setattr(range_op, "default_engine", lambda: YardstickEngine())


def _frame(zero_based=True):
    df = pd.DataFrame({
        "chrom": ["chr1", "chr1", "chr1", "chr2", "chr2", None, "chr1"],
        "start": [10, 15, 100, 5, 6, 1, 200],
        "end": [20, 30, 110, 9, 8, 2, 210],
        "strand": ["+", "+", "-", "+", "+", "+", "-"],
        "score": np.array([3, 4, 5, 6, 7, 1000, -8], np.int16),
        "qual": np.array([0.5, 1.5, np.nan, 2.0, 4.0, 9.0, np.nan], np.float32),
    })
    df.attrs["coordinate_system_zero_based"] = zero_based
    return df


def test_front_door_names_types_and_nulls(stand_in):
    df = _frame()
    base = pb.merge(df, output_type="pandas.DataFrame")
    res = pb.merge(df, output_type="pandas.DataFrame", agg={"score": ["sum", "max", "min", "count"], "qual": ["mean", "min", "sum", "count"]})
    assert list(res.columns) == ["chrom", "start", "end", "n_intervals", "score_sum", "score_max", "score_min", "score_count",
                                 "qual_mean", "qual_min", "qual_sum", "qual_count"]
    pd.testing.assert_frame_equal(res[list(base.columns)], base)
    # clusters: chr1 [10,30) rows 0,1; chr1 [100,110) row 2; chr1 [200,210) row 6; chr2 [5,9) rows 3,4; the null-chrom row is gone
    assert res["n_intervals"].tolist() == [2, 1, 1, 2]
    assert res["score_sum"].tolist() == [7, 5, -8, 13] and res["score_max"].tolist() == [4, 5, -8, 7] and res["score_count"].tolist() == [2, 1, 1, 2]
    assert res["qual_count"].tolist() == [2, 0, 0, 2] and res["qual_sum"].tolist() == [2.0, 0.0, 0.0, 6.0]
    assert res["qual_mean"].isna().tolist() == [False, True, True, False] and res["qual_mean"][0] == 1.0 and res["qual_mean"][3] == 3.0
    assert res["qual_min"].isna().tolist() == [False, True, True, False] and res["qual_min"][0] == 0.5
    t = pb.merge(df, output_type="pyarrow.Table", agg={"score": ["sum", "max", "min", "mean", "count"], "qual": ["min", "max", "sum"]})
    types = {f.name: f.type for f in t.schema}
    assert types["score_sum"] == pa.int64() and types["score_max"] == pa.int16() and types["score_min"] == pa.int16()
    assert types["score_mean"] == pa.float64() and types["score_count"] == pa.int64()
    assert types["qual_min"] == pa.float32() and types["qual_max"] == pa.float32() and types["qual_sum"] == pa.float64()
    assert t.column("qual_min").null_count == 2 and t.column("qual_sum").null_count == 0
    # what reached the engine: int64 / float64 values without the dropped row, nulls as validity, count always along
    values, valid, ops = YardstickEngine.calls[-2]
    assert values.dtype == I64 and values.tolist() == [3, 4, 5, 6, 7, -8] and valid is None and ops[-1] == "count"
    values, valid, ops = YardstickEngine.calls[-1]
    assert values.dtype == F64 and valid.astype(bool).tolist() == [True, True, False, True, True, False]


def test_front_door_on_cols_min_dist_and_coordinate_systems(stand_in):
    df = _frame()
    res = pb.merge(df, on_cols=["strand"], output_type="pandas.DataFrame", agg={"score": "sum"})
    assert list(res.columns) == ["chrom", "start", "end", "strand", "n_intervals", "score_sum"]
    assert res[["chrom", "strand", "score_sum"]].values.tolist() == [["chr1", "+", 7], ["chr1", "-", 5], ["chr1", "-", -8], ["chr2", "+", 13]]
    res = pb.merge(df, min_dist=100, output_type="pandas.DataFrame", agg={"score": ["sum", "count"]})
    assert res["score_sum"].tolist() == [4, 13] and res["score_count"].tolist() == [4, 2]
    one = _frame(zero_based=False)
    one.loc[1, "start"] = 20                       # [10,20] and [20,30] share position 20 when closed, only touch when half-open
    assert pb.merge(one, output_type="pandas.DataFrame", agg={"score": "sum"})["score_sum"].tolist() == [7, 5, -8, 13]
    zero = one.copy()
    zero.attrs["coordinate_system_zero_based"] = True
    assert pb.merge(zero, output_type="pandas.DataFrame", agg={"score": "sum"})["score_sum"].tolist() == [3, 4, 5, -8, 13]
    assert df.pb.merge(agg={"score": "max"})["score_max"].tolist() == [4, 5, -8, 7]          # the namespace hands agg on
    assert list(pb.merge(df, output_type="pandas.DataFrame").columns) == ["chrom", "start", "end", "n_intervals"]


def test_front_door_refuses_what_it_cannot_aggregate(stand_in):
    df = _frame()
    df["u64"] = np.arange(len(df), dtype=np.uint64)
    df["flag"] = [True, False] * 3 + [True]
    df["name"] = list("abcdefg")
    df["u32"] = np.arange(len(df), dtype=np.uint32)
    t = pa.Table.from_pandas(df, preserve_index=False)
    t = t.append_column("dec", pa.array([1] * len(df), type=pa.decimal128(10, 2)))
    t = t.replace_schema_metadata({b"coordinate_system_zero_based": b"true"})
    merge = lambda agg, frame=df, **kw: pb.merge(frame, output_type="pandas.DataFrame", agg=agg, **kw)
    for col in ("u64", "flag", "name"):
        with pytest.raises(ValueError, match=col):
            merge({col: "sum"})
    with pytest.raises(ValueError, match="dec"):
        merge({"dec": "sum"}, frame=t)
    with pytest.raises(ValueError, match="nope"):
        merge({"nope": "sum"})
    with pytest.raises(ValueError, match="start"):
        merge({"start": "max"})
    with pytest.raises(ValueError, match="strand"):
        merge({"strand": "count"}, on_cols=["strand"])
    with pytest.raises(ValueError, match="median"):
        merge({"score": ["sum", "median"]})
    with pytest.raises(ValueError, match="score"):
        merge({"score": []})
    with pytest.raises(ValueError, match="score"):
        merge({"score": ["sum", "sum"]})                     # score_sum twice
    clash = df.assign(score_sum=df["strand"])              # an on_cols column that is also the name of an aggregate's output
    with pytest.raises(ValueError, match="score_sum"):
        merge({"score": "sum"}, frame=clash, on_cols=["score_sum"])
    many = df.copy()
    for k in range(_engine.MAX_AGG_COLS + 1):
        many[f"v{k}"] = k
    with pytest.raises(ValueError, match=str(_engine.MAX_AGG_COLS)):
        merge({f"v{k}": "sum" for k in range(_engine.MAX_AGG_COLS + 1)}, frame=many)
    with pytest.raises(ValueError):
        merge({})
    with pytest.raises(ValueError):
        merge(["score"])
    with pytest.raises(TypeError):
        pb.merge(df, 0, ["chrom", "start", "end"], None, "pandas.DataFrame", True, {"score": "sum"})      # agg is keyword-only
    assert merge({"u32": ["sum", "max"]})["u32_max"].dtype == np.uint32
