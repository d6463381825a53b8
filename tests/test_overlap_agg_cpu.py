"""pb.map_overlaps without a GPU: the yardstick of tests/_overlap_agg_util.py on hand-written cases whose answers are written out
here, its count against oracle.np_count_overlaps, the header <-> binding consistency of the two new entries, and the front door's
validation, naming and typing against a stand-in engine that answers with the yardstick."""
import math
import re

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
from polars_bio_amd import _engine, namespace, range_op
from oracle import oracle as O
import _overlap_agg_util as U

I64, F64 = np.int64, np.float64


def _side(rows):
    c, s, e = zip(*rows)
    return np.array(c, np.int32), np.array(s, np.int32), np.array(e, np.int32)


# ---- the yardstick on cases answered by hand ---------------------------------------------------------------------------------

def test_yardstick_plain_predicate_by_hand():
    #              row 0          1           2           3            4
    build = _side([(0, 10, 20), (0, 15, 30), (0, 20, 25), (1, 0, 100), (0, 40, 50)])
    v = np.array([1, 2, 4, 8, 16], I64)
    #              [12,18): rows 0,1   [20,22): strict 1,2; weak 0,1,2   [30,40): strict none; weak 1,4   contig 1   outside
    probe = _side([(0, 12, 18), (0, 20, 22), (0, 30, 40), (1, 5, 6), (3, 0, 100)])
    g = U.expected(probe, build, 2, True, v)
    assert g["count"] == [2, 2, 0, 1, 0] and g["sum"] == [3, 6, 0, 8, 0]
    assert g["min"] == [1, 2, None, 8, None] and g["max"] == [2, 4, None, 8, None] and g["mean"] == [1.5, 3.0, None, 8.0, None]
    g = U.expected(probe, build, 2, False, v)
    assert g["count"] == [2, 3, 2, 1, 0] and g["sum"] == [3, 7, 18, 8, 0] and g["mean"][2] == 9.0


def test_yardstick_validity_n_values_and_thresholds_by_hand():
    build = _side([(0, 0, 100), (0, 10, 20), (0, 12, 14), (0, 50, 60)])
    v = np.array([1.5, 2.0, -4.0, 8.0], F64)
    probe = _side([(0, 11, 15), (0, 55, 56), (0, 200, 300)])
    g = U.expected(probe, build, 1, True, v, valid=np.array([1, 0, 1, 1], np.uint8))
    assert g["count"] == [2, 2, 0] and g["sum"] == [-2.5, 9.5, 0.0] and g["min"][0] == -4.0 and g["max"][1] == 8.0
    g = U.expected(probe, build, 1, True, v, n_values=2)             # rows 2 and 3 carry no value
    assert g["count"] == [2, 1, 0] and g["sum"] == [3.5, 1.5, 0.0]
    # ov of probe 0 with rows 0, 1, 2 = 4, 4, 2: with min_overlap 3 row 2 goes; the 1-base probe 1 cannot reach 3 bases
    g = U.expected(probe, build, 1, True, v, min_overlap=3)
    assert g["count"] == [2, 0, 0] and g["sum"] == [3.5, 0.0, 0.0]
    g = U.expected(probe, build, 1, True, v, build_min=np.array([0, U.T.NEVER, 0, 2], np.uint32))
    assert g["count"] == [2, 1, 0] and g["sum"] == [-2.5, 1.5, 0.0]     # row 1 never, row 3 needs 2 bases of a 1-base probe


def test_yardstick_int64_wraps_and_nan_rules():
    build = _side([(0, 0, 10)] * 3 + [(0, 100, 110)] * 2)
    probe = _side([(0, 5, 6), (0, 105, 106)])
    g = U.expected(probe, build, 1, True, np.array([2 ** 62, 2 ** 62, 2 ** 62, -5, 3], I64))
    assert int(g["sum"][0]) == 3 * 2 ** 62 - 2 ** 64 and g["sum"][1] == -2 and g["min"][1] == -5 and g["max"][1] == 3
    g = U.expected(probe, build, 1, True, np.array([1.0, np.nan, 3.0, np.nan, np.nan], F64))
    assert g["min"][0] == 1.0 and g["max"][0] == 3.0 and math.isnan(g["sum"][0]) and math.isnan(g["mean"][0])
    assert math.isnan(g["min"][1]) and g["count"][1] == 2


@pytest.mark.parametrize("strict", [True, False])
def test_yardstick_count_is_count_overlaps(strict):
    rng = np.random.default_rng(3)
    n, m = 700, 500
    mk = lambda k: (rng.integers(0, 3, k).astype(np.int32), (s := rng.integers(0, 5000, k).astype(np.int32)),
                    (s + rng.integers(1, 200, k)).astype(np.int32))
    probe, build = mk(n), mk(m)
    g = U.expected(probe, build, 3, strict, np.ones(m, I64))
    want = O.np_count_overlaps(O.Side(*probe), O.Side(*build), strict)
    assert (np.array(g["count"]) == want).all() and (np.array(g["sum"]) == want).all() and want.sum() > 1000


def test_geometry_reads_the_headers():
    tile, chunk, threads, wave = U.kernel_geometry()
    assert tile % wave == 0 and chunk % threads == 0 and U.per_wave(chunk) * (threads // wave) == chunk
    assert U.per_wave(1) == wave


# ---- the ABI -----------------------------------------------------------------------------------------------------------------

def test_abi_symbols_and_header():
    names = ("ivj_overlap_agg", "ivj_overlap_agg_dev")
    L = _engine.load_library()
    hdr = open(f"{U.ROOT}/include/ivjoin.h").read()
    for s in names:
        assert s in _engine.ABI_SYMBOLS and hasattr(L, s)
        assert re.search(rf"\bint {s}\(ivj_ctx\* ctx,", hdr), s
    assert "#define IVJ_ABI_VERSION 6" in hdr and _engine.ABI_VERSION == 6 and L.ivj_abi_version() == 6
    # the argument lists the binding declares are as long as the header's
    for s in names:
        decl = hdr[hdr.index(f"int {s}("):]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        assert len(decl.split(",")) == len(getattr(L, s).argtypes), s
    assert callable(_engine.Engine.overlap_agg) and callable(_engine.Engine.overlap_agg_dev)


# ---- the front door against a stand-in engine --------------------------------------------------------------------------------

class YardstickEngine:
    """Answers overlap_agg with the yardstick; records what the front door handed it."""
    calls = []

    def overlap_agg(self, probe, build, strict, n_contigs, agg, min_overlap=0, probe_min=None, build_min=None):
        thr = {}
        if min_overlap:
            thr["min_overlap"] = min_overlap
        if probe_min is not None:
            thr["probe_min"] = probe_min
        if build_min is not None:
            thr["build_min"] = build_min
        p, b = U.pairs(probe, build, n_contigs, strict, **thr)
        results = []
        for values, valid, ops in agg:
            assert values.dtype in (I64, F64) and values.shape == build[0].shape and (valid is None or valid.shape == values.shape)
            YardstickEngine.calls.append((values.copy(), None if valid is None else valid.copy(), list(ops), dict(thr)))
            g = U.group_by(p, b, len(probe[0]), values, valid)
            kinds = {"sum": values.dtype, "min": values.dtype, "max": values.dtype, "mean": F64, "count": I64}
            results.append({op: np.array([0 if x is None else x for x in g[op]], kinds[op]) for op in ops})
        return results


@pytest.fixture
def stand_in(monkeypatch):
    YardstickEngine.calls = []
    monkeypatch.setattr(range_op, "default_engine", lambda: YardstickEngine())


def _frames(zero_based=True):
    df1 = pd.DataFrame({"chrom": ["chr1", "chr1", "chr2", None, "chr1"], "start": [0, 100, 0, 0, 1000], "end": [50, 200, 10, 50, 1100],
                        "strand": ["+", "-", "+", "+", "+"], "gene": list("abcde")})
    df2 = pd.DataFrame({"chrom": ["chr1", "chr1", "chr1", "chr2", "chr1", None], "start": [10, 40, 150, 5, 160, 0],
                        "end": [20, 120, 160, 6, 170, 100], "strand": ["+", "+", "-", "-", "+", "+"],
                        "score": np.array([3, 4, 5, 6, 7, 1000], np.int16),
                        "qual": np.array([0.5, np.nan, 2.0, 4.0, np.nan, 9.0], np.float32), "name": list("uvwxyz")})
    df1.attrs["coordinate_system_zero_based"] = zero_based
    df2.attrs["coordinate_system_zero_based"] = zero_based
    return df1, df2


def test_front_door_names_types_nulls_and_order(stand_in):
    df1, df2 = _frames()
    res = pb.map_overlaps(df1, df2, {"score": ["sum", "max", "count"], "qual": ["mean", "min", "sum", "count"]}, output_type="pandas.DataFrame")
    assert list(res.columns) == list(df1.columns) + ["score_sum", "score_max", "score_count", "qual_mean", "qual_min", "qual_sum", "qual_count"]
    assert res["gene"].tolist() == list("abcde")
    # gene a: rows 0, 1; b: rows 1, 2, 4; c: row 3; d (null chrom): nothing; e: nothing
    assert res["score_sum"].tolist() == [7, 16, 6, 0, 0] and res["score_count"].tolist() == [2, 3, 1, 0, 0]
    assert res["score_max"].isna().tolist() == [False, False, False, True, True] and res["score_max"][1] == 7
    assert res["qual_count"].tolist() == [1, 1, 1, 0, 0] and res["qual_sum"].tolist() == [0.5, 2.0, 4.0, 0.0, 0.0]
    assert res["qual_mean"].isna().tolist() == [False, False, False, True, True] and res["qual_min"][2] == 4.0
    t = pb.map_overlaps(df1, df2, {"score": ["sum", "max", "min", "mean", "count"], "qual": ["min", "max", "sum"]}, output_type="pyarrow.Table")
    types = {f.name: f.type for f in t.schema}
    assert types["score_sum"] == pa.int64() and types["score_max"] == pa.int16() and types["score_min"] == pa.int16()
    assert types["score_mean"] == pa.float64() and types["score_count"] == pa.int64()
    assert types["qual_min"] == pa.float32() and types["qual_max"] == pa.float32() and types["qual_sum"] == pa.float64()
    assert t.column("qual_min").null_count == 2 and t.column("qual_sum").null_count == 0
    # what reached the engine: every df2 row, int64 / float64 values, nulls as validity, count always along
    values, valid, ops, thr = YardstickEngine.calls[-2]
    assert values.dtype == I64 and values.tolist() == [3, 4, 5, 6, 7, 1000] and valid is None and ops[-1] == "count" and not thr
    values, valid, ops, thr = YardstickEngine.calls[-1]
    assert values.dtype == F64 and valid.astype(bool).tolist() == [True, False, True, True, False, True]


def test_front_door_on_cols_thresholds_limit_and_accessor(stand_in):
    df1, df2 = _frames()
    res = pb.map_overlaps(df1, df2, {"score": "sum"}, on_cols=["strand"], output_type="pandas.DataFrame")
    assert res["score_sum"].tolist() == [7, 5, 0, 0, 0]            # a(+): rows 0, 1; b(-): row 2 only; c(+): row 3 is "-"
    res = pb.map_overlaps(df1, df2, {"score": ["sum", "count"]}, output_type="pandas.DataFrame", min_overlap=11)
    assert res["score_sum"].tolist() == [0, 4, 0, 0, 0]            # only [40,120) x [100,200) shares 20 bases
    assert YardstickEngine.calls[-1][3] == {"min_overlap": 11}
    res = pb.map_overlaps(df1, df2, {"score": "count"}, output_type="pandas.DataFrame", min_frac2=1.0)
    assert res["score_count"].tolist() == [1, 2, 1, 0, 0]          # df2 rows wholly inside the df1 row
    assert YardstickEngine.calls[-1][3]["build_min"].tolist() == [10, 80, 10, 1, 10, 100]
    assert len(pb.map_overlaps(df1, df2, {"score": "sum"}, output_type="pandas.DataFrame", limit=2)) == 2
    reader = pb.map_overlaps(df1, df2, {"score": "sum"}, output_type="pyarrow.RecordBatchReader")
    assert reader.read_all().column("score_sum").to_pylist() == [7, 16, 6, 0, 0]
    assert df1.pb.map_overlaps(df2, agg={"score": "max"})["score_max"].tolist()[:3] == [4, 7, 6]
    assert "map_overlaps" in pb.__all__ and "map_overlaps" in range_op.__all__ and namespace._ALIASES["map_overlaps"] == (range_op.map_overlaps, True)
    one1, one2 = _frames(zero_based=False)         # closed ends: every 10-base df2 row has 11 positions, [0,50] and [40,120] share 11
    assert pb.map_overlaps(one1, one2, {"score": "sum"}, output_type="pandas.DataFrame", min_overlap=11)["score_sum"].tolist() == [7, 16, 0, 0, 0]


def test_front_door_refuses_what_it_cannot_aggregate(stand_in):
    df1, df2 = _frames()
    call = lambda agg, a=df1, b=df2, **kw: pb.map_overlaps(a, b, agg, output_type="pandas.DataFrame", **kw)
    with pytest.raises(ValueError, match="nope"):
        call({"nope": "sum"})
    with pytest.raises(ValueError, match="gene"):
        call({"gene": "sum"})                                       # a df1 column is not a df2 column
    with pytest.raises(ValueError, match="median"):
        call({"score": ["sum", "median"]})
    with pytest.raises(ValueError, match="name"):
        call({"name": "max"})                                       # a string column
    with pytest.raises(ValueError, match="start"):
        call({"start": "max"})
    with pytest.raises(ValueError, match="strand"):
        call({"strand": "count"}, on_cols=["strand"])
    with pytest.raises(ValueError, match="score_sum"):
        call({"score": "sum"}, a=df1.assign(score_sum=1))
    with pytest.raises(ValueError, match="score"):
        call({"score": []})
    for empty in ({}, None, ["score"]):
        with pytest.raises(ValueError):
            call(empty)
    for bad in (dict(min_overlap=0), dict(min_overlap=True), dict(min_frac1=0.0), dict(min_frac2=1.5), dict(min_frac1=float("nan"))):
        with pytest.raises(ValueError):
            call({"score": "sum"}, **bad)
    with pytest.raises(TypeError):
        pb.map_overlaps(df1, df2, {"score": "sum"}, None, ["chrom", "start", "end"], ["chrom", "start", "end"], "pandas.DataFrame", None, 5)
    assert not YardstickEngine.calls, "a refused call reached the engine"


def test_front_door_refuses_a_multi_device_engine(monkeypatch):
    class Many:
        pass
    monkeypatch.setattr(range_op, "default_engine", lambda: Many())
    df1, df2 = _frames()
    with pytest.raises(NotImplementedError, match="single-device"):
        pb.map_overlaps(df1, df2, {"score": "sum"}, output_type="pandas.DataFrame")
