"""pb.map_quantiles / pb.map_median without a GPU: the yardstick of tests/_map_quantiles_util.py on cases answered by hand, the
header <-> binding consistency of the two new entries, and the front door's validation, naming, typing and interpolation against a
stand-in engine that answers ``overlap_quantiles`` with the yardstick."""
import math
import re

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
from polars_bio_amd import _engine, namespace, range_op
import _map_quantiles_util as U

I64, F64 = np.int64, np.float64


def _side(rows):
    c, s, e = zip(*rows)
    return np.array(c, np.int32), np.array(s, np.int32), np.array(e, np.int32)


# ---- the yardstick by hand ------------------------------------------------------------------------------------------------------

def test_yardstick_by_hand():
    build = _side([(0, 0, 100)] * 4 + [(0, 200, 300), (1, 0, 10)])
    v = np.array([7, -3, 5, 5, 9, 1], I64)
    probe = _side([(0, 10, 20), (0, 250, 260), (0, 150, 160), (5, 0, 10)])
    out, cnt = U.expected(probe, build, 2, True, v, None, [0.0, 0.5, 0.5, 1.0], [0, 0, 1, 0])
    assert cnt.tolist() == [4, 1, 0, 0]
    assert out.tolist() == [[-3, 5, 5, 7], [9, 9, 9, 9], [0, 0, 0, 0], [0, 0, 0, 0]]       # sorted: -3 5 5 7; h = 1.5 -> ranks 1, 2
    out, cnt = U.expected(probe, build, 2, True, v, np.array([1, 0, 1, 1, 1, 1], bool), [0.5], [1])
    assert cnt.tolist() == [3, 1, 0, 0] and out[:, 0].tolist() == [5, 9, 0, 0]
    out, cnt = U.expected(probe, build, 2, True, v, None, [0.0], [0], n_values=2)
    assert cnt.tolist() == [2, 0, 0, 0] and out[0, 0] == -3
    f = np.array([np.nan, -0.0, np.inf, -np.inf, 1.0, 1.0], F64)
    out, cnt = U.expected(probe, build, 2, True, f, None, [0.0, 1 / 3, 1.0], [0, 0, 0])
    assert out[0, 0] == -np.inf and out[0, 1] == 0.0 and math.isnan(out[0, 2])              # NaN sorts last
    U.assert_same(np.array([0.0, np.nan]), np.array([-0.0, -np.nan]))
    with pytest.raises(AssertionError):
        U.assert_same(np.array([1.0]), np.array([np.nextafter(1.0, 2.0)]))


def test_tile_sizes_read_the_header():
    assert U.rows_per_workgroup(1) == 512 and U.rows_per_workgroup(16) >= 1
    assert all(U.rows_per_workgroup(k) * k * 16 * 4 <= 49152 for k in range(1, 17))


# ---- the ABI --------------------------------------------------------------------------------------------------------------------

def test_abi_symbols_and_header():
    names = ("ivj_overlap_quantiles", "ivj_overlap_quantiles_dev")
    L = _engine.load_library()
    hdr = open(f"{U.ROOT}/include/ivjoin.h").read()
    for s in names:
        assert s in _engine.ABI_SYMBOLS and hasattr(L, s)
        assert re.search(rf"\bint {s}\(ivj_ctx\* ctx,", hdr), s
        decl = hdr[hdr.index(f"int {s}("):]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        assert len(decl.split(",")) == len(getattr(L, s).argtypes), s
    assert "#define IVJ_ABI_VERSION 6" in hdr and _engine.ABI_VERSION == 6 and L.ivj_abi_version() == 6
    assert "#define IVJ_MAX_OVQ_RANKS 16" in hdr and _engine.MAX_OVQ_RANKS == 16
    assert f"#define IVJ_OVQ_BITS {_engine.OVQ_BITS}" in hdr and f"#define IVJ_OVQ_LDS_BYTES {_engine.OVQ_LDS_BYTES}" in hdr
    assert f"#define IVJ_OVQ_MAX_TILE {_engine.OVQ_MAX_TILE}" in hdr
    assert callable(_engine.Engine.overlap_quantiles) and callable(_engine.Engine.overlap_quantiles_dev)


# ---- the front door against a stand-in engine -----------------------------------------------------------------------------------

class YardstickEngine:
    """Answers overlap_quantiles with the yardstick; records what the front door handed it."""
    calls = []

    def overlap_quantiles(self, probe, build, strict, n_contigs, values, valid, q, upper, min_overlap=0, probe_min=None, build_min=None):
        thr = {}
        if min_overlap:
            thr["min_overlap"] = min_overlap
        if probe_min is not None:
            thr["probe_min"] = probe_min
        if build_min is not None:
            thr["build_min"] = build_min
        assert values.dtype in (I64, F64) and values.shape == build[0].shape and (valid is None or valid.shape == values.shape)
        assert len(q) == len(upper) and 1 <= len(q) <= 16
        YardstickEngine.calls.append((values.copy(), None if valid is None else valid.copy(), list(q), [bool(u) for u in upper], dict(thr)))
        return U.expected(probe, build, n_contigs, strict, values, valid, q, upper, **thr)


@pytest.fixture
def stand_in(monkeypatch):
    YardstickEngine.calls = []
    monkeypatch.setattr(range_op, "default_engine", lambda: YardstickEngine())


def _frames(zero_based=True):
    df1 = pd.DataFrame({"chrom": ["chr1", "chr1", "chr2", None, "chr1"], "start": [0, 100, 0, 0, 1000], "end": [50, 200, 10, 50, 1100],
                        "strand": ["+", "-", "+", "+", "+"], "gene": list("abcde")})
    df2 = pd.DataFrame({"chrom": ["chr1", "chr1", "chr1", "chr2", "chr1", None], "start": [10, 40, 150, 5, 160, 0],
                        "end": [20, 120, 160, 6, 170, 100], "strand": ["+", "+", "-", "-", "+", "+"],
                        "score": np.array([3, 4, 5, 6, 8, 1000], np.int16),
                        "qual": np.array([0.5, np.nan, 2.0, 4.0, None, 9.0], object), "name": list("uvwxyz")})
    df2["qual"] = pa.array([0.5, float("nan"), 2.0, 4.0, None, 9.0], pa.float32()).to_pandas(types_mapper=pd.ArrowDtype)
    df1.attrs["coordinate_system_zero_based"] = zero_based
    df2.attrs["coordinate_system_zero_based"] = zero_based
    return df1, df2


def test_front_door_names_types_nulls_per_method(stand_in):
    df1, df2 = _frames()
    # gene a: rows 0, 1 (3, 4); b: rows 1, 2, 4 (4, 5, 8); c: row 3 (6); d (null chrom): nothing; e: nothing
    t = pb.map_quantiles(df1, df2, "score", q=[0.5, 0, 1.0], method="lower", output_type="pyarrow.Table")
    assert t.column_names == list(df1.columns) + ["score_q0.5", "score_q0.0", "score_q1.0"]
    assert all(t.schema.field(n).type == pa.int16() for n in t.column_names[-3:])
    assert t.column("score_q0.5").to_pylist() == [3, 5, 6, None, None] and t.column("score_q1.0").to_pylist() == [4, 8, 6, None, None]
    values, valid, q, upper, thr = YardstickEngine.calls[-1]
    assert values.dtype == I64 and values.tolist() == [3, 4, 5, 6, 8, 1000] and valid is None and q == [0.5, 0.0, 1.0] and upper == [False] * 3 and not thr
    t = pb.map_quantiles(df1, df2, "score", q=0.5, method="higher", output_type="pyarrow.Table")
    assert t.column("score_q0.5").to_pylist() == [4, 5, 6, None, None] and YardstickEngine.calls[-1][3] == [True]
    t = pb.map_quantiles(df1, df2, "score", q=[0.5, 0.25], method="midpoint", output_type="pyarrow.Table")
    assert t.schema.field("score_q0.5").type == pa.float64()
    assert t.column("score_q0.5").to_pylist() == [3.5, 5.0, 6.0, None, None] and t.column("score_q0.25").to_pylist() == [3.5, 4.5, 6.0, None, None]
    values, valid, q, upper, thr = YardstickEngine.calls[-1]
    assert values.dtype == F64 and q == [0.5, 0.5, 0.25, 0.25] and upper == [False, True, False, True]
    res = pb.map_quantiles(df1, df2, "score", output_type="pandas.DataFrame")                    # the defaults: quartiles, linear
    assert list(res.columns[-3:]) == ["score_q0.25", "score_q0.5", "score_q0.75"]
    assert res["score_q0.25"].tolist()[:3] == [3.25, 4.5, 6.0] and res["score_q0.75"].tolist()[:3] == [3.75, 6.5, 6.0]
    assert res["score_q0.5"].isna().tolist() == [False, False, False, True, True] and res["gene"].tolist() == list("abcde")
    # nulls are skipped, NaN sorts last: a: 0.5, NaN; b: NaN, 2.0 (row 4 is null); c: 4.0
    t = pb.map_quantiles(df1, df2, "qual", q=[0, 1], method="lower", output_type="pyarrow.Table")
    assert t.schema.field("qual_q0.0").type == pa.float32() and t.column("qual_q0.0").to_pylist()[:3] == [0.5, 2.0, 4.0]
    hi = t.column("qual_q1.0").to_pylist()
    assert math.isnan(hi[0]) and math.isnan(hi[1]) and hi[2:] == [4.0, None, None]
    assert YardstickEngine.calls[-1][1].astype(bool).tolist() == [True, True, True, True, False, True]
    med = pb.map_median(df1, df2, "score", output_type="pyarrow.Table")
    assert med.column_names == list(df1.columns) + ["score_median"] and med.schema.field("score_median").type == pa.float64()
    assert med.column("score_median").to_pylist() == [3.5, 5.0, 6.0, None, None]


def test_front_door_on_cols_thresholds_limit_reader_ndarray_and_accessor(stand_in):
    df1, df2 = _frames()
    res = pb.map_median(df1, df2, "score", on_cols=["strand"], output_type="pandas.DataFrame")
    assert res["score_median"].tolist()[:2] == [3.5, 5.0] and res["score_median"].isna().tolist() == [False, False, True, True, True]
    res = pb.map_quantiles(df1, df2, "score", q=[0.5], method="lower", output_type="pandas.DataFrame", min_overlap=11)
    assert res["score_q0.5"].tolist()[1] == 4 and res["score_q0.5"].isna().tolist() == [True, False, True, True, True]
    assert YardstickEngine.calls[-1][4] == {"min_overlap": 11}
    pb.map_median(df1, df2, "score", output_type="pandas.DataFrame", min_frac2=1.0)
    assert YardstickEngine.calls[-1][4]["build_min"].tolist() == [10, 80, 10, 1, 10, 100]
    assert len(pb.map_quantiles(df1, df2, "score", output_type="pandas.DataFrame", limit=2)) == 2
    assert len(pb.map_median(df1, df2, "score", output_type="pandas.DataFrame", limit=3)) == 3
    reader = pb.map_median(df1, df2, "score", output_type="pyarrow.RecordBatchReader")
    assert reader.read_all().column("score_median").to_pylist() == [3.5, 5.0, 6.0, None, None]
    m = pb.map_quantiles(df1, df2, "score", q=[0.5, 1.0], method="lower", output_type="numpy.ndarray")
    assert m.dtype == F64 and m.shape == (5, 2) and m[:3].tolist() == [[3.0, 4.0], [5.0, 8.0], [6.0, 6.0]] and np.isnan(m[3:]).all()
    m = pb.map_median(df1, df2, "score", output_type="numpy.ndarray")
    assert m.shape == (5, 1) and m[:3, 0].tolist() == [3.5, 5.0, 6.0] and np.isnan(m[3:]).all()
    assert df1.pb.map_median(df2, value="score")["score_median"].tolist()[:3] == [3.5, 5.0, 6.0]
    assert df1.pb.map_quantiles(df2, value="score", q=[1.0], method="higher")["score_q1.0"].tolist()[:3] == [4, 8, 6]
    for name in ("map_quantiles", "map_median"):
        assert name in pb.__all__ and name in range_op.__all__ and namespace._ALIASES[name] == (getattr(range_op, name), True)
    one1, one2 = _frames(zero_based=False)         # closed ends: [0,50] and [40,120] share 11 positions
    assert pb.map_median(one1, one2, "score", output_type="pandas.DataFrame", min_overlap=11)["score_median"].tolist()[:2] == [3.5, 5.0]


def test_front_door_refuses(stand_in):
    df1, df2 = _frames()
    call = lambda value="score", a=df1, b=df2, **kw: pb.map_quantiles(a, b, value, output_type="pandas.DataFrame", **kw)
    with pytest.raises(ValueError, match="nope"):
        call("nope")
    with pytest.raises(ValueError, match="name"):
        call("name")                                                # a string column
    with pytest.raises(ValueError, match="start"):
        call("start")
    with pytest.raises(ValueError, match="strand"):
        call("strand", on_cols=["strand"])
    with pytest.raises(ValueError):
        call(["score", "qual"])                                     # one column per call
    for bad_q in (1.5, -0.1, float("nan"), [0.5, 0.5], [], list(np.linspace(0, 1, 9)), "half"):
        with pytest.raises(ValueError):
            call(q=bad_q)
    with pytest.raises(ValueError, match="method"):
        call(method="nearest")
    with pytest.raises(ValueError, match="score_q0.5"):
        call(a=df1.assign(**{"score_q0.5": 1}))
    with pytest.raises(ValueError, match="score_median"):
        pb.map_median(df1.assign(score_median=1), df2, "score", output_type="pandas.DataFrame")
    for bad in (dict(min_overlap=0), dict(min_frac1=0.0), dict(min_frac2=1.5)):
        with pytest.raises(ValueError):
            call(**bad)
    with pytest.raises(TypeError):
        pb.map_quantiles(df1, df2, "score", 0.5, "linear", None, ["chrom", "start", "end"], ["chrom", "start", "end"], "pandas.DataFrame", None, 5)
    assert not YardstickEngine.calls, "a refused call reached the engine"


def test_front_door_refuses_a_multi_device_engine(monkeypatch):
    class Many:
        pass
    monkeypatch.setattr(range_op, "default_engine", lambda: Many())
    df1, df2 = _frames()
    for f in (pb.map_quantiles, pb.map_median):
        with pytest.raises(NotImplementedError, match="single-device"):
            f(df1, df2, "score", output_type="pandas.DataFrame")


def _one_interval_frames(values):
    df1 = pd.DataFrame({"chrom": ["chr1"], "start": [0], "end": [100]})
    df2 = pd.DataFrame({"chrom": ["chr1"] * len(values), "start": np.arange(len(values)), "end": np.arange(len(values)) + 1, "x": values})
    df1.attrs["coordinate_system_zero_based"] = True
    df2.attrs["coordinate_system_zero_based"] = True
    return df1, df2


@pytest.mark.parametrize("method", ["lower", "higher", "midpoint", "linear"])
@pytest.mark.parametrize("m", [1, 2, 5, 10, 37])
def test_methods_are_numpy_quantile_on_finite_values(stand_in, method, m):
    rng = np.random.default_rng(m)
    # values are multiples of 1/4 and q of 1/8: h, g and every interpolation are exact in float64, whichever way they are written
    x = rng.integers(-50, 50, m).astype(F64) / 4
    qs = [0.0, 0.125, 0.25, 0.5, 0.75, 1.0]
    got = pb.map_quantiles(*_one_interval_frames(x), "x", q=qs, method=method, output_type="numpy.ndarray")[0]
    assert (got == np.quantile(x, qs, method=method)).all()


def test_equal_neighbours_give_the_value_itself_also_at_infinity(stand_in):
    x = np.array([-np.inf, -np.inf, 1.0, np.inf, np.inf, np.inf], F64)
    for method in ("midpoint", "linear"):
        got = pb.map_quantiles(*_one_interval_frames(x), "x", q=[0.1, 0.9, 0.5, 0.3], method=method, output_type="numpy.ndarray")[0]
        # h = 0.5, 4.5, 2.5, 1.5: (-inf, -inf), (inf, inf), (1, inf), (-inf, 1); the first two would be inf - inf without the rule
        assert got[0] == -np.inf and got[1] == np.inf and got[2] == np.inf
        assert got[3] == -np.inf if method == "midpoint" else math.isnan(got[3])        # -inf + (1 - -inf) / 2, as numpy has it
    big = np.array([2 ** 53 - 1, 2 ** 53 - 3], I64)
    assert pb.map_median(*_one_interval_frames(big), "x", output_type="numpy.ndarray")[0, 0] == float(2 ** 53 - 2)
