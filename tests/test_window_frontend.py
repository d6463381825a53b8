"""pb.window / pb.count_window through the front door on the GPU, against the brute force of tests/_window_util.py evaluated on the
same tables; polars frames in and out against tests/_fake_polars.py (the image has no polars), with the brute force as the engine
where there is no GPU and on the GPU."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
from polars_bio_amd import namespace, range_op
import _fake_polars
import _window_util as WU

gpu = pytest.mark.gpu

COLS = ("chrom", "start", "end")


def _frames(seed=5, n1=400, n2=500, zero_based=True, strands=("+", "-")):
    rng = np.random.default_rng(seed)

    def frame(n, max_len):
        s = rng.integers(0, 30_000, n)
        df = pd.DataFrame({"chrom": rng.choice(["chr1", "chr2", "chrX"], n), "start": s, "end": s + rng.integers(0, max_len, n),
                           "strand": rng.choice(list(strands), n), "score": rng.integers(0, 100, n)})
        df.attrs["coordinate_system_zero_based"] = zero_based
        return df
    return frame(n1, 150), frame(n2, 250)


def _sides(df1, df2, on=None):
    def key(df):
        k = df["chrom"].astype(str)
        for c in on or ():
            k = k + "\x00" + df[c].astype(str)
        return k
    k1, k2 = key(df1), key(df2)
    ids = {v: i for i, v in enumerate(sorted(set(k1) | set(k2)))}
    side = lambda df, k: (k.map(ids).to_numpy(np.int32), df["start"].to_numpy(np.int32), df["end"].to_numpy(np.int32))
    return side(df1, k1), side(df2, k2), len(ids)


def _expected(df1, df2, zero_based, up, down, min_distance=0, on=None, minus=None, signed=False, suffixes=("_1", "_2")):
    """The joined frame with its distance column from the brute force; minus: bool per df1 row (the extents are swapped there)."""
    probe, build, nc = _sides(df1, df2, on)
    n = len(df1)
    minus = np.zeros(n, bool) if minus is None else minus
    ext_l = np.where(minus, down, up).astype(np.uint32)
    ext_r = np.where(minus, up, down).astype(np.uint32)
    p, b, d, cnt = WU.brute(probe, build, nc, zero_based, 0, 0, min_distance, probe_left=ext_l, probe_right=ext_r)
    left = df1.iloc[p].reset_index(drop=True).add_suffix(suffixes[0])
    right = df2.iloc[b].reset_index(drop=True).add_suffix(suffixes[1])
    dist = np.where(minus[p], -d, d) if signed else np.abs(d)
    return pd.concat([left, right, pd.DataFrame({"distance": dist})], axis=1), p, cnt


def _sorted(df):
    return df.sort_values(by=list(df.columns)).reset_index(drop=True)


@gpu
@pytest.mark.parametrize("zero_based", [True, False])
def test_pandas_in_every_output_type(zero_based):
    df1, df2 = _frames(zero_based=zero_based)
    exp, p, cnt = _expected(df1, df2, zero_based, 500, 500)
    assert len(exp) > 200 and (exp["distance"] > 0).sum() > 100 and (exp["distance"] == 0).sum() > 10
    res = pb.window(df1, df2, 500, output_type="pandas.DataFrame")
    assert list(res.columns) == list(exp.columns) and str(res["distance"].dtype).lower() == "int64"
    pd.testing.assert_frame_equal(_sorted(res), _sorted(exp), check_dtype=False)
    assert res.attrs["coordinate_system_zero_based"] is zero_based
    tab = pb.window(df1, df2, 500, output_type="pyarrow.Table")
    assert isinstance(tab, pa.Table) and tab.num_rows == len(exp) and tab.schema.field("distance").type == pa.int64()
    reader = pb.window(df1, df2, 500, output_type="pyarrow.RecordBatchReader")
    assert isinstance(reader, pa.RecordBatchReader)
    pd.testing.assert_frame_equal(_sorted(reader.read_all().to_pandas()), _sorted(exp), check_dtype=False)
    assert len(pb.window(df1, df2, 500, output_type="pandas.DataFrame", limit=7)) == 7


@gpu
def test_pyarrow_in_suffixes_and_no_distance():
    df1, df2 = _frames(seed=6)
    t1, t2 = pa.Table.from_pandas(df1), pa.Table.from_pandas(df2)
    from polars_bio_amd import set_coordinate_system
    t1, t2 = set_coordinate_system(t1, True), set_coordinate_system(t2, True)
    exp, _, _ = _expected(df1, df2, True, 300, 300, suffixes=("_a", "_b"))
    res = pb.window(t1, t2, 300, suffixes=("_a", "_b"), distance=False, output_type="pandas.DataFrame")
    assert "distance" not in res.columns and list(res.columns) == list(exp.columns)[:-1]
    pd.testing.assert_frame_equal(_sorted(res), _sorted(exp.drop(columns="distance")), check_dtype=False)


@gpu
def test_on_cols_strand():
    df1, df2 = _frames(seed=7)
    exp, _, cnt = _expected(df1, df2, True, 800, 800, 5, on=["strand"])
    res = pb.window(df1, df2, 800, min_distance=5, on_cols=["strand"], output_type="pandas.DataFrame")
    assert len(exp) > 50 and (res["strand_1"] == res["strand_2"]).all()
    pd.testing.assert_frame_equal(_sorted(res), _sorted(exp), check_dtype=False)
    got = pb.count_window(df1, df2, 800, min_distance=5, on_cols=["strand"], output_type="pandas.DataFrame")
    assert (got["count"].to_numpy() == cnt).all()


@gpu
@pytest.mark.parametrize("zero_based", [True, False])
def test_direction_col_swaps_the_extents_and_the_sign(zero_based):
    df1, df2 = _frames(seed=8, zero_based=zero_based, strands=("+", "-", "."))
    minus = (df1["strand"] == "-").to_numpy()
    assert 50 < minus.sum() < 350
    exp, _, cnt = _expected(df1, df2, zero_based, 1500, 100, minus=minus, signed=True)
    undirected, _, _ = _expected(df1, df2, zero_based, 1500, 100, signed=True)
    assert len(exp) > 200 and len(exp) != len(undirected)
    res = pb.window(df1, df2, upstream=1500, downstream=100, direction_col="strand", signed_distance=True, output_type="pandas.DataFrame")
    pd.testing.assert_frame_equal(_sorted(res), _sorted(exp), check_dtype=False)
    # the sign reads along the strand: upstream (negative) reaches 1500 bases, downstream (positive) 100, on both strands
    for strand_is_minus in (False, True):
        d = res["distance"][(res["strand_1"] == "-") == strand_is_minus]
        assert d.min() < -100 and d.min() >= -1500 and 0 < d.max() <= 100
    plain = pb.window(df1, df2, upstream=1500, downstream=100, direction_col="strand", output_type="pandas.DataFrame")
    assert (plain["distance"] >= 0).all() and (np.sort(plain["distance"].to_numpy()) == np.sort(np.abs(exp["distance"].to_numpy()))).all()
    nodir = pb.window(df1, df2, upstream=1500, downstream=100, signed_distance=True, output_type="pandas.DataFrame")
    pd.testing.assert_frame_equal(_sorted(nodir), _sorted(undirected), check_dtype=False)
    got = pb.count_window(df1, df2, upstream=1500, downstream=100, direction_col="strand", output_type="pandas.DataFrame")
    assert (got["count"].to_numpy() == cnt).all()


@gpu
def test_count_window_keeps_order_and_columns_and_min_distance_above_the_extents():
    df1, df2 = _frames(seed=9)
    _, p, cnt = _expected(df1, df2, True, 250, 250, 3)
    got = pb.count_window(df1, df2, 250, min_distance=3, output_type="pandas.DataFrame")
    assert list(got.columns) == list(df1.columns) + ["count"] and str(got["count"].dtype).lower() == "int64"
    pd.testing.assert_frame_equal(got[list(df1.columns)], df1, check_dtype=False)
    assert cnt.sum() > 100 and (got["count"].to_numpy() == cnt).all()
    empty = pb.window(df1, df2, 250, min_distance=251, output_type="pandas.DataFrame")
    assert len(empty) == 0 and "distance" in empty.columns
    assert not pb.count_window(df1, df2, 250, min_distance=251, output_type="pandas.DataFrame")["count"].any()


@gpu
def test_pb_accessor():
    df1, df2 = _frames(seed=10)
    a = df1.pb.window(df2, window=100, min_distance=1)
    b = pb.window(df1, df2, 100, min_distance=1, output_type="pandas.DataFrame")
    assert isinstance(a, pd.DataFrame) and len(a) > 0
    pd.testing.assert_frame_equal(a, b)
    c = df1.pb.count_window(df2, window=100)
    assert isinstance(c, pd.DataFrame) and int(c["count"].sum()) == len(pb.window(df1, df2, 100, output_type="pandas.DataFrame"))


class _BruteEngine:
    """the engine's window entries from the brute force: lets the polars glue run where there is no GPU"""

    def overlap_window(self, probe, build, strict, n_contigs, left=0, right=0, min_distance=0, probe_left=None, probe_right=None,
                       distance=True, partition_mode=0):
        p, b, d, _ = WU.brute(probe, build, n_contigs, strict, left, right, min_distance, probe_left, probe_right)
        return p, b, (d if distance else None)

    def count_window(self, probe, build, strict, n_contigs, left=0, right=0, min_distance=0, probe_left=None, probe_right=None,
                     partition_mode=0):
        return WU.brute(probe, build, n_contigs, strict, left, right, min_distance, probe_left, probe_right)[3]


class _Meta:
    """polars-config-meta's accessor, as far as the package reads and writes it"""

    def __init__(self, **kw):
        self._d = dict(kw)

    def get_metadata(self):
        return self._d

    def set(self, **kw):
        self._d.update(kw)


@pytest.fixture(params=["cpu", pytest.param("gpu", marks=gpu)])
def fake_pl(request, monkeypatch):
    """tests/_fake_polars.py as ``polars`` (the image has none); "cpu": the brute force stands in for the engine as well"""
    if request.param == "cpu":
        monkeypatch.setattr(range_op, "default_engine", lambda: _BruteEngine())
    return _fake_polars.install(monkeypatch)


def _polars(pl, df, zero_based, lazy=False):
    out = pl.from_arrow(pa.Table.from_pandas(df, preserve_index=False))
    out = out.lazy() if lazy else out
    out.config_meta = _Meta(coordinate_system_zero_based=zero_based)
    return out


@pytest.mark.parametrize("zero_based", [True, False])
def test_polars_frames_in_and_out(fake_pl, zero_based):
    """A DataFrame and a LazyFrame in; polars.DataFrame, the default polars.LazyFrame and ``limit`` out; the accessor a LazyFrame
    gets (namespace._make_accessor, what polars' register_lazyframe_namespace instantiates) with a LazyFrame as the other frame."""
    pl = fake_pl
    df1, df2 = _frames(seed=11, zero_based=zero_based, strands=("+", "-", "."))
    minus = (df1["strand"] == "-").to_numpy()
    kw = dict(upstream=700, downstream=60, direction_col="strand", signed_distance=True, min_distance=2)
    exp, _, cnt = _expected(df1, df2, zero_based, 700, 60, 2, minus=minus, signed=True)
    assert len(exp) > 100 and (exp["distance"] < 0).sum() > 20 and (exp["distance"] > 0).sum() > 5
    p1, p2 = _polars(pl, df1, zero_based), _polars(pl, df2, zero_based, lazy=True)
    res = pb.window(p1, p2, output_type="polars.DataFrame", **kw)
    assert isinstance(res, pl.DataFrame) and res.columns == list(exp.columns)
    assert res.to_arrow().schema.field("distance").type == pa.int64()
    pd.testing.assert_frame_equal(_sorted(res.to_arrow().to_pandas()), _sorted(exp), check_dtype=False)
    lazy = pb.window(p1, p2, **kw)                                                   # the default output kind
    assert isinstance(lazy, pl.LazyFrame)
    got = lazy.collect()
    assert isinstance(got, pl.DataFrame) and got.to_arrow().equals(res.to_arrow())
    assert pb.window(p1, p2, limit=9, **kw).collect().to_arrow().equals(res.to_arrow().slice(0, 9))
    ckw = {k: v for k, v in kw.items() if k != "signed_distance"}
    c = pb.count_window(p1, p2, output_type="polars.DataFrame", **ckw)
    assert isinstance(c, pl.DataFrame) and c.columns == list(df1.columns) + ["count"]
    assert c.to_arrow().column("count").type == pa.int64() and (c.to_arrow().column("count").to_numpy() == cnt).all()
    assert c.to_arrow().column("start").to_pylist() == df1["start"].tolist()
    clazy = pb.count_window(p1, p2, **ckw)
    assert isinstance(clazy, pl.LazyFrame) and clazy.collect().to_arrow().equals(c.to_arrow())
    acc = namespace._make_accessor("polars.LazyFrame")(_polars(pl, df1, zero_based, lazy=True))
    via = acc.window(p2, **kw)
    assert isinstance(via, pl.LazyFrame) and via.collect().to_arrow().equals(res.to_arrow())
    cvia = acc.count_window(p2, **ckw)
    assert isinstance(cvia, pl.LazyFrame) and cvia.collect().to_arrow().equals(c.to_arrow())
    dacc = namespace._make_accessor("polars.DataFrame")(p1)
    assert isinstance(dacc.window(p2, **kw), pl.DataFrame) and isinstance(dacc.count_window(p2, **ckw), pl.DataFrame)


@gpu
def test_real_polars_frames():
    """the same against the real package, where it is installed (an extra: the case above is the one that always runs)"""
    pl = pytest.importorskip("polars")
    df1, df2 = _frames(seed=12)
    exp, _, cnt = _expected(df1, df2, True, 300, 300)
    p1, p2 = (pb.set_coordinate_system(pl.from_pandas(d), True) for d in (df1, df2))
    out = pb.window(p1, p2.lazy(), 300, output_type="polars.DataFrame")
    assert out.columns == list(exp.columns) and out.height == len(exp)
    lazy = p1.lazy().pb.count_window(p2, window=300)
    assert isinstance(lazy, pl.LazyFrame) and lazy.collect()["count"].to_list() == cnt.tolist()
