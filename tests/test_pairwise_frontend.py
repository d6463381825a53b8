"""pb.pairwise_jaccard, the front door: the argument checks (made before an engine exists), string chroms in different
first-occurrence order, both coordinate systems, the long form and the matrix of every statistic, empty unions, on_cols, pandas and
polars inputs."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
from polars_bio_amd import _engine
import _fake_polars
import _pairwise_util as P

gpu = pytest.mark.gpu

ROWS = [
    [("chr2", 10, 30), ("chr1", 0, 20), ("chr10", 5, 9), ("chr1", 40, 50)],
    [("chr10", 7, 12), ("chr2", 20, 40), ("chr1", 10, 45)],
    [("chr1", 15, 42), ("chrX", 1, 4), ("chr2", 30, 35), ("chr2", 35, 38)],
]
NAMES = ["rep1", "rep2", "rep3"]
COLUMNS = ["frame_1", "frame_2", "intersection", "union", "jaccard", "n_intersections"]


def _frame(rows, zero_based=True, extra=None):
    df = pd.DataFrame(rows, columns=["chrom", "start", "end"])
    for name, values in (extra or {}).items():
        df[name] = values
    df.attrs["coordinate_system_zero_based"] = zero_based
    return df


def _reference(rows_by_frame, zero_based):
    names = sorted({r[0] for rows in rows_by_frame for r in rows})
    frames = [P.S.as_i32([names.index(r[0]) for r in rows], [r[1] for r in rows], [r[2] for r in rows]) for rows in rows_by_frame]
    return P.pairwise_events(frames, zero_based, max(len(names), 1))


@pytest.fixture
def no_engine(monkeypatch):
    """any attempt to create or fetch an engine fails the test"""
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_engine, "default_engine", boom)
    monkeypatch.setattr(_engine, "Engine", boom)
    monkeypatch.setattr(pb.range_op, "default_engine", boom)


def test_bad_arguments_raise_before_the_engine_is_touched(no_engine):
    df = _frame([("chr1", 0, 5)])
    for bad in (df, "frames", None, {"a": df}):
        with pytest.raises(ValueError, match="list of interval frames"):
            pb.pairwise_jaccard(bad, output_type="pandas.DataFrame")
    with pytest.raises(ValueError, match="between 1 and 64 frames"):
        pb.pairwise_jaccard([], output_type="pandas.DataFrame")
    with pytest.raises(ValueError, match="between 1 and 64 frames"):
        pb.pairwise_jaccard([df] * 65, output_type="numpy.ndarray")
    for names in (["a"], ["a", "b", "c"], ["a", "a"], ["a", 3], "ab"):
        with pytest.raises(ValueError, match="names"):
            pb.pairwise_jaccard([df, df], names=names, output_type="pandas.DataFrame")
    for statistic in ("dice", "", None, "Jaccard"):
        with pytest.raises(ValueError, match="unknown statistic"):
            pb.pairwise_jaccard([df, df], statistic=statistic, output_type="numpy.ndarray")
    with pytest.raises(pb.CoordinateSystemMismatchError):
        pb.pairwise_jaccard([df, df, _frame([("chr1", 1, 5)], zero_based=False)], output_type="pandas.DataFrame")


def test_exports():
    from polars_bio_amd import namespace
    assert "pairwise_jaccard" in pb.__all__ and callable(pb.pairwise_jaccard) and "pairwise_jaccard" in pb.range_op.__all__
    assert namespace._ALIASES["pairwise_jaccard"] == (pb.range_op.pairwise_jaccard, "frames")
    assert {"ivj_multi_pairwise", "ivj_multi_pairwise_dev"} <= set(_engine.ABI_SYMBOLS)


@gpu
@pytest.mark.parametrize("zero_based", [True, False], ids=["0-based", "1-based"])
def test_the_long_form_on_pandas_frames(zero_based):
    frames = [_frame(rows, zero_based) for rows in ROWS]
    res = pb.pairwise_jaccard(frames, names=NAMES, output_type="pandas.DataFrame")
    assert list(res.columns) == COLUMNS and len(res) == 9
    assert [str(res[c].dtype) for c in COLUMNS[2:]] == ["int64", "int64", "float64", "int64"]
    assert list(res["frame_1"]) == [a for a in NAMES for _ in NAMES] and list(res["frame_2"]) == NAMES * 3      # row-major
    bases, runs = _reference(ROWS, zero_based)
    union, jac = P.jaccard_of(bases)
    assert (res["intersection"].to_numpy() == bases.reshape(-1)).all() and (res["union"].to_numpy() == union.reshape(-1)).all()
    assert (res["n_intersections"].to_numpy() == runs.reshape(-1)).all()
    assert (res["jaccard"].to_numpy() == jac.reshape(-1)).all()             # the same quotient of the same two integers
    assert (res["jaccard"][res["frame_1"] == res["frame_2"]] == 1.0).all()
    assert pb.get_coordinate_system(res) is zero_based
    wide = res.pivot(index="frame_1", columns="frame_2", values="jaccard")
    assert (wide.loc[NAMES, NAMES].to_numpy() == jac).all()
    bare = pb.pairwise_jaccard(frames, output_type="pandas.DataFrame")
    assert str(bare["frame_1"].dtype) == "int64" and list(bare["frame_2"]) == [0, 1, 2] * 3
    assert bare[COLUMNS[2:]].equals(res[COLUMNS[2:]])
    # every pair against pb.jaccard
    for i in range(3):
        for j in range(3):
            one = pb.jaccard(frames[i], frames[j], output_type="pandas.DataFrame").iloc[0]
            row = res.iloc[3 * i + j]
            assert (row.intersection, row.union, row.jaccard, row.n_intersections) == (one.intersection, one.union, one.jaccard, one.n_intersections)


@gpu
@pytest.mark.parametrize("zero_based", [True, False], ids=["0-based", "1-based"])
def test_the_matrix_of_every_statistic(zero_based):
    frames = [_frame(rows, zero_based) for rows in ROWS]
    bases, runs = _reference(ROWS, zero_based)
    union, jac = P.jaccard_of(bases)
    exp = {"jaccard": jac, "intersection": bases, "union": union, "n_intersections": runs, "fraction": bases / np.diagonal(bases)[:, None]}
    for statistic, want in exp.items():
        got = pb.pairwise_jaccard(frames, statistic=statistic, output_type="numpy.ndarray")
        assert isinstance(got, np.ndarray) and got.shape == (3, 3) and got.dtype == want.dtype, statistic
        assert (got == want).all(), statistic
    assert (pb.pairwise_jaccard(frames, output_type="numpy.ndarray") == jac).all()          # "jaccard" is the default
    frac = exp["fraction"]
    assert (np.diagonal(frac) == 1.0).all() and not (frac == frac.T).all()


@gpu
def test_empty_unions_are_null_and_nan():
    empty = _frame([("chr1", 3, 9)], True).iloc[:0]
    empty.attrs["coordinate_system_zero_based"] = True
    nothing = _frame([("chr1", 7, 7)], True)                                # a row that covers no position
    a = _frame(ROWS[0], True)
    frames = [empty, a, nothing]
    res = pb.pairwise_jaccard(frames, names=["e", "a", "n"], output_type="pandas.DataFrame")
    dead = (res["frame_1"] != "a") & (res["frame_2"] != "a")
    assert (res["union"][dead] == 0).all() and res["jaccard"][dead].isna().all() and dead.sum() == 4
    assert (res["jaccard"][~dead & (res["frame_1"] != res["frame_2"])] == 0.0).all()
    assert res["jaccard"][4] == 1.0
    jac = pb.pairwise_jaccard(frames, output_type="numpy.ndarray")
    assert np.isnan(jac[[0, 0, 2, 2], [0, 2, 0, 2]]).all() and jac[1, 1] == 1.0 and (jac[1, [0, 2]] == 0.0).all()
    frac = pb.pairwise_jaccard(frames, statistic="fraction", output_type="numpy.ndarray")
    assert np.isnan(frac[[0, 2]]).all() and (frac[1] == [0.0, 1.0, 0.0]).all()
    for statistic in ("intersection", "union", "n_intersections"):
        m = pb.pairwise_jaccard([empty, nothing], statistic=statistic, output_type="numpy.ndarray")
        assert m.dtype == np.int64 and m.shape == (2, 2) and not m.any()
    one = pb.pairwise_jaccard([a], output_type="pandas.DataFrame")
    assert len(one) == 1 and one["jaccard"][0] == 1.0 and one["n_intersections"][0] == 4


@gpu
def test_on_cols_sums_the_per_strand_calls():
    strands = [["+", "-", "+", None], ["+", "+", "-"], ["-", "+", "+", "+"]]
    frames = [_frame(rows, True, {"strand": st}) for rows, st in zip(ROWS, strands)]
    for statistic in ("intersection", "n_intersections", "union"):
        got = pb.pairwise_jaccard(frames, statistic=statistic, on_cols=["strand"], output_type="numpy.ndarray")
        parts = np.zeros((3, 3), np.int64)
        for strand in ("+", "-"):
            sub = [f[f["strand"] == strand].drop(columns="strand") for f in frames]
            for s in sub:
                s.attrs["coordinate_system_zero_based"] = True
            parts += pb.pairwise_jaccard(sub, statistic=statistic, output_type="numpy.ndarray")
        assert (got == parts).all(), statistic
    plain = pb.pairwise_jaccard([f.drop(columns="strand") for f in frames], statistic="intersection", output_type="numpy.ndarray")
    inter = pb.pairwise_jaccard(frames, statistic="intersection", on_cols=["strand"], output_type="numpy.ndarray")
    assert (inter <= plain).all() and (inter < plain).any(), "positions match within a strand only"


class _Meta(dict):
    """what polars-config-meta hangs on a frame"""
    def get_metadata(self):
        return dict(self)


@gpu
def test_polars_frames_in_and_out(monkeypatch):
    """tests/_fake_polars.py as ``polars`` (the image has none): a DataFrame and LazyFrames in, each output kind out"""
    pl = _fake_polars.install(monkeypatch)
    frames = [_frame(rows, True) for rows in ROWS]
    exp = pb.pairwise_jaccard(frames, names=NAMES, output_type="pandas.DataFrame")
    pls = []
    for k, f in enumerate(frames):
        df = pl.from_arrow(pa.Table.from_pandas(f, preserve_index=False))
        df = df.lazy() if k else df
        df.config_meta = _Meta(coordinate_system_zero_based=True)
        pls.append(df)
    lazy = pb.pairwise_jaccard(pls, names=NAMES)                                       # the default output kind
    assert isinstance(lazy, pl.LazyFrame)
    for got in (lazy.collect(), pb.pairwise_jaccard(pls, names=NAMES, output_type="polars.DataFrame")):
        assert isinstance(got, pl.DataFrame) and got.columns == COLUMNS and got.height == 9
        t = got.to_arrow()
        assert all(t.column(c).to_pylist() == exp[c].tolist() for c in COLUMNS)
    assert (pb.pairwise_jaccard(pls, statistic="union", output_type="numpy.ndarray").reshape(-1) == exp["union"].to_numpy()).all()


@gpu
def test_namespace_takes_the_other_frames_as_a_list():
    frames = [_frame(rows, True) for rows in ROWS]
    res = frames[0].pb.pairwise_jaccard(frames[1:], names=NAMES)
    assert isinstance(res, pd.DataFrame) and res.equals(pb.pairwise_jaccard(frames, names=NAMES, output_type="pandas.DataFrame"))
