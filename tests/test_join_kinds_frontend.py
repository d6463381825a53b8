"""pb.overlap(how="semi" / "anti" / "left") through the front door on the GPU, against the yardstick of
tests/_join_kinds_util.py evaluated on the same tables."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
from polars_bio_amd import range_op
import _join_kinds_util as J
from _util import GOLDEN

pytestmark = pytest.mark.gpu

COLS = ("contig", "pos_start", "pos_end")
STD = ("chrom", "start", "end")


def _csv(name, zero_based):
    df = pd.read_csv(f"{GOLDEN}/overlap/{name}.csv")
    df.attrs["coordinate_system_zero_based"] = zero_based
    return df


def _sides(df1, df2, cols, on=None):
    """Both frames as (contig id, start, end) over one dictionary of (chrom, on values); a null component gives id -1."""
    def key(df):
        k = df[cols[0]].astype(object)
        null = df[cols[0]].isna()
        for c in on or ():
            k = k.astype(str) + "\x00" + df[c].astype(str)
            null = null | df[c].isna()
        return k.astype(str).where(~null, None)
    k1, k2 = key(df1), key(df2)
    ids = {v: i for i, v in enumerate(sorted(set(k1.dropna()) | set(k2.dropna())))}
    side = lambda df, k: (k.map(ids).fillna(-1).to_numpy(np.int32), df[cols[1]].to_numpy(np.int32), df[cols[2]].to_numpy(np.int32))
    return side(df1, k1), side(df2, k2), max(len(ids), 1)


def _expected(df1, df2, zero_based, cols=STD, on=None, **thr):
    probe, build, nc = _sides(df1, df2, cols, on)
    return J.expected(probe, build, nc, zero_based, **thr)


def _rows(df1, idx):
    return df1.iloc[idx].reset_index(drop=True)


def _sorted(df):
    return df.sort_values(by=list(df.columns)).reset_index(drop=True)


def _random_frames(seed=5, n1=400, n2=500, zero_based=True):
    rng = np.random.default_rng(seed)
    def frame(n, max_len):
        s = rng.integers(0, 30_000, n)
        df = pd.DataFrame({"chrom": rng.choice(["chr1", "chr2", "chrX"], n), "start": s, "end": s + rng.integers(0, max_len, n),
                           "strand": rng.choice(["+", "-"], n), "score": rng.integers(0, 100, n)})
        df.attrs["coordinate_system_zero_based"] = zero_based
        return df
    return frame(n1, 150), frame(n2, 250)


def _check_left(res, inner, df1, df2, e, suffixes=("_1", "_2")):
    """The left outer frame: len(inner) + len(anti) rows, the inner join's rows first, then the anti rows of df1 in order with every
    df2 column null."""
    n_inner, anti = len(inner), e["anti"]
    assert list(res.columns) == list(inner.columns) and len(res) == n_inner + len(anti) and n_inner == len(e["inner"][0])
    cols2 = [c + suffixes[1] for c in df2.columns]
    cols1 = [c + suffixes[0] for c in df1.columns]
    null_rows = res[cols2].isna().all(axis=1).to_numpy()
    assert (res[cols2].isna().any(axis=1).to_numpy() == null_rows).all(), "a row is null in some df2 columns only"
    assert (np.flatnonzero(null_rows) == n_inner + np.arange(len(anti))).all(), "nulls are not exactly on the unmatched tail"
    assert not res[cols1].isna().any().any()
    pd.testing.assert_frame_equal(_sorted(res.iloc[:n_inner].astype(inner.dtypes.to_dict())), _sorted(inner), check_dtype=False)
    tail = res.iloc[n_inner:][cols1].reset_index(drop=True)
    tail.columns = list(df1.columns)
    pd.testing.assert_frame_equal(tail, _rows(df1, anti), check_dtype=False)


@pytest.mark.parametrize("extended", [False, True], ids=["golden", "golden_plus_unmatched_rows"])
@pytest.mark.parametrize("zero_based", [False, True])
def test_golden_tables(zero_based, extended):
    df1, df2 = _csv("reads", zero_based), _csv("targets", zero_based)
    if extended:                                           # every golden read overlaps a target: rows that overlap none, in between
        extra = pd.DataFrame({COLS[0]: ["chrZ", "chr1"], COLS[1]: [100, 5_000_000], COLS[2]: [200, 5_000_100]})
        df1 = pd.concat([df1.iloc[:4], extra.iloc[:1], df1.iloc[4:], extra.iloc[1:]]).reset_index(drop=True)
        df1.attrs["coordinate_system_zero_based"] = zero_based
    kw = dict(cols1=COLS, cols2=COLS, output_type="pandas.DataFrame")
    e = _expected(df1, df2, zero_based, COLS)
    semi, anti = pb.overlap(df1, df2, how="semi", **kw), pb.overlap(df1, df2, how="anti", **kw)
    assert list(semi.columns) == list(df1.columns) == list(anti.columns)
    old = pb.overlap(df1, df2, overlap_output="left", distinct_output=True, **kw)
    pd.testing.assert_frame_equal(semi, old)
    pd.testing.assert_frame_equal(semi, _rows(df1, e["semi"]), check_dtype=False)
    pd.testing.assert_frame_equal(anti, _rows(df1, e["anti"]), check_dtype=False)
    assert len(semi) > 0 and len(anti) == (2 if extended else 0) and len(semi) + len(anti) == len(df1)
    # semi and anti partition df1 in order
    both = pd.concat([semi.assign(_k=e["semi"]), anti.assign(_k=e["anti"])]).sort_values("_k").drop(columns="_k").reset_index(drop=True)
    pd.testing.assert_frame_equal(both, df1.reset_index(drop=True), check_dtype=False)
    assert semi.attrs["coordinate_system_zero_based"] is zero_based
    inner, left = pb.overlap(df1, df2, **kw), pb.overlap(df1, df2, how="left", **kw)
    _check_left(left, inner, df1, df2, e)
    # dtypes of the inner join wherever nothing is null: the Arrow schemas agree
    ti = pb.overlap(df1, df2, cols1=COLS, cols2=COLS, output_type="pyarrow.Table")
    tl = pb.overlap(df1, df2, cols1=COLS, cols2=COLS, output_type="pyarrow.Table", how="left")
    assert tl.schema.names == ti.schema.names and [f.type for f in tl.schema] == [f.type for f in ti.schema]
    for name in tl.schema.names:
        assert tl.column(name).null_count == (len(e["anti"]) if name.endswith("_2") else 0)
    assert pb.overlap(df1, df2, how="inner", **kw).equals(inner)


def test_on_cols_with_a_null_strand():
    df1, df2 = _random_frames()
    df1.loc[[3, 50, 51], "strand"] = None
    df2.loc[[7], "strand"] = None
    e = _expected(df1, df2, True, on=["strand"])
    plain = _expected(df1, df2, True)
    assert len(e["semi"]) < len(plain["semi"]) and {3, 50, 51} <= set(e["anti"])
    kw = dict(on_cols=["strand"], output_type="pandas.DataFrame")
    pd.testing.assert_frame_equal(pb.overlap(df1, df2, how="semi", **kw), _rows(df1, e["semi"]), check_dtype=False)
    pd.testing.assert_frame_equal(pb.overlap(df1, df2, how="anti", **kw), _rows(df1, e["anti"]), check_dtype=False)
    left, inner = pb.overlap(df1, df2, how="left", **kw), pb.overlap(df1, df2, **kw)
    n_inner = len(inner)
    assert len(left) == n_inner + len(e["anti"]) and (left["strand_1"].iloc[:n_inner] == left["strand_2"].iloc[:n_inner]).all()
    tail = left.iloc[n_inner:]
    assert tail[[c + "_2" for c in df2.columns]].isna().all().all()
    assert tail["strand_1"].isna().sum() == 3 and (tail["score_1"].to_numpy() == df1["score"].to_numpy()[e["anti"]]).all()


@pytest.mark.parametrize("thr", [dict(min_frac1=0.5), dict(min_overlap=20), dict(min_overlap=10, min_frac2=0.25)], ids=str)
@pytest.mark.parametrize("zero_based", [True, False])
def test_thresholds_with_every_how(thr, zero_based):
    df1, df2 = _random_frames(seed=6, zero_based=zero_based)
    e = _expected(df1, df2, zero_based, **thr)
    plain = _expected(df1, df2, zero_based)
    assert 0 < len(e["semi"]) < len(plain["semi"])
    kw = dict(output_type="pandas.DataFrame", **thr)
    pd.testing.assert_frame_equal(pb.overlap(df1, df2, how="semi", **kw), _rows(df1, e["semi"]), check_dtype=False)
    pd.testing.assert_frame_equal(pb.overlap(df1, df2, how="anti", **kw), _rows(df1, e["anti"]), check_dtype=False)
    _check_left(pb.overlap(df1, df2, how="left", **kw), pb.overlap(df1, df2, **kw), df1, df2, e)
    cnt = pb.count_overlaps(df1, df2, **kw)["count"].to_numpy()
    assert (np.flatnonzero(cnt > 0) == e["semi"]).all()


def test_suffixes_and_custom_columns():
    df1, df2 = _random_frames(seed=7)
    ren = {"chrom": "contig", "start": "pos_start", "end": "pos_end"}
    r1, r2 = df1.rename(columns=ren), df2.rename(columns=ren)
    r1.attrs, r2.attrs = dict(df1.attrs), dict(df2.attrs)
    e = _expected(df1, df2, True)
    kw = dict(cols1=COLS, cols2=COLS, suffixes=("_a", "_b"), output_type="pandas.DataFrame")
    semi = pb.overlap(r1, r2, how="semi", **kw)
    assert list(semi.columns) == list(r1.columns)                          # no suffix on semi / anti
    pd.testing.assert_frame_equal(semi, _rows(r1, e["semi"]), check_dtype=False)
    left = pb.overlap(r1, r2, how="left", **kw)
    assert list(left.columns) == [c + "_a" for c in r1.columns] + [c + "_b" for c in r2.columns]
    _check_left(left, pb.overlap(r1, r2, **kw), r1, r2, e, suffixes=("_a", "_b"))


def test_limit_and_output_types():
    df1, df2 = _random_frames(seed=8)
    e = _expected(df1, df2, True)
    for how, n in (("semi", len(e["semi"])), ("anti", len(e["anti"])), ("left", len(e["left"][0]))):
        head = pb.overlap(df1, df2, how=how, output_type="pandas.DataFrame", limit=5, low_memory=True)
        full = pb.overlap(df1, df2, how=how, output_type="pandas.DataFrame")
        assert len(full) == n > 5
        pd.testing.assert_frame_equal(head, full.iloc[:5].reset_index(drop=True), check_dtype=False)     # eager: limit takes the head
        tab = pb.overlap(df1, df2, how=how, output_type="pyarrow.Table")
        assert isinstance(tab, pa.Table) and tab.num_rows == n
        reader = pb.overlap(df1, df2, how=how, output_type="pyarrow.RecordBatchReader")
        assert isinstance(reader, pa.RecordBatchReader)
        got = reader.read_all()
        assert got.num_rows == n and got.column_names == tab.column_names
        pd.testing.assert_frame_equal(got.to_pandas(), full, check_dtype=False)
        limited = pb.overlap(df1, df2, how=how, output_type="pyarrow.RecordBatchReader", limit=7)
        assert limited.read_all().num_rows == 7


def test_empty_df2_leaves_every_row_unmatched():
    df1, df2 = _random_frames(seed=9, n1=50)
    none = df2.iloc[:0].copy()
    none.attrs = dict(df2.attrs)
    kw = dict(output_type="pandas.DataFrame")
    assert len(pb.overlap(df1, none, how="semi", **kw)) == 0
    pd.testing.assert_frame_equal(pb.overlap(df1, none, how="anti", **kw), df1.reset_index(drop=True), check_dtype=False)
    left = pb.overlap(df1, none, how="left", **kw)
    assert len(left) == len(df1) and left[[c + "_2" for c in df2.columns]].isna().all().all()


def test_accessor_passes_how_through():
    df1, df2 = _random_frames(seed=10)
    e = _expected(df1, df2, True, min_overlap=5)
    got = df1.pb.overlap(df2, how="anti", min_overlap=5)
    assert isinstance(got, pd.DataFrame)
    pd.testing.assert_frame_equal(got, _rows(df1, e["anti"]), check_dtype=False)
    assert len(df1.pb.overlap(df2, how="left")) == len(_expected(df1, df2, True)["left"][0])


def test_multi_device_engine_is_refused(monkeypatch):
    class MultiEngine:                                     # what an engine over several devices without these joins looks like to the front door
        last_shards = None
    df1, df2 = _random_frames(seed=11, n1=20, n2=20)
    monkeypatch.setattr(range_op, "default_engine", lambda: MultiEngine())
    for how in ("semi", "anti", "left"):
        with pytest.raises(NotImplementedError, match="single-device engine.*MultiEngine"):
            pb.overlap(df1, df2, how=how, output_type="pandas.DataFrame")
    with pytest.raises(NotImplementedError, match="single-device engine"):
        pb.overlap(df1, df2, how="semi", min_overlap=3, output_type="pandas.DataFrame")
