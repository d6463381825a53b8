"""pb.depth_profile, the front door: the int32 check of the windows (CPU); input kinds, the fixed-size-list schema, df1 order, both
coordinate systems, both outputs and the numpy form, on_cols, nulls, direction_col with the three anchors, the equivalence with
pb.mean_depth on the explicit bin frame, and the .pb accessor (GPU); polars frames in and out against tests/_fake_polars.py
(the image has no polars), with the util as the engine where there is no GPU and on the GPU."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
from polars_bio_amd import range_op
import _depth_profile_util as P
import _fake_polars
import _depth_sum_util as S

gpu = pytest.mark.gpu
NAMES = np.array(["chr10", "chr2", "chrX", "chr1"])
ZB = [pytest.param(True, id="zero_based"), pytest.param(False, id="one_based")]


def _frame(zero_based, seed, n, max_len, strand=False, null_chrom=False, null_strand=False, empty_rows=False, odd_strand=False):
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
        if odd_strand:
            d["strand"][rng.integers(0, n, n // 10)] = "."
        if null_strand:
            d["strand"][rng.integers(0, n, n // 10)] = None
    if null_chrom:
        d["chrom"][rng.integers(0, n, n // 10)] = None
    df = pd.DataFrame(d)
    df.attrs["coordinate_system_zero_based"] = zero_based
    return df


def _sides(df1, df2, on=None):
    """(contig ids of df1, df2, n_contigs); rows with a null key get the id -1, which matches nothing"""
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
    return c1, c2, len(names)


def _expected(df1, df2, zero_based, n_bins, windows=None, reverse=None, on=None):
    """(bases, bin lengths) from the util; windows = (start, end) arrays in the frames' convention, default the df1 rows"""
    c1, c2, nc = _sides(df1, df2, on)
    ws, we = (df1["start"].to_numpy(), df1["end"].to_numpy()) if windows is None else windows
    build = (c2, df2["start"].to_numpy(), df2["end"].to_numpy())
    w = (c1, np.asarray(ws, np.int64), np.asarray(we, np.int64))
    return P.expected_bases(w, build, zero_based, nc, n_bins, reverse), P.bin_lengths(w, n_bins, zero_based, reverse)


def _matrix(col):
    """the profile column of a pandas result -> (n, B) float64 matrix with NaN for null"""
    return np.array([np.array([np.nan if v is None else v for v in row], np.float64) for row in col])


def _check_mean(mean, bases, lens):
    assert mean.dtype == np.float64 and mean.shape == bases.shape
    assert (np.isnan(mean) == (lens == 0)).all()                       # null exactly on the empty bins
    ok = lens > 0
    assert (mean[ok] == bases[ok].astype(np.float64) / lens[ok].astype(np.float64)).all()      # exactly this quotient


def test_a_window_outside_int32_is_a_value_error():
    df = pd.DataFrame({"chrom": ["chr1"] * 3, "start": [100, 2 ** 31 - 50, 7], "end": [200, 2 ** 31 - 10, 9]})
    df.attrs["coordinate_system_zero_based"] = True
    with pytest.raises(ValueError, match="window of df1 row 1 leaves the int32 range"):
        pb.depth_profile(df, df, anchor="end", upstream=5, downstream=100, output_type="pandas.DataFrame")
    with pytest.raises(ValueError, match="window of df1 row 2 leaves the int32 range"):
        pb.depth_profile(df, df, anchor="start", upstream=2 ** 31 + 8, downstream=1, n_bins=4, output_type="numpy.ndarray")


@gpu
@pytest.mark.parametrize("zero_based", ZB)
def test_pandas_frames_bases_and_order(zero_based):
    df1 = _frame(zero_based, 3, 1500, 400, empty_rows=True)
    df2 = _frame(zero_based, 4, 4000, 90, empty_rows=True)
    res = pb.depth_profile(df1, df2, n_bins=12, output="bases", output_type="pandas.DataFrame")
    bases, lens = _expected(df1, df2, zero_based, 12)
    assert (bases > 0).any() and (lens == 0).any() and ((df1["end"] - df1["start"]) < 0).any()
    assert list(res.columns) == ["chrom", "start", "end", "profile"]
    assert res.attrs["coordinate_system_zero_based"] == zero_based
    assert (res["start"].to_numpy() == df1["start"].to_numpy()).all() and (res["end"].to_numpy() == df1["end"].to_numpy()).all()
    assert (np.array([np.asarray(r, np.int64) for r in res["profile"]]) == bases).all()
    mat = pb.depth_profile(df1, df2, n_bins=12, output="bases", output_type="numpy.ndarray")
    P.assert_profile_equal(mat, bases, "numpy.ndarray")


@gpu
@pytest.mark.parametrize("zero_based", ZB)
def test_mean_is_bases_over_bin_length_with_nulls_on_empty_bins(zero_based):
    df1 = _frame(zero_based, 5, 1200, 60, empty_rows=True)             # many windows shorter than 25 bins
    df2 = _frame(zero_based, 6, 3000, 90)
    bases, lens = _expected(df1, df2, zero_based, 25)
    assert (lens == 0).any() and (lens > 1).any()
    mean = pb.depth_profile(df1, df2, n_bins=25, output_type="numpy.ndarray")
    _check_mean(mean, bases, lens)
    res = pb.depth_profile(df1, df2, n_bins=25, output_type="pandas.DataFrame")
    got = _matrix(res["profile"])
    assert (np.isnan(got) == np.isnan(mean)).all() and (got[~np.isnan(got)] == mean[~np.isnan(mean)]).all()


@gpu
@pytest.mark.parametrize("output, value_type", [("mean", pa.float64()), ("bases", pa.int64())])
def test_arrow_schema_and_input_kinds(output, value_type):
    df1, df2 = _frame(True, 7, 800, 300), _frame(True, 8, 2000, 80)
    meta = {"coordinate_system_zero_based": "true"}
    t1, t2 = (pa.Table.from_pandas(d, preserve_index=False).replace_schema_metadata(meta) for d in (df1, df2))
    res = pb.depth_profile(t1, t2, n_bins=10, output=output, output_type="pyarrow.Table")
    assert res.column_names == ["chrom", "start", "end", "profile"]
    assert res.schema.field("profile").type == pa.list_(value_type, 10)          # fixed_size_list<...>[10]
    bases, lens = _expected(df1, df2, True, 10)
    flat = res.column("profile").combine_chunks().flatten()
    if output == "bases":
        assert flat.null_count == 0 and (flat.to_numpy().reshape(-1, 10) == bases).all()
    else:
        assert flat.null_count == int((lens == 0).sum())
        _check_mean(flat.to_numpy(zero_copy_only=False).reshape(-1, 10), bases, lens)
    # the record-batch reader reads the finished table
    rd = pb.depth_profile(t1, t2, n_bins=10, output=output, output_type="pyarrow.RecordBatchReader")
    assert rd.read_all().column("profile").combine_chunks().flatten().to_pylist() == flat.to_pylist()


class _NumpyEngine:
    """the engine's depth_profile from the util: lets the polars glue run where there is no GPU"""

    def depth_profile(self, windows, reverse, n_bins, build, strict, n_contigs):
        return P.expected_bases(windows, build, strict, n_contigs, n_bins, reverse)


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
    """tests/_fake_polars.py as ``polars`` (the image has none); "cpu": the util stands in for the engine as well"""
    if request.param == "cpu":
        monkeypatch.setattr(range_op, "default_engine", lambda: _NumpyEngine())
    return _fake_polars.install(monkeypatch)


def _polars(pl, df, zero_based, lazy=False):
    out = pl.from_arrow(pa.Table.from_pandas(df, preserve_index=False))
    out = out.lazy() if lazy else out
    out.config_meta = _Meta(coordinate_system_zero_based=zero_based)
    return out


@pytest.mark.parametrize("zero_based", ZB)
@pytest.mark.parametrize("output, value_type", [("mean", pa.float64()), ("bases", pa.int64())])
def test_polars_frames_in_and_out(fake_pl, output, value_type, zero_based):
    pl = fake_pl
    df1, df2 = _frame(zero_based, 7, 800, 300, strand=True), _frame(zero_based, 8, 2000, 80)
    minus = (df1["strand"] == "-").to_numpy()
    bases, lens = _expected(df1, df2, zero_based, 10, reverse=minus)
    p1, p2 = _polars(pl, df1, zero_based), _polars(pl, df2, zero_based, lazy=True)          # a DataFrame and a LazyFrame in
    res = pb.depth_profile(p1, p2, n_bins=10, direction_col="strand", output=output, output_type="polars.DataFrame")
    assert isinstance(res, pl.DataFrame) and res.columns == ["chrom", "start", "end", "strand", "profile"] and res.height == len(df1)
    t = res.to_arrow()
    assert t.schema.field("profile").type == pa.list_(value_type, 10)
    assert t.column("start").to_pylist() == df1["start"].tolist() and t.column("chrom").to_pylist() == df1["chrom"].tolist()
    flat = t.column("profile").combine_chunks().flatten()
    if output == "bases":
        assert flat.null_count == 0 and (flat.to_numpy().reshape(-1, 10) == bases).all()
    else:
        assert flat.null_count == int((lens == 0).sum())
        _check_mean(flat.to_numpy(zero_copy_only=False).reshape(-1, 10), bases, lens)
    # the default output kind is the LazyFrame over the finished table
    lazy = pb.depth_profile(p1, p2, n_bins=10, direction_col="strand", output=output)
    assert isinstance(lazy, pl.LazyFrame)
    assert lazy.collect().to_arrow().column("profile").combine_chunks().flatten().to_pylist() == flat.to_pylist()


@gpu
def test_real_polars_frames():
    """the same against the real package, where it is installed (an extra: the case above is the one that always runs)"""
    pl = pytest.importorskip("polars")
    df1, df2 = _frame(True, 7, 800, 300), _frame(True, 8, 2000, 80)
    p1, p2 = (pb.set_coordinate_system(pl.from_pandas(d), True) for d in (df1, df2))
    out = pb.depth_profile(p1, p2, n_bins=10, output="bases", output_type="polars.DataFrame")
    assert out.columns == ["chrom", "start", "end", "profile"] and out.height == len(df1)
    bases, _ = _expected(df1, df2, True, 10)
    assert (np.array(out["profile"].to_list(), np.int64) == bases).all()


@gpu
@pytest.mark.parametrize("zero_based", ZB)
def test_on_cols_and_nulls(zero_based):
    df1 = _frame(zero_based, 9, 1200, 300, strand=True, null_chrom=True, null_strand=True)
    df2 = _frame(zero_based, 10, 2500, 90, strand=True, null_chrom=True, null_strand=True)
    got = pb.depth_profile(df1, df2, n_bins=8, on_cols=["strand"], output="bases", output_type="numpy.ndarray")
    bases, _ = _expected(df1, df2, zero_based, 8, on="strand")
    P.assert_profile_equal(got, bases, "on_cols")
    null = (df1["chrom"].isna() | df1["strand"].isna()).to_numpy()
    assert null.any() and (got[null] == 0).all() and (got[~null] > 0).any()
    plain = pb.depth_profile(df1, df2, n_bins=8, output="bases", output_type="numpy.ndarray")
    P.assert_profile_equal(plain, _expected(df1, df2, zero_based, 8)[0], "no on_cols")
    assert (got <= plain).all() and (got < plain).any()
    assert (plain[df1["chrom"].isna().to_numpy()] == 0).all()


def _windows_by_hand(df1, zero_based, anchor, up, down):
    """explicit windows, row by row: a minus row swaps start / end and upstream / downstream"""
    w = 0 if zero_based else 1
    ws, we = [], []
    for s, e, strand in zip(df1["start"], df1["end"], df1["strand"]):
        minus = strand == "-"
        first = int(s)
        length = max(int(e) + w - first, 0)                  # a row without positions reads as L = 0 from its start
        past = first + length
        which = anchor if not minus else {"start": "end", "end": "start", "center": "center"}[anchor]
        a = {"start": first, "end": past, "center": first + length // 2}[which]
        lo, hi = (a - down, a + up) if minus else (a - up, a + down)
        ws.append(lo)
        we.append(hi - w)
    return np.array(ws, np.int64), np.array(we, np.int64)


@gpu
@pytest.mark.parametrize("zero_based", ZB)
@pytest.mark.parametrize("anchor", ["start", "end", "center"])
def test_direction_col_and_anchors(anchor, zero_based):
    df1 = _frame(zero_based, 11, 900, 500, strand=True, odd_strand=True, null_strand=True, empty_rows=True)       # "." and null read as "+"
    assert ((df1["end"] - df1["start"]) < -1).any()                      # rows without positions are anchored at their start
    df2 = _frame(zero_based, 12, 3000, 90)
    minus = (df1["strand"] == "-").to_numpy()
    assert minus.any() and (~minus).any() and df1["strand"].isna().any() and (df1["strand"] == ".").any()
    windows = _windows_by_hand(df1, zero_based, anchor, 70, 31)
    bases, lens = _expected(df1, df2, zero_based, 20, windows=windows, reverse=minus)
    got = pb.depth_profile(df1, df2, n_bins=20, anchor=anchor, upstream=70, downstream=31, direction_col="strand", output="bases",
                           output_type="numpy.ndarray")
    P.assert_profile_equal(got, bases, anchor)
    assert (lens.sum(axis=1) == 101).all() and (got[minus] != got[minus][:, ::-1]).any()
    # without the column every row reads as "+"
    plus = pb.depth_profile(df1, df2, n_bins=20, anchor=anchor, upstream=70, downstream=31, output="bases", output_type="numpy.ndarray")
    df_plus = df1.assign(strand="+")
    df_plus.attrs.update(df1.attrs)
    P.assert_profile_equal(plus, _expected(df1, df2, zero_based, 20, windows=_windows_by_hand(df_plus, zero_based, anchor, 70, 31))[0], "no direction_col")


@gpu
def test_a_minus_gene_is_profiled_from_its_end():
    # reads pile up just past position 200; the minus gene [100, 200) has its TSS there: 10 bp downstream (inside), 30 upstream
    df1 = pd.DataFrame({"chrom": ["chr1"], "start": [100], "end": [200], "strand": ["-"]})
    df2 = pd.DataFrame({"chrom": ["chr1"] * 3, "start": [195, 220, 50], "end": [205, 230, 60]})
    for d in (df1, df2):
        d.attrs["coordinate_system_zero_based"] = True
    got = pb.depth_profile(df1, df2, n_bins=4, anchor="start", upstream=30, downstream=10, direction_col="strand", output="bases",
                           output_type="numpy.ndarray")
    # window [190, 230) in bins of 10, read from 230 down: [220,230) [210,220) [200,210) [190,200)
    assert got.tolist() == [[10, 0, 5, 5]]


@gpu
@pytest.mark.parametrize("zero_based", ZB)
def test_scale_regions_equals_mean_depth_on_the_explicit_bin_frame(zero_based):
    df1 = _frame(zero_based, 13, 700, 900)
    df2 = _frame(zero_based, 14, 3000, 90)
    mean = pb.depth_profile(df1, df2, n_bins=100, output_type="numpy.ndarray")
    c, s, e = P.explicit_bins((np.arange(len(df1)), df1["start"].to_numpy(), df1["end"].to_numpy()), 100, zero_based)
    bins = pd.DataFrame({"chrom": df1["chrom"].to_numpy()[c], "start": s, "end": e})
    bins.attrs["coordinate_system_zero_based"] = zero_based
    md = pb.mean_depth(bins, df2, output_type="pandas.DataFrame")
    exp = md["mean_depth"].to_numpy().reshape(len(df1), 100)
    assert (np.isnan(mean) == np.isnan(exp)).all() and (mean[~np.isnan(mean)] == exp[~np.isnan(exp)]).all()
    bases = pb.depth_profile(df1, df2, n_bins=100, output="bases", output_type="numpy.ndarray")
    assert (bases.reshape(-1) == md["bases"].to_numpy()).all()


@gpu
def test_pb_accessor():
    df1, df2 = _frame(True, 15, 300, 300), _frame(True, 16, 600, 80)
    res = df1.pb.depth_profile(df2, n_bins=6, output="bases")
    assert isinstance(res, pd.DataFrame)
    ref = pb.depth_profile(df1, df2, n_bins=6, output="bases", output_type="pandas.DataFrame")
    assert list(res.columns) == list(ref.columns) and (res["start"] == ref["start"]).all()
    assert [list(r) for r in res["profile"]] == [list(r) for r in ref["profile"]]
