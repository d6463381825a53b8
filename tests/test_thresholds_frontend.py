"""pb.overlap / pb.count_overlaps with min_overlap, min_frac1, min_frac2 through the front door on the GPU, against the brute force
of tests/_thresholds_util.py evaluated on the same tables."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
import _thresholds_util as T
from _util import GOLDEN

pytestmark = pytest.mark.gpu

COLS = ("contig", "pos_start", "pos_end")


def _csv(name, zero_based):
    df = pd.read_csv(f"{GOLDEN}/overlap/{name}.csv")
    df.attrs["coordinate_system_zero_based"] = zero_based
    return df


def _sides(df1, df2, cols=COLS, on=None):
    """Both frames as (contig id, start, end) over one dictionary of (chrom, on values)."""
    def key(df):
        k = df[cols[0]].astype(str)
        for c in on or ():
            k = k + "\x00" + df[c].astype(str)
        return k
    k1, k2 = key(df1), key(df2)
    ids = {v: i for i, v in enumerate(sorted(set(k1) | set(k2)))}
    side = lambda df, k: (k.map(ids).to_numpy(np.int32), df[cols[1]].to_numpy(np.int32), df[cols[2]].to_numpy(np.int32))
    return side(df1, k1), side(df2, k2), len(ids)


def _expected_join(df1, df2, zero_based, cols=COLS, on=None, **thr):
    probe, build, nc = _sides(df1, df2, cols, on)
    p, b, cnt = T.brute(probe, build, nc, zero_based, **thr)
    left = df1.iloc[p].reset_index(drop=True).add_suffix("_1")
    right = df2.iloc[b].reset_index(drop=True).add_suffix("_2")
    return pd.concat([left, right], axis=1), p, cnt


def _sorted(df):
    return df.sort_values(by=list(df.columns)).reset_index(drop=True)


def _random_frames(seed=5, n1=400, n2=500, zero_based=True):
    rng = np.random.default_rng(seed)
    def frame(n, max_len):
        s = rng.integers(0, 3000, n)
        df = pd.DataFrame({"chrom": rng.choice(["chr1", "chr2", "chrX"], n), "start": s, "end": s + rng.integers(0, max_len, n),
                           "strand": rng.choice(["+", "-"], n), "score": rng.integers(0, 100, n)})
        df.attrs["coordinate_system_zero_based"] = zero_based
        return df
    return frame(n1, 150), frame(n2, 250)


@pytest.mark.parametrize("zero_based", [False, True])
def test_golden_tables(zero_based):
    df1, df2 = _csv("reads", zero_based), _csv("targets", zero_based)
    res = pb.overlap(df1, df2, cols1=COLS, cols2=COLS, output_type="pandas.DataFrame", min_frac1=0.5, min_frac2=0.5)
    exp, _, _ = _expected_join(df1, df2, zero_based, min_frac1=0.5, min_frac2=0.5)
    plain = pb.overlap(df1, df2, cols1=COLS, cols2=COLS, output_type="pandas.DataFrame")
    assert 0 < len(exp) < len(plain)
    pd.testing.assert_frame_equal(_sorted(res), _sorted(exp), check_dtype=False)
    assert res.attrs["coordinate_system_zero_based"] is zero_based
    for mo in (1, 30, 60, 10_000):
        cnt = pb.count_overlaps(df1, df2, cols1=COLS, cols2=COLS, output_type="pandas.DataFrame", min_overlap=mo)
        _, _, ecnt = _expected_join(df1, df2, zero_based, min_overlap=mo)
        assert list(cnt.columns) == list(df1.columns) + ["count"] and (cnt["count"].to_numpy() == ecnt).all(), mo
        assert (ecnt.sum() == 0) == (mo == 10_000)


def test_on_cols_strand():
    df1, df2 = _random_frames()
    cols = ("chrom", "start", "end")
    res = pb.overlap(df1, df2, on_cols=["strand"], output_type="pandas.DataFrame", min_overlap=20, min_frac2=0.25)
    exp, _, ecnt = _expected_join(df1, df2, True, cols, on=["strand"], min_overlap=20, min_frac2=0.25)
    assert len(exp) > 50 and (res["strand_1"] == res["strand_2"]).all()
    pd.testing.assert_frame_equal(_sorted(res[exp.columns]), _sorted(exp), check_dtype=False)
    cnt = pb.count_overlaps(df1, df2, on_cols=["strand"], output_type="pandas.DataFrame", min_overlap=20, min_frac2=0.25)
    assert (cnt["count"].to_numpy() == ecnt).all()


def test_left_distinct_limit_and_output_types():
    df1, df2 = _random_frames(seed=6)
    cols = ("chrom", "start", "end")
    kw = dict(min_frac1=0.6)
    exp, p, _ = _expected_join(df1, df2, True, cols, **kw)
    left = pb.overlap(df1, df2, overlap_output="left", distinct_output=True, output_type="pandas.DataFrame", **kw)
    assert 0 < len(left) == len(np.unique(p)) < len(p)
    pd.testing.assert_frame_equal(_sorted(left), _sorted(df1.iloc[np.unique(p)].reset_index(drop=True)), check_dtype=False)
    head = pb.overlap(df1, df2, output_type="pandas.DataFrame", limit=3, **kw)
    assert len(head) == 3 and len(pd.merge(head, exp.drop_duplicates(), how="inner", on=list(exp.columns))) == 3
    tab = pb.overlap(df1, df2, output_type="pyarrow.Table", **kw)
    assert isinstance(tab, pa.Table) and tab.num_rows == len(exp)
    reader = pb.overlap(df1, df2, output_type="pyarrow.RecordBatchReader", **kw)
    assert isinstance(reader, pa.RecordBatchReader)
    got = reader.read_all()
    assert got.num_rows == len(exp) and got.column_names == tab.column_names
    pd.testing.assert_frame_equal(_sorted(got.to_pandas()), _sorted(exp), check_dtype=False)
    cnt_reader = pb.count_overlaps(df1, df2, output_type="pyarrow.RecordBatchReader", limit=7, min_overlap=5)
    assert cnt_reader.read_all().num_rows == 7


def test_one_based_metadata():
    df1, df2 = _random_frames(seed=7, zero_based=False)
    cols = ("chrom", "start", "end")
    res = pb.overlap(df1, df2, output_type="pandas.DataFrame", min_overlap=10, min_frac1=0.3)
    exp, _, _ = _expected_join(df1, df2, False, cols, min_overlap=10, min_frac1=0.3)
    exp0, _, _ = _expected_join(df1, df2, True, cols, min_overlap=10, min_frac1=0.3)
    assert len(exp) > len(exp0) > 0                        # the closed frame counts one more base per pair
    pd.testing.assert_frame_equal(_sorted(res), _sorted(exp), check_dtype=False)
    assert res.attrs["coordinate_system_zero_based"] is False


def test_count_is_the_group_by_of_overlap_and_thresholds_are_monotone():
    df1, df2 = _random_frames(seed=8)
    def pairs(**kw):
        r = pb.overlap(df1.assign(row=np.arange(len(df1))), df2.assign(row=np.arange(len(df2))), output_type="pandas.DataFrame", **kw)
        return set(zip(r["row_1"], r["row_2"]))
    ladder = [dict(min_overlap=1), dict(min_overlap=15), dict(min_overlap=15, min_frac1=0.2), dict(min_overlap=15, min_frac1=0.5),
              dict(min_overlap=15, min_frac1=0.5, min_frac2=0.1), dict(min_overlap=40, min_frac1=0.5, min_frac2=0.4),
              dict(min_overlap=40, min_frac1=1.0, min_frac2=0.4)]
    prev = None
    for kw in ladder:
        got = pairs(**kw)
        cnt = pb.count_overlaps(df1, df2, output_type="pandas.DataFrame", **kw)["count"].to_numpy()
        by_row = np.bincount(np.array([p for p, _ in got], np.int64), minlength=len(df1))
        assert (cnt == by_row).all(), kw
        assert prev is None or got <= prev, f"raising a threshold added a pair: {kw}"
        prev = got
    assert len(prev) > 0
    plain = pb.overlap(df1, df2, output_type="pandas.DataFrame")
    assert len(pairs(min_overlap=1)) <= len(plain)
