"""pb.depth, the front door: input kinds, output schema and order, null chroms, on_cols, both coordinate systems, the .pb
accessor (GPU), and the refusal of an alignment-file path (CPU)."""
import pathlib

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
import _depth_util as U

gpu = pytest.mark.gpu


def test_a_path_argument_is_refused():
    for arg in ("reads.bam", b"reads.cram"):
        with pytest.raises(ValueError, match="interval frame"):
            pb.depth(arg)
    with pytest.raises(ValueError, match="alignment files"):
        pb.depth(pathlib.Path("reads.bam"))


def test_depth_is_exported():
    assert "depth" in pb.__all__ and callable(pb.depth)


def _frame(zero_based, seed=3, n=4000, nulls=False, strand=False):
    rng = np.random.default_rng(seed)
    names = np.array(["chr10", "chr2", "chrX", "chr1"])
    c, s, e = U.random_rows(rng, n, len(names), 1500, max_len=90)
    d = {"chrom": names[c].astype(object), "start": s.astype(np.int64), "end": e.astype(np.int64)}
    if strand:
        d["strand"] = np.array(["+", "-"])[rng.integers(0, 2, n)]
    if nulls:
        d["chrom"][rng.integers(0, n, n // 10)] = None
    df = pd.DataFrame(d)
    df.attrs["coordinate_system_zero_based"] = zero_based
    return df


def _expected_frame(df, zero_based, cols=("chrom", "start", "end")):
    """event form on the frame's rows; chrom ids in sorted-name order, as the front door numbers them"""
    d = df[df[cols[0]].notna()]
    names = np.array(sorted(d[cols[0]].unique()))
    ids = np.searchsorted(names, d[cols[0]].to_numpy().astype(str))
    c, s, e, dep = U.depth_events(ids, d[cols[1]].to_numpy(), d[cols[2]].to_numpy(), zero_based, len(names))
    return pd.DataFrame({cols[0]: names[c].astype(object), cols[1]: s, cols[2]: e, "coverage": dep})


@gpu
@pytest.mark.parametrize("zero_based", [True, False])
def test_pandas_frame_schema_order_and_values(zero_based):
    df = _frame(zero_based)
    res = pb.depth(df, output_type="pandas.DataFrame")
    assert list(res.columns) == ["chrom", "start", "end", "coverage"]
    assert [str(t) for t in res.dtypes[1:]] == ["int64"] * 3
    assert res.attrs["coordinate_system_zero_based"] == zero_based
    exp = _expected_frame(df, zero_based)
    pd.testing.assert_frame_equal(res.reset_index(drop=True).astype({"chrom": object}), exp, check_dtype=False)
    # (chrom, start) order, chroms in sorted-name order
    key = list(zip(res["chrom"], res["start"]))
    assert key == sorted(key)


@gpu
def test_pyarrow_table_and_custom_column_names():
    df = _frame(True, seed=4).rename(columns={"chrom": "contig", "start": "pos_start", "end": "pos_end"})
    t = pa.Table.from_pandas(df, preserve_index=False).replace_schema_metadata({"coordinate_system_zero_based": "true"})
    cols = ["contig", "pos_start", "pos_end"]
    res = pb.depth(t, cols=cols, output_type="pandas.DataFrame")
    assert list(res.columns) == cols + ["coverage"]
    pd.testing.assert_frame_equal(res.reset_index(drop=True).astype({"contig": object}), _expected_frame(df, True, cols), check_dtype=False)


@gpu
def test_rows_with_a_null_chrom_are_dropped():
    df = _frame(True, seed=5, nulls=True)
    assert df["chrom"].isna().any()
    res = pb.depth(df, output_type="pandas.DataFrame")
    pd.testing.assert_frame_equal(res.reset_index(drop=True).astype({"chrom": object}), _expected_frame(df, True), check_dtype=False)


@gpu
@pytest.mark.parametrize("zero_based", [True, False])
def test_on_cols_equals_every_strand_on_its_own(zero_based):
    df = _frame(zero_based, seed=6, strand=True)
    res = pb.depth(df, on_cols=["strand"], output_type="pandas.DataFrame")
    assert list(res.columns) == ["chrom", "start", "end", "strand", "coverage"]
    parts = []
    for strand in ("+", "-"):
        sub = df[df["strand"] == strand].drop(columns=["strand"])
        sub.attrs["coordinate_system_zero_based"] = zero_based
        one = pb.depth(sub, output_type="pandas.DataFrame")
        one.insert(3, "strand", strand)
        parts.append(one)
    exp = pd.concat(parts).sort_values(["chrom", "strand", "start"], kind="stable").reset_index(drop=True)
    pd.testing.assert_frame_equal(res.reset_index(drop=True).astype({"chrom": object, "strand": object}),
                                  exp.astype({"chrom": object, "strand": object}), check_dtype=False)
    # and every strand on its own equals the event form
    plus = df[df["strand"] == "+"]
    pd.testing.assert_frame_equal(parts[0].drop(columns=["strand"]).reset_index(drop=True).astype({"chrom": object}),
                                  _expected_frame(plus, zero_based), check_dtype=False)


@gpu
def test_blocks_feed_back_into_coverage():
    df = _frame(True, seed=7, n=800)
    blocks = pb.depth(df, output_type="pandas.DataFrame")
    assert blocks.attrs["coordinate_system_zero_based"] is True
    b3 = blocks[["chrom", "start", "end"]].copy()
    b3.attrs["coordinate_system_zero_based"] = True
    cov = pb.coverage(b3, df, output_type="pandas.DataFrame")
    assert (cov["coverage"].to_numpy() == (blocks["end"] - blocks["start"]).to_numpy()).all()      # every block is wholly covered


@gpu
def test_pb_accessor():
    df = _frame(True, seed=8, n=500)
    res = df.pb.depth()
    assert isinstance(res, pd.DataFrame) and list(res.columns) == ["chrom", "start", "end", "coverage"]
    pd.testing.assert_frame_equal(res, pb.depth(df, output_type="pandas.DataFrame"))
