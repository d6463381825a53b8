"""pb.depth_histogram and pb.genome_depth_histogram, the front door: export, accessor entries, argument validation (CPU); output
schema and order, fraction and its null rows, cumulative, the bare matrix, on_cols, null chroms, both coordinate systems, and
genome_depth_histogram against a genomecov table written by hand (GPU)."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
from polars_bio_amd import namespace, range_op
import _depth_hist_util as H
from test_depth_sum_frontend import _frame
from test_depth_summary_frontend import _ids

gpu = pytest.mark.gpu
MD = 6


def _expected(df1, df2, zero_based, max_depth, on=None):
    c1, c2, nc = _ids(df1, df2, on)
    probe = (c1, df1["start"].to_numpy(), df1["end"].to_numpy())
    build = (c2, df2["start"].to_numpy(), df2["end"].to_numpy())
    return H.block_form(probe, build, zero_based, nc, max_depth)


def _matrix(res):
    return np.stack([np.asarray(x) for x in res["histogram"]]) if len(res) else np.zeros((0, 0))


def test_both_are_exported():
    for name in ("depth_histogram", "genome_depth_histogram"):
        assert name in pb.__all__ and callable(getattr(pb, name)) and name in range_op.__all__
    assert namespace._ALIASES["depth_histogram"] == (range_op.depth_histogram, True)
    assert namespace._ALIASES["genome_depth_histogram"] == (range_op.genome_depth_histogram, False)


def test_argument_validation():
    df = _frame(True, 1, 10, 20, strand=True)
    with pytest.raises(AssertionError):
        pb.depth_histogram(df, df, output_type="numpy")
    with pytest.raises(AssertionError, match="interval columns"):
        pb.depth_histogram(df, df, on_cols=["start"], output_type="pandas.DataFrame")
    for bad in (0, -1, 1024, 2.0, "5", True, None):
        with pytest.raises(ValueError, match="max_depth must be an int in 1 .. 1023"):
            pb.depth_histogram(df, df, max_depth=bad, output_type="pandas.DataFrame")
        with pytest.raises(ValueError, match="max_depth must be an int in 1 .. 1023"):
            pb.genome_depth_histogram(df, max_depth=bad, output_type="pandas.DataFrame")
    with pytest.raises(ValueError, match="output must be 'bases' or 'fraction'"):
        pb.depth_histogram(df, df, output="mean", output_type="pandas.DataFrame")
    with pytest.raises(AssertionError, match="not found"):
        pb.depth_histogram(df, _frame(True, 2, 10, 20), on_cols=["strand"], output_type="pandas.DataFrame")
    with pytest.raises(pb.CoordinateSystemMismatchError):
        pb.depth_histogram(_frame(True, 1, 10, 20), _frame(False, 2, 10, 20), output_type="pandas.DataFrame")


@gpu
@pytest.mark.parametrize("zero_based", [True, False])
def test_columns_types_and_values(zero_based):
    df1 = _frame(zero_based, 3, 3000, 400, empty_rows=True)
    df2 = _frame(zero_based, 4, 4000, 90, empty_rows=True)
    exp = _expected(df1, df2, zero_based, MD)
    assert (exp[:, MD] > 0).any() and (exp.sum(axis=1) == 0).any()
    tab = pb.depth_histogram(df1, df2, max_depth=MD, output_type="pyarrow.Table")
    assert tab.column_names == ["chrom", "start", "end", "histogram"]
    assert tab.schema.field("histogram").type == pa.list_(pa.int64(), MD + 1)
    res = pb.depth_histogram(df1, df2, max_depth=MD, output_type="pandas.DataFrame")
    assert res.attrs["coordinate_system_zero_based"] == zero_based
    assert (res["start"].to_numpy() == df1["start"].to_numpy()).all() and (res["end"].to_numpy() == df1["end"].to_numpy()).all()
    assert (_matrix(res) == exp).all()
    default = pb.depth_histogram(df1, df2, output_type="pyarrow.Table")
    assert default.schema.field("histogram").type == pa.list_(pa.int64(), 101)


@gpu
def test_the_bare_matrix_and_the_identities():
    df1, df2 = _frame(True, 13, 1500, 400, empty_rows=True), _frame(True, 14, 2000, 90, empty_rows=True)
    m = pb.depth_histogram(df1, df2, max_depth=200, output_type="numpy.ndarray")
    assert isinstance(m, np.ndarray) and m.dtype == np.int64 and m.shape == (len(df1), 201) and (m[:, 200] == 0).all()
    assert (m[:, 1:].sum(axis=1) == pb.coverage(df1, df2, output_type="pandas.DataFrame")["coverage"].to_numpy()).all()
    assert ((m * np.arange(201)).sum(axis=1) == pb.mean_depth(df1, df2, output_type="pandas.DataFrame")["bases"].to_numpy()).all()
    s = pb.depth_summary(df1, df2, thresholds=(1, 2, 3), output_type="pandas.DataFrame")
    for t in (1, 2, 3):
        assert (m[:, t:].sum(axis=1) == s[f"bases_ge_{t}"].to_numpy()).all()


@gpu
def test_fraction_and_its_null_rows():
    df1, df2 = _frame(True, 21, 1200, 400, empty_rows=True), _frame(True, 22, 2000, 90)
    exp = _expected(df1, df2, True, MD)
    none = exp.sum(axis=1) == 0
    assert none.any() and not none.all()
    tab = pb.depth_histogram(df1, df2, max_depth=MD, output="fraction", output_type="pyarrow.Table")
    assert tab.schema.field("histogram").type == pa.list_(pa.float64(), MD + 1)
    flat = tab.column("histogram").combine_chunks().flatten()
    assert (np.asarray(flat.is_null()).reshape(-1, MD + 1) == none[:, None]).all()
    m = pb.depth_histogram(df1, df2, max_depth=MD, output="fraction", output_type="numpy.ndarray")
    assert m.dtype == np.float64 and np.isnan(m[none]).all()
    assert (m[~none] == exp[~none] / exp[~none].sum(axis=1, keepdims=True)).all()
    assert np.allclose(m[~none].sum(axis=1), 1.0)


@gpu
def test_cumulative_is_depth_at_least_d():
    df1, df2 = _frame(True, 23, 1200, 400, empty_rows=True), _frame(True, 24, 2000, 90)
    exp = _expected(df1, df2, True, MD)
    m = pb.depth_histogram(df1, df2, max_depth=MD, cumulative=True, output_type="numpy.ndarray")
    assert (m == np.cumsum(exp[:, ::-1], axis=1)[:, ::-1]).all() and (m[:, 0] == exp.sum(axis=1)).all()
    f = pb.depth_histogram(df1, df2, max_depth=MD, cumulative=True, output="fraction", output_type="numpy.ndarray")
    live = exp.sum(axis=1) > 0
    assert (f[live, 0] == 1.0).all() and (np.diff(f[live], axis=1) <= 0).all()


@gpu
@pytest.mark.parametrize("zero_based", [True, False])
def test_on_cols_restricts_to_the_group(zero_based):
    df1 = _frame(zero_based, 7, 2500, 300, strand=True)
    df2 = _frame(zero_based, 8, 3000, 90, strand=True)
    res = pb.depth_histogram(df1, df2, max_depth=MD, on_cols=["strand"], output_type="pandas.DataFrame")
    assert list(res.columns) == ["chrom", "start", "end", "strand", "histogram"]
    assert (_matrix(res) == _expected(df1, df2, zero_based, MD, on="strand")).all()
    both = _matrix(pb.depth_histogram(df1, df2, max_depth=MD, output_type="pandas.DataFrame"))
    assert (_matrix(res)[:, 0] >= both[:, 0]).all() and (_matrix(res)[:, 0] > both[:, 0]).any()


@gpu
def test_null_chrom_and_null_on_value_rows_receive_zeros():
    df1 = _frame(True, 9, 2000, 300, strand=True, null_chrom=True, null_strand=True)
    df2 = _frame(True, 10, 2500, 90, strand=True, null_chrom=True, null_strand=True)
    res = pb.depth_histogram(df1, df2, max_depth=MD, on_cols=["strand"], output_type="pandas.DataFrame")
    null = (df1["chrom"].isna() | df1["strand"].isna()).to_numpy()
    m = _matrix(res)
    assert null.any() and (m[null] == 0).all()
    assert (m == _expected(df1, df2, True, MD, on="strand")).all()


@gpu
def test_pb_accessor():
    df1, df2 = _frame(True, 11, 500, 300), _frame(True, 12, 600, 80)
    res = df1.pb.depth_histogram(df2, max_depth=4)
    assert isinstance(res, pd.DataFrame)
    assert (_matrix(res) == _matrix(pb.depth_histogram(df1, df2, max_depth=4, output_type="pandas.DataFrame"))).all()
    g = df2.pb.genome_depth_histogram(max_depth=4)
    assert isinstance(g, pd.DataFrame) and list(g.columns) == ["chrom", "depth", "bases"]


# ---- genome_depth_histogram against bedtools genomecov's table, by hand ----
# chr1 (length 20): [0,10) [5,15) [5,8) -> depth 1 on [0,5) and [10,15), 3 on [5,8), 2 on [8,10), 0 on [15,20)
# chr2 (length 10): [2,6) [4,6)        -> depth 1 on [2,4), 2 on [4,6), 0 elsewhere;  chr3 (length 5): untouched
GENOME = {"chr2": 10, "chr1": 20, "chr3": 5}
ROWS = [("chr1", 0, 10), ("chr2", 2, 6), ("chr1", 5, 15), ("chr1", 5, 8), ("chr2", 4, 6)]
TABLE = [("chr1", 0, 5, 20), ("chr1", 1, 10, 20), ("chr1", 2, 2, 20), ("chr1", 3, 3, 20),
         ("chr2", 0, 6, 10), ("chr2", 1, 2, 10), ("chr2", 2, 2, 10), ("chr3", 0, 5, 5),
         ("genome", 0, 16, 35), ("genome", 1, 12, 35), ("genome", 2, 4, 35), ("genome", 3, 3, 35)]
TABLE_MAX2 = [("chr1", 0, 5, 20), ("chr1", 1, 10, 20), ("chr1", 2, 5, 20), ("chr2", 0, 6, 10), ("chr2", 1, 2, 10), ("chr2", 2, 2, 10),
              ("chr3", 0, 5, 5), ("genome", 0, 16, 35), ("genome", 1, 12, 35), ("genome", 2, 7, 35)]
TABLE_NO_GENOME = [("chr1", 1, 10), ("chr1", 2, 2), ("chr1", 3, 3), ("chr2", 1, 2), ("chr2", 2, 2), ("all", 1, 12), ("all", 2, 4), ("all", 3, 3)]


def _five(zero_based, rows=ROWS, **extra):
    c, s, e = zip(*rows)
    s, e = np.array(s, np.int64), np.array(e, np.int64)
    if not zero_based:
        s = s + 1                                                # the same positions, closed and counted from 1
    df = pd.DataFrame({"chrom": np.array(c, object), "start": s, "end": e, **extra})
    df.attrs["coordinate_system_zero_based"] = zero_based
    return df


def _rows(res, cols):
    return [tuple(r) for r in res[cols].itertuples(index=False, name=None)]


@gpu
@pytest.mark.parametrize("zero_based", [True, False])
def test_genomecov_table_with_a_genome(zero_based):
    res = pb.genome_depth_histogram(_five(zero_based), genome=GENOME, output_type="pandas.DataFrame")
    assert list(res.columns) == ["chrom", "depth", "bases", "size", "fraction"]
    assert [str(res[c].dtype) for c in ("depth", "bases", "size", "fraction")] == ["int64", "int64", "int64", "float64"]
    assert _rows(res, ["chrom", "depth", "bases", "size"]) == TABLE
    assert (res["fraction"].to_numpy() == res["bases"].to_numpy() / res["size"].to_numpy()).all()
    low = pb.genome_depth_histogram(_five(zero_based), genome=GENOME, max_depth=2, output_type="pandas.DataFrame")
    assert _rows(low, ["chrom", "depth", "bases", "size"]) == TABLE_MAX2
    # the genome as a two-column frame
    frame = pd.DataFrame({"name": list(GENOME), "length": list(GENOME.values())})
    again = pb.genome_depth_histogram(_five(zero_based), genome=frame, output_type="pandas.DataFrame")
    pd.testing.assert_frame_equal(again, res)


@gpu
@pytest.mark.parametrize("zero_based", [True, False])
def test_genomecov_table_without_a_genome(zero_based):
    res = pb.genome_depth_histogram(_five(zero_based), output_type="pandas.DataFrame")
    assert list(res.columns) == ["chrom", "depth", "bases"]
    assert _rows(res, ["chrom", "depth", "bases"]) == TABLE_NO_GENOME


@gpu
def test_an_untouched_genome_contig_gets_its_depth_0_row():
    res = pb.genome_depth_histogram(_five(True), genome=GENOME, output_type="pandas.DataFrame")
    assert _rows(res[res["chrom"] == "chr3"], ["chrom", "depth", "bases", "size", "fraction"]) == [("chr3", 0, 5, 5, 1.0)]
    # rows that cover nothing touch a contig by name only
    rows = ROWS + [("chr3", 4, 4), ("chr3", 3, 1)]
    res = pb.genome_depth_histogram(_five(True, rows), genome=GENOME, output_type="pandas.DataFrame")
    assert _rows(res, ["chrom", "depth", "bases", "size"]) == TABLE


@gpu
def test_on_cols_gives_one_table_per_on_value():
    strand = np.array(["+", "-", "+", "-", "-"], object)
    res = pb.genome_depth_histogram(_five(True, strand=strand), genome=GENOME, on_cols=["strand"], output_type="pandas.DataFrame")
    assert list(res.columns) == ["chrom", "strand", "depth", "bases", "size", "fraction"]
    # "+": chr1 [0,10) [5,15); "-": chr2 [2,6) [4,6), chr1 [5,8)
    assert _rows(res, ["chrom", "strand", "depth", "bases", "size"]) == [
        ("chr1", "+", 0, 5, 20), ("chr1", "+", 1, 10, 20), ("chr1", "+", 2, 5, 20), ("chr1", "-", 0, 17, 20), ("chr1", "-", 1, 3, 20),
        ("chr2", "+", 0, 10, 10), ("chr2", "-", 0, 6, 10), ("chr2", "-", 1, 2, 10), ("chr2", "-", 2, 2, 10),
        ("chr3", "+", 0, 5, 5), ("chr3", "-", 0, 5, 5),
        ("genome", "+", 0, 20, 35), ("genome", "+", 1, 10, 35), ("genome", "+", 2, 5, 35),
        ("genome", "-", 0, 28, 35), ("genome", "-", 1, 5, 35), ("genome", "-", 2, 2, 35)]


@gpu
def test_the_three_value_errors():
    with pytest.raises(ValueError, match="genome lacks contig 'chr2'"):
        pb.genome_depth_histogram(_five(True), genome={"chr1": 20, "chr3": 5}, output_type="pandas.DataFrame")
    with pytest.raises(ValueError, match=r"df row 1 \(chr2: 2 \.\. 6\) reaches outside the contig, whose length is 5"):
        pb.genome_depth_histogram(_five(True), genome={"chr1": 20, "chr2": 5}, output_type="pandas.DataFrame")
    with pytest.raises(ValueError, match=r"df row 0 \(chr1: 0 \.\. 10\) reaches outside"):
        bad = _five(False)
        bad.loc[0, "start"] = 0                                  # a 1-based frame starts at 1
        pb.genome_depth_histogram(bad, genome=GENOME, output_type="pandas.DataFrame")
    pb.genome_depth_histogram(_five(False), genome={"chr1": 15, "chr2": 6}, output_type="pandas.DataFrame")      # [1, length] is inside
    with pytest.raises(ValueError, match="max_depth must be an int in 1 .. 1023"):
        pb.genome_depth_histogram(_five(True), genome=GENOME, max_depth=1024, output_type="pandas.DataFrame")
