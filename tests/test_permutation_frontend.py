"""pb.permutation_test end to end on the GPU: frames in, frames out.  The null table is compared with the yardstick of
tests/_permutation_util.py fed with offsets built OUTSIDE the library by the documented recipe; the summary with a numpy
recomputation from the null table."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
import _permutation_util as U

pytestmark = pytest.mark.gpu
GENOME = {"chr2": 40_000, "chr1": 90_000, "chrX": 1000, "chrUn": 123}
NAMES = sorted(GENOME)


def _frames(n1=400, n2=600, seed=0, zero_based=True):
    rng = np.random.default_rng(seed)
    chroms = np.array(["chr1", "chr2", "chrX"])
    one = 0 if zero_based else 1

    def intervals(n, max_len):
        c = chroms[rng.integers(0, 3, n)]
        L = np.array([GENOME[k] for k in c])
        ln = np.minimum(rng.integers(1, max_len, n), L)
        hs = (rng.random(n) * (L - ln + 1)).astype(np.int64)
        return c, hs + one, hs + ln
    c1, s1, e1 = intervals(n1, 700)
    c2, s2, e2 = intervals(n2, 400)
    df1 = pd.DataFrame({"chrom": c1, "start": s1, "end": e1, "strand": rng.choice(["+", "-"], n1)})
    df2 = pd.DataFrame({"chrom": c2, "start": s2, "end": e2, "strand": rng.choice(["+", "-"], n2)})
    df1.loc[3, "chrom"] = None                                 # no chrom: takes no part, no error
    df2.loc[5, "chrom"] = "chrOther"                           # a df2 contig the genome does not name
    df1.attrs["coordinate_system_zero_based"] = zero_based
    df2.attrs["coordinate_system_zero_based"] = zero_based
    return df1, df2


def _recipe(n_perm, seed):
    """The documented recipe, written out."""
    lengths = np.array([GENOME[k] for k in NAMES])
    rng = np.random.default_rng(seed)
    return rng.integers(0, lengths[None, :], size=(n_perm, len(NAMES)))


def _sides(df1, df2, keys=None):
    """The frames as the yardstick takes them: contig = position in NAMES (or the group of (chrom, keys)), -1 for a null."""
    def ids(df):
        c = df["chrom"].map({k: j for j, k in enumerate(NAMES)}).fillna(-1).astype(np.int64).to_numpy()
        if keys:
            k = df[keys[0]].map({"+": 0, "-": 1}).fillna(-1).astype(np.int64).to_numpy()
            c = np.where((c >= 0) & (k >= 0), 2 * c + k, -1)
        return c.astype(np.int32)
    side = lambda df: (ids(df), df["start"].to_numpy().astype(np.int32), df["end"].to_numpy().astype(np.int32))
    return side(df1), side(df2)


def _expected(df1, df2, off, zero_based, keys=None):
    probe, build = _sides(df1, df2, keys)
    lengths = np.array([GENOME[k] for k in NAMES])
    if keys:                                                   # a group takes its chrom's length and offset
        lengths, off = np.repeat(lengths, 2), np.repeat(off, 2, axis=1)
    return U.expected(probe, build, len(lengths), zero_based, lengths, off)


@pytest.mark.parametrize("zero_based", [True, False], ids=["zero_based", "one_based"])
def test_null_table_follows_the_documented_recipe(zero_based):
    df1, df2 = _frames(zero_based=zero_based)
    null = pb.permutation_test(df1, df2, GENOME, n_perm=40, seed=7, output="null", output_type="pandas.DataFrame")
    assert list(null.columns) == ["permutation", "n_pairs", "n_rows"] and null["permutation"].tolist() == list(range(40))
    pairs, rows = _expected(df1, df2, _recipe(40, 7), zero_based)
    assert null["n_pairs"].tolist() == pairs.tolist() and null["n_rows"].tolist() == rows.tolist() and pairs.sum() > 0
    other = pb.permutation_test(df1, df2, GENOME, n_perm=40, seed=8, output="null", output_type="pandas.DataFrame")
    assert other["n_pairs"].tolist() != pairs.tolist()


def test_genome_as_a_frame_offsets_override_and_arrow():
    df1, df2 = _frames(seed=2)
    off = _recipe(12, 99)[::-1].copy()
    exp = _expected(df1, df2, off, True)
    genome = pd.DataFrame({"contig": list(GENOME), "length": list(GENOME.values())})
    for g in (genome, pa.Table.from_pandas(genome), GENOME):
        null = pb.permutation_test(df1, df2, g, offsets=off, seed=5, n_perm=3, output="null", output_type="pandas.DataFrame")
        assert null["n_pairs"].tolist() == exp[0].tolist() and null["n_rows"].tolist() == exp[1].tolist()
    t1, t2 = (pb.set_coordinate_system(pa.Table.from_pandas(df, preserve_index=False), True) for df in (df1, df2))
    null = pb.permutation_test(t1, t2, GENOME, offsets=off, output="null", output_type="pyarrow.Table")
    assert isinstance(null, pa.Table) and null.column("n_pairs").to_pylist() == exp[0].tolist()


def test_on_cols_strand():
    df1, df2 = _frames(seed=3)
    df1.loc[7, "strand"] = None                                # a null on-value: takes no part
    null = pb.permutation_test(df1, df2, GENOME, n_perm=25, seed=1, on_cols=["strand"], output="null", output_type="pandas.DataFrame")
    pairs, rows = _expected(df1, df2, _recipe(25, 1), True, keys=["strand"])
    assert null["n_pairs"].tolist() == pairs.tolist() and null["n_rows"].tolist() == rows.tolist()
    plain = _expected(df1, df2, _recipe(25, 1), True)
    assert pairs.sum() < plain[0].sum()


@pytest.mark.parametrize("n_perm", [1, 30])
def test_summary_against_numpy(n_perm):
    df1, df2 = _frames(seed=4)
    kw = dict(n_perm=n_perm, seed=11, output_type="pandas.DataFrame")
    null = pb.permutation_test(df1, df2, GENOME, output="null", **kw)
    summary = pb.permutation_test(df1, df2, GENOME, **kw)
    assert list(summary.columns) == ["statistic", "observed", "n_perm", "null_mean", "null_sd", "z_score", "p_greater", "p_less"]
    assert summary["statistic"].tolist() == ["n_pairs", "n_rows"] and summary["n_perm"].tolist() == [n_perm] * 2
    observed = _expected(df1, df2, np.zeros((1, len(NAMES)), np.int64), True)
    counts = pb.count_overlaps(df1, df2, output_type="pandas.DataFrame")["count"].to_numpy()
    assert observed[0][0] == counts.sum() and observed[1][0] == (counts > 0).sum()
    for k, stat in enumerate(("n_pairs", "n_rows")):
        row, v = summary.iloc[k], null[stat].to_numpy().astype(np.float64)
        obs = int(observed[k][0])
        assert row["observed"] == obs and row["null_mean"] == v.mean()
        assert row["p_greater"] == (1 + (v >= obs).sum()) / (n_perm + 1) and row["p_less"] == (1 + (v <= obs).sum()) / (n_perm + 1)
        if n_perm < 2:
            assert pd.isna(row["null_sd"]) and pd.isna(row["z_score"])
        else:
            sd = v.std(ddof=1)
            assert row["null_sd"] == sd and sd > 0 and row["z_score"] == (obs - v.mean()) / sd


def test_zero_sd_has_no_z_score_and_errors_reach_the_user():
    df1 = pd.DataFrame({"chrom": ["chrUn"], "start": [0], "end": [123]})          # covers its contig: every shift matches the same
    df2 = pd.DataFrame({"chrom": ["chrUn", "chrUn"], "start": [5, 100], "end": [9, 123]})
    for df in (df1, df2):
        df.attrs["coordinate_system_zero_based"] = True
    s = pb.permutation_test(df1, df2, GENOME, n_perm=5, output_type="pandas.DataFrame")
    # (n_pairs varies: a shift that cuts df1 inside a df2 row counts that row twice)
    assert s["observed"].tolist() == [2, 1] and s["null_sd"][1] == 0.0 and pd.isna(s["z_score"][1])
    assert s["p_greater"][1] == 1.0 and s["p_less"][1] == 1.0 and s["null_mean"][1] == 1.0
    with pytest.raises(ValueError, match="not in genome"):
        pb.permutation_test(df1, df2, {"chr1": 5}, output_type="pandas.DataFrame")
    with pytest.raises(ValueError, match="df1 row 0"):
        pb.permutation_test(df1, df2, {"chrUn": 122}, output_type="pandas.DataFrame")


def test_pb_accessor():
    df1, df2 = _frames(seed=6)
    a = df1.pb.permutation_test(df2, genome=GENOME, n_perm=9, seed=3, output="null")
    b = pb.permutation_test(df1, df2, GENOME, n_perm=9, seed=3, output="null", output_type="pandas.DataFrame")
    assert isinstance(a, pd.DataFrame) and a.equals(b) and a["n_pairs"].sum() > 0
