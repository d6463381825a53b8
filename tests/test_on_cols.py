"""on_cols (joins keyed on extra columns such as strand) on the CPU: argument checks, the host group-id entry
ivj_host_group_ids against a numpy restatement of its numbering rule, and the front door's per-op semantics with the engine
replaced by the oracle-backed test double (the GPU runs of the same checks: tests/test_on_cols_gpu.py)."""
import numpy as np
import pandas as pd
import pytest

import polars_bio_amd as pb
from polars_bio_amd import _host as H, range_op
from _util import OracleEngine
import _on_cols_util as U


@pytest.fixture
def oracle_engine(monkeypatch):
    monkeypatch.setattr(range_op, "default_engine", lambda: OracleEngine())


def _frame(d):
    df = pd.DataFrame(d)
    df.attrs["coordinate_system_zero_based"] = True
    return df


# ---- validation -------------------------------------------------------------------------------------------------------

def test_absent_or_interval_on_col_is_refused(oracle_engine):
    a = _frame({"chrom": ["chr1"], "start": [1], "end": [5], "strand": ["+"]})
    b = _frame({"chrom": ["chr1"], "start": [2], "end": [6]})
    for op in (pb.overlap, pb.nearest, pb.count_overlaps, pb.coverage):
        with pytest.raises(AssertionError):
            op(a, b, on_cols=["strand"], output_type="pandas.DataFrame")       # absent from df2
        with pytest.raises(AssertionError):
            op(a, a, on_cols=["chrom"], output_type="pandas.DataFrame")
        with pytest.raises(AssertionError):
            op(a, a, on_cols=["strand", "end"], output_type="pandas.DataFrame")
    with pytest.raises(AssertionError):
        pb.merge(b, on_cols=["strand"], output_type="pandas.DataFrame")
    with pytest.raises(AssertionError):
        pb.overlap_batches(a, b, on_cols=["strand"]).__next__()


def test_empty_on_cols_is_none(oracle_engine):
    df1, df2 = U.pair_frames(3)
    for op in (pb.overlap, pb.count_overlaps, pb.nearest, pb.coverage):
        pd.testing.assert_frame_equal(op(df1, df2, on_cols=[], output_type="pandas.DataFrame"), op(df1, df2, output_type="pandas.DataFrame"))
    pd.testing.assert_frame_equal(pb.merge(df1, on_cols=[], output_type="pandas.DataFrame"), pb.merge(df1, output_type="pandas.DataFrame"))


def test_oversized_key_space_is_a_value_error(oracle_engine):
    n = 1400
    d = {"chrom": ["chr1"] * n, "start": np.arange(n), "end": np.arange(n) + 1, "a": np.arange(n), "b": np.arange(n), "c": np.arange(n)}
    df = _frame(d)
    with pytest.raises(ValueError, match="1400"):
        pb.overlap(df, df, on_cols=["a", "b", "c"], output_type="pandas.DataFrame")      # 1400^3 > 2^31 keys
    with pytest.raises(ValueError, match="2\\^31"):
        pb.merge(df, on_cols=["a", "b", "c"], output_type="pandas.DataFrame")
    with pytest.raises(pb.range_op.EngineError, match="exceeds 2\\^31"):
        z = np.zeros(1, np.int32)
        H.group_ids(z, [z, z], z, [z, z], [1 << 16, 1 << 16], 1)


def test_on_col_types_that_cannot_be_unified_are_a_value_error(oracle_engine):
    a = _frame({"chrom": ["chr1"], "start": [1], "end": [5], "g": ["x"]})
    b = _frame({"chrom": ["chr1"], "start": [2], "end": [6], "g": [1]})
    with pytest.raises(ValueError, match="'g'"):
        pb.overlap(a, b, on_cols=["g"], output_type="pandas.DataFrame")


# ---- ivj_host_group_ids == numpy restatement ----------------------------------------------------------------------------

def numpy_group_ids(pc, pcodes, bc, bcodes, cards, n_contigs):
    """The numbering rule restated: np.unique over the build keys, searchsorted for both sides."""
    def keys(c, codes):
        k = c.astype(np.int64)
        ok = (c >= 0) & (c < n_contigs)
        for v, card in zip(codes, cards):
            ok &= (v >= 0) & (v < card)
            k = k * card + v
        return np.where(ok, k, -1)
    bk, pk = keys(bc, bcodes), keys(pc, pcodes)
    u = np.unique(bk[bk >= 0])

    def gid(k):
        if len(u) == 0:
            return np.full(len(k), -1, np.int32)
        i = np.searchsorted(u, k)
        hit = (k >= 0) & (u[np.minimum(i, len(u) - 1)] == k)
        return np.where(hit, i, -1).astype(np.int32)
    table = np.empty((len(u), 1 + len(cards)), np.int32)
    rem = u.copy()
    for j in range(len(cards) - 1, -1, -1):
        table[:, 1 + j] = rem % cards[j]
        rem //= cards[j]
    table[:, 0] = rem
    return gid(pk), gid(bk), len(u), table


# (n_contigs, cards) with D = 1, 32, 33 and about 2^20, for K = 1 and 2
DOMAINS = [(1, [1]), (1, [1, 1]), (1, [32]), (2, [4, 4]), (3, [11]), (1, [3, 11]), (24, [43690]), (24, [2, 21845])]


def random_keys(rng, n_probe, n_build, cards, n_contigs, null_frac=0.05):
    pc = rng.integers(0, n_contigs + 1, n_probe).astype(np.int32)           # n_contigs: a chrom df2 lacks
    bc = rng.integers(0, n_contigs, n_build).astype(np.int32)
    pc[rng.random(n_probe) < null_frac] = -1
    bc[rng.random(n_build) < null_frac] = -1
    pcodes = [rng.integers(-1, c + 1, n_probe).astype(np.int32) for c in cards]   # -1 null, c: unseen in df2
    bcodes = [rng.integers(0, c, n_build).astype(np.int32) for c in cards]
    for b in bcodes:
        b[rng.random(n_build) < null_frac] = -1
    return pc, pcodes, bc, bcodes


@pytest.mark.parametrize("n_contigs,cards", DOMAINS)
@pytest.mark.parametrize("n_probe,n_build", [(0, 0), (1, 1), (5000, 700), (300_000, 200_000)])
def test_host_group_ids_equal_the_numpy_restatement(n_contigs, cards, n_probe, n_build):
    rng = np.random.default_rng(n_contigs * 1000 + len(cards) * 100 + n_build % 97)
    pc, pcodes, bc, bcodes = random_keys(rng, n_probe, n_build, cards, n_contigs)
    pg, bg, g, table = H.group_ids(pc, pcodes, bc, bcodes, cards, n_contigs)
    epg, ebg, eg, etable = numpy_group_ids(pc, pcodes, bc, bcodes, cards, n_contigs)
    assert g == eg
    assert (pg == epg).all() and (bg == ebg).all()
    assert table.shape == etable.shape and (table == etable).all()


# ---- front-door semantics with the oracle-backed engine ----------------------------------------------------------------

@pytest.mark.parametrize("on_cols", [["strand"], ["strand", "sample"]])
def test_front_door_equals_the_per_group_decomposition(oracle_engine, on_cols):
    df1, df2 = U.pair_frames(7)
    U.check_ops(df1, df2, on_cols, outputs=("pandas.DataFrame", "pyarrow.Table", "pyarrow.RecordBatchReader"), batch_rows=(53, 10_000))


def test_integer_and_categorical_on_cols(oracle_engine):
    df1, df2 = U.pair_frames(11)
    df1 = df1.assign(strand=df1["strand"].astype("category"), sample=df1["sample"].map({"s0": 0, "s1": 1, "s2": 2, "s3": 3}).astype(np.int64))
    df2 = df2.assign(sample=df2["sample"].map({"s0": 0, "s1": 1, "s2": 2, "s3": 3}).astype(np.int32))
    for d in (df1, df2):
        d.attrs["coordinate_system_zero_based"] = True
    ep, eb = U.expected_pairs(df1, df2, ["strand", "sample"])
    gp, gb = U.got_pairs(pb.overlap(df1, df2, on_cols=["strand", "sample"], output_type="pandas.DataFrame"))
    assert (gp == ep).all() and (gb == eb).all()
    m = pb.merge(df1, on_cols=["sample"], output_type="pandas.DataFrame")
    assert [tuple(r) for r in m.itertuples(index=False, name=None)] == U.expected_merge(df1, ["sample"])


def test_accessor_forwards_on_cols(oracle_engine):
    df1, df2 = U.pair_frames(5)
    got = df1.pb.overlap(df2, on_cols=["strand"], output_type="pandas.DataFrame")
    ep, eb = U.expected_pairs(df1, df2, ["strand"])
    gp, gb = U.got_pairs(got)
    assert (gp == ep).all() and (gb == eb).all()
