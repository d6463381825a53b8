"""Directional nearest at the front door: ``pb.nearest(..., ignore_upstream, ignore_downstream, direction_col)``.

The expected rows come from the oracle's ordered candidate lists with a PER-ROW mask (tests/_nearest_direction_util.py): a df1 row
whose direction value is the string "-" has upstream and downstream swapped, every other value reads as "+"."""
import ctypes

import numpy as np
import pandas as pd
import pytest

import polars_bio_amd as pb
from polars_bio_amd import _engine, range_op
from _nearest_direction_util import IGNORE_LEFT, IGNORE_RIGHT, directed, full_lists
from _util import OracleEngine, _OracleStream


class _DirectedStream(_OracleStream):
    """The oracle-backed session double with a direction mask: the mask in force at submit answers the batch."""

    def __init__(self, *a, nearest_ignore=0):
        super().__init__(*a)
        self.ignore = nearest_ignore

    def set_nearest_ignore(self, mask):
        self.ignore = mask

    def _answer(self, batch):
        out = super()._answer(batch)
        if self.op == 2:
            lists = full_lists(batch, (self.ix.build.contig, self.ix.build.start, self.ix.build.end), self.strict, self.inc)
            out["build_idx"], out["dist"], out["n_found"] = directed(lists, self.ignore, self.k)
        return out


class _DirectedOracleEngine(OracleEngine):
    """Engine double of the CPU runs: the front door's own work (orientation split, scatter back, sub-batches) against oracle answers."""
    calls = []

    def nearest(self, probe, build, strict, n_contigs, k=1, include_overlaps=True, nearest_ignore=0):
        _DirectedOracleEngine.calls.append((len(probe[0]), nearest_ignore))
        return directed(full_lists(probe, build, strict, include_overlaps), nearest_ignore, k)

    def probe_stream(self, build, strict, n_contigs, op=0, max_batch_rows=8_000_000, k=1, include_overlaps=True, partition_mode=0, copy=True,
                     nearest_ignore=0):
        return _DirectedStream(build, strict, n_contigs, op, k, include_overlaps, nearest_ignore=nearest_ignore)


@pytest.fixture(params=["cpu", pytest.param("gpu", marks=pytest.mark.gpu)])
def engine(request, monkeypatch):
    if request.param == "cpu":
        _DirectedOracleEngine.calls = []
        monkeypatch.setattr(range_op, "default_engine", lambda: _DirectedOracleEngine())
    return request.param


def _frame(d, zero_based=True):
    df = pd.DataFrame(d)
    df.attrs["coordinate_system_zero_based"] = zero_based
    return df


# ---- CPU -----------------------------------------------------------------------------------------------------------------------

def test_missing_direction_col_is_a_value_error():
    df1 = _frame({"chrom": ["chr1"], "start": [100], "end": [110], "strand": ["+"]})
    df2 = _frame({"chrom": ["chr1"], "start": [50], "end": [60]})
    for out in ("pandas.DataFrame", "pyarrow.RecordBatchReader", "polars.LazyFrame"):
        with pytest.raises(ValueError, match="direction_col"):
            pb.nearest(df1, df2, ignore_upstream=True, direction_col="orientation", output_type=out)
    with pytest.raises(ValueError, match="direction_col"):
        pb.nearest(df1, df2, direction_col="orientation", output_type="pandas.DataFrame")      # checked even when no flag is set
    with pytest.raises(ValueError, match="direction_col"):
        pb.nearest_batches(df1, df2, ignore_downstream=True, direction_col="orientation")


def test_abi_6_and_the_opts_layout():
    assert ctypes.sizeof(_engine._Opts) == 40
    assert _engine.load_library().ivj_abi_version() == 6 == _engine.ABI_VERSION
    assert "ivj_stream_set_nearest_ignore" in _engine.ABI_SYMBOLS


def test_make_opts_round_trips_the_mask():
    for m in (0, 1, 2, 3):
        assert _engine.make_opts(True, 3, nearest_ignore=m).nearest_ignore == m
    assert _engine.make_opts(True, 3).nearest_ignore == 0
    with pytest.raises(ValueError):
        _engine.make_opts(True, 3, nearest_ignore=4)


def test_new_keywords_are_keyword_only():
    import inspect
    for fn in (pb.nearest, pb.nearest_batches):
        p = inspect.signature(fn).parameters
        assert all(p[n].kind is inspect.Parameter.KEYWORD_ONLY for n in ("ignore_upstream", "ignore_downstream", "direction_col"))


# ---- GPU: the case one checks by hand ------------------------------------------------------------------------------------------

def _hand():
    df1 = _frame({"chrom": ["chr1", "chr1"], "start": [100, 100], "end": [110, 110], "strand": ["+", "-"]})
    df2 = _frame({"chrom": ["chr1", "chr1"], "start": [50, 150], "end": [60, 170]})
    return df1, df2


def _by_strand(res):
    res = res.sort_values("strand_1").reset_index(drop=True)           # "+" < "-"
    return [(None if pd.isna(s) else int(s), None if pd.isna(e) else int(e), None if pd.isna(d) else int(d))
            for s, e, d in zip(res["start_2"], res["end_2"], res["distance"])]


@pytest.mark.parametrize("output_type", ["pandas.DataFrame", "pyarrow.RecordBatchReader"])
def test_hand_checked_case(engine, output_type):
    df1, df2 = _hand()

    def run(**kw):
        res = pb.nearest(df1, df2, output_type=output_type, direction_col="strand", **kw)
        return _by_strand(res if output_type == "pandas.DataFrame" else res.read_all().to_pandas())
    assert run(ignore_upstream=True) == [(150, 170, 40), (50, 60, 40)]           # "+": downstream = higher coordinates; "-": lower
    assert run(ignore_downstream=True) == [(50, 60, 40), (150, 170, 40)]
    assert run(ignore_upstream=True, ignore_downstream=True) == [(None, None, None)] * 2
    assert run() == [(50, 60, 40), (50, 60, 40)]                                 # undirected: the left row wins the tie on both
    # without a direction column every row is "+"
    res = pb.nearest(df1, df2, output_type="pandas.DataFrame", ignore_upstream=True)
    assert _by_strand(res) == [(150, 170, 40), (150, 170, 40)]


# ---- GPU: 2000 x 300 with mixed strands ------------------------------------------------------------------------------------------

CHROMS = ["chr1", "chr2", "chr3"]
STRANDS = ["+", "-", "."]


def _frames():
    rng = np.random.default_rng(77)
    n1, n2 = 2000, 300
    s1 = rng.integers(0, 30000, n1)
    strand1 = rng.choice(np.array(["+", "-", ".", None], dtype=object), n1, p=[0.4, 0.4, 0.1, 0.1])
    df1 = _frame({"chrom": rng.choice(CHROMS + ["chr9"], n1), "start": s1, "end": s1 + rng.integers(1, 200, n1), "strand": strand1,
                  "id": np.arange(n1)})
    s2 = rng.integers(0, 30000, n2)
    df2 = _frame({"chrom": rng.choice(CHROMS, n2), "start": s2, "end": s2 + rng.integers(1, 400, n2), "strand": rng.choice(STRANDS, n2),
                  "id": np.arange(n2)})
    return df1, df2


DF1, DF2 = _frames()


def _ids(df, on_strand, probe):
    """contig ids of the oracle call: the chrom, or the (chrom, strand) group; a df1 row df2 cannot match gets -1."""
    chrom = df["chrom"].map({c: i for i, c in enumerate(CHROMS)}).fillna(-1).to_numpy().astype(np.int64)
    if not on_strand:
        return chrom.astype(np.int32)
    strand = df["strand"].map({s: i for i, s in enumerate(STRANDS)}).fillna(-1).to_numpy().astype(np.int64)
    return np.where((chrom < 0) | (strand < 0), -1, chrom * len(STRANDS) + strand).astype(np.int32)


def _expected(on_strand, k, ignore_upstream, ignore_downstream, oriented=True):
    """The result frame, row for row, from the oracle's ordered lists and the per-row mask (oriented=False: every row is "+")."""
    probe = (_ids(DF1, on_strand, True), DF1["start"].to_numpy().astype(np.int32), DF1["end"].to_numpy().astype(np.int32))
    build = (_ids(DF2, on_strand, False), DF2["start"].to_numpy().astype(np.int32), DF2["end"].to_numpy().astype(np.int32))
    minus = (DF1["strand"] == "-").to_numpy() & oriented
    up = np.where(minus, IGNORE_RIGHT, IGNORE_LEFT)                          # upstream of a "-" row is higher coordinates
    down = np.where(minus, IGNORE_LEFT, IGNORE_RIGHT)
    mask = (up if ignore_upstream else 0) | (down if ignore_downstream else 0)
    idx, dist, nf = directed(full_lists(probe, build, True), mask, k)
    rows = []
    for i in range(len(DF1)):
        for r in range(max(int(nf[i]), 1)):
            rows.append((i, int(idx[i, r]), int(dist[i, r])))
    return rows


def _canon(df):
    """Every column of the result, rows as sorted tuples (None for a null)."""
    cols = ["chrom_1", "start_1", "end_1", "strand_1", "id_1", "chrom_2", "start_2", "end_2", "strand_2", "id_2", "distance"]
    assert list(df.columns) == cols
    out = []
    for row in df.itertuples(index=False):
        out.append(tuple(None if pd.isna(v) else (v if isinstance(v, str) else int(v)) for v in row))
    return sorted(out, key=lambda r: tuple((v is None, "" if v is None else str(v)) for v in r))


def _expected_frame(rows):
    a = DF1.iloc[[i for i, _, _ in rows]].reset_index(drop=True).add_suffix("_1")
    j = np.array([b for _, b, _ in rows])
    b = DF2.iloc[np.maximum(j, 0)].reset_index(drop=True).add_suffix("_2").astype(object)
    b.loc[j < 0, :] = None
    d = pd.Series([None if b_ < 0 else d_ for _, b_, d_ in rows], dtype=object, name="distance")
    return pd.concat([a, b, d], axis=1)


@pytest.fixture(scope="module")
def small_batches():
    pb.set_option("ivj.low_memory_batch_rows", 1024)
    yield
    pb.set_option("ivj.low_memory_batch_rows", 8_000_000)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("on_strand", [False, True])
@pytest.mark.parametrize("flags", [(True, False), (False, True)], ids=["ignore_upstream", "ignore_downstream"])
def test_mixed_strands_against_the_oracle(engine, small_batches, flags, on_strand, k):
    kw = dict(k=k, ignore_upstream=flags[0], ignore_downstream=flags[1], direction_col="strand", on_cols=["strand"] if on_strand else None)
    exp = _canon(_expected_frame(_expected(on_strand, k, *flags)))
    eager = pb.nearest(DF1, DF2, output_type="pandas.DataFrame", **kw)
    assert _canon(eager) == exp
    if engine == "cpu":                                                        # two engine calls: the "+" rows, then the "-" rows under the mirror mask
        n_minus = int((DF1["strand"] == "-").sum())
        up, down = (IGNORE_LEFT, IGNORE_RIGHT) if flags[0] else (IGNORE_RIGHT, IGNORE_LEFT)
        assert _DirectedOracleEngine.calls == [(len(DF1) - n_minus, up), (n_minus, down)]
    # the streaming session: df1 cut into three batches, each submitted as its "+" and its "-" rows
    reader = pb.nearest_batches(DF1, DF2, batch_rows=700, as_reader=True, **kw)
    batches = [b for b in reader]
    assert len(batches) >= 6
    assert _canon(pd.concat([b.to_pandas() for b in batches], ignore_index=True)) == exp
    lazy = pb.nearest(DF1, DF2, output_type="pyarrow.RecordBatchReader", **kw).read_all().to_pandas()
    assert _canon(lazy) == exp
    lim = pb.nearest(DF1, DF2, output_type="pandas.DataFrame", limit=50, **kw)
    assert len(lim) == 50
    assert set(_canon(lim)) <= set(exp)


def test_flags_without_effect_take_one_undirected_or_uniform_call(engine, small_batches):
    """No flag: today's result, whatever direction_col says.  Both flags: overlapping rows only, for both orientations."""
    plain = _canon(pb.nearest(DF1, DF2, output_type="pandas.DataFrame", k=3))
    assert _canon(pb.nearest(DF1, DF2, output_type="pandas.DataFrame", k=3, direction_col="strand")) == plain
    assert plain == _canon(_expected_frame(_expected(False, 3, False, False)))
    both = _canon(pb.nearest(DF1, DF2, output_type="pandas.DataFrame", k=3, direction_col="strand", ignore_upstream=True, ignore_downstream=True))
    assert both == _canon(_expected_frame(_expected(False, 3, True, True)))
    assert all(r[-1] in (0, None) for r in both)
    if engine == "cpu":
        assert _DirectedOracleEngine.calls == [(len(DF1), 0)] * 2 + [(len(DF1), 3)]
    # overlap=False and distance=False compose with a direction
    no = pb.nearest(DF1, DF2, output_type="pandas.DataFrame", overlap=False, ignore_upstream=True, direction_col="strand", distance=False)
    assert "distance" not in no.columns and len(no) == len(DF1)


@pytest.mark.gpu
@pytest.mark.parametrize("lazy", [False, True])
def test_one_call_arrow_entries_take_the_uniform_mask(lazy):
    """ivj_nearest_arrow_stream[_lazy]: opts->nearest_ignore applies to every df1 row alike."""
    import pyarrow as pa
    t1, t2 = pa.Table.from_pandas(DF1, preserve_index=False), pa.Table.from_pandas(DF2, preserve_index=False)
    eng = _engine.Engine(0)
    try:
        for mask, flags in ((IGNORE_LEFT, (True, False)), (IGNORE_RIGHT, (False, True))):
            got = _engine.nearest_arrow_stream(eng, t1, t2, strict=True, k=3, nearest_ignore=mask, lazy=lazy, max_batch_rows=700).read_all().to_pandas()
            assert _canon(got) == _canon(_expected_frame(_expected(False, 3, *flags, oriented=False)))
        with pytest.raises(ValueError):
            _engine.nearest_arrow_stream(eng, t1, t2, strict=True, nearest_ignore=5)
    finally:
        eng.close()
