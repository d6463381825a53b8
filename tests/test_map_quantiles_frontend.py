"""pb.map_quantiles / pb.map_median end to end on the GPU: small pandas frames (Arrow-backed value columns) with int16, uint32, float32 and float64
columns that hold nulls, both coordinate systems and on_cols=["strand"], against the yardstick of tests/_map_quantiles_util.py
applied to the frames."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
from polars_bio_amd import range_op
import _map_quantiles_util as U

pytestmark = pytest.mark.gpu

COLUMNS = {"i16": pa.int16(), "u32": pa.uint32(), "f32": pa.float32(), "f64": pa.float64()}
QS = [0.0, 0.3, 0.5, 1.0]


def _frames(zero_based, seed=0, n1=300, n2=900):
    rng = np.random.default_rng(seed)
    def frame(n, maxlen):
        s = rng.integers(1, 5000, n)
        d = {"chrom": rng.choice(["chr1", "chr2", "chrX"], n), "start": s, "end": s + rng.integers(1, maxlen, n), "strand": rng.choice(["+", "-"], n)}
        return d
    d1, d2 = frame(n1, 400), frame(n2, 300)
    d1["chrom"][::40] = "chrU"                               # rows without a match: null results
    raw = {"i16": rng.integers(-300, 300, n2), "u32": rng.integers(0, 2 ** 32, n2), "f32": rng.standard_normal(n2).astype(np.float32),
           "f64": rng.standard_normal(n2) * 1e6}
    raw["f64"][rng.random(n2) < 0.02] = np.nan
    t2 = pa.table({**{k: pa.array(v) for k, v in d2.items()},
                   **{name: pa.array(raw[name], type=typ, mask=rng.random(n2) < 0.15) for name, typ in COLUMNS.items()}})
    df1 = pd.DataFrame(d1)
    df2 = t2.to_pandas(types_mapper=pd.ArrowDtype)
    for df in (df1, df2):
        df.attrs["coordinate_system_zero_based"] = zero_based
    return df1, df2, t2


def _yardstick(df1, t2, name, zero_based, on_strand):
    """-> per df1 row the sorted non-null values (float64 / int64) of the matching df2 rows."""
    key = (lambda c, s: [f"{a}|{b}" for a, b in zip(c, s)]) if on_strand else (lambda c, s: list(c))
    k1, k2 = key(df1["chrom"], df1["strand"]), key(t2.column("chrom").to_pylist(), t2.column("strand").to_pylist())
    ids = {k: i for i, k in enumerate(sorted(set(k1) | set(k2)))}
    side = lambda keys, s, e: (np.array([ids[k] for k in keys], np.int32), np.asarray(s, np.int32), np.asarray(e, np.int32))
    probe = side(k1, df1["start"], df1["end"])
    build = side(k2, t2.column("start").to_numpy(), t2.column("end").to_numpy())
    col = t2.column(name).combine_chunks()
    valid = col.is_valid().to_numpy(zero_copy_only=False)
    wide = np.float64 if pa.types.is_floating(col.type) else np.int64
    values = col.fill_null(0).to_numpy(zero_copy_only=False).astype(wide)
    p, b = U.pairs(probe, build, len(ids), zero_based)
    return [np.sort(v) for v in U.matched_values(p, b, len(df1), values, valid)]


@pytest.mark.parametrize("zero_based", [True, False], ids=["0-based", "1-based"])
@pytest.mark.parametrize("on_strand", [False, True], ids=["chrom", "strand"])
def test_quantiles_and_median_of_every_column_type(zero_based, on_strand):
    df1, df2, t2 = _frames(zero_based, seed=int(zero_based) + 2 * int(on_strand))
    kw = dict(on_cols=["strand"]) if on_strand else {}
    for name in COLUMNS:
        lists = _yardstick(df1, t2, name, zero_based, on_strand)
        m = np.array([len(v) for v in lists])
        assert (m == 0).sum() >= 5
        assert (m > 3).sum() > 50
        lo, hi, g = range_op.quantile_ranks(m[:, None], np.array(QS)[None, :])
        pick = lambda r: np.array([[v[i] if len(v) else 0 for i in row] for v, row in zip(lists, r)])
        vlo, vhi = pick(lo), pick(hi)
        for method in ("lower", "higher"):
            got = pb.map_quantiles(df1, df2, name, q=QS, method=method, output_type="pyarrow.Table", **kw)
            want = vlo if method == "lower" else vhi
            for k, x in enumerate(QS):
                col = got.column(f"{name}_q{x!r}")
                assert col.type == COLUMNS[name] and (np.asarray(col.is_null()) == (m == 0)).all(), (name, method, x)
                a = col.fill_null(0).to_numpy(zero_copy_only=False)
                U.assert_same(a.astype(want.dtype)[m > 0], want[m > 0, k], f"{name} {method} q={x}")
        flo, fhi = vlo.astype(np.float64), vhi.astype(np.float64)
        with np.errstate(invalid="ignore"):
            exp = {"midpoint": np.where(flo == fhi, flo, (flo + fhi) / 2.0), "linear": np.where((flo == fhi) | (g == 0), flo, flo + (fhi - flo) * g)}
        for method in ("midpoint", "linear"):
            got = pb.map_quantiles(df1, df2, name, q=QS, method=method, output_type="numpy.ndarray", **kw)
            assert got.dtype == np.float64 and (np.isnan(got[m == 0])).all()
            U.assert_same(got[m > 0], exp[method][m > 0], f"{name} {method}")
        med = pb.map_median(df1, df2, name, output_type="pandas.DataFrame", **kw)[f"{name}_median"]
        assert (med.isna().to_numpy() == ((m == 0) | np.isnan(exp["linear"][:, 2]))).all()
        U.assert_same(med.to_numpy(np.float64, na_value=np.nan)[m > 0], exp["linear"][m > 0, 2], f"{name} median")


def test_thresholds_limit_and_the_accessor():
    df1, df2, t2 = _frames(True, seed=9)
    plain = pb.map_quantiles(df1, df2, "i16", q=[0.25, 0.75], method="higher", output_type="pandas.DataFrame")
    thr = pb.map_quantiles(df1, df2, "i16", q=[0.25, 0.75], method="higher", output_type="pandas.DataFrame", min_overlap=20, min_frac2=0.5)
    assert thr["i16_q0.25"].isna().sum() > plain["i16_q0.25"].isna().sum() and thr["i16_q0.25"].notna().sum() > 50
    cnt = pb.map_overlaps(df1, df2, {"i16": ["count", "min"]}, output_type="pandas.DataFrame", min_overlap=20, min_frac2=0.5)
    low = pb.map_quantiles(df1, df2, "i16", q=[0.0], method="lower", output_type="pandas.DataFrame", min_overlap=20, min_frac2=0.5)["i16_q0.0"]
    assert (low.isna().to_numpy() == (cnt["i16_count"].to_numpy() == 0)).all()
    assert (low.dropna().to_numpy() == cnt["i16_min"].dropna().to_numpy()).all()
    via = df1.pb.map_median(df2, value="f32", limit=7)
    assert list(via.columns)[-1] == "f32_median" and len(via) == 7
    assert via.attrs["coordinate_system_zero_based"] is True
