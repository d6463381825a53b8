"""on_cols test helpers: random stranded frames and the per-group decomposition of every operation, built from the CPU
oracle's brute-force kernels on each group's sub-frames (one contig per call) with the row indices mapped back."""
import numpy as np
import pandas as pd
import pyarrow as pa

import polars_bio_amd as pb
from oracle import oracle as O

CHROMS = ["chr1", "chr2", "chr3", "chrX"]
STRANDS = ["+", "-", "."]
SAMPLES = ["s0", "s1", "s2", "s3"]


def frame(rng, n, span=400, max_len=40, chroms=CHROMS, strands=STRANDS, samples=SAMPLES, null_frac=0.03):
    """Intervals on few positions (ties), a few null chroms / strands, an ``id`` column = row number."""
    chrom = np.array(chroms, dtype=object)[rng.integers(0, len(chroms), n)]
    strand = np.array(strands, dtype=object)[rng.integers(0, len(strands), n)]
    sample = np.array(samples, dtype=object)[rng.integers(0, len(samples), n)]
    chrom[rng.random(n) < null_frac] = None
    strand[rng.random(n) < null_frac] = None
    start = rng.integers(0, span, n)
    end = start + rng.integers(0, max_len, n)
    df = pd.DataFrame({"chrom": chrom, "start": start.astype(np.int64), "end": end.astype(np.int64), "strand": strand, "sample": sample,
                       "id": np.arange(n, dtype=np.int64)})
    df.attrs["coordinate_system_zero_based"] = True
    return df


def pair_frames(seed, n1=600, n2=300):
    """df1 / df2 where df2 lacks some groups df1 has: no 'chrX' at all, no '.' strand on chr3."""
    rng = np.random.default_rng(seed)
    df1 = frame(rng, n1)
    df2 = frame(rng, n2, chroms=CHROMS[:3])
    drop = (df2["chrom"] == "chr3") & (df2["strand"] == ".")
    df2 = df2[~drop].reset_index(drop=True)
    df2["id"] = np.arange(len(df2), dtype=np.int64)
    df2.attrs["coordinate_system_zero_based"] = True
    return df1, df2


def _keys(df, on_cols):
    cols = ["chrom"] + list(on_cols)
    ok = df[cols].notna().all(axis=1).to_numpy()
    return [tuple(r) if o else None for r, o in zip(df[cols].itertuples(index=False, name=None), ok)]


def groups(df1, df2, on_cols):
    """{key: (df1 rows, df2 rows)} over the keys of df1 (df2 rows may be empty), plus df1 rows with a null component."""
    k1, k2 = _keys(df1, on_cols), _keys(df2, on_cols)
    rows2 = {}
    for j, k in enumerate(k2):
        if k is not None:
            rows2.setdefault(k, []).append(j)
    out = {}
    for i, k in enumerate(k1):
        if k is not None:
            out.setdefault(k, ([], rows2.get(k, [])))[0].append(i)
    return {k: (np.array(a, np.int64), np.array(b, np.int64)) for k, (a, b) in out.items()}


def _side(df, rows):
    return O.Side(np.zeros(len(rows), np.int32), df["start"].to_numpy()[rows], df["end"].to_numpy()[rows])


def expected_pairs(df1, df2, on_cols, strict=True):
    ps, bs = [], []
    for _, (r1, r2) in groups(df1, df2, on_cols).items():
        if len(r2) == 0:
            continue
        p, b = O.overlap_brute(_side(df1, r1), _side(df2, r2), strict)
        ps.append(r1[p]); bs.append(r2[b])
    p = np.concatenate(ps) if ps else np.empty(0, np.int64)
    b = np.concatenate(bs) if bs else np.empty(0, np.int64)
    o = np.lexsort((b, p))
    return p[o], b[o]


def expected_counts(df1, df2, on_cols, strict=True):
    out = np.zeros(len(df1), np.int64)
    for _, (r1, r2) in groups(df1, df2, on_cols).items():
        if len(r2):
            out[r1] = O.count_overlaps_brute(_side(df1, r1), _side(df2, r2), strict)
    return out


def expected_coverage(df1, df2, on_cols, strict=True):
    out = np.zeros(len(df1), np.int64)
    for _, (r1, r2) in groups(df1, df2, on_cols).items():
        if len(r2):
            out[r1] = O.np_coverage_brute(_side(df1, r1), _side(df2, r2), strict)
    return out


def expected_nearest(df1, df2, on_cols, k, overlap, strict=True):
    """[(df1 row, df2 row or -1, distance or -1)] in df1 order, slot order."""
    per = {}
    for _, (r1, r2) in groups(df1, df2, on_cols).items():
        if len(r2) == 0:
            continue
        idx, dist, nf = O.nearest_brute(_side(df1, r1), _side(df2, r2), strict, k, overlap)
        for t, i in enumerate(r1):
            per[int(i)] = [(int(r2[idx[t, s]]), int(dist[t, s])) for s in range(nf[t])]
    rows = []
    for i in range(len(df1)):
        slots = per.get(i) or [(-1, -1)]
        rows.extend((i, b, d) for b, d in slots)
    return rows


def expected_merge(df, on_cols, strict=True, min_dist=0):
    """[(chrom, start, end, *on values, n)] in (chrom, on values, start) order."""
    g = groups(df, df, on_cols)
    out = []
    for key in sorted(g):
        r = g[key][0]
        _, _, _, (c, s, e, n) = O.np_cluster(_side(df, r), strict, min_dist)
        out.extend((key[0], int(a), int(b)) + key[1:] + (int(m),) for a, b, m in zip(s, e, n))
    return out


# ---- front-door results as plain lists ----------------------------------------------------------------------------------

def to_pandas(res):
    if isinstance(res, pd.DataFrame):
        return res
    if isinstance(res, pa.RecordBatchReader):
        return res.read_all().to_pandas()
    if isinstance(res, pa.Table):
        return res.to_pandas()
    if hasattr(res, "to_pandas"):
        return res.to_pandas()
    raise TypeError(type(res))


def concat_batches(gen):
    tabs = [t for t in gen]
    return pa.concat_tables(tabs).to_pandas() if tabs else None


def got_pairs(df):
    p, b = df["id_1"].to_numpy(np.int64), df["id_2"].to_numpy(np.int64)
    o = np.lexsort((b, p))
    return p[o], b[o]


def got_nearest(df):
    b = df["id_2"]
    d = df["distance"]
    return [(int(i), -1 if pd.isna(x) else int(x), -1 if pd.isna(y) else int(y)) for i, x, y in zip(df["id_1"], b, d)]


def check_ops(df1, df2, on_cols, outputs=("pandas.DataFrame", "pyarrow.Table", "pyarrow.RecordBatchReader"), batch_rows=(97,), strict=True):
    """Every operation with ``on_cols`` through the front door (every output kind, the _batches forms) == the per-group oracle.
    ``strict``: the frames' coordinate system (True: 0-based half-open, False: 1-based closed)."""
    ep, eb = expected_pairs(df1, df2, on_cols, strict)
    ec = expected_counts(df1, df2, on_cols, strict)
    for out in outputs:
        res = to_pandas(pb.overlap(df1, df2, on_cols=on_cols, output_type=out))
        gp, gb = got_pairs(res)
        assert len(gp) == len(ep) and (gp == ep).all() and (gb == eb).all(), f"overlap {out}"
        assert (res["strand_1"].to_numpy() == res["strand_2"].to_numpy()).all()
        left = to_pandas(pb.overlap(df1, df2, on_cols=on_cols, overlap_output="left", output_type=out))
        assert sorted(left["id"].tolist()) == sorted(ep.tolist()), f"overlap left {out}"
        dist = to_pandas(pb.overlap(df1, df2, on_cols=on_cols, overlap_output="left", distinct_output=True, output_type=out))
        assert sorted(dist["id"].tolist()) == sorted(set(ep.tolist())), f"overlap left distinct {out}"
        cnt = to_pandas(pb.count_overlaps(df1, df2, on_cols=on_cols, output_type=out))
        assert (cnt["count"].to_numpy() == ec).all(), f"count_overlaps {out}"
        sweep = to_pandas(pb.count_overlaps(df1, df2, on_cols=on_cols, naive_query=False, output_type=out))
        assert list(sweep.columns) == ["chrom", "start", "end"] + list(on_cols) + ["count"]
        assert (sweep["count"].to_numpy() == ec).all(), f"count_overlaps sweep {out}"
        for k in (1, 3):
            for ov in (True, False):
                got = got_nearest(to_pandas(pb.nearest(df1, df2, on_cols=on_cols, k=k, overlap=ov, output_type=out)))
                assert got == expected_nearest(df1, df2, on_cols, k, ov, strict), f"nearest k={k} overlap={ov} {out}"
    cov = pb.coverage(df1, df2, on_cols=on_cols, output_type="pandas.DataFrame")
    assert (cov["coverage"].to_numpy() == expected_coverage(df1, df2, on_cols, strict)).all()
    m = pb.merge(df1, on_cols=on_cols, output_type="pandas.DataFrame")
    assert list(m.columns) == ["chrom", "start", "end"] + list(on_cols) + ["n_intervals"]
    assert [tuple(r) for r in m.itertuples(index=False, name=None)] == expected_merge(df1, on_cols, strict)
    for br in batch_rows:
        gp, gb = got_pairs(concat_batches(pb.overlap_batches(df1, df2, on_cols=on_cols, batch_rows=br)))
        assert (gp == ep).all() and (gb == eb).all(), "overlap_batches"
        c = concat_batches(pb.count_overlaps_batches(df1, df2, on_cols=on_cols, batch_rows=br))
        assert (c["count"].to_numpy() == ec).all(), "count_overlaps_batches"
        got = got_nearest(concat_batches(pb.nearest_batches(df1, df2, on_cols=on_cols, k=3, batch_rows=br)))
        assert got == expected_nearest(df1, df2, on_cols, 3, True, strict), "nearest_batches"
