"""pb.multi_intersect / pb.consensus, the front door: string chroms in different first-occurrence order, both coordinate
systems, the names columns, on_cols with a null value, the result's coordinate-system metadata, and the result as an input."""
import numpy as np
import pandas as pd
import pytest

import polars_bio_amd as pb
import _multi_util as U

pytestmark = pytest.mark.gpu

ROWS = [
    [("chr2", 10, 30), ("chr1", 0, 20), ("chr10", 5, 9), ("chr1", 40, 50)],
    [("chr10", 7, 12), ("chr2", 20, 40), ("chr1", 10, 45)],
    [("chr1", 15, 42), ("chrX", 1, 4), ("chr2", 30, 35), ("chr2", 35, 38)],
]


def _frame(rows, zero_based, extra=None):
    df = pd.DataFrame(rows, columns=["chrom", "start", "end"])
    for name, values in (extra or {}).items():
        df[name] = values
    df.attrs["coordinate_system_zero_based"] = zero_based
    return df


def _reference(rows_by_frame, zero_based, k, consensus):
    names = sorted({r[0] for rows in rows_by_frame for r in rows})
    frames = [U.S.as_i32([names.index(r[0]) for r in rows], [r[1] for r in rows], [r[2] for r in rows]) for rows in rows_by_frame]
    c, s, e, mask = U.multi_events(frames, zero_based, len(names), k, consensus)
    return [names[i] for i in c], s, e, mask


@pytest.mark.parametrize("zero_based", [True, False], ids=["0-based", "1-based"])
@pytest.mark.parametrize("k", [1, 2, 3])
def test_multi_intersect_and_consensus_on_pandas_frames(zero_based, k):
    frames = [_frame(rows, zero_based) for rows in ROWS]
    res = pb.multi_intersect(frames, min_frames=k, names=["rep1", "rep2", "rep3"], output_type="pandas.DataFrame")
    assert list(res.columns) == ["chrom", "start", "end", "n_frames", "mask", "rep1", "rep2", "rep3"]
    assert str(res["start"].dtype) == "int64" and str(res["n_frames"].dtype) == "int64" and str(res["mask"].dtype) == "uint64"
    chrom, s, e, mask = _reference(ROWS, zero_based, k, False)
    assert list(res["chrom"]) == chrom
    assert (res["start"].to_numpy() == s).all() and (res["end"].to_numpy() == e).all()
    assert (res["mask"].to_numpy() == mask).all() and (res["n_frames"].to_numpy() == U.popcount(mask)).all()
    assert (res["n_frames"] >= k).all()
    for f, name in enumerate(["rep1", "rep2", "rep3"]):
        assert res[name].dtype == bool and (res[name].to_numpy() == ((mask >> np.uint64(f)) & np.uint64(1)).astype(bool)).all()
    assert pb.get_coordinate_system(res) is zero_based
    bare = pb.multi_intersect(frames, min_frames=k, output_type="pandas.DataFrame")
    assert list(bare.columns) == ["chrom", "start", "end", "n_frames", "mask"] and len(bare) == len(res)

    cons = pb.consensus(frames, k, output_type="pandas.DataFrame")
    assert list(cons.columns) == ["chrom", "start", "end"]
    chrom, s, e, _ = _reference(ROWS, zero_based, k, True)
    assert list(cons["chrom"]) == chrom and (cons["start"].to_numpy() == s).all() and (cons["end"].to_numpy() == e).all()
    assert pb.get_coordinate_system(cons) is zero_based


def test_a_boundary_between_frames_splits_and_one_inside_a_frame_does_not():
    a = _frame([("chr1", 0, 5), ("chr1", 5, 8)], True)          # two touching rows of one frame
    b = _frame([("chr1", 8, 12)], True)                        # starts where a ends
    res = pb.multi_intersect([a, b], output_type="pandas.DataFrame")
    assert res[["start", "end", "mask"]].values.tolist() == [[0, 8, 1], [8, 12, 2]]
    assert pb.consensus([a, b], 1, output_type="pandas.DataFrame")[["start", "end"]].values.tolist() == [[0, 12]]
    assert len(pb.consensus([a, b], 2, output_type="pandas.DataFrame")) == 0


def test_on_cols_with_a_null_strand():
    strands = [["+", "-", "+", None], ["+", "+", "-"], ["-", "+", "+", "+"]]
    frames = [_frame(rows, True, {"strand": st}) for rows, st in zip(ROWS, strands)]
    res = pb.multi_intersect(frames, on_cols=["strand"], names=["a", "b", "c"], output_type="pandas.DataFrame")
    assert list(res.columns) == ["chrom", "start", "end", "strand", "n_frames", "mask", "a", "b", "c"]
    assert res["strand"].notna().all()
    parts = []
    for strand in ("+", "-"):
        sub = [[r for r, st in zip(rows, sts) if st == strand] for rows, sts in zip(ROWS, strands)]
        chrom, s, e, mask = _reference(sub, True, 1, False)
        parts += [(ch, strand, int(x), int(y), int(m)) for ch, x, y, m in zip(chrom, s, e, mask)]
    got = [(r.chrom, r.strand, r.start, r.end, r.mask) for r in res.itertuples()]
    assert got == sorted(parts, key=lambda p: (p[0], p[1], p[2]))
    cons = pb.consensus(frames, 2, on_cols=["strand"], output_type="pandas.DataFrame")
    assert list(cons.columns) == ["chrom", "start", "end", "strand"]
    two = res[res["n_frames"] >= 2]
    assert int((cons["end"] - cons["start"]).sum()) == int((two["end"] - two["start"]).sum())


def test_the_result_feeds_back_into_overlap():
    frames = [_frame(rows, True) for rows in ROWS]
    cons = pb.consensus(frames, 2, output_type="pandas.DataFrame")
    back = pb.overlap(cons, frames[0], output_type="pandas.DataFrame")
    assert len(back) >= len(cons) > 0                          # every region of two frames overlaps a row of some frame...
    seg = pb.multi_intersect(frames, output_type="pandas.DataFrame")
    hits = pb.count_overlaps(seg, frames[0], output_type="pandas.DataFrame")
    assert ((hits["count"] > 0).to_numpy() == ((seg["mask"].to_numpy() & np.uint64(1)) == 1)).all()


def test_namespace_takes_the_other_frames_as_a_list():
    frames = [_frame(rows, True) for rows in ROWS]
    cons = frames[0].pb.consensus(frames[1:], 2)
    assert isinstance(cons, pd.DataFrame) and cons.equals(pb.consensus(frames, 2, output_type="pandas.DataFrame"))
    seg = frames[0].pb.multi_intersect(frames[1:], names=["a", "b", "c"])
    assert seg.equals(pb.multi_intersect(frames, names=["a", "b", "c"], output_type="pandas.DataFrame"))
    assert len(frames[0].pb.consensus([], 1)) == len(pb.consensus(frames[:1], 1, output_type="pandas.DataFrame"))
    with pytest.raises(ValueError, match="as a list"):
        frames[0].pb.consensus(frames[1], 1)
