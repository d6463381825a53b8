"""CPU checks of the distance-window join: the yardstick of tests/_window_util.py pinned to what exists (the overlap and nearest
definitions of the oracle), a hand-written table, and the front door's validation and extent columns.  No GPU."""
import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
from polars_bio_amd import _arrow as A
from polars_bio_amd import range_op
from oracle import oracle as O
import _window_util as WU
from _util import random_side


def test_zero_window_on_closed_frames_is_the_overlap_join():
    """1-based closed: d = 0 iff the rows overlap, so left = right = 0 keeps exactly the overlapping pairs (random_side plants
    zero-length rows, which cover one position in a closed frame, but no inverted ones)."""
    for seed in (1, 2, 3):
        rng = np.random.default_rng(seed)
        probe, build = random_side(rng, 600, 3, 20_000, 300), random_side(rng, 800, 3, 20_000, 400)
        p, b, d, cnt = WU.brute(probe, build, 3, False, 0, 0, 0)
        ep, eb = O.overlap_brute(O.Side(*probe), O.Side(*build), False)
        ep, eb = WU.sort_pairs(ep, eb)
        assert len(p) > 1000 and (p == ep).all() and (b == eb).all() and not d.any()
        assert (cnt == np.bincount(ep, minlength=600)).all()


@pytest.mark.parametrize("strict", [True, False])
def test_minimum_distance_per_probe_is_the_nearest_distance(strict):
    probe, build = WU.no_empty_rows(5, 300, 400, 3)
    p, b, d, cnt = WU.brute(probe, build, 3, strict, WU.U32, WU.U32, 0)
    assert (cnt == np.bincount(build[0], minlength=3)[probe[0]]).all(), "extents of 2^32 - 1 reach every row of the contig"
    best = np.full(300, -1, np.int64)
    best[np.unique(p)] = np.minimum.reduceat(np.abs(d), np.nonzero(np.r_[True, p[1:] != p[:-1]])[0])
    exp = O.np_nearest_distance(O.Side(*probe), O.Side(*build), strict)
    assert (best == exp).all() and (exp > 0).sum() > 50 and (exp == 0).sum() > 10


def test_hand_written_table():
    """Probe [100, 200) / [100, 200]; eight build rows with the distance written out for both frames."""
    probe = WU.side([(100, 200)])
    build = WU.side([(150, 160),      # 0 contained: 0 / 0
                     (200, 210),      # 1 bookended after: half-open d = 0 without overlap; closed: shares 200, d = 0
                     (201, 210),      # 2 half-open gap 1; closed: adjacent, d = 1
                     (205, 210),      # 3 gap 5 after
                     (90, 100),       # 4 bookended before: half-open d = 0 (before); closed: shares 100
                     (80, 95),        # 5 gap 5 before
                     (50, 60),        # 6 gap 40 before
                     (300, 300)])     # 7 half-open: covers nothing; closed: gap 100 after
    exp = {True: {0: 0, 1: 0, 2: 1, 3: 5, 4: 0, 5: -5, 6: -40}, False: {0: 0, 1: 0, 2: 1, 3: 5, 4: 0, 5: -5, 6: -40, 7: 100}}
    for strict in (True, False):
        p, b, d, _ = WU.brute(probe, build, 1, strict, 1000, 1000, 0)
        assert dict(zip(b.tolist(), d.tolist())) == exp[strict]
        # asymmetric extents and a minimum distance
        _, b, d, _ = WU.brute(probe, build, 1, strict, 5, 1, 1)
        assert dict(zip(b.tolist(), d.tolist())) == {2: 1, 5: -5}
        _, b, _, _ = WU.brute(probe, build, 1, strict, 0, 0, 0)
        assert b.tolist() == [0, 1, 4]
    # bedtools window -w W reports b iff [a.start - W, a.end + W) and b share a base (0-based half-open): W = 6 reaches gap 5 and
    # not gap 6, i.e. window = W - 1 on half-open frames; on closed frames the same rows read as gap + 1, i.e. window = W
    far = WU.side([(206, 210), (205, 210), (85, 94), (85, 95)])
    for strict, window in ((True, 6 - 1), (False, 6)):
        _, b, d, _ = WU.brute(probe, far, 1, strict, window, window, 0)
        bedtools = [j for j in range(4) if max(100 - 6, int(far[1][j])) < min(200 + 6, int(far[2][j]))]
        if strict:
            assert b.tolist() == bedtools == [1, 3]
        else:                                              # the closed rows [s + 1, e] of the same intervals
            closed = (far[0], far[1] + 1, far[2])
            _, b, _, _ = WU.brute((probe[0], probe[1] + 1, probe[2]), closed, 1, False, window, window, 0)
            assert b.tolist() == bedtools


def test_every_shape_is_not_vacuous():
    for name in WU.SHAPES:
        total = 0
        for probe, build, nc, w in WU.cases(name):
            for strict in (True, False):
                total += len(WU.brute(probe, build, nc, strict, **w)[0])
        assert total > 0, name


def _frames():
    df1 = pd.DataFrame({"chrom": ["chr1"] * 4, "start": [100, 200, 300, 400], "end": [150, 250, 350, 450], "strand": ["+", "-", ".", None]})
    df2 = pd.DataFrame({"chrom": ["chr1"], "start": [10], "end": [20]})
    for d in (df1, df2):
        d.attrs["coordinate_system_zero_based"] = True
    return df1, df2


@pytest.mark.parametrize("fn", [pb.window, pb.count_window])
def test_front_door_validation(fn):
    df1, df2 = _frames()
    kw = dict(output_type="pandas.DataFrame")
    for bad in (dict(window=-1), dict(window=1.5), dict(window=True), dict(window="5"), dict(window=1 << 32), dict(upstream=-3),
                dict(downstream=2.0), dict(upstream=(1 << 32)), dict(min_distance=-1), dict(min_distance=0.5), dict(window=None)):
        with pytest.raises(ValueError):
            fn(df1, df2, **bad, **kw)
    with pytest.raises(ValueError, match="direction_col"):
        fn(df1, df2, direction_col="orientation", **kw)
    with pytest.raises(ValueError, match="direction_col"):
        fn(df1, df2, direction_col=3, **kw)


def test_extent_columns_of_a_direction_col():
    df1, _ = _frames()
    is_minus = A.minus_rows(pa.Table.from_pandas(df1).column("strand"))
    assert is_minus.tolist() == [False, True, False, False]       # "+", "-", ".", null
    left, right, pl, pr = range_op.window_extents(is_minus, 1000, 50)
    assert pl.dtype == np.uint32 and pr.dtype == np.uint32
    assert pl.tolist() == [1000, 50, 1000, 1000] and pr.tolist() == [50, 1000, 50, 50]
    # scalars wherever every row agrees
    assert range_op.window_extents(None, 7, 9) == (7, 9, None, None)
    assert range_op.window_extents(is_minus, 8, 8) == (8, 8, None, None)
    assert range_op.window_extents(np.zeros(4, bool), 7, 9) == (7, 9, None, None)
    assert range_op.window_extents(np.ones(4, bool), 7, 9) == (9, 7, None, None)
    left, right, pl, pr = range_op.window_extents(is_minus, (1 << 32) - 1, 0)
    assert pl.tolist() == [(1 << 32) - 1, 0, (1 << 32) - 1, (1 << 32) - 1] and pr.tolist() == [0, (1 << 32) - 1, 0, 0]
    assert range_op._validate_window(5, None, None, 0) == (5, 5, 0)
    assert range_op._validate_window(5, 0, 9, 2) == (0, 9, 2)
    assert range_op._validate_window(np.int64(5), None, np.int32(3), 0) == (5, 3, 0)


def test_public_names():
    assert "window" in pb.__all__ and "count_window" in pb.__all__
    df1, _ = _frames()
    assert hasattr(df1.pb, "window") and hasattr(df1.pb, "count_window")
