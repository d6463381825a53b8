"""Overlap thresholds without a GPU: the rule that turns a fraction into a per-row minimum base count, the front door's
validation, and the pin of the brute-force yardstick (tests/_thresholds_util.py) to the existing oracle."""
import numpy as np
import pandas as pd
import pytest

import polars_bio_amd as pb
from polars_bio_amd import range_op
from oracle import oracle as O
import _thresholds_util as T
from _util import random_side

FRACS = [0.1, 0.3, 0.5, 0.7, 0.9, 1 / 3, 1.0]


def _smallest_passing(length: int, f: float) -> int:
    """The definition, by search: the smallest integer m >= 1 with m / length >= f in float64 (the test is monotone in m)."""
    lo, hi = 1, length                                     # f <= 1: m = length passes
    while lo < hi:
        mid = (lo + hi) // 2
        if np.float64(mid) / np.float64(length) >= f:
            hi = mid
        else:
            lo = mid + 1
    return lo


@pytest.mark.parametrize("f", FRACS)
def test_minimum_is_the_smallest_integer_passing_the_float64_test(f):
    lens = np.arange(1, 2001, dtype=np.int64)
    got = range_op.min_bases(lens, f).astype(np.int64)
    m = np.arange(1, 2001, dtype=np.float64)
    for ln, g in zip(lens, got):
        passing = (m[:ln] / np.float64(ln)) >= f           # every candidate count 1 .. len, literally
        assert passing.any() and g == int(np.argmax(passing)) + 1, (f, int(ln), int(g))
    for ln in ((1 << 31) - 1, 1 << 31):
        g = int(range_op.min_bases(np.array([ln], np.int64), f)[0])
        assert g == _smallest_passing(ln, f), (f, ln, g)
        assert np.float64(g) / np.float64(ln) >= f and (g == 1 or not (np.float64(g - 1) / np.float64(ln) >= f))


def test_known_minima():
    assert int(range_op.min_bases(np.array([10]), 0.3)[0]) == 3            # not 4: 3 / 10 >= 0.3 holds in float64
    assert int(range_op.min_bases(np.array([10]), 1 / 3)[0]) == 4
    assert int(range_op.min_bases(np.array([3]), 1 / 3)[0]) == 1
    assert int(range_op.min_bases(np.array([1 << 31]), 1.0)[0]) == 1 << 31
    assert range_op.min_bases(np.array([7]), 1e-9)[0] == 1                  # never below one base


def test_rows_without_positions_get_never():
    got = range_op.min_bases(np.array([0, -1, -(1 << 31), 5], np.int64), 0.5)
    assert got.dtype == np.uint32
    assert list(got[:3]) == [T.NEVER] * 3 and got[3] == 3
    # the lengths the front door derives: end - start, + 1 for closed frames
    side = (np.zeros(3, np.int32), np.array([5, 5, 9], np.int32), np.array([5, 4, 2], np.int32))
    assert list(range_op._side_lengths(side, True)) == [0, -1, -7]
    assert list(range_op._side_lengths(side, False)) == [1, 0, -6]


def _df(zero_based=True):
    df = pd.DataFrame({"chrom": ["chr1", "chr1"], "start": [1, 10], "end": [8, 20]})
    df.attrs["coordinate_system_zero_based"] = zero_based
    return df


@pytest.mark.parametrize("kw", [dict(min_overlap=0), dict(min_overlap=-3), dict(min_overlap=True), dict(min_overlap=2.0), dict(min_overlap="5"),
                                dict(min_frac1=0.0), dict(min_frac1=-0.5), dict(min_frac1=1.0000001), dict(min_frac1=float("nan")),
                                dict(min_frac2=0), dict(min_frac2=2), dict(min_frac2=float("nan")), dict(min_frac2="0.5"),
                                dict(min_overlap=3, min_frac1=7.0)])
@pytest.mark.parametrize("fn", [pb.overlap, pb.count_overlaps])
def test_front_door_refuses_bad_thresholds(fn, kw):
    with pytest.raises(ValueError):
        fn(_df(), _df(), output_type="pandas.DataFrame", **kw)


def test_engine_without_thresholds_is_a_clear_error(monkeypatch):
    class Plain:                                           # what a multi-device engine looks like to the front door
        pass
    monkeypatch.setattr(range_op, "default_engine", lambda: Plain())
    with pytest.raises(NotImplementedError, match="min_overlap"):
        pb.overlap(_df(), _df(), output_type="pandas.DataFrame", min_overlap=2)
    with pytest.raises(NotImplementedError, match="min_overlap"):
        pb.count_overlaps(_df(), _df(), output_type="pandas.DataFrame", min_frac1=0.5)


@pytest.mark.parametrize("strict", [True, False])
def test_yardstick_equals_the_oracle_at_min_overlap_one(strict):
    """With min_overlap = 1 on rows that all cover a position the thresholded join IS the plain join."""
    rng = np.random.default_rng(7)
    pc, ps, pe = random_side(rng, 700, 5, 4000, 120, zero_len_frac=0.0)
    bc, bs, be = random_side(rng, 900, 5, 4000, 200, zero_len_frac=0.0)
    pe, be = np.maximum(pe, ps + 1).astype(np.int32), np.maximum(be, bs + 1).astype(np.int32)      # every row covers a position in both frames
    gp, gb, cnt = T.brute((pc, ps, pe), (bc, bs, be), 5, strict, min_overlap=1)
    ep, eb = T.sort_pairs(*O.overlap_brute(O.Side(pc, ps, pe), O.Side(bc, bs, be), strict))
    assert len(gp) == len(ep) > 1000 and (gp == ep).all() and (gb == eb).all()
    assert (cnt == O.count_overlaps_brute(O.Side(pc, ps, pe), O.Side(bc, bs, be), strict)).all()


def test_yardstick_evaluates_the_literal_fraction():
    probe = (np.zeros(1, np.int32), np.array([0], np.int32), np.array([10], np.int32))
    build = (np.zeros(3, np.int32), np.array([7, 6, 8], np.int32), np.array([30, 30, 9], np.int32))
    p, b, cnt = T.brute(probe, build, 1, True, min_frac1=0.3)              # ov = 3, 4, 1 of len 10
    assert list(b) == [0, 1] and list(cnt) == [2]
    p, b, cnt = T.brute(probe, build, 1, True, min_frac2=1.0)              # only the row that lies inside the probe
    assert list(b) == [2]
    p, b, cnt = T.brute(probe, build, 1, True, probe_min=np.array([T.NEVER], np.uint32))
    assert len(p) == 0 and list(cnt) == [0]
