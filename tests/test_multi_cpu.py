"""The two numpy forms of multi_intersect / consensus (tests/_multi_util.py) against each other on every small-universe shape,
and the argument checks of the front door, which are made before an engine exists."""
import numpy as np
import pandas as pd
import pytest

import polars_bio_amd as pb
from polars_bio_amd import _engine
import _multi_util as U

MODES = [pytest.param(True, id="strict"), pytest.param(False, id="weak")]
KINDS = [pytest.param(False, id="segments"), pytest.param(True, id="consensus")]


@pytest.mark.parametrize("consensus", KINDS)
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", U.SMALL_UNIVERSE)
def test_the_two_references_agree(shape, strict, consensus):
    frames, nc = U.case(shape, strict)
    for k in U.min_frames_of(len(frames)):
        exp = U.expected(shape, strict, k, consensus)
        U.assert_equal(U.multi_brute(frames, strict, nc, k, consensus), exp, f"{shape} k={k}")
        if not consensus:
            assert (U.popcount(exp[3]) >= k).all()


def test_shapes_hold_what_their_names_say():
    for n in (U.T - 2, U.T, U.T + 2, 3 * U.T, 3 * U.T + 2):
        frames, nc = U.case(f"events_{n}", True)
        assert len(frames) == 3 and sum(2 * len(U.S.union_runs(f, True, nc)[0]) for f in frames) == n
    for name, before, ends_in_tile_0 in (("group_of_64_begins_in_the_previous_tile", U.T - 20, 0), ("group_of_64_ends_on_the_tile_edge", U.T - 64, 32),
                                         ("group_of_64_leaves_ends_in_the_previous_tile", U.T - 20, 12)):
        for strict in (True, False):
            frames, nc = U.case(name, strict)
            assert len(frames) == U.MAX_FRAMES
            runs = [U.S.union_runs(f, strict, nc) for f in frames]
            keys = np.sort(np.concatenate([np.concatenate([s, e1]) for _c, s, e1 in runs]))
            values, counts = np.unique(keys, return_counts=True)
            X = values[np.argmax(counts)]
            assert counts.max() == U.MAX_FRAMES and int((keys < X).sum()) == before
            assert before < U.T <= before + U.MAX_FRAMES
            n_starts = sum(int((s == X).sum()) for _c, s, _e1 in runs)                 # the group's starts come first in the merged order
            assert max(U.T - before - n_starts, 0) == ends_in_tile_0
            masks = U.expected(name, strict, 1, False)[3]
            assert (masks >> np.uint64(63)).any(), "bit 63 is in the expected masks"


def _frame(rows, zero_based=True):
    df = pd.DataFrame(rows, columns=["chrom", "start", "end"])
    df.attrs["coordinate_system_zero_based"] = zero_based
    return df


@pytest.fixture
def no_engine(monkeypatch):
    """any attempt to create or fetch an engine fails the test"""
    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(_engine, "default_engine", boom)
    monkeypatch.setattr(_engine, "Engine", boom)
    monkeypatch.setattr(pb.range_op, "default_engine", boom)


@pytest.mark.parametrize("fn", ["multi_intersect", "consensus"])
def test_bad_arguments_raise_before_the_engine_is_touched(no_engine, fn):
    call = getattr(pb, fn)
    df = _frame([("chr1", 0, 5)])
    with pytest.raises(ValueError, match="between 1 and 64 frames"):
        call([], 1, output_type="pandas.DataFrame")
    with pytest.raises(ValueError, match="between 1 and 64 frames"):
        call([df] * 65, 1, output_type="pandas.DataFrame")
    for bad in (0, 4, -1):
        with pytest.raises(ValueError, match="min_frames must be in 1 .. 3"):
            call([df, df, df], bad, output_type="pandas.DataFrame")
    for bad in (True, False, 1.0, "2", None):
        with pytest.raises(ValueError, match="min_frames must be an int"):
            call([df, df, df], bad, output_type="pandas.DataFrame")
    with pytest.raises(pb.CoordinateSystemMismatchError):
        call([df, df, _frame([("chr1", 1, 5)], zero_based=False)], 1, output_type="pandas.DataFrame")


def test_bad_names_raise_before_the_engine_is_touched(no_engine):
    df = _frame([("chr1", 0, 5)])
    for names in (["a"], ["a", "b", "c"], ["a", "a"], ["a", 3], "ab", ["a", "mask"], ["n_frames", "b"], ["chrom", "b"]):
        with pytest.raises(ValueError, match="names"):
            pb.multi_intersect([df, df], names=names, output_type="pandas.DataFrame")
    with pytest.raises(ValueError, match="names collide"):
        pb.multi_intersect([df.assign(strand="+"), df.assign(strand="+")], names=["strand", "b"], on_cols=["strand"], output_type="pandas.DataFrame")


def test_engine_level_checks():
    for n, k in ((0, 1), (65, 1), (3, 0), (3, 4), (3, True), (3, 2.0)):
        with pytest.raises(ValueError):
            _engine.check_multi(n, k)
    with pytest.raises(ValueError):
        _engine.check_multi(3, 2, mode=2)
    assert _engine.check_multi(64, np.int64(64), _engine.MULTI_CONSENSUS) == 64
    assert (_engine.MAX_FRAMES, _engine.MULTI_SEGMENTS, _engine.MULTI_CONSENSUS) == (64, 0, 1)


def test_exports():
    for name in ("multi_intersect", "consensus"):
        assert name in pb.__all__ and callable(getattr(pb, name)) and name in pb.range_op.__all__
