"""pb.signal_summary / pb.signal_profile without a GPU: the yardstick of tests/_signal_util.py against hand-written cases and its
invariants, and the argument validation of both front-end functions, which fails before any engine is touched."""
import numpy as np
import pandas as pd
import pytest

import polars_bio_amd as pb
from polars_bio_amd import range_op
import _signal_util as U

I64, F64 = np.int64, np.float64


def _side(rows):
    a = np.array(rows, np.int64).reshape(-1, 3)
    return a[:, 0], a[:, 1], a[:, 2]


# ---- the yardstick, by hand ---------------------------------------------------------------------------------------------------------

def test_touching_intervals_in_both_conventions():
    probe = _side([(0, 10, 20)])
    build = _side([(0, 0, 10), (0, 20, 30), (0, 5, 11), (0, 19, 25)])
    v = np.array([100, 1000, 3, 7], I64)
    half_open = U.summary(probe, build, 1, True, v)                 # [0,10) and [20,30) touch [10,20): nothing shared
    assert half_open["count"] == [2] and half_open["sum"] == [3 * 1 + 7 * 1] and half_open["n"] == [2]
    closed = U.summary(probe, build, 1, False, v)                   # [0,10] and [20,30] share one position each with [10,20]
    assert closed["count"] == [1 + 1 + 2 + 2] and closed["sum"] == [100 + 1000 + 3 * 2 + 7 * 2]
    assert closed["min"] == [3] and closed["max"] == [1000]


def test_inside_around_and_across():
    probe = _side([(0, 100, 200)])
    build = _side([(0, 120, 130), (0, 0, 1000), (0, 50, 150), (0, 190, 400), (1, 100, 200)])
    v = np.array([2.0, 0.5, -4.0, 8.0, 99.0])
    got = U.summary(probe, build, 2, True, v)
    assert got["count"] == [10 + 100 + 50 + 10] and got["sum"] == [2.0 * 10 + 0.5 * 100 - 4.0 * 50 + 8.0 * 10]
    assert got["mean"] == [got["sum"][0] / 170.0] and got["min"] == [-4.0] and got["max"] == [8.0]


def test_null_values_zero_length_rows_and_rows_outside():
    probe = _side([(0, 10, 20), (0, 15, 15), (0, 20, 10), (5, 10, 20), (-1, 10, 20)])
    build = _side([(0, 12, 18), (0, 14, 14), (0, 0, 100), (0, 16, 12)])
    v = np.array([3, 1000, 5, 1000], I64)
    got = U.summary(probe, build, 1, True, v, valid=[True, True, False, True])
    assert got["count"] == [6, 0, 0, 0, 0] and got["sum"] == [18, 0, 0, 0, 0]
    assert got["mean"][1:] == [None] * 4 and got["min"][0] == 3
    closed = U.summary(probe, build, 1, False, v)                   # closed: (15, 15) and (14, 14) cover one position each
    assert closed["count"][:3] == [7 + 1 + 11, 1 + 1, 0] and closed["sum"][1] == 3 + 5


def test_thresholds_and_n_values_in_the_yardstick():
    probe = _side([(0, 0, 100)])
    build = _side([(0, 0, 3), (0, 10, 20), (0, 90, 200)])
    v = np.array([1, 10, 100], I64)
    assert U.summary(probe, build, 1, True, v, min_overlap=5)["sum"] == [10 * 10 + 100 * 10]
    assert U.summary(probe, build, 1, True, v, build_min=[0, U.NEVER, 11])["sum"] == [3]
    assert U.summary(probe, build, 1, True, v, n_values=2)["sum"] == [3 + 100]


def test_int64_sums_wrap_explicitly():
    probe = _side([(0, 0, 8)])
    build = _side([(0, 0, 4), (0, 4, 8)])
    got = U.summary(probe, build, 1, True, np.array([2 ** 62, 2 ** 62], I64))
    assert got["sum"] == [0] and got["count"] == [8] and got["max"] == [2 ** 62]          # 8 * 2^62 = 2^65 = 0 mod 2^64
    assert U.wrap64(2 ** 63) == -2 ** 63 and U.wrap64(-1) == -1


def test_reversed_window_and_fewer_positions_than_bins():
    windows = _side([(0, 10, 13), (0, 10, 13)])                     # 3 positions, 5 bins: lengths 0 1 0 1 1
    build = _side([(0, 10, 11), (0, 11, 13)])
    v = np.array([7, 2], I64)
    got = U.profile(windows, build, 1, True, 5, v, reverse=[False, True])
    assert got["sum"] == [0, 7, 0, 2, 2] + [2, 2, 0, 7, 0]
    assert got["count"] == [0, 1, 0, 1, 1] + [1, 1, 0, 1, 0]
    frame, lens = U.bin_frame(windows, False, 5, [False, True])
    assert lens.tolist() == [[0, 1, 1, 1, 1], [1, 1, 1, 1, 0]]      # closed: 4 positions
    assert frame[1].tolist()[:5] == [0, 10, 11, 12, 13] and frame[2].tolist()[:5] == [-1, 10, 11, 12, 13]


# ---- invariants ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strict", [True, False])
def test_value_one_gives_the_bases_of_mean_depth(strict):
    from _util import random_side
    rng = np.random.default_rng(3)
    probe, build = random_side(rng, 300, 3, 5000, 300), random_side(rng, 400, 3, 5000, 400)
    got = U.summary(probe, build, 3, strict, np.ones(400, I64))
    want = U.mean_depth_bases(probe, build, 3, strict)
    assert sum(want) > 1000
    assert got["sum"] == got["count"] == want.tolist()


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("n_bins", [1, 7, 64])
def test_a_profile_row_sums_to_the_summary_of_its_window(strict, n_bins):
    from _util import random_side
    rng = np.random.default_rng(n_bins)
    windows, build = random_side(rng, 40, 2, 3000, 200), random_side(rng, 300, 2, 3000, 100)
    v = rng.integers(-50, 50, 300).astype(I64)
    whole = U.summary(windows, build, 2, strict, v)
    bins = U.profile(windows, build, 2, strict, n_bins, v, reverse=rng.random(40) < 0.5)
    assert sum(whole["count"]) > 500
    assert np.array(bins["sum"], I64).reshape(40, n_bins).sum(axis=1).tolist() == whole["sum"]
    assert np.array(bins["count"], I64).reshape(40, n_bins).sum(axis=1).tolist() == whole["count"]


# ---- the front end's argument checks --------------------------------------------------------------------------------------------------

def _frames():
    df1 = pd.DataFrame({"chrom": ["1", "1"], "start": [0, 100], "end": [50, 200], "strand": ["+", "-"], "sum": [1, 2]})
    df2 = pd.DataFrame({"chrom": ["1", "1"], "start": [10, 120], "end": [20, 130], "score": [1.5, 2.5], "name": ["a", "b"], "n": [1, 2]})
    for df in (df1, df2):
        df.attrs["coordinate_system_zero_based"] = True
    return df1, df2


def test_the_operations_are_exported():
    assert "signal_summary" in pb.__all__ and "signal_profile" in pb.__all__
    df1, _ = _frames()
    assert callable(df1.pb.signal_summary) and callable(df1.pb.signal_profile)


@pytest.mark.parametrize("value, message", [("nope", "not found"), ("name", "has type"), ("start", "interval or on_cols"),
                                            ([], "non-empty list"), (["score", "score"], "twice"), (3, "name of a df2 column")])
def test_signal_summary_refuses_bad_value_columns(value, message):
    df1, df2 = _frames()
    with pytest.raises(ValueError, match=message):
        pb.signal_summary(df1, df2, value, output_type="pandas.DataFrame")


def test_signal_summary_refuses_name_collisions_and_bad_thresholds():
    df1, df2 = _frames()
    with pytest.raises(ValueError, match="'sum' of column 'score' collides"):
        pb.signal_summary(df1, df2, "score", output_type="pandas.DataFrame")
    with pytest.raises(ValueError, match="'size_n' of column 'n' collides"):
        pb.signal_summary(df1.rename(columns={"sum": "size_n"}), df2, ["score", "n"], output_type="pandas.DataFrame")
    with pytest.raises(ValueError):
        pb.signal_summary(df1.drop(columns="sum"), df2, "score", min_overlap=0, output_type="pandas.DataFrame")


@pytest.mark.parametrize("kw, message", [
    (dict(n_bins=0), "n_bins must be an int in 1 .. 4096"), (dict(n_bins=4097), "n_bins"), (dict(n_bins=2.0), "n_bins"), (dict(n_bins=True), "n_bins"),
    (dict(output="median"), "output must be one of"), (dict(anchor="tss"), "anchor must be None or one of"),
    (dict(upstream=5), "need an anchor"), (dict(anchor="start"), "needs upstream"), (dict(direction_col="nope"), "not found"),
    (dict(value="nope"), "not found"), (dict(value="name"), "has type"), (dict(value=["score"]), "one df2 column")])
def test_signal_profile_refuses_bad_arguments(kw, message):
    df1, df2 = _frames()
    kw = dict(dict(value="score"), **kw)
    with pytest.raises(ValueError, match=message):
        pb.signal_profile(df1, df2, output_type="pandas.DataFrame", **kw)


def test_depth_profile_keeps_its_messages():
    df1, df2 = _frames()
    with pytest.raises(ValueError, match="output must be 'mean' or 'bases', got 'sum'"):
        pb.depth_profile(df1, df2, output="sum")
    with pytest.raises(ValueError, match=r"n_bins must be an int in 1 \.\. 4096, got 0"):
        pb.depth_profile(df1, df2, n_bins=0)


def test_several_devices_are_refused(monkeypatch):
    class Many:
        pass
    monkeypatch.setattr(range_op, "default_engine", lambda: Many())
    df1, df2 = _frames()
    with pytest.raises(NotImplementedError, match="signal_summary needs a single-device engine"):
        pb.signal_summary(df1.drop(columns="sum"), df2, "score", output_type="pandas.DataFrame")
    with pytest.raises(NotImplementedError, match="signal_profile needs a single-device engine"):
        pb.signal_profile(df1, df2, "score", n_bins=4, output_type="pandas.DataFrame")
