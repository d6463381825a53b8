"""pb.signal_summary / pb.signal_profile on the GPU (signal.hip.h) through both entries -- host (Engine.overlap_wagg /
signal_profile) and device (DeviceJoin.overlap_wagg / signal_profile) -- compared bit for bit with the all-pairs yardstick of
tests/_signal_util.py.  Doubles are integer-valued with |sum of value * ov| < 2^53 unless a test says otherwise, so any summation
order is exact.  Every vacuity guard is asserted on the yardstick's output."""
import math

import numpy as np
import pytest

from polars_bio_amd import _engine, range_op
import _signal_util as U
from _util import random_side

pytestmark = pytest.mark.gpu

TILE, CHUNK, THREADS, WAVE = U.kernel_geometry()
PER = U.per_wave(CHUNK)
NEVER = U.NEVER
I64, F64 = np.int64, np.float64
ALL = ["sum", "min", "max", "mean", "count"]
OUTSIDE = 1 << 20                                    # a contig id outside every dictionary used here
IMIN, IMAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope="module")
def eng():
    return _engine.Engine(0)


@pytest.fixture(scope="module")
def dj():
    import torch  # noqa: F401
    from polars_bio_amd.device_api import DeviceJoin
    return DeviceJoin(0)


def _i32(side):
    return tuple(np.ascontiguousarray(a, np.int32) for a in side)


def _side(cols, row_id=None):
    import torch
    from polars_bio_amd.device_api import DeviceSide
    t = [torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in cols]
    return DeviceSide(*t, row_id=None if row_id is None else torch.from_numpy(np.ascontiguousarray(row_id, np.int32)).cuda())


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _min_dev(m):
    return None if m is None else _dev(np.ascontiguousarray(m, np.uint32).view(np.int32).copy())


def _lengths(side, strict):
    return np.asarray(side[2]).astype(np.int64) - np.asarray(side[1]).astype(np.int64) + (0 if strict else 1)


def _engine_kw(probe, build, strict, min_overlap=None, min_frac1=None, min_frac2=None, probe_min=None, build_min=None):
    """What the engine receives for a threshold set: fractions become minima (ANDed with given minima by the maximum)."""
    pm = None if probe_min is None else np.asarray(probe_min, np.uint32)
    bm = None if build_min is None else np.asarray(build_min, np.uint32)
    if min_frac1 is not None:
        f = range_op.min_bases(_lengths(probe, strict), min_frac1)
        pm = f if pm is None else np.maximum(pm, f)
    if min_frac2 is not None:
        f = range_op.min_bases(_lengths(build, strict), min_frac2)
        bm = f if bm is None else np.maximum(bm, f)
    return dict(min_overlap=int(min_overlap or 0), probe_min=pm, build_min=bm)


def _host(eng, probe, build, nc, strict, cols, kw, partition_mode=0):
    return eng.overlap_wagg(_i32(probe), _i32(build), strict, nc, agg=cols, partition_mode=partition_mode, **kw)


def _dev_cols(cols, n_values):
    return [(_dev(v[:n_values]), None if m is None else _dev(np.asarray(m)[:n_values].astype(np.uint8)), ops) for v, m, ops in cols]


def _device(dj, probe, build, nc, strict, cols, kw, partition_mode=0, n_values=None, row_id=None):
    n_values = len(build[0]) if n_values is None else n_values
    dkw = dict(min_overlap=kw["min_overlap"], probe_min=_min_dev(kw["probe_min"]), build_min=_min_dev(kw["build_min"]))
    res = dj.overlap_wagg(_side(probe, row_id), _side(build), strict, nc, _dev_cols(cols, n_values), partition_mode=partition_mode, **dkw)
    return [{op: t.cpu().numpy() for op, t in r.items()} for r in res]


def check(eng, dj, probe, build, nc, strict, cols, what="", partition_mode=0, **thr):
    """cols: [(values, valid or None, ops)].  Both entries against the yardstick -> the expected dicts, one per column."""
    kw = _engine_kw(probe, build, strict, **thr)
    exp = [U.summary(probe, build, nc, strict, v, m, **kw) for v, m, _ in cols]
    for name, got in (("host", _host(eng, probe, build, nc, strict, cols, kw, partition_mode)),
                      ("device", _device(dj, probe, build, nc, strict, cols, kw, partition_mode))):
        assert len(got) == len(cols)
        for k, (v, _, ops) in enumerate(cols):
            assert sorted(got[k]) == sorted(ops), f"{what} {name} column {k}: operations {sorted(got[k])}"
            U.assert_column(got[k], exp[k], v.dtype.type, f"{what} {name} column {k}")
    return exp


def _random(seed, n_probe, n_build, nc, span=20_000):
    rng = np.random.default_rng(seed)
    return random_side(rng, n_probe, nc, span, 300), random_side(rng, n_build, nc, span, 400)


def _values(rng, n, dtype, lo=-1000, hi=1000):
    return rng.integers(lo, hi, n).astype(dtype)


def _two_columns(rng, n):
    """One int64 and one double column (integer-valued), all five operations, the second with alternating-ish validity."""
    return [(_values(rng, n, I64), None, ALL), (_values(rng, n, F64), rng.random(n) < 0.6, ALL)]


# ---- summary: tile edges of the probe side, empty sides --------------------------------------------------------------------------

@pytest.mark.parametrize("n_probe", [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 1])
def test_probe_counts(eng, dj, n_probe):
    strict = n_probe % 2 == 0
    probe, build = _random(100 + n_probe, n_probe, 2000, 3, span=6000)
    exp = check(eng, dj, probe, build, 3, strict, _two_columns(np.random.default_rng(n_probe), 2000), f"{n_probe} probes")
    assert n_probe < 2 * TILE or sum(exp[0]["n"]) > 1000, "the case is vacuous"


@pytest.mark.parametrize("strict", [True, False])
def test_empty_build_side(eng, dj, strict):
    probe, _ = _random(7, TILE + 3, 1, 2)
    build = tuple(np.empty(0, np.int32) for _ in range(3))
    for thr in ({}, dict(min_overlap=2)):
        exp = check(eng, dj, probe, build, 2, strict, [(np.empty(0, I64), None, ALL), (np.empty(0, F64), None, ["sum", "count"])], "empty build", **thr)
        assert not any(exp[0]["count"])


# ---- one probe's run against the wavefront sub-ranges and the chunks ---------------------------------------------------------------

RUNS = [1, WAVE - 1, WAVE, WAVE + 1, PER - 1, PER, PER + 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
STARTS = sorted({0, 1} | {k * PER + d for k in range(1, CHUNK // PER + 1) for d in (-1, 0, 1)})


def _run_tiles(cases):
    """One tile of probes per (before, run) case, each in a contig of its own: a probe over `before` build rows, directly followed
    by a probe over `run` build rows, a probe over 3 rows further on; every other probe of the tile lies outside the dictionary.
    The build rows of a run END at different positions inside the probe (at + 3 + i % 7), so their overlap lengths with the probe
    (at + 2 .. at + 8) differ: a part folded into the wrong probe, or twice, changes the sum."""
    pc, ps, pe, bc, bs, be = [], [], [], [], [], []
    for t, (before, run) in enumerate(cases):
        c = np.full(TILE, OUTSIDE, np.int32)
        s, e = np.zeros(TILE, np.int32), np.ones(TILE, np.int32)
        for slot, at in ((5, 0), (6, 1000), (TILE - 7, 2000)):
            c[slot], s[slot], e[slot] = t, at + 2, at + 8
        pc.append(c); ps.append(s); pe.append(e)
        for at, k in ((0, before), (1000, run), (2000, 3)):
            bc.append(np.full(k, t, np.int32)); bs.append(np.full(k, at, np.int32) + (np.arange(k) % 3).astype(np.int32))
            be.append(np.full(k, at + 3, np.int32) + (np.arange(k) % 7).astype(np.int32))
    cat = lambda parts: np.concatenate(parts).astype(np.int32)
    return (cat(pc), cat(ps), cat(pe)), (cat(bc), cat(bs), cat(be)), len(cases)


@pytest.mark.parametrize("strict", [pytest.param(True, id="strict"), pytest.param(False, id="weak")])
def test_run_lengths_and_run_starts(eng, dj, strict):
    cases = [(before, run) for run in RUNS for before in (0, 3, PER)] + [(before, run) for before in STARTS for run in (PER + 1, 3 * CHUNK + 5)]
    probe, build, nc = _run_tiles(cases)
    rng = np.random.default_rng(9)
    nb = len(build[0])
    cols = [(_values(rng, nb, I64), None, ALL), (_values(rng, nb, F64), np.arange(nb) % 2 == 0, ALL)]
    exp = check(eng, dj, probe, build, nc, strict, cols, "runs")
    n = np.array(exp[0]["n"]).reshape(len(cases), TILE)
    # every row of a run starts at or before at + 2 and ends at or after at + 3: it shares a position with its probe in both conventions
    assert (n[:, 6] == [run for _, run in cases]).all() and (n[:, 5] == [before for before, _ in cases]).all() and (n[:, TILE - 7] == 3).all()
    bases = np.array(exp[0]["count"]).reshape(len(cases), TILE)
    assert len(set((bases[:, 6] / np.maximum(n[:, 6], 1)).round(3))) > 3, "the overlap lengths of the runs do not differ"


def test_candidates_that_share_nothing_interleaved_with_contributing_ones(eng, dj):
    # under one start: a row that ends where the probes begin (touches them in half-open frames), a zero-length row, a long row
    nb = 3000
    s = (np.arange(nb) // 3 * 4).astype(np.int32)
    kind = np.arange(nb) % 3
    e = np.where(kind == 0, 3000, np.where(kind == 1, s, s + 4000)).astype(np.int32)
    build = (np.zeros(nb, np.int32), s, e)
    ps = np.full(TILE + 5, 3000, np.int32)
    probe = (np.zeros(len(ps), np.int32), ps, (ps + 1 + np.arange(len(ps)) % 50).astype(np.int32))
    rng = np.random.default_rng(6)
    cols = _two_columns(rng, nb)
    exp = check(eng, dj, probe, build, 1, True, cols, "interleaved, half-open")
    plain = U.OU.expected(probe, build, 1, True, cols[0][0])
    assert min(exp[0]["n"]) > 300 and sum(exp[0]["n"]) < sum(plain["count"]), "no candidate of the plain predicate was left out"
    exp = check(eng, dj, probe, build, 1, False, cols, "interleaved, closed")
    assert min(exp[0]["n"]) > 600


# ---- values ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("validity", ["none_invalid", "alternating", "all_invalid", "null_pointer"])
def test_validity(eng, dj, validity):
    probe, build = _random(21, TILE + 9, 3000, 2, span=5000)
    rng = np.random.default_rng(1)
    nb = 3000
    valid = {"none_invalid": np.ones(nb, bool), "alternating": np.arange(nb) % 2 == 1, "all_invalid": np.zeros(nb, bool), "null_pointer": None}[validity]
    exp = check(eng, dj, probe, build, 2, True, [(_values(rng, nb, I64), valid, ALL), (_values(rng, nb, F64), valid, ALL)], validity)
    if validity == "all_invalid":
        assert not any(exp[0]["count"]) and not any(exp[1]["sum"])
    else:
        assert sum(exp[0]["n"]) > 10_000


def test_nan_and_wrapping_int64_sums(eng, dj):
    probe, build = _random(22, TILE - 1, 1998, 1, span=3000)
    # contig 1: two probes that meet one row each, ov = 4 and 5 (closed): 4 * 2^62 = 2^64 wraps to 0, 5 * -2^62 to -2^62
    probe = tuple(np.concatenate([a, np.array(x, np.int32)]) for a, x in zip(probe, ([1, 1], [0, 100], [10, 110])))
    build = tuple(np.concatenate([a, np.array(x, np.int32)]) for a, x in zip(build, ([1, 1], [2, 100], [5, 104])))
    rng = np.random.default_rng(8)
    nb = 2000
    x = _values(rng, nb, F64)
    x[rng.random(nb) < 0.003] = np.nan                              # few enough that some probes meet none
    big = rng.choice(np.array([2 ** 62, -2 ** 62], I64), nb)
    big[-2:] = [2 ** 62, -2 ** 62]
    exp = check(eng, dj, probe, build, 2, False, [(x, None, ALL), (big, None, ALL), (np.full(nb, np.nan), None, ALL)], "nan / wrap")
    assert any(isinstance(v, float) and math.isnan(v) for v in exp[0]["sum"]) and any(v is not None and not math.isnan(v) for v in exp[0]["mean"])
    assert exp[1]["count"][-2:] == [4, 5] and exp[1]["sum"][-2:] == [0, -2 ** 62] and exp[1]["min"][-2:] == [2 ** 62, -2 ** 62]
    assert max(exp[1]["n"]) > 50 and all(math.isnan(v) for v in exp[2]["min"] if v is not None)


def test_coordinates_at_the_int32_limits(eng, dj):
    # closed frames: the whole int32 range shares 2^32 positions with itself
    build = (np.zeros(4, np.int32), np.array([IMIN, IMIN, IMAX, 0], np.int32), np.array([IMAX, IMIN, IMAX, IMAX], np.int32))
    probe = (np.zeros(3, np.int32), np.array([IMIN, IMAX, IMIN], np.int32), np.array([IMAX, IMAX, IMIN + 9], np.int32))
    cols = [(np.array([3, 5, 7, 11], I64), None, ALL), (np.array([3.0, 5.0, 7.0, 11.0]), None, ALL)]
    exp = check(eng, dj, probe, build, 1, False, cols, "int32 limits, closed")
    assert exp[0]["count"][0] == 2 ** 32 + 1 + 1 + 2 ** 31 and exp[0]["sum"][0] == 3 * 2 ** 32 + 5 + 7 + 11 * 2 ** 31
    exp = check(eng, dj, probe, build, 1, True, cols, "int32 limits, half-open")
    assert exp[0]["count"][0] == 2 ** 32 - 1 + 2 ** 31 - 1


def test_n_values_smaller_than_the_build_side(eng, dj):
    probe, build = _random(23, TILE + 1, 2000, 2, span=4000)
    cols = _two_columns(np.random.default_rng(3), 2000)
    for n_values in (700, 1):
        got = _device(dj, probe, build, 2, False, cols, _engine_kw(probe, build, False), n_values=n_values)
        for k, (v, m, _) in enumerate(cols):
            U.assert_column(got[k], U.summary(probe, build, 2, False, v, m, n_values), v.dtype.type, f"n_values {n_values} column {k}")


def test_probe_row_id_is_ignored(eng, dj):
    probe, build = _random(24, TILE + 30, 2000, 2, span=4000)
    rng = np.random.default_rng(5)
    cols = _two_columns(rng, 2000)
    row_id = rng.permutation(len(probe[0])).astype(np.int32)
    exp = [U.summary(probe, build, 2, True, v, m) for v, m, _ in cols]
    assert sum(exp[0]["n"]) > 5000
    for pm in (0, 1):
        got = _device(dj, probe, build, 2, True, cols, _engine_kw(probe, build, True), partition_mode=pm, row_id=row_id)
        for k, (v, _, _) in enumerate(cols):
            U.assert_column(got[k], exp[k], v.dtype.type, f"row_id, partition_mode {pm}, column {k}")


@pytest.mark.parametrize("strict", [pytest.param(True, id="strict"), pytest.param(False, id="weak")])
def test_value_one_is_overlap_bases(eng, dj, strict):
    probe, build = _random(13, 2 * TILE, 3000, 3, span=5000)       # random_side makes zero-length rows on both sides
    probe[2][::7] = probe[1][::7] - 5                               # ... and these probes are inverted
    exp = check(eng, dj, probe, build, 3, strict, [(np.ones(3000, I64), None, ["count", "sum"])], "value 1")
    assert exp[0]["sum"] == exp[0]["count"] == U.mean_depth_bases(probe, build, 3, strict).tolist() and sum(exp[0]["count"]) > 100_000
    assert (eng.overlap_bases(_i32(probe), _i32(build), strict, 3) == np.array(exp[0]["count"])).all()


# ---- thresholds, bucketed probes ---------------------------------------------------------------------------------------------------

THRESHOLD_SETS = {
    "min_overlap": lambda p, b, rng: dict(min_overlap=7),
    "probe_min": lambda p, b, rng: dict(min_frac1=0.5),
    "build_min": lambda p, b, rng: dict(min_frac2=0.7),
    "all_three": lambda p, b, rng: dict(min_overlap=5, min_frac1=0.2, min_frac2=1 / 3),
    "never": lambda p, b, rng: dict(min_overlap=2, probe_min=rng.choice(np.array([0, 3, 40, NEVER], np.uint32), len(p[0])),
                                    build_min=rng.choice(np.array([0, 3, 40, NEVER], np.uint32), len(b[0]))),
}


@pytest.mark.parametrize("strict", [pytest.param(True, id="strict"), pytest.param(False, id="weak")])
@pytest.mark.parametrize("name", list(THRESHOLD_SETS))
def test_threshold_kinds(eng, dj, name, strict):
    probe, build = _random(11, TILE + 1, 4000, 24)
    thr = THRESHOLD_SETS[name](probe, build, np.random.default_rng(5))
    cols = _two_columns(np.random.default_rng(12), 4000)
    exp = check(eng, dj, probe, build, 24, strict, cols, name, **thr)
    plain = U.summary(probe, build, 24, strict, cols[0][0])
    assert 100 < sum(exp[0]["n"]) < sum(plain["n"]), "the threshold removed nothing, or everything"


@pytest.mark.parametrize("thresholded", [pytest.param(False, id="plain"), pytest.param(True, id="thresh")])
def test_bucketed_probes_write_at_their_position(eng, dj, thresholded):
    probe, build = _random(14, 3 * TILE + 77, 4000, 5)
    thr = dict(min_frac1=0.25, min_frac2=0.1) if thresholded else {}
    cols = _two_columns(np.random.default_rng(15), 4000)
    for pm in (0, 1):
        exp = check(eng, dj, probe, build, 5, True, cols, f"partition_mode {pm}", partition_mode=pm, **thr)
    assert sum(exp[0]["n"]) > 5000


@pytest.mark.parametrize("seed", range(20))
def test_random_sweep(eng, dj, seed):
    rng = np.random.default_rng(1000 + seed)
    n, m, nc = int(rng.integers(1, 2000)), int(rng.integers(1, 1500)), int(rng.integers(1, 6))
    probe, build = random_side(rng, n, nc, int(rng.integers(500, 30_000)), 300), random_side(rng, m, nc, 20_000, int(rng.integers(1, 3000)))
    cols = []
    for _ in range(int(rng.integers(1, 4))):
        ops = [op for op in ALL if rng.random() < 0.5] or ["sum"]
        valid = [None, rng.random(m) < rng.random()][int(rng.integers(0, 2))]
        cols.append((_values(rng, m, [I64, F64][int(rng.integers(0, 2))]), valid, ops))
    thr = [{}, dict(min_overlap=int(rng.integers(1, 50))), dict(min_frac1=float(rng.random() * 0.9 + 0.05)),
           dict(min_frac2=float(rng.random() * 0.9 + 0.05), min_overlap=3)][int(rng.integers(0, 4))]
    check(eng, dj, probe, build, nc, bool(seed % 2), cols, f"seed {seed}", partition_mode=int(seed % 3 == 0), **thr)


# ---- profile ---------------------------------------------------------------------------------------------------------------------

def _profile_both(eng, dj, windows, build, nc, strict, n_bins, cols, reverse):
    host = eng.signal_profile(_i32(windows), reverse, n_bins, _i32(build), strict, nc, agg=cols)
    dev = dj.signal_profile(_side(windows), _side(build), strict, nc, n_bins, _dev_cols(cols, len(build[0])),
                            reverse=None if reverse is None else _dev(np.asarray(reverse).astype(np.uint8)))
    return (("host", host), ("device", [{op: t.cpu().numpy() for op, t in r.items()} for r in dev]))


def check_profile(eng, dj, windows, build, nc, strict, n_bins, cols, reverse=None, what=""):
    """Both entries: each matrix equals the yardstick, and equals overlap_wagg over the explicit bin frame."""
    n = len(windows[0])
    frame, _ = U.bin_frame(windows, strict, n_bins, reverse)
    exp = [U.summary(frame, build, nc, strict, v, m) for v, m, _ in cols]
    flat = _host(eng, frame, build, nc, strict, cols, _engine_kw(frame, build, strict))
    for name, got in _profile_both(eng, dj, windows, build, nc, strict, n_bins, cols, reverse):
        for k, (v, _, ops) in enumerate(cols):
            assert sorted(got[k]) == sorted(ops)
            for op in ops:
                assert got[k][op].shape == (n, n_bins), f"{what} {name} {op}: shape {got[k][op].shape}"
            U.assert_column({op: a.reshape(-1) for op, a in got[k].items()}, exp[k], v.dtype.type, f"{what} {name} B={n_bins} column {k}")
            U.assert_column(flat[k], exp[k], v.dtype.type, f"{what} explicit bin frame B={n_bins} column {k}")
    return exp


def _windows(rng, n, n_bins, nc, span):
    """Windows of every interesting length around n_bins (0, 1, n_bins - 1, n_bins, n_bins + 1) and random ones, some on a contig
    without build rows (nc) and outside the dictionary."""
    special = np.array([0, 1, max(n_bins - 1, 0), n_bins, n_bins + 1])
    ln = np.where(np.arange(n) % 2 == 0, special[(np.arange(n) // 2) % 5], rng.integers(0, 3 * n_bins + 50, n))
    s = rng.integers(0, span, n)
    c = rng.integers(0, nc, n)
    c[rng.random(n) < 0.1] = nc                                    # a contig of the dictionary that has no build rows
    c[rng.random(n) < 0.05] = OUTSIDE
    return c.astype(np.int32), s.astype(np.int32), ln


@pytest.mark.parametrize("strict", [pytest.param(True, id="strict"), pytest.param(False, id="weak")])
@pytest.mark.parametrize("n_bins", [1, 2, 3, 63, 64, 65, TILE - 1, TILE, TILE + 1, 4096])
def test_profile_bin_counts(eng, dj, n_bins, strict):
    rng = np.random.default_rng(n_bins)
    # n * n_bins both a multiple of the tile and not
    for n in ([TILE, TILE + 3] if n_bins <= 3 else [16, 11] if n_bins < TILE - 1 else [2, 3]):
        c, s, ln = _windows(rng, n, n_bins, 2, 4000)
        windows = (c, s, (s + ln - (0 if strict else 1)).astype(np.int32))
        build = random_side(rng, 600, 2, 4000 + 3 * n_bins, 60)
        cols = [(_values(rng, 600, I64), None, ALL), (_values(rng, 600, F64), rng.random(600) < 0.7, ["sum", "mean", "count"])]
        exp = check_profile(eng, dj, windows, build, 3, strict, n_bins, cols, reverse=rng.random(n) < 0.4, what=f"n={n}")
        assert sum(exp[0]["n"]) > 50


@pytest.mark.parametrize("strict", [pytest.param(True, id="strict"), pytest.param(False, id="weak")])
def test_profile_at_the_int32_limits_and_rows_over_all_bins(eng, dj, strict):
    w = 0 if strict else 1
    windows = (np.array([0, 0, 0, 0, 1], np.int32), np.array([IMAX - 700, IMIN, IMIN, 100, 0], np.int32),
               np.array([IMAX, IMIN + 500 - w, IMAX, 900 - w, 50], np.int32))
    # a build row over everything, one over the first windows' bins, short rows at both ends
    build = (np.zeros(6, np.int32), np.array([IMIN, IMIN, IMAX - 300, 0, 400, IMAX - 5], np.int32),
             np.array([IMAX, IMIN + 40, IMAX, 1000, 410, IMAX], np.int32))
    cols = [(np.array([1, 10, 100, 1000, 5, -3], I64), None, ALL), (np.array([1.0, 10, 100, 1000, 5, -3]), None, ALL)]
    for n_bins in (7, 64):
        exp = check_profile(eng, dj, windows, build, 2, strict, n_bins, cols, reverse=[False, True, False, True, False], what="limits")
        n = np.array(exp[0]["n"]).reshape(5, n_bins)
        assert (n[:4] >= 1).all() and (n[3] >= 2).all() and (n[4] == 0).all()


def test_profile_without_build_rows_or_windows(eng, dj):
    rng = np.random.default_rng(2)
    empty = tuple(np.empty(0, np.int32) for _ in range(3))
    c, s, ln = _windows(rng, 9, 5, 2, 100)
    windows = (c, s, (s + ln).astype(np.int32))
    for name, got in _profile_both(eng, dj, windows, empty, 2, True, 5, [(np.empty(0, I64), None, ["sum", "count"])], None):
        assert got[0]["sum"].shape == (9, 5) and not got[0]["sum"].any() and not got[0]["count"].any(), name
    build = random_side(rng, 50, 2, 100, 30)
    for name, got in _profile_both(eng, dj, empty, build, 2, True, 5, [(np.ones(50, I64), None, ALL)], None):
        assert got[0]["sum"].shape == (0, 5), name


# ---- argument errors, untouched buffers --------------------------------------------------------------------------------------------

def test_einval_estate_and_untouched_buffers(eng, dj):
    import torch
    probe, build = _random(41, 10, 20, 1, span=300)
    v = np.arange(20, dtype=I64)
    for bad_agg in ([], [(v, None, 32)], [(v, None, 0)], [(v, None, ["sum"])] * (_engine.MAX_AGG_COLS + 1)):
        with pytest.raises(_engine.EngineError) as e:
            eng.overlap_wagg(probe, build, True, 1, agg=bad_agg)
        assert e.value.code == -1, bad_agg
        with pytest.raises(_engine.EngineError) as e:
            eng.signal_profile(probe, None, 4, build, True, 1, agg=bad_agg)
        assert e.value.code == -1, bad_agg
    for n_bins in (0, -1, 4097):
        with pytest.raises(_engine.EngineError) as e:
            eng.signal_profile(probe, None, n_bins, build, True, 1, agg=[(v, None, ["sum"])])
        assert e.value.code == -1, n_bins
    opts = _engine.make_opts(True, 1)
    dp, db = _side(probe), _side(build)
    SENT = 0x5A5A5A5A5A5A5A5A
    bufs = {op: torch.full((10 * 4,), SENT, dtype=torch.int64, device="cuda") for op in ALL}
    dv = _dev(v)
    good = [(dv.data_ptr(), 0, _engine.AGG_I64, _engine.AGG_SUM | _engine.AGG_COUNT)]
    outs = [{op: t.data_ptr() for op, t in bufs.items()}]
    summary = lambda ix, thr, cols, o: eng.overlap_wagg_dev(ix, dp.as_c(), opts, thr, 20, cols, o)
    profile = lambda ix, thr, cols, o, n_bins=4: eng.signal_profile_dev(ix, dp.as_c(), 0, n_bins, opts, 20, cols, o)
    ix = eng.index_build_dev(db.as_c(), opts, False)
    try:
        for call, n_out, exp in ((summary, 10, U.summary(probe, build, 1, True, v)), (profile, 40, U.profile(probe, build, 1, True, 4, v))):
            for t in bufs.values():
                t.fill_(SENT)
            call(ix, None, good, outs)                                                                                    # the valid call
            eng.sync()
            assert sum(exp["n"]) > 5
            U.assert_column({op: bufs[op].cpu().numpy()[:n_out] for op in ("sum", "count")}, exp, I64, "valid call")
            for op in ("min", "max", "mean"):
                assert (bufs[op].cpu().numpy() == SENT).all(), f"the buffer of '{op}' was written"
            for cols, o, thr in (
                    ([(dv.data_ptr(), 0, 7, _engine.AGG_SUM)], outs, None),                                                 # unknown dtype
                    ([(0, 0, _engine.AGG_I64, _engine.AGG_SUM)], outs, None),                                               # NULL values
                    ([(dv.data_ptr(), 0, _engine.AGG_I64, _engine.AGG_SUM | _engine.AGG_MAX)], [{"sum": bufs["sum"].data_ptr()}], None)):   # NULL output
                with pytest.raises(_engine.EngineError) as e:
                    call(ix, thr, cols, o)
                assert e.value.code == -1
        with pytest.raises(_engine.EngineError) as e:                                                                     # thresholds with nothing set
            summary(ix, _engine.make_thresholds(0, 0, 0), good, outs)
        assert e.value.code == -1
        for n_bins in (0, 4097):
            with pytest.raises(_engine.EngineError) as e:
                profile(ix, None, good, outs, n_bins)
            assert e.value.code == -1
    finally:
        ix.close()
    sweep = eng.index_build_dev(db.as_c(), opts, False, sweep_only=True)
    try:
        for call in (summary, profile):
            with pytest.raises(_engine.EngineError) as e:
                call(sweep, None, good, outs)
            assert e.value.code == _engine.IVJ_ESTATE
    finally:
        sweep.close()
    eng.sync()


# ---- doubles that do round --------------------------------------------------------------------------------------------------------

def test_random_doubles_error_bound_and_repeatability(eng, dj):
    """Per probe |sum - fsum(v_i * ov_i)| <= (n + 1) * 2^-53 * sum|v_i * ov_i| * (1 + 2^-40): n - 1 additions, one rounding per
    product on the device and one for the yardstick's own float products, each at most 2^-53 relative to a quantity bounded by
    sum|v_i * ov_i| -- to first order; the factor of the higher orders is granted as in the map_overlaps test.  The same call
    twice, on the host entry and on the device entry: identical bits."""
    probe, build = _random(31, 2 * TILE + 5, 6000, 2, span=3000)
    rng = np.random.default_rng(32)
    x = rng.standard_normal(6000) * np.exp(rng.uniform(-20, 20, 6000))
    cols = [(x, None, ALL)]
    kw = _engine_kw(probe, build, True)
    a = _host(eng, probe, build, 2, True, cols, kw)[0]
    b = _host(eng, probe, build, 2, True, cols, kw)[0]
    d1 = _device(dj, probe, build, 2, True, cols, kw)[0]
    d2 = _device(dj, probe, build, 2, True, cols, kw)[0]
    for op in ALL:
        for other in (b, d1, d2):
            assert (a[op].view(np.uint64) == other[op].view(np.uint64)).all(), f"{op} differs between two calls"
    pc, ps, pe = (np.asarray(t).astype(np.int64) for t in probe)
    bc, bs, be = (np.asarray(t).astype(np.int64) for t in build)
    worst = 0
    for k in range(len(pc)):
        ov = np.minimum(pe[k], be) - np.maximum(ps[k], bs)
        hit = (bc == pc[k]) & (ov >= 1)
        n = int(hit.sum())
        assert a["count"][k] == ov[hit].sum()
        if n == 0:
            continue
        prods = [float(v) * float(o) for v, o in zip(x[hit], ov[hit])]
        bound = (n + 1) * 2.0 ** -53 * math.fsum(abs(p) for p in prods) * (1 + 2.0 ** -40)
        err = abs(a["sum"][k] - math.fsum(prods))
        print(f"probe {k}: n = {n}, |sum - fsum| = {err}, bound = {bound}")
        assert err <= bound, f"probe {k}: |sum - fsum| = {err} > {bound} over {n} values"
        assert a["min"][k] == x[hit].min() and a["max"][k] == x[hit].max()
        worst = max(worst, n)
    assert worst > 500
