"""pb.map_overlaps on the GPU (overlap_agg.hip.h) through both entries -- host (Engine.overlap_agg = ivj_overlap_agg) and device
(DeviceJoin.overlap_agg = ivj_overlap_agg_dev) -- compared bit for bit with the literal group-by of tests/_overlap_agg_util.py.
Doubles are integer-valued with |sum| < 2^53 unless a test says otherwise, so any summation order is exact."""
import math

import numpy as np
import pytest

from polars_bio_amd import _engine, range_op
import _overlap_agg_util as U
from _util import random_side

pytestmark = pytest.mark.gpu

TILE, CHUNK, THREADS, WAVE = U.kernel_geometry()
NEVER = U.T.NEVER
I64, F64 = np.int64, np.float64
ALL = ["sum", "min", "max", "mean", "count"]
OUTSIDE = 1 << 20                                    # a contig id outside every dictionary used here


@pytest.fixture(scope="module")
def eng():
    return _engine.Engine(0)


@pytest.fixture(scope="module")
def dj():
    import torch  # noqa: F401
    from polars_bio_amd.device_api import DeviceJoin
    return DeviceJoin(0)


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
    return side[2].astype(np.int64) - side[1].astype(np.int64) + (0 if strict else 1)


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
    return eng.overlap_agg(probe, build, strict, nc, agg=cols, partition_mode=partition_mode, **kw)


def _device(dj, probe, build, nc, strict, cols, kw, partition_mode=0, n_values=None, row_id=None):
    n_values = len(build[0]) if n_values is None else n_values
    agg = [(_dev(v[:n_values]), None if m is None else _dev(np.asarray(m)[:n_values].astype(np.uint8)), ops) for v, m, ops in cols]
    dkw = dict(min_overlap=kw["min_overlap"], probe_min=_min_dev(kw["probe_min"]), build_min=_min_dev(kw["build_min"]))
    res = dj.overlap_agg(_side(probe, row_id), _side(build), strict, nc, agg, partition_mode=partition_mode, **dkw)
    return [{op: t.cpu().numpy() for op, t in r.items()} for r in res]


def check(eng, dj, probe, build, nc, strict, cols, what="", partition_mode=0, **thr):
    """cols: [(values, valid or None, ops)].  Both entries against the yardstick -> the expected dicts, one per column."""
    kw = _engine_kw(probe, build, strict, **thr)
    p, b = U.pairs(probe, build, nc, strict, **thr)
    exp = [U.group_by(p, b, len(probe[0]), v, m) for v, m, _ in cols]
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


# ---- tile edges of the probe side, empty sides -------------------------------------------------------------------------------

@pytest.mark.parametrize("n_probe", [0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 1])
def test_probe_counts(eng, dj, n_probe):
    strict = n_probe % 2 == 0
    probe, build = _random(100 + n_probe, n_probe, 3000, 3, span=6000)
    exp = check(eng, dj, probe, build, 3, strict, _two_columns(np.random.default_rng(n_probe), 3000), f"{n_probe} probes")
    assert n_probe < 2 * TILE or sum(exp[0]["count"]) > 1000, "the case is vacuous"


@pytest.mark.parametrize("strict", [True, False])
def test_empty_build_side(eng, dj, strict):
    probe, _ = _random(7, TILE + 3, 1, 2)
    build = tuple(np.empty(0, np.int32) for _ in range(3))
    for thr in ({}, dict(min_overlap=2)):
        exp = check(eng, dj, probe, build, 2, strict, [(np.empty(0, I64), None, ALL), (np.empty(0, F64), None, ["sum", "count"])], "empty build", **thr)
        assert not any(exp[0]["count"])


def test_probes_without_candidates_between_probes_with_many(eng, dj):
    rng = np.random.default_rng(2)
    nb = 6000
    build = (np.zeros(nb, np.int32), rng.integers(0, 2000, nb).astype(np.int32), None)
    build = (build[0], build[1], (build[1] + rng.integers(1, 50, nb)).astype(np.int32))
    n = 2 * TILE + 40
    c = np.where(np.arange(n) % 3 == 1, 0, np.where(np.arange(n) % 3 == 0, 1, OUTSIDE)).astype(np.int32)   # contig 1 has no build rows
    s = rng.integers(0, 2000, n).astype(np.int32)
    probe = (c, s, (s + rng.integers(1, 400, n)).astype(np.int32))
    for strict in (True, False):
        exp = check(eng, dj, probe, build, 2, strict, _two_columns(rng, nb), "gaps")
        cnt = np.array(exp[0]["count"])
        assert (cnt[c != 0] == 0).all() and cnt[c == 0].min() >= 0 and cnt.max() > 500


# ---- one probe's run against the wavefront sub-ranges and the chunks -----------------------------------------------------------

PER = U.per_wave(CHUNK)
RUNS = [1, WAVE - 1, WAVE, WAVE + 1, PER - 1, PER, PER + 1, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5]
# candidates before the run inside its tile: the run begins at (and around, should a loose range hold a row more) every
# wavefront sub-range boundary of a full chunk and at the chunk boundary
STARTS = sorted({0, 1} | {k * PER + d for k in range(1, CHUNK // PER + 1) for d in (-1, 0, 1)})


def _run_tiles(cases):
    """One tile of probes per (before, run) case, each in a contig of its own: a probe over `before` build rows, directly followed
    by a probe over `run` build rows, a probe over 3 rows further on; every other probe of the tile lies outside the dictionary."""
    pc, ps, pe, bc, bs, be = [], [], [], [], [], []
    for t, (before, run) in enumerate(cases):
        c = np.full(TILE, OUTSIDE, np.int32)
        s, e = np.zeros(TILE, np.int32), np.ones(TILE, np.int32)
        for slot, at in ((5, 0), (6, 1000), (TILE - 7, 2000)):
            c[slot], s[slot], e[slot] = t, at + 2, at + 8
        pc.append(c); ps.append(s); pe.append(e)
        for at, k in ((0, before), (1000, run), (2000, 3)):
            bc.append(np.full(k, t, np.int32)); bs.append(np.full(k, at, np.int32) + (np.arange(k) % 3).astype(np.int32))
            be.append(np.full(k, at + 10, np.int32))
    cat = lambda parts: np.concatenate(parts).astype(np.int32)
    return (cat(pc), cat(ps), cat(pe)), (cat(bc), cat(bs), cat(be)), len(cases)


@pytest.mark.parametrize("strict", [pytest.param(True, id="strict"), pytest.param(False, id="weak")])
@pytest.mark.parametrize("thresholded", [pytest.param(False, id="plain"), pytest.param(True, id="thresh")])
def test_run_lengths_and_run_starts(eng, dj, strict, thresholded):
    # every run length after a short neighbour, and a chunk-sized as well as a multi-chunk run at every start
    cases = [(before, run) for run in RUNS for before in (0, 3, PER)] + [(before, run) for before in STARTS for run in (PER + 1, 3 * CHUNK + 5)]
    probe, build, nc = _run_tiles(cases)
    rng = np.random.default_rng(9)
    nb = len(build[0])
    cols = [(_values(rng, nb, I64), None, ALL), (_values(rng, nb, F64), np.arange(nb) % 2 == 0, ALL)]
    exp = check(eng, dj, probe, build, nc, strict, cols, "runs", **(dict(min_overlap=2) if thresholded else {}))
    cnt = np.array(exp[0]["count"]).reshape(len(cases), TILE)
    assert (cnt[:, 6] == [run for _, run in cases]).all() and (cnt[:, 5] == [before for before, _ in cases]).all() and (cnt[:, TILE - 7] == 3).all()


def test_contig_wide_row_keeps_ranges_open(eng, dj):
    # one row over the whole contig in front of 5000 short rows: the ranges of the probes at the far end reach back to it
    nb = 5001
    s = np.concatenate([[0], 10 + 20 * np.arange(5000)]).astype(np.int32)
    e = np.concatenate([[200_000], 10 + 20 * np.arange(5000) + 15]).astype(np.int32)
    build = (np.zeros(nb, np.int32), s, e)
    ps = (99_000 + 20 * np.arange(40)).astype(np.int32)
    probe = (np.zeros(40, np.int32), ps, (ps + 30).astype(np.int32))
    rng = np.random.default_rng(4)
    for strict in (True, False):
        exp = check(eng, dj, probe, build, 1, strict, _two_columns(rng, nb), "contig-wide")
        assert max(exp[0]["count"]) <= 4 and min(exp[0]["count"]) >= 2
        check(eng, dj, probe, build, 1, strict, _two_columns(rng, nb), "contig-wide, thresholded", min_overlap=12)


def test_failing_candidates_interleaved_with_passing_ones(eng, dj):
    # nested rows of alternating length under one start: every other candidate of a probe fails the predicate
    nb = 3000
    s = (np.arange(nb) // 2 * 4).astype(np.int32)
    e = np.where(np.arange(nb) % 2 == 0, s + 3, s + 4000).astype(np.int32)
    build = (np.zeros(nb, np.int32), s, e)
    ps = (3000 + 7 * np.arange(TILE + 5)).astype(np.int32)
    probe = (np.zeros(len(ps), np.int32), ps, (ps + 2).astype(np.int32))
    rng = np.random.default_rng(6)
    exp = check(eng, dj, probe, build, 1, True, _two_columns(rng, nb), "interleaved")
    assert min(exp[0]["count"]) > 300
    check(eng, dj, probe, build, 1, False, _two_columns(rng, nb), "interleaved, thresholded", min_frac2=0.0004)


# ---- values ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("validity", ["none_invalid", "alternating", "all_invalid", "null_pointer"])
def test_validity(eng, dj, validity):
    probe, build = _random(21, TILE + 9, 4000, 2, span=5000)
    rng = np.random.default_rng(1)
    nb = 4000
    valid = {"none_invalid": np.ones(nb, bool), "alternating": np.arange(nb) % 2 == 1, "all_invalid": np.zeros(nb, bool), "null_pointer": None}[validity]
    exp = check(eng, dj, probe, build, 2, True, [(_values(rng, nb, I64), valid, ALL), (_values(rng, nb, F64), valid, ALL)], validity)
    if validity == "all_invalid":
        assert not any(exp[0]["count"]) and not any(exp[1]["sum"])
    else:
        assert sum(exp[0]["count"]) > 10_000


def test_nan_wrapping_sums_and_int64_limits(eng, dj):
    probe, build = _random(22, TILE + 1, 3000, 1, span=3000)
    rng = np.random.default_rng(8)
    nb = 3000
    x = _values(rng, nb, F64)
    x[rng.random(nb) < 0.002] = np.nan                              # few enough that some probes meet none
    big = rng.choice(np.array([2 ** 62, -2 ** 62, 2 ** 63 - 1, -2 ** 63, 5, -7], I64), nb)
    exp = check(eng, dj, probe, build, 1, True, [(x, None, ALL), (big, None, ALL), (np.full(nb, np.nan), None, ALL)], "nan / wrap / limits")
    assert any(isinstance(v, float) and math.isnan(v) for v in exp[0]["sum"]) and any(v is not None and not math.isnan(v) for v in exp[0]["sum"])
    assert 2 ** 63 - 1 in exp[1]["max"] and -2 ** 63 in exp[1]["min"]
    assert all(math.isnan(v) for v in exp[2]["min"] if v is not None)


def test_n_values_smaller_than_the_build_side(eng, dj):
    probe, build = _random(23, TILE + 1, 3000, 2, span=4000)
    rng = np.random.default_rng(3)
    cols = _two_columns(rng, 3000)
    for n_values in (1000, 1):
        p, b = U.pairs(probe, build, 2, False)
        got = _device(dj, probe, build, 2, False, cols, _engine_kw(probe, build, False), n_values=n_values)
        for k, (v, m, _) in enumerate(cols):
            U.assert_column(got[k], U.group_by(p, b, len(probe[0]), v, m, n_values), v.dtype.type, f"n_values {n_values} column {k}")


def test_probe_row_id_is_ignored(eng, dj):
    probe, build = _random(24, TILE + 30, 2000, 2, span=4000)
    rng = np.random.default_rng(5)
    cols = _two_columns(rng, 2000)
    row_id = rng.permutation(len(probe[0])).astype(np.int32)
    p, b = U.pairs(probe, build, 2, True)
    for pm in (0, 1):
        got = _device(dj, probe, build, 2, True, cols, _engine_kw(probe, build, True), partition_mode=pm, row_id=row_id)
        for k, (v, m, _) in enumerate(cols):
            U.assert_column(got[k], U.group_by(p, b, len(probe[0]), v, m), v.dtype.type, f"row_id, partition_mode {pm}, column {k}")


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
    probe, build = _random(11, TILE + 1, 5000, 24)
    thr = THRESHOLD_SETS[name](probe, build, np.random.default_rng(5))
    cols = _two_columns(np.random.default_rng(12), 5000)
    exp = check(eng, dj, probe, build, 24, strict, cols, name, **thr)
    plain = U.expected(probe, build, 24, strict, cols[0][0])
    assert 100 < sum(exp[0]["count"]) < sum(plain["count"]), "the threshold removed nothing, or everything"
    cnt = eng.count_overlaps_thresh(probe, build, strict, 24, **_engine_kw(probe, build, strict, **thr))
    assert (cnt == np.array(exp[0]["count"])).all()


@pytest.mark.parametrize("strict", [pytest.param(True, id="strict"), pytest.param(False, id="weak")])
def test_plain_count_is_count_overlaps_also_for_rows_without_a_position(eng, dj, strict):
    probe, build = _random(13, 2 * TILE, 4000, 3, span=5000)       # random_side makes zero-length rows on both sides
    probe[2][::7] = probe[1][::7] - 5                               # ... and these probes are inverted
    exp = check(eng, dj, probe, build, 3, strict, [(np.ones(4000, I64), None, ["count", "sum"])], "plain count")
    assert (eng.count_overlaps(probe, build, strict, 3) == np.array(exp[0]["count"])).all()


@pytest.mark.parametrize("thresholded", [pytest.param(False, id="plain"), pytest.param(True, id="thresh")])
def test_bucketed_probes_write_at_their_position(eng, dj, thresholded):
    probe, build = _random(14, 3 * TILE + 77, 6000, 5)
    thr = dict(min_frac1=0.25, min_frac2=0.1) if thresholded else {}
    cols = _two_columns(np.random.default_rng(15), 6000)
    exp = check(eng, dj, probe, build, 5, True, cols, "partition_mode 1", partition_mode=1, **thr)
    assert sum(exp[0]["count"]) > 10_000


# ---- several columns, untouched buffers -------------------------------------------------------------------------------------------

def test_three_columns_with_different_masks_leave_other_buffers_alone(eng, dj):
    import torch
    probe, build = _random(16, TILE + 20, 3000, 2, span=5000)
    rng = np.random.default_rng(17)
    nb, n = 3000, TILE + 20
    cols = [(_values(rng, nb, I64), None, ["sum"]), (_values(rng, nb, F64), rng.random(nb) < 0.5, ["min", "max", "count"]),
            (_values(rng, nb, I64), None, ["mean", "count"])]
    check(eng, dj, probe, build, 2, True, cols, "three columns")
    # the device entry with all five buffers given per column, sentinel-filled: only the operations asked for are written
    opts = _engine.make_opts(True, 2)
    dp, db = _side(probe), _side(build)
    ix = eng.index_build_dev(db.as_c(), opts, True)
    try:
        vals = [_dev(v) for v, _, _ in cols]
        valid = [None if m is None else _dev(np.asarray(m).astype(np.uint8)) for _, m, _ in cols]
        bufs = [{op: torch.full((n,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda") for op in ALL} for _ in cols]
        eng.overlap_agg_dev(ix, dp.as_c(), opts, None, nb,
                            [(vals[k].data_ptr(), valid[k].data_ptr() if valid[k] is not None else 0,
                              _engine.AGG_I64 if cols[k][0].dtype == I64 else _engine.AGG_F64, _engine.agg_ops_mask(cols[k][2])) for k in range(3)],
                            [{op: t.data_ptr() for op, t in b.items()} for b in bufs])
        eng.sync()
        p, b = U.pairs(probe, build, 2, True)
        for k, (v, m, ops) in enumerate(cols):
            exp = U.group_by(p, b, n, v, m)
            kinds = {"sum": v.dtype, "min": v.dtype, "max": v.dtype, "mean": F64, "count": I64}
            for op in ALL:
                raw = bufs[k][op].cpu().numpy()
                if op in ops:
                    U.assert_column({op: raw.view(kinds[op])}, exp, v.dtype.type, f"column {k}")
                else:
                    assert (raw == 0x5A5A5A5A5A5A5A5A).all(), f"column {k}: the buffer of '{op}' was written"
    finally:
        ix.close()


# ---- random sweep -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(30))
def test_random_sweep(eng, dj, seed):
    rng = np.random.default_rng(1000 + seed)
    n, m, nc = int(rng.integers(1, 4000)), int(rng.integers(1, 2000)), int(rng.integers(1, 6))
    probe, build = random_side(rng, n, nc, int(rng.integers(500, 30_000)), 300), random_side(rng, m, nc, 20_000, int(rng.integers(1, 3000)))
    cols = []
    for _ in range(int(rng.integers(1, 4))):
        ops = [op for op in ALL if rng.random() < 0.5] or ["sum"]
        valid = [None, rng.random(m) < rng.random()][int(rng.integers(0, 2))]
        cols.append((_values(rng, m, [I64, F64][int(rng.integers(0, 2))]), valid, ops))
    thr = [{}, dict(min_overlap=int(rng.integers(1, 50))), dict(min_frac1=float(rng.random() * 0.9 + 0.05)),
           dict(min_frac2=float(rng.random() * 0.9 + 0.05), min_overlap=3)][int(rng.integers(0, 4))]
    check(eng, dj, probe, build, nc, bool(seed % 2), cols, f"seed {seed}", partition_mode=int(seed % 3 == 0), **thr)


# ---- doubles that do round --------------------------------------------------------------------------------------------------------

def test_random_doubles_error_bound_and_repeatability(eng, dj):
    """|sum - fsum| <= (n - 1) * 2^-53 * sum|x| per probe: the bound of any summation order of n doubles (every one of the n - 1
    additions rounds by at most 2^-53 relative to a partial sum that is at most sum|x| -- to first order; the factor the higher
    orders add, (1 + 2^-53)^(n-1), is below 1 + 2^-40 for the n here and is granted).  The same call twice: identical bits."""
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
    p, bb = U.pairs(probe, build, 2, True)
    order = np.argsort(p, kind="stable")
    p, bb = p[order], bb[order]
    first, last = np.searchsorted(p, np.arange(len(probe[0])), "left"), np.searchsorted(p, np.arange(len(probe[0])), "right")
    worst = 0
    for k in range(len(probe[0])):
        v = x[bb[first[k]:last[k]]]
        n = len(v)
        assert a["count"][k] == n
        if n == 0:
            continue
        bound = (n - 1) * 2.0 ** -53 * math.fsum(np.abs(v)) * (1 + 2.0 ** -40)
        err = abs(a["sum"][k] - math.fsum(v))
        assert err <= bound, f"probe {k}: |sum - fsum| = {err} > {bound} over {n} values"
        assert a["min"][k] == v.min() and a["max"][k] == v.max()
        worst = max(worst, n)
    assert worst > 500


# ---- argument errors --------------------------------------------------------------------------------------------------------------

def test_einval_and_estate(eng, dj):
    import torch
    probe, build = _random(41, 10, 20, 1)
    v = np.arange(20, dtype=I64)
    for bad_agg in ([], [(v, None, 32)], [(v, None, 0)], [(v, None, ["sum"])] * (_engine.MAX_AGG_COLS + 1)):
        with pytest.raises(_engine.EngineError) as e:
            eng.overlap_agg(probe, build, True, 1, agg=bad_agg)
        assert e.value.code == -1, bad_agg
    opts = _engine.make_opts(True, 1)
    dp, db = _side(probe), _side(build)
    out = torch.zeros(10, dtype=torch.int64, device="cuda")
    dv = _dev(v)
    call = lambda ix, thr, cols, outs: eng.overlap_agg_dev(ix, dp.as_c(), opts, thr, 20, cols, outs)
    ix = eng.index_build_dev(db.as_c(), opts, True)
    try:
        call(ix, None, [(dv.data_ptr(), 0, _engine.AGG_I64, _engine.AGG_SUM)], [{"sum": out.data_ptr()}])            # the valid call
        for cols, outs, thr in (
                ([(dv.data_ptr(), 0, 7, _engine.AGG_SUM)], [{"sum": out.data_ptr()}], None),                             # unknown dtype
                ([(0, 0, _engine.AGG_I64, _engine.AGG_SUM)], [{"sum": out.data_ptr()}], None),                           # NULL values
                ([(dv.data_ptr(), 0, _engine.AGG_I64, _engine.AGG_SUM | _engine.AGG_MAX)], [{"sum": out.data_ptr()}], None),   # NULL output
                ([(dv.data_ptr(), 0, _engine.AGG_I64, _engine.AGG_SUM)], [{"sum": out.data_ptr()}], _engine.make_thresholds(0, 0, 0))):
            with pytest.raises(_engine.EngineError) as e:
                call(ix, thr, cols, outs)
            assert e.value.code == -1
    finally:
        ix.close()
    sweep = eng.index_build_dev(db.as_c(), opts, False, sweep_only=True)
    try:
        with pytest.raises(_engine.EngineError) as e:
            call(sweep, None, [(dv.data_ptr(), 0, _engine.AGG_I64, _engine.AGG_SUM)], [{"sum": out.data_ptr()}])
        assert e.value.code == _engine.IVJ_ESTATE
    finally:
        sweep.close()
    eng.sync()
