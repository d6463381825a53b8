"""The thresholded join and count on the GPU (thresh.hip.h), compared exactly -- sorted pairs and per-probe counts -- with the brute
force of tests/_thresholds_util.py through all four entries: host (Engine.overlap_thresh / count_overlaps_thresh) and device
(ivj_overlap_thresh_dev / ivj_count_overlaps_thresh_dev via device_api).  Fractions are given to the brute force literally and to
the engine as the minima of range_op.min_bases."""
import numpy as np
import pytest

from polars_bio_amd import _engine, range_op
import _limits as L
import _thresholds_util as T
from _util import random_side

pytestmark = pytest.mark.gpu

TILE = T.kernel_tile()
NEVER = T.NEVER


@pytest.fixture(scope="module")
def eng():
    return _engine.Engine(0)


@pytest.fixture(scope="module")
def dj():
    import torch  # noqa: F401
    from polars_bio_amd.device_api import DeviceJoin
    return DeviceJoin(0)


def _side(cols):
    import torch
    from polars_bio_amd.device_api import DeviceSide
    return DeviceSide(*(torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in cols))


def _min_dev(m):
    import torch
    return None if m is None else torch.from_numpy(np.ascontiguousarray(m, np.uint32).view(np.int32).copy()).cuda()


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


def check(eng, dj, probe, build, nc, strict, what="", **thr):
    """All four entries against the brute force -> the expected pairs."""
    ep, eb, ecnt = T.brute(probe, build, nc, strict, **thr)
    kw = _engine_kw(probe, build, strict, **thr)
    p, b = eng.overlap_thresh(probe, build, strict, nc, **kw)
    T.assert_order(p, b, build)
    T.assert_pairs((p, b), (ep, eb), f"{what} host pairs")
    cnt = eng.count_overlaps_thresh(probe, build, strict, nc, **kw)
    assert cnt.dtype == np.int64 and (cnt == ecnt).all(), f"{what} host counts"
    dp, db = _side(probe), _side(build)
    dkw = dict(min_overlap=kw["min_overlap"], probe_min=_min_dev(kw["probe_min"]), build_min=_min_dev(kw["build_min"]))
    gp, gb = dj.overlap_thresh(dp, db, strict, nc, **dkw)
    gp, gb = gp.cpu().numpy(), gb.cpu().numpy()
    T.assert_order(gp, gb, build)
    T.assert_pairs((gp, gb), (ep, eb), f"{what} device pairs")
    gc = dj.count_overlaps_thresh(dp, db, strict, nc, **dkw).cpu().numpy()
    assert (gc == ecnt).all(), f"{what} device counts"
    return ep, eb, ecnt


def _random(seed, n_probe, n_build, nc, span=20_000):
    rng = np.random.default_rng(seed)
    return random_side(rng, n_probe, nc, span, 300), random_side(rng, n_build, nc, span, 400)


def _never_mix(rng, n):
    return rng.choice(np.array([0, 3, 40, NEVER], np.uint32), n)


THRESHOLD_SETS = {
    "min_overlap_1": lambda p, b, rng: dict(min_overlap=1),
    "min_overlap_7": lambda p, b, rng: dict(min_overlap=7),
    "min_overlap_above_every_row": lambda p, b, rng: dict(min_overlap=1 << 31),
    "probe_min_only": lambda p, b, rng: dict(min_frac1=0.5),
    "build_min_only": lambda p, b, rng: dict(min_frac2=0.7),
    "both_minima": lambda p, b, rng: dict(min_frac1=0.3, min_frac2=0.3),
    "all_three": lambda p, b, rng: dict(min_overlap=5, min_frac1=0.2, min_frac2=1 / 3),
    "never_mixed_in": lambda p, b, rng: dict(min_overlap=2, probe_min=_never_mix(rng, len(p[0])), build_min=_never_mix(rng, len(b[0]))),
}


@pytest.mark.parametrize("strict", [pytest.param(True, id="strict"), pytest.param(False, id="weak")])
@pytest.mark.parametrize("name", list(THRESHOLD_SETS))
def test_threshold_sets(eng, dj, name, strict):
    probe, build = _random(11, TILE + 1, 5000, 24)
    thr = THRESHOLD_SETS[name](probe, build, np.random.default_rng(5))
    ep, _, ecnt = check(eng, dj, probe, build, 24, strict, name, **thr)
    if name == "min_overlap_above_every_row":
        assert len(ep) == 0 and not ecnt.any()
    else:
        assert len(ep) > 100, "the case is vacuous"
        plain = T.brute(probe, build, 24, strict, min_overlap=1)[0]
        assert name == "min_overlap_1" or len(ep) < len(plain), "the threshold removed nothing"


@pytest.mark.parametrize("n_build", [1, 64, 5000])
@pytest.mark.parametrize("n_probe", [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 17])
def test_row_counts(eng, dj, n_probe, n_build):
    strict = (n_probe + n_build) % 2 == 0
    probe, build = _random(100 + n_probe + n_build, n_probe, n_build, 3, span=6000)
    if n_build == 1:
        build = (np.zeros(1, np.int32), np.array([100], np.int32), np.array([5900], np.int32))      # one row under most probes of contig 0
    if n_probe == 1:
        probe = (np.zeros(1, np.int32), np.array([1000], np.int32), np.array([5000], np.int32))
    # (a single probe is measured against the build rows it contains, many probes against the rows that contain them)
    thr = dict(min_overlap=3, min_frac2=0.25) if n_probe == 1 else dict(min_overlap=3, min_frac1=0.25)
    ep, _, _ = check(eng, dj, probe, build, 3, strict, f"{n_probe}x{n_build}", **thr)
    assert len(ep) > 0


@pytest.mark.parametrize("nc", [1, 24, 257, 1025])
def test_contig_dictionaries(eng, dj, nc):
    strict = nc in (1, 257)
    probe, build = _random(nc, 2 * TILE + 5, 5000, nc, span=max(400_000 // nc, 2000))
    ep, _, _ = check(eng, dj, probe, build, nc, strict, f"{nc} contigs", min_overlap=4, min_frac2=0.4)
    assert len(ep) > 100


@pytest.mark.parametrize("strict", [pytest.param(True, id="strict"), pytest.param(False, id="weak")])
def test_rows_that_cover_nothing(eng, dj, strict):
    """Zero-length and inverted rows on both sides, touching intervals, null-contig rows, contigs present on one side only."""
    rows_p = [(0, 10, 10), (0, 20, 12), (0, 10, 20), (0, 30, 40), (0, 40, 50), (-1, 10, 20), (2, 10, 20), (0, 19, 31), (1, 5, 5), (1, 0, 100)]
    rows_b = [(0, 10, 10), (0, 25, 15), (0, 20, 30), (0, 15, 15), (0, 12, 18), (-1, 10, 20), (3, 10, 20), (0, 40, 50), (1, 7, 3), (1, 50, 50),
              (0, 50, 60), (1, 99, 101)]
    rng = np.random.default_rng(3)
    rp, rb = _random(9, 300, 400, 4, span=300)
    probe = tuple(np.concatenate([np.array([r[k] for r in rows_p], np.int32), rp[k]]) for k in range(3))
    build = tuple(np.concatenate([np.array([r[k] for r in rows_b], np.int32), rb[k]]) for k in range(3))
    for side, planted in ((probe, rows_p), (build, rows_b)):           # null contigs among the random rows (the planted rows stay as written)
        null = rng.random(len(side[0])) < 0.05
        null[:len(planted)] = False
        side[0][null] = -1
    build[0][build[0] == 2] = 0                            # contig 2 on the probe side only, contig 3 ...
    probe[0][probe[0] == 3] = 1                            # ... on the build side only
    for thr in (dict(min_overlap=1), dict(min_frac1=0.01, min_frac2=0.01), dict(min_overlap=2, min_frac1=0.5)):
        ep, eb, ecnt = check(eng, dj, probe, build, 4, strict, str(thr), **thr)
        assert len(ep) > 50
        degenerate_p = (probe[2] < probe[1]) | ((probe[2] == probe[1]) & strict) | (probe[0] < 0)
        degenerate_b = (build[2] < build[1]) | ((build[2] == build[1]) & strict) | (build[0] < 0)
        assert degenerate_p.sum() > 5 and degenerate_b.sum() > 5
        assert not degenerate_p[ep].any() and not degenerate_b[eb].any() and not ecnt[degenerate_p].any()
    # touching: [10, 20) | [20, 30) share nothing; [10, 20] | [20, 30] share position 20
    p, b, _ = T.brute(probe, build, 4, strict, min_overlap=1)
    assert (((p == 2) & (b == 2)).any()) == (not strict)


def test_long_candidate_ranges(eng, dj):
    """One contig-wide build row over 20 000 short ones: the candidate range of every probe reaches down to the wide row, far
    beyond what the plain flat kernel accepts per probe; probes at both ends of the contig."""
    n = 20_000
    starts = 100 * np.arange(n, dtype=np.int32) + 100
    build = (np.zeros(n + 1, np.int32), np.concatenate([[0], starts]).astype(np.int32), np.concatenate([[2_100_000], starts + 50]).astype(np.int32))
    ps = np.concatenate([100 + 97 * np.arange(20), 1_990_000 + 97 * np.arange(20)]).astype(np.int32)
    probe = (np.zeros(40, np.int32), ps, (ps + 180).astype(np.int32))
    for wide_min, kept in ((1_000_000, False), (150, True)):
        bm = np.full(n + 1, 10, np.uint32)
        bm[0] = wide_min
        ep, eb, ecnt = check(eng, dj, probe, build, 1, True, f"wide row minimum {wide_min}", build_min=bm)
        assert (eb == 0).any() == kept and (ecnt[20:] >= (2 if kept else 1)).all()
        assert int((eb == 0).sum()) == (40 if kept else 0)


def test_nested_dense_windows(eng, dj):
    """200 probes x 3000 stacked build rows on one position range: a tile's candidates exceed one chunk many times over and the
    pairs of one probe span chunks."""
    i = np.arange(3000)
    build = (np.zeros(3000, np.int32), (1000 + i % 7).astype(np.int32), (2000 - i % 5).astype(np.int32))
    j = np.arange(200)
    probe = (np.zeros(200, np.int32), (1000 + j).astype(np.int32), (1500 + 2 * j).astype(np.int32))
    ep, _, ecnt = check(eng, dj, probe, build, 1, True, "nested", min_overlap=600, min_frac2=0.6)
    assert 0 < len(ep) < 200 * 3000 and ecnt.max() == 3000 and ecnt.min() == 0


def test_coordinate_limits(eng, dj):
    """Rows at 0 and 2^31 - 1; a closed row of 2^31 positions with min_frac1 = min_frac2 = 1.0 matches only itself."""
    rows_b = [(0, L.MAX), (1, L.MAX), (0, L.MAX - 1), (0, 0), (L.MAX, L.MAX), (L.MAX - 1, L.MAX), (0, 1)]
    rows_p = [(0, L.MAX), (L.MAX, L.MAX), (0, 0), (L.MAX - 1, L.MAX), (5, 4)]
    build = (np.zeros(len(rows_b), np.int32), np.array([r[0] for r in rows_b], np.int32), np.array([r[1] for r in rows_b], np.int32))
    probe = (np.zeros(len(rows_p), np.int32), np.array([r[0] for r in rows_p], np.int32), np.array([r[1] for r in rows_p], np.int32))
    assert int(_lengths(probe, False)[0]) == 1 << 31
    ep, eb, _ = check(eng, dj, probe, build, 1, False, "closed, both fractions 1.0", min_frac1=1.0, min_frac2=1.0)
    assert list(zip(ep, eb)) == [(0, 0), (1, 4), (2, 3), (3, 5)]
    ep, eb, _ = check(eng, dj, probe, build, 1, True, "half-open, both fractions 1.0", min_frac1=1.0, min_frac2=1.0)
    assert list(zip(ep, eb)) == [(0, 0), (3, 5)]
    check(eng, dj, probe, build, 1, False, "closed, 2^31 bases", min_overlap=1 << 31)
    # limit-hugging rows over all of int32 (overlaps of up to 2^32 positions): the base-count threshold
    rng = np.random.default_rng(17)
    lp, lb = L.limit_rows(rng, 300, 3, inverted=True, outside=True), L.limit_rows(rng, 300, 3, inverted=True)
    for strict in (True, False):
        ep, _, _ = check(eng, dj, lp, lb, 3, strict, "limit rows", min_overlap=2)
        assert len(ep) > 100
        check(eng, dj, lp, lb, 3, strict, "limit rows, 2^31 + 1 bases", min_overlap=(1 << 31) + 1)


def test_capacity_contract(dj):
    import torch
    probe, build = _random(21, TILE + 100, 3000, 5)
    ep, eb, _ = T.brute(probe, build, 5, True, min_overlap=4)
    n = len(ep)
    assert n > 1000
    dp, db = _side(probe), _side(build)
    opts = _engine.make_opts(True, 5)
    thr = _engine.make_thresholds(4)
    ix = dj.engine.index_build_dev(db.as_c(), opts, False)
    try:
        guard = 64
        bufs = [torch.full((n + guard,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
        got, fits = dj.engine.overlap_thresh_dev(ix, dp.as_c(), opts, thr, bufs[0].data_ptr(), bufs[1].data_ptr(), n - 1)
        torch.cuda.synchronize()
        assert (got, fits) == (n, False)
        assert all(bool((t == -7).all()) for t in bufs), "IVJ_ECAPACITY must write nothing"
        got, fits = dj.engine.overlap_thresh_dev(ix, dp.as_c(), opts, thr, 0, 0, 0)                 # NULL buffers, capacity 0: count only
        assert (got, fits) == (n, True)
        got, fits = dj.engine.overlap_thresh_dev(ix, dp.as_c(), opts, thr, bufs[0].data_ptr(), bufs[1].data_ptr(), n)
        torch.cuda.synchronize()
        assert (got, fits) == (n, True)
        T.assert_pairs((bufs[0][:n].cpu().numpy(), bufs[1][:n].cpu().numpy()), (ep, eb), "exact capacity")
        assert all(bool((t[n:] == -7).all()) for t in bufs), "written past the capacity"
        with pytest.raises(_engine.EngineError, match="no threshold is set"):
            dj.engine.overlap_thresh_dev(ix, dp.as_c(), opts, _engine.make_thresholds(0), 0, 0, 0)
    finally:
        ix.close()


def test_one_index_serves_plain_and_thresholded_calls(dj):
    import torch
    probe, build = _random(33, 2 * TILE, 4000, 24)
    dp, db = _side(probe), _side(build)
    ix = dj.build_index(db, True, 24)
    try:
        def plain():
            out = [torch.empty(200_000, dtype=torch.int32, device="cuda") for _ in range(2)]
            p, b = dj.overlap(dp, db, True, 24, index=ix, out=out)
            c = dj.count_overlaps(dp, db, True, 24, index=ix)
            return T.sort_pairs(p.cpu().numpy(), b.cpu().numpy()), c.cpu().numpy()
        (p0, b0), c0 = plain()
        tp, tb = dj.overlap_thresh(dp, db, True, 24, min_overlap=6, index=ix)
        tc = dj.count_overlaps_thresh(dp, db, True, 24, min_overlap=6, index=ix)
        (p1, b1), c1 = plain()
        ep, eb, ecnt = T.brute(probe, build, 24, True, min_overlap=6)
        T.assert_pairs((tp.cpu().numpy(), tb.cpu().numpy()), (ep, eb), "thresholded call between plain calls")
        assert (tc.cpu().numpy() == ecnt).all()
        assert len(p0) > len(ep) > 0
        assert (p0 == p1).all() and (b0 == b1).all() and (c0 == c1).all()
        assert (c0 == np.bincount(p0, minlength=len(c0))).all()
    finally:
        ix.close()
