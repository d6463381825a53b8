"""Semi / anti / left outer join on the GPU (select.hip.h) through the C ABI: the host entries (Engine.overlap_select /
overlap_outer) and the device entry (ivj_overlap_select_dev via device_api and raw), compared EXACTLY with the yardstick of
tests/_join_kinds_util.py.  Sizes stay at or below ~20 k probes x ~2 k build rows: the brute forces take well under a second."""
import numpy as np
import pytest

from polars_bio_amd import _engine, range_op
import _join_kinds_util as J
import _thresholds_util as T
from _util import random_side

pytestmark = pytest.mark.gpu

TILE = J.kernel_tile()
NEVER = T.NEVER
MODES = (("semi", J.SEMI), ("anti", J.ANTI))


@pytest.fixture(scope="module")
def eng():
    return _engine.Engine(0)


@pytest.fixture(scope="module")
def dj():
    import torch  # noqa: F401
    from polars_bio_amd.device_api import DeviceJoin
    return DeviceJoin(0)


def _dev(a, dtype=np.int32):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def _side(cols, row_id=None):
    from polars_bio_amd.device_api import DeviceSide
    return DeviceSide(*(_dev(a) for a in cols), row_id=None if row_id is None else _dev(row_id))


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


def check(eng, dj, probe, build, nc, strict, what="", partition_mode=0, row_id=None, outer=True, **thr):
    """Host and device entries of both modes (and the host outer join) against the yardstick -> the expectation."""
    e = J.expected(probe, build, nc, strict, **thr)
    kw = _engine_kw(probe, build, strict, **thr)
    dp, db = _side(probe, row_id), _side(build)
    dkw = dict(min_overlap=kw["min_overlap"], probe_min=_min_dev(kw["probe_min"]), build_min=_min_dev(kw["build_min"]))
    for name, mode in MODES:
        want = e[name]
        got = eng.overlap_select(probe, build, strict, nc, name, partition_mode=partition_mode, **kw)
        assert got.dtype == np.int32 and len(got) == len(want) and (got == want).all(), f"{what}: host {name}"
        got = dj.overlap_select(dp, db, strict, nc, mode, partition_mode=partition_mode, **dkw).cpu().numpy()
        ids = want if row_id is None else np.asarray(row_id, np.int32)[want]
        assert len(got) == len(ids) and (got == ids).all(), f"{what}: device {name}"
    if outer:
        p, b = eng.overlap_outer(probe, build, strict, nc, partition_mode=partition_mode, **kw)
        J.assert_outer((p, b), e, build, what)
    return e


def _random(seed, n_probe, n_build, nc, span=20_000):
    rng = np.random.default_rng(seed)
    return random_side(rng, n_probe, nc, span, 60), random_side(rng, n_build, nc, span, 80)


def _mixed(e, n):
    """The case is not vacuous: both kinds of rows occur."""
    assert len(e["semi"]) + len(e["anti"]) == n
    assert n < 2 or (len(e["semi"]) > 0 and len(e["anti"]) > 0)


@pytest.mark.parametrize("strict", [pytest.param(True, id="strict"), pytest.param(False, id="weak")])
@pytest.mark.parametrize("n_probe", [0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 5 * TILE + 3])
def test_tile_edges(eng, dj, n_probe, strict):
    probe, build = _random(100 + n_probe, n_probe, 2000, 3, span=60_000)
    e = check(eng, dj, probe, build, 3, strict, f"{n_probe} probes")
    if n_probe > 1:
        _mixed(e, n_probe)


def _pattern_probes(n, hit):
    """n probes on contig 0: [1100, 1200) where hit, [5000, 5100) elsewhere; the build side is the one row [1000, 2000)."""
    hit = np.asarray(hit, bool)
    s = np.where(hit, 1100, 5000).astype(np.int32)
    return (np.zeros(n, np.int32), s, (s + 100).astype(np.int32))


@pytest.mark.parametrize("pattern", ["all", "none", "alternating", "single_at_tile"])
def test_keep_patterns(eng, dj, pattern):
    n = 2 * TILE + 5
    i = np.arange(n)
    hit = {"all": i >= 0, "none": i < 0, "alternating": i % 2 == 0, "single_at_tile": i == TILE}[pattern]
    probe = _pattern_probes(n, hit)
    build = (np.zeros(1, np.int32), np.array([1000], np.int32), np.array([2000], np.int32))
    for strict in (True, False):
        e = check(eng, dj, probe, build, 1, strict, pattern)
        assert (e["semi"] == np.flatnonzero(hit)).all() and (e["anti"] == np.flatnonzero(~hit)).all()
        check(eng, dj, probe, build, 1, strict, pattern + " thresholded", min_overlap=50)
    # the complementary selection through the other mode of the same pattern is the same set
    if pattern == "single_at_tile":
        assert list(e["semi"]) == [TILE]


@pytest.mark.parametrize("strict", [pytest.param(True, id="strict"), pytest.param(False, id="weak")])
def test_empty_build_side(eng, dj, strict):
    probe, _ = _random(5, TILE + 7, 10, 3)
    empty = tuple(np.empty(0, np.int32) for _ in range(3))
    e = check(eng, dj, probe, empty, 3, strict, "empty build")
    assert len(e["semi"]) == 0 and (e["anti"] == np.arange(TILE + 7)).all()
    check(eng, dj, probe, empty, 3, strict, "empty build, thresholded", min_overlap=2)


@pytest.mark.parametrize("strict", [pytest.param(True, id="strict"), pytest.param(False, id="weak")])
def test_contigs_outside_the_dictionary(eng, dj, strict):
    probe, build = _random(6, 2 * TILE + 9, 1500, 3, span=30_000)
    rng = np.random.default_rng(7)
    bad = rng.random(len(probe[0]))
    probe[0][bad < 0.1] = -1
    probe[0][(bad >= 0.1) & (bad < 0.2)] = 3
    probe[0][(bad >= 0.2) & (bad < 0.25)] = 1000
    e = check(eng, dj, probe, build, 3, strict, "contigs outside")
    outside = (probe[0] < 0) | (probe[0] >= 3)
    assert outside.sum() > 100 and not e["cnt"][outside].any() and np.isin(np.flatnonzero(outside), e["anti"]).all()
    _mixed(e, len(probe[0]))
    check(eng, dj, probe, build, 3, strict, "contigs outside, thresholded", min_overlap=3)


@pytest.mark.parametrize("inverted_build", [False, True])
@pytest.mark.parametrize("strict", [pytest.param(True, id="strict"), pytest.param(False, id="weak")])
def test_degenerate_rows(eng, dj, strict, inverted_build):
    """Zero-length and inverted probes take the bounded scan of the count kernel; one inverted build row sends every probe there."""
    probe, build = _random(8, TILE + 300, 1200, 2, span=8000)
    rng = np.random.default_rng(9)
    z = rng.random(len(probe[0]))
    probe[2][z < 0.2] = probe[1][z < 0.2]                                         # zero length
    inv = (z >= 0.2) & (z < 0.4)
    probe[2][inv] = probe[1][inv] - rng.integers(1, 50, int(inv.sum())).astype(np.int32)      # start > end
    if inverted_build:
        build[1][17], build[2][17] = 4000, 3900
    e = check(eng, dj, probe, build, 2, strict, "degenerate rows")
    _mixed(e, len(probe[0]))
    e = check(eng, dj, probe, build, 2, strict, "degenerate rows, thresholded", min_overlap=1)
    covers_nothing = (probe[2] < probe[1]) | ((probe[2] == probe[1]) & strict)
    assert covers_nothing.sum() > 100 and np.isin(np.flatnonzero(covers_nothing), e["anti"]).all()


def test_row_ids(eng, dj):
    probe, build = _random(10, 3 * TILE + 11, 1800, 3, span=50_000)
    perm = np.random.default_rng(11).permutation(len(probe[0])).astype(np.int32)
    e = check(eng, dj, probe, build, 3, True, "row ids", row_id=perm, outer=False)
    _mixed(e, len(probe[0]))
    check(eng, dj, probe, build, 3, False, "row ids, thresholded", row_id=perm, outer=False, min_overlap=5)


@pytest.mark.parametrize("partition_mode", [1, 2])
def test_partition_modes(eng, dj, partition_mode):
    probe, build = _random(12, 4 * TILE + 1, 2000, 3, span=60_000)
    for strict in (True, False):
        e = check(eng, dj, probe, build, 3, strict, f"partition_mode {partition_mode}", partition_mode=partition_mode)
        _mixed(e, len(probe[0]))
        check(eng, dj, probe, build, 3, strict, f"partition_mode {partition_mode}, thresholded", partition_mode=partition_mode,
              min_overlap=4, min_frac1=0.3)


def _never_mix(rng, n):
    return rng.choice(np.array([0, 3, 40, NEVER], np.uint32), n)


THRESHOLD_SETS = {
    "min_overlap": lambda p, b, rng: dict(min_overlap=12),
    "minima_with_never_and_zero": lambda p, b, rng: dict(probe_min=_never_mix(rng, len(p[0])), build_min=_never_mix(rng, len(b[0]))),
    "all_three": lambda p, b, rng: dict(min_overlap=5, min_frac1=0.4, min_frac2=0.25),
}


@pytest.mark.parametrize("strict", [pytest.param(True, id="strict"), pytest.param(False, id="weak")])
@pytest.mark.parametrize("name", list(THRESHOLD_SETS))
def test_thresholded(eng, dj, name, strict):
    probe, build = _random(13, 2 * TILE + 1, 2000, 3, span=40_000)
    thr = THRESHOLD_SETS[name](probe, build, np.random.default_rng(14))
    e = check(eng, dj, probe, build, 3, strict, name, **thr)
    _mixed(e, len(probe[0]))
    plain = J.expected(probe, build, 3, strict)
    assert len(e["semi"]) < len(plain["semi"]), "the threshold removed no row"
    if "probe_min" in thr:
        never = np.flatnonzero(thr["probe_min"] == NEVER)
        assert len(never) > 100 and np.isin(never, e["anti"]).all()


def test_contig_wide_build_row(eng, dj):
    """One contig-wide build row over 2000 short ones: the candidate range of every probe spans chunks of the thresholded kernel;
    its minimum decides whether every probe of the contig, or only those under a short row, is a semi row."""
    n = 2000
    starts = 100 * np.arange(n, dtype=np.int32) + 100
    build = (np.zeros(n + 1, np.int32), np.concatenate([[0], starts]).astype(np.int32), np.concatenate([[300_000], starts + 30]).astype(np.int32))
    m = TILE + 40
    ps = (50 + 97 * np.arange(m)).astype(np.int32)
    probe = (np.zeros(m, np.int32), ps, (ps + 20).astype(np.int32))
    for wide_min, all_kept in ((1_000_000, False), (20, True)):
        bm = np.full(n + 1, 10, np.uint32)
        bm[0] = wide_min
        e = check(eng, dj, probe, build, 1, True, f"wide row minimum {wide_min}", build_min=bm)
        assert (len(e["anti"]) == 0) == all_kept
        if not all_kept:
            _mixed(e, m)
    e = check(eng, dj, probe, build, 1, True, "wide row, plain predicate")
    assert len(e["anti"]) == 0


def test_capacity_contract(dj):
    import torch
    probe, build = _random(21, 2 * TILE + 100, 2000, 3, span=60_000)
    dp, db = _side(probe), _side(build)
    opts = _engine.make_opts(True, 3)
    ix = dj.engine.index_build_dev(db.as_c(), opts, True)
    try:
        for thr, tkw in ((None, {}), (_engine.make_thresholds(4), dict(min_overlap=4))):
            e = J.expected(probe, build, 3, True, **tkw)
            for name, mode in MODES:
                want = e[name]
                n = len(want)
                assert n > 100
                bufs = [torch.full((n + 64,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
                got, fits = dj.engine.overlap_select_dev(ix, dp.as_c(), opts, thr, mode, bufs[0].data_ptr(), bufs[1].data_ptr(), n - 1)
                torch.cuda.synchronize()
                assert (got, fits) == (n, False)
                assert all(bool((t == -7).all()) for t in bufs), "IVJ_ECAPACITY must write nothing"
                got, fits = dj.engine.overlap_select_dev(ix, dp.as_c(), opts, thr, mode, 0, 0, 0)      # NULL buffers, capacity 0: count only
                assert (got, fits) == (n, True)
                got, fits = dj.engine.overlap_select_dev(ix, dp.as_c(), opts, thr, mode, bufs[0].data_ptr(), 0, n)
                torch.cuda.synchronize()
                assert (got, fits) == (n, True)
                assert (bufs[0][:n].cpu().numpy() == want).all()
                assert bool((bufs[0][n:] == -7).all()) and bool((bufs[1] == -7).all()), "written past the capacity / into an absent pad"
        with pytest.raises(_engine.EngineError, match="no threshold is set") as ei:
            dj.engine.overlap_select_dev(ix, dp.as_c(), opts, _engine.make_thresholds(0), J.SEMI, 0, 0, 0)
        assert ei.value.code == -1
        with pytest.raises(_engine.EngineError, match="mode") as ei:
            dj.engine.overlap_select_dev(ix, dp.as_c(), opts, None, 2, 0, 0, 0)
        assert ei.value.code == -1
    finally:
        ix.close()
    sweep = dj.engine.index_build_dev(db.as_c(), opts, False, sweep_only=True)
    try:
        with pytest.raises(_engine.EngineError) as ei:
            dj.engine.overlap_select_dev(sweep, dp.as_c(), opts, None, J.ANTI, 0, 0, 0)
        assert ei.value.code == _engine.IVJ_ESTATE
    finally:
        sweep.close()


@pytest.mark.parametrize("thresholded", [False, True])
def test_pad_at_odd_offsets(dj, thresholded):
    """The way the outer join uses the kernel: both outputs start an odd number of elements into their buffers (4-byte alignment
    only); -1 lands at exactly the selected positions, the guard words before and after stay intact."""
    import torch
    probe, build = _random(22, 2 * TILE + 77, 1500, 3, span=60_000)
    tkw = dict(min_overlap=6) if thresholded else {}
    thr = _engine.make_thresholds(6) if thresholded else None
    e = J.expected(probe, build, 3, False, **tkw)
    dp, db = _side(probe), _side(build)
    opts = _engine.make_opts(False, 3)
    ix = dj.engine.index_build_dev(db.as_c(), opts, True)
    try:
        for (name, mode), (off_r, off_p) in zip(MODES, ((3, 5), (1, 7))):
            want = e[name]
            n = len(want)
            assert n > 100
            rows = torch.full((n + 32,), -7, dtype=torch.int32, device="cuda")
            pad = torch.full((n + 32,), -9, dtype=torch.int32, device="cuda")
            rp, pp = rows.data_ptr() + 4 * off_r, pad.data_ptr() + 4 * off_p
            assert rp % 8 == 4 and pp % 8 == 4
            got, fits = dj.engine.overlap_select_dev(ix, dp.as_c(), opts, thr, mode, rp, pp, n)
            torch.cuda.synchronize()
            assert (got, fits) == (n, True)
            r, p = rows.cpu().numpy(), pad.cpu().numpy()
            assert (r[off_r:off_r + n] == want).all() and (r[:off_r] == -7).all() and (r[off_r + n:] == -7).all()
            assert (p[off_p:off_p + n] == -1).all() and (p[:off_p] == -9).all() and (p[off_p + n:] == -9).all()
    finally:
        ix.close()


@pytest.mark.parametrize("strict", [pytest.param(True, id="strict"), pytest.param(False, id="weak")])
def test_outer_join(eng, strict):
    probe, build = _random(23, 3 * TILE + 5, 2000, 3, span=50_000)
    probe[0][::17] = -1
    for tkw in ({}, dict(min_overlap=8), dict(min_frac1=0.5, min_frac2=0.2)):
        e = J.expected(probe, build, 3, strict, **tkw)
        kw = _engine_kw(probe, build, strict, **tkw)
        p, b = eng.overlap_outer(probe, build, strict, 3, **kw)
        J.assert_outer((p, b), e, build, str(tkw))
        assert len(e["inner"][0]) > 500 and len(e["anti"]) > 500
        inner = eng.overlap_thresh(probe, build, strict, 3, **kw) if tkw else eng.overlap(probe, build, strict, 3)
        n = len(inner[0])
        assert (p[:n] == inner[0]).all() and (b[:n] == inner[1]).all(), "the inner part is not what the inner join of the same call returns"
    empty = tuple(np.empty(0, np.int32) for _ in range(3))
    p, b = eng.overlap_outer(probe, empty, strict, 3)
    assert (p == np.arange(len(probe[0]))).all() and (b == -1).all()
    p, b = eng.overlap_outer(empty, build, strict, 3)
    assert len(p) == 0 and len(b) == 0


def test_determinism(eng, dj):
    probe, build = _random(24, 5 * TILE + 3, 2000, 3, span=60_000)
    dp, db = _side(probe), _side(build)
    for tkw in ({}, dict(min_overlap=7)):
        for name, mode in MODES:
            a = eng.overlap_select(probe, build, True, 3, name, **tkw)
            b = eng.overlap_select(probe, build, True, 3, name, **tkw)
            assert (a == b).all() and len(a) > 100
            c = dj.overlap_select(dp, db, True, 3, mode, **tkw).cpu().numpy()
            d = dj.overlap_select(dp, db, True, 3, mode, **tkw).cpu().numpy()
            assert (c == d).all() and (a == c).all()


def test_out_buffer_of_the_tensor_entry(dj):
    import torch
    probe, build = _random(25, TILE + 9, 1000, 3, span=30_000)
    e = J.expected(probe, build, 3, True)
    dp, db = _side(probe), _side(build)
    big = torch.full((len(probe[0]),), -7, dtype=torch.int32, device="cuda")
    got = dj.overlap_select(dp, db, True, 3, "semi", out=big)
    assert got.data_ptr() == big.data_ptr() and (got.cpu().numpy() == e["semi"]).all()
    small = torch.full((3,), -7, dtype=torch.int32, device="cuda")
    got = dj.overlap_select(dp, db, True, 3, "anti", out=small)
    assert (got.cpu().numpy() == e["anti"]).all() and bool((small == -7).all())
