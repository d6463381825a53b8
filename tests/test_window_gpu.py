"""The distance-window join and count on the GPU (window.hip.h), compared exactly -- sorted pairs, signed distances and per-probe
counts -- with the brute force of tests/_window_util.py through all four entries: host (Engine.overlap_window / count_window) and
device (ivj_overlap_window_dev / ivj_count_window_dev via device_api)."""
import numpy as np
import pytest

from polars_bio_amd import _engine
import _window_util as WU

pytestmark = pytest.mark.gpu

TILE = WU.kernel_tile()


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


def _u32_dev(m):
    import torch
    return None if m is None else torch.from_numpy(np.ascontiguousarray(m, np.uint32).view(np.int32).copy()).cuda()


def _dev_kw(w):
    return dict(w, probe_left=_u32_dev(w["probe_left"]), probe_right=_u32_dev(w["probe_right"]))


def check(eng, dj, probe, build, nc, strict, w, what="", partition_mode=0):
    """All four entries against the brute force -> the expected (pairs, distances, counts)."""
    ep, eb, ed, ecnt = WU.brute(probe, build, nc, strict, **w)
    p, b, d = eng.overlap_window(probe, build, strict, nc, partition_mode=partition_mode, **w)
    assert p.dtype == np.int32 and b.dtype == np.int32 and d.dtype == np.int64
    WU.assert_order(p, b, build)
    sp, sb, sd = WU.sort_pairs(p, b, d)
    assert len(sp) == len(ep), f"{what}: {len(sp)} host pairs, expected {len(ep)}"
    assert (sp == ep).all() and (sb == eb).all(), f"{what}: host pair sets differ"
    assert (sd == ed).all(), f"{what}: host distances differ"
    assert (np.bincount(p, minlength=len(probe[0])) == ecnt).all()
    p2, b2, none = eng.overlap_window(probe, build, strict, nc, distance=False, partition_mode=partition_mode, **w)
    assert none is None and p2.tobytes() == p.tobytes() and b2.tobytes() == b.tobytes(), f"{what}: host pairs without distance"
    cnt = eng.count_window(probe, build, strict, nc, partition_mode=partition_mode, **w)
    assert cnt.dtype == np.int64 and (cnt == ecnt).all(), f"{what}: host counts"
    dp, db = _side(probe), _side(build)
    dkw = _dev_kw(w)
    gp, gb, gd = dj.overlap_window(dp, db, strict, nc, partition_mode=partition_mode, **dkw)
    assert gp.cpu().numpy().tobytes() == p.tobytes() and gb.cpu().numpy().tobytes() == b.tobytes(), f"{what}: device pairs"
    assert gd.cpu().numpy().tobytes() == d.tobytes(), f"{what}: device distances"
    gc = dj.count_window(dp, db, strict, nc, partition_mode=partition_mode, **dkw).cpu().numpy()
    assert (gc == ecnt).all(), f"{what}: device counts"
    return ep, eb, ed, ecnt


@pytest.mark.parametrize("strict", [pytest.param(True, id="strict"), pytest.param(False, id="weak")])
@pytest.mark.parametrize("name", list(WU.SHAPES))
def test_shapes(eng, dj, name, strict):
    total = 0
    for k, (probe, build, nc, w) in enumerate(WU.cases(name)):
        total += len(check(eng, dj, probe, build, nc, strict, w, f"{name}[{k}]")[0])
    assert total > 0, "the shape is vacuous"


def test_int32_limits_reach_the_extremes(eng, dj):
    """The pads of the int32_limits shape overflow int32 on either side, and one pair lies 2^32 - 1 apart."""
    probe, build, nc, _ = WU.cases("int32_limits")[0]
    _, _, ed, _ = check(eng, dj, probe, build, nc, False, WU.W(WU.U32, WU.U32, WU.U32), "distance 2^32 - 1 only")
    assert sorted(ed.tolist()) == [-WU.U32, WU.U32]
    ep, eb, ed, _ = check(eng, dj, probe, build, nc, False, WU.W(WU.U32, WU.U32), "everything")
    assert ed.min() == -WU.U32 and ed.max() == WU.U32
    covers_p, covers_b = probe[1] <= probe[2], build[1] <= build[2]
    assert len(ep) == int(covers_p.sum()) * int(covers_b.sum())


def test_device_contract(dj):
    """Count-only with NULL buffers, IVJ_ECAPACITY leaves prefilled buffers untouched, dist_dev NULL, and an index built without the
    end order serving two calls into the caller's buffers."""
    import torch
    rng = np.random.default_rng(21)
    probe, build = WU._random_side(rng, TILE + 100, 5, 50_000, 200), WU._random_side(rng, 3000, 5, 50_000, 200)
    w = WU.W(300, 120, 2)
    ep, eb, ed, ecnt = WU.brute(probe, build, 5, True, **w)
    n = len(ep)
    assert n > 1000
    dp, db = _side(probe), _side(build)
    opts = _engine.make_opts(True, 5)
    win = _engine.make_window(300, 120, 0, 0, 2)
    ix = dj.engine.index_build_dev(db.as_c(), opts, False)
    try:
        guard = 64
        bufs = [torch.full((n + guard,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
        dist = torch.full((n + guard,), -7, dtype=torch.int64, device="cuda")
        ptrs = (bufs[0].data_ptr(), bufs[1].data_ptr(), dist.data_ptr())
        got, fits = dj.engine.overlap_window_dev(ix, dp.as_c(), opts, win, *ptrs, n - 1)
        torch.cuda.synchronize()
        assert (got, fits) == (n, False)
        assert all(bool((t == -7).all()) for t in bufs + [dist]), "IVJ_ECAPACITY must write nothing"
        got, fits = dj.engine.overlap_window_dev(ix, dp.as_c(), opts, win, 0, 0, 0, 0)           # NULL buffers, capacity 0: count only
        assert (got, fits) == (n, True)
        got, fits = dj.engine.overlap_window_dev(ix, dp.as_c(), opts, win, ptrs[0], ptrs[1], 0, n)  # dist_dev NULL
        torch.cuda.synchronize()
        assert (got, fits) == (n, True) and bool((dist == -7).all())
        first = [t[:n].cpu().numpy().copy() for t in bufs]
        for _ in range(2):                                  # the same index and buffers, twice
            got, fits = dj.engine.overlap_window_dev(ix, dp.as_c(), opts, win, *ptrs, n)
            torch.cuda.synchronize()
            assert (got, fits) == (n, True)
            sp, sb, sd = WU.sort_pairs(bufs[0][:n].cpu().numpy(), bufs[1][:n].cpu().numpy(), dist[:n].cpu().numpy())
            assert (sp == ep).all() and (sb == eb).all() and (sd == ed).all()
            assert bufs[0][:n].cpu().numpy().tobytes() == first[0].tobytes() and bufs[1][:n].cpu().numpy().tobytes() == first[1].tobytes()
            assert all(bool((t[n:] == -7).all()) for t in bufs + [dist]), "written past the capacity"
        counts = torch.full((dp.n,), -7, dtype=torch.int64, device="cuda")
        dj.engine.count_window_dev(ix, dp.as_c(), opts, win, counts.data_ptr())
        assert (counts.cpu().numpy() == ecnt).all()
        out = [torch.empty(n + 5, dtype=torch.int32, device="cuda") for _ in range(2)] + [torch.empty(n + 5, dtype=torch.int64, device="cuda")]
        vp, vb, vd = dj.overlap_window(dp, db, True, 5, index=ix, out=out, **w)
        assert vp.data_ptr() == out[0].data_ptr() and vd.data_ptr() == out[2].data_ptr() and len(vp) == n
        with pytest.raises(_engine.EngineError, match="window is NULL"):
            import ctypes as C
            rc = dj.engine.L.ivj_count_window_dev(dj.engine.h, ix.handle, C.byref(dp.as_c()), C.byref(opts), None, C.c_void_p(counts.data_ptr()))
            _engine._check(dj.engine.L, rc, "ivj_count_window_dev")
    finally:
        ix.close()


def test_two_calls_are_byte_identical(eng):
    probe, build, nc, w = WU.cases("random_2000")[0]
    a = eng.overlap_window(probe, build, True, nc, **w)
    b = eng.overlap_window(probe, build, True, nc, **w)
    assert len(a[0]) > 1000 and all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_zero_struct_on_closed_frames_is_overlap(eng):
    probe, build, nc, _ = WU.cases("random_2000")[0]
    p, b, d = eng.overlap_window(probe, build, False, nc)
    covers = (probe[1] <= probe[2])[p] & (build[1] <= build[2])[b]
    assert covers.all() and not d.any()
    op, ob = eng.overlap(probe, build, False, nc)
    keep = (probe[1] <= probe[2])[op] & (build[1] <= build[2])[ob]          # the plain predicate also pairs inverted rows
    sp, sb = WU.sort_pairs(p, b)
    ep, eb = WU.sort_pairs(op[keep], ob[keep])
    assert len(sp) > 100 and (sp == ep).all() and (sb == eb).all()


@pytest.mark.parametrize("strict", [pytest.param(True, id="strict"), pytest.param(False, id="weak")])
def test_minimum_distance_per_probe_is_nearest(eng, strict):
    probe, build = WU.no_empty_rows(9, 1500, 1200, 3)
    window = 60                                            # about a fifth of the probes have their nearest row farther away
    p, b, d = eng.overlap_window(probe, build, strict, 3, left=window, right=window)
    _, nd, nf = eng.nearest(probe, build, strict, 3, k=1)
    nd = np.asarray(nd).reshape(-1)
    mins = np.full(1500, np.iinfo(np.int64).max)
    np.minimum.at(mins, p, np.abs(d))
    within = (np.asarray(nf).reshape(-1) > 0) & (nd <= window)
    assert within.sum() > 500 and (~within).sum() > 100
    assert (mins[within] == nd[within]).all()
    assert not np.isin(np.nonzero(~within)[0], p).any(), "a probe whose nearest row lies outside the window has no pair"


@pytest.mark.parametrize("pm", [1, 5, 6])
def test_bucketed_probes_land_by_position(eng, dj, pm):
    """partition_mode 1, 5, 6 bucket the probes: counts still land at the probe's position and the per-row extent columns are read
    by position."""
    probe, build, nc, w = WU.cases("random_2000")[3]
    assert w["probe_left"] is not None
    base = eng.overlap_window(probe, build, True, nc, partition_mode=2, **w)
    ep, eb, ed, ecnt = check(eng, dj, probe, build, nc, True, w, f"partition_mode {pm}", partition_mode=pm)
    assert len(ep) == len(base[0]) > 1000
    sp, sb, sd = WU.sort_pairs(*base)
    assert (sp == ep).all() and (sb == eb).all() and (sd == ed).all()
