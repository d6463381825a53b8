"""The set operations on the GPU, compared exactly with the event form of tests/_setop_util.py through the host entries
(Engine.setop, Engine.set_stats) and the device entries (ivj_setop_dev / ivj_set_stats_dev via device_api, capacity protocol
included).  The shapes sit around the walk's merged-sequence tile (U.T = SO_TILE of polars-bio_amd/csrc/setop.hip.h)."""
import numpy as np
import pytest

from polars_bio_amd import _engine
import _setop_util as U

pytestmark = pytest.mark.gpu

MODES = [pytest.param(True, id="strict"), pytest.param(False, id="weak")]


@pytest.fixture(scope="module")
def eng():
    return _engine.Engine(0)


@pytest.fixture(scope="module")
def dj():
    import torch  # noqa: F401
    from polars_bio_amd.device_api import DeviceJoin
    return DeviceJoin(0)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


_expected = {}


def expected(shape, strict):
    """the reference of a shape (all four operations and the totals), computed once and shared by the tests of both entries"""
    key = (shape, strict)
    if key not in _expected:
        a, b, nc = U.SHAPES[shape](strict)
        regions, totals = {}, None
        for op in U.OPS:
            regions[op], totals = U.setop_events(a, b, strict, nc, op)
            for x in regions[op]:
                x.setflags(write=False)
        _expected[key] = (a, b, nc, regions, totals)
    return _expected[key]


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", list(U.SHAPES))
def test_host_entry(eng, shape, strict):
    a, b, nc, regions, totals = expected(shape, strict)
    for op in U.OPS:
        got = eng.setop(a, b, op, strict, nc)
        assert all(x.dtype == np.int32 for x in got)
        assert len(got[0]) <= len(a[0]) + len(b[0])
        U.assert_regions_equal(got, regions[op], f"{shape} {op}")
    assert eng.set_stats(a, b, strict, nc) == (*totals, len(regions["intersection"][0]))


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", list(U.SHAPES))
def test_device_entry(dj, shape, strict):
    import torch
    from polars_bio_amd.device_api import DeviceSide
    a, b, nc, regions, totals = expected(shape, strict)
    da, db = DeviceSide(*(_t(x) for x in a)), DeviceSide(*(_t(x) for x in b))
    assert dj.set_stats(da, db, strict, nc) == (*totals, len(regions["intersection"][0]))
    for op in U.OPS:
        exp = regions[op]
        got = dj.setop(da, db, op, strict, nc)
        assert all(t.dtype == torch.int32 and t.is_cuda for t in got)
        U.assert_regions_equal([t.cpu().numpy() for t in got], exp, f"{shape} {op}")
        n = len(exp[0])
        # the caller's buffers, exactly large enough
        out = tuple(torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
        got = dj.setop(da, db, op, strict, nc, out=out)
        U.assert_regions_equal([t.cpu().numpy() for t in got], exp, f"{shape} {op}")
        if n > 0:
            # one element too small: the total comes back, nothing is written
            small = tuple(torch.full((n - 1,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
            with pytest.raises(ValueError, match=f"fewer than {n} regions"):
                dj.setop(da, db, op, strict, nc, out=small)
            torch.cuda.synchronize()
            assert all(bool((t == -7).all()) for t in small)


@pytest.mark.parametrize("strict", MODES)
def test_device_entry_completes_a_missing_end_order(dj, strict):
    """indexes built without the end order and with the lookup tables are accepted; the capacity protocol at the C entry"""
    import torch
    from polars_bio_amd.device_api import DeviceSide
    a, b, nc, regions, totals = expected("events_%d" % (U.T + 2), strict)
    da, db = DeviceSide(*(_t(x) for x in a)), DeviceSide(*(_t(x) for x in b))
    opts = _engine.make_opts(strict, nc)
    ix_a = dj.engine.index_build_dev(da.as_c(), opts, False)
    ix_b = dj.engine.index_build_dev(db.as_c(), opts, False)
    try:
        exp = regions["symmetric_difference"]
        n = len(exp[0])
        small = tuple(torch.full((n - 1,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
        out = tuple(torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
        assert dj.engine.setop_dev(ix_a, ix_b, opts, "symmetric_difference", n - 1, *(t.data_ptr() for t in small)) == (n, False)
        assert dj.engine.setop_dev(ix_a, ix_b, opts, "symmetric_difference", n, *(t.data_ptr() for t in out)) == (n, True)
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in small)
        U.assert_regions_equal([t.cpu().numpy() for t in out], exp)
        assert dj.engine.set_stats_dev(ix_a, ix_b, opts) == (*totals, len(regions["intersection"][0]))
    finally:
        ix_a.close()
        ix_b.close()


def test_unknown_operation_is_refused(eng):
    a, b, nc = U.SHAPES["events_2"](True)
    with pytest.raises(ValueError):
        eng.setop(a, b, "complement", True, nc)
    with pytest.raises(ValueError):
        eng.setop(a, b, 4, True, nc)


def test_two_calls_return_identical_arrays(eng):
    rng = np.random.default_rng(2025)
    a = U.random_rows(rng, 30_000, 24, 200_000, max_len=30)
    b = U.random_rows(rng, 30_000, 24, 200_000, max_len=30)
    for op in U.OPS:
        x = eng.setop(a, b, op, True, 24)
        y = eng.setop(a, b, op, True, 24)
        assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y))
        U.assert_regions_equal(x, U.setop_events(a, b, True, 24, op)[0], op)
    assert eng.set_stats(a, b, True, 24) == eng.set_stats(a, b, True, 24)


@pytest.mark.parametrize("seed", range(30))
def test_random_sweep(eng, seed):
    a, b, nc, strict, op = U.sweep_case(seed)
    what = f"seed {seed}: n={len(a[0])}+{len(b[0])} strict={strict} {op}"
    exp, totals = U.setop_events(a, b, strict, nc, op)
    U.assert_regions_equal(eng.setop(a, b, op, strict, nc), exp, what)
    assert eng.set_stats(a, b, strict, nc)[:3] == totals, what


CROSS = ["events_%d" % (2 * U.T + 2), "degenerate_mixed", "contig_layout"]


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", CROSS)
def test_cross_checks_against_the_existing_engine(eng, shape, strict):
    a, b, nc, regions, totals = expected(shape, strict)
    only_a, only_b, both, n_int = eng.set_stats(a, b, strict, nc)
    # the positions both cover = the coverage by B of A's union runs, summed
    probe = U.union_rows(a, strict, nc)
    assert both == int(eng.coverage(probe, b, strict, nc).sum())
    assert n_int == len(eng.setop(a, b, "intersection", strict, nc)[0])
    # the union with an empty frame = the frame's depth blocks, coalesced
    for frame, got in ((a, eng.setop(a, U.EMPTY, "union", strict, nc)), (b, eng.setop(U.EMPTY, b, "union", strict, nc))):
        c, s, e, _d = (x.astype(np.int64) for x in eng.depth(frame, strict, nc))
        e1 = e if strict else e + 1
        first = np.concatenate([[True], (c[1:] != c[:-1]) | (s[1:] != e1[:-1])]) if c.size else np.empty(0, bool)
        idx = np.flatnonzero(first)
        last = np.concatenate([idx[1:] - 1, [c.size - 1]]) if c.size else idx
        U.assert_regions_equal(got, (c[idx], s[idx], e[last]), shape)
