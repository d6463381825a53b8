"""depth on the GPU, compared exactly with the event form of tests/_depth_util.py through the host entry (Engine.depth),
the device entry (ivj_depth_dev via device_api, capacity protocol included) and, in tests/test_depth_frontend.py, the front
door.  The shapes sit around the kernel's merged-sequence tile (U.T = DP_TILE of polars-bio_amd/csrc/depth.hip.h)."""
import numpy as np
import pytest

from polars_bio_amd import _engine
import _depth_util as U

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
    """the reference of a shape, computed once and shared by the tests of both entries"""
    key = (shape, strict)
    if key not in _expected:
        c, s, e, nc = U.SHAPES[shape](strict)
        exp = U.depth_events(c, s, e, strict, nc)
        for a in exp:
            a.setflags(write=False)
        _expected[key] = (c, s, e, nc, exp)
    return _expected[key]


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", list(U.SHAPES))
def test_host_entry(eng, shape, strict):
    c, s, e, nc, exp = expected(shape, strict)
    got = eng.depth((c, s, e), strict, nc)
    assert all(a.dtype == np.int32 for a in got)
    assert len(got[0]) <= 2 * len(c)
    U.assert_blocks_equal(got, exp, shape)


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", list(U.SHAPES))
def test_device_entry(dj, shape, strict):
    import torch
    from polars_bio_amd.device_api import DeviceSide
    c, s, e, nc, exp = expected(shape, strict)
    frame = DeviceSide(_t(c), _t(s), _t(e))
    got = dj.depth(frame, strict, nc)
    assert all(t.dtype == torch.int32 and t.is_cuda for t in got)
    U.assert_blocks_equal([t.cpu().numpy() for t in got], exp, shape)
    n = len(exp[0])
    # the caller's buffers, exactly large enough
    out = tuple(torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(4))
    got = dj.depth(frame, strict, nc, out=out)
    U.assert_blocks_equal([t.cpu().numpy() for t in got], exp, shape)
    if n > 0:
        # one element too small: the total comes back, nothing is written
        small = tuple(torch.full((n - 1,), -7, dtype=torch.int32, device="cuda") for _ in range(4))
        with pytest.raises(ValueError, match=f"fewer than {n} blocks"):
            dj.depth(frame, strict, nc, out=small)
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in small)
        opts = _engine.make_opts(strict, nc)
        ix = dj.engine.index_build_dev(frame.as_c(), opts, False)          # no end order: completed on demand
        try:
            total, fits = dj.engine.depth_dev(ix, opts, n - 1, *(t.data_ptr() for t in small))
            assert (total, fits) == (n, False)
            total, fits = dj.engine.depth_dev(ix, opts, n, *(t.data_ptr() for t in out))
            assert (total, fits) == (n, True)
        finally:
            ix.close()
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in small)
        U.assert_blocks_equal([t.cpu().numpy() for t in out], exp, shape)


def test_two_calls_return_identical_arrays(eng):
    rng = np.random.default_rng(2024)
    c, s, e = U.random_rows(rng, 100_000, 24, 40_000, max_len=300)
    a = eng.depth((c, s, e), True, 24)
    b = eng.depth((c, s, e), True, 24)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    U.assert_blocks_equal(a, U.depth_events(c, s, e, True, 24))


@pytest.mark.parametrize("seed", range(30))
def test_random_sweep(eng, seed):
    c, s, e, nc, strict = U.sweep_case(seed)
    U.assert_blocks_equal(eng.depth((c, s, e), strict, nc), U.depth_events(c, s, e, strict, nc), f"seed {seed}: n={len(c)} strict={strict}")
