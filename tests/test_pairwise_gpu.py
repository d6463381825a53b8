"""pairwise_jaccard's two matrices on the GPU, compared exactly with the event form of tests/_pairwise_util.py through the host
entry (Engine.multi_pairwise) and the device entry (ivj_multi_pairwise_dev via device_api), Strict and Weak.  The extra shapes
sit around the kernel's wavefront step and workgroup tile (P.STEP / P.TILE = PW_STEP / PW_TILE of
polars-bio_amd/csrc/pairwise.hip.h)."""
import numpy as np
import pytest

from polars_bio_amd import _engine
import _pairwise_util as P

U, S = P.U, P.S
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
    return torch.from_numpy(np.array(a, np.int32)).cuda()          # a copy: the shared cases are read-only


def _sides(frames):
    from polars_bio_amd.device_api import DeviceSide
    return [DeviceSide(*(_t(x) for x in f)) for f in frames]


def _check_matrices(got, frames, strict, nc, exp, what):
    assert all(isinstance(x, np.ndarray) and x.dtype == np.int64 for x in got)
    P.assert_equal(got, exp, what)
    bases, runs = got
    assert (bases == bases.T).all() and (runs == runs.T).all()
    for f, frame in enumerate(frames):                              # the diagonal: the frame's own positions and union runs
        c, s, e1 = S.union_runs(frame, strict, nc)
        assert (int(bases[f, f]), int(runs[f, f])) == (int((e1 - s).sum()), len(c)), f"{what}: frame {f}"


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", list(P.SHAPES))
def test_host_entry(eng, shape, strict):
    frames, nc = P.case(shape, strict)
    _check_matrices(eng.multi_pairwise(frames, strict, nc), frames, strict, nc, P.expected(shape, strict), shape)


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", list(P.SHAPES))
def test_device_entry(dj, shape, strict):
    """frames without rows reach the entry as NULL indexes; caller tensors are filled in place"""
    import torch
    frames, nc = P.case(shape, strict)
    n = len(frames)
    sides = _sides(frames)
    exp = P.expected(shape, strict)
    got = dj.multi_pairwise(sides, strict, nc)
    assert all(t.dtype == torch.int64 and t.is_cuda and tuple(t.shape) == (n, n) for t in got)
    _check_matrices([t.cpu().numpy() for t in got], frames, strict, nc, exp, shape)
    out = tuple(torch.full((n * n,), -7, dtype=torch.int64, device="cuda") for _ in range(2))
    got = dj.multi_pairwise(sides, strict, nc, out=out)
    assert all(g.data_ptr() == o.data_ptr() for g, o in zip(got, out))
    P.assert_equal([t.cpu().numpy().reshape(n, n) for t in out], exp, f"{shape} out=")


@pytest.mark.parametrize("strict", MODES)
def test_device_entry_takes_prebuilt_indexes(dj, strict):
    """indexes built without the end order and with the lookup tables are accepted; a NULL index in the middle is an empty frame:
    its row and column are zero, the other frames keep their places"""
    import torch
    shape = f"segments_{P.TILE + 1}"
    frames, nc = P.case(shape, strict)
    n = len(frames)
    sides = _sides(frames)
    opts = _engine.make_opts(strict, nc)
    ixs = [dj.engine.index_build_dev(side.as_c(), opts, False) for side in sides]
    try:
        got = dj.multi_pairwise(sides, strict, nc, indexes=ixs)
        P.assert_equal([t.cpu().numpy() for t in got], P.expected(shape, strict), shape)
        out = tuple(torch.full((n, n), -7, dtype=torch.int64, device="cuda") for _ in range(2))
        dj.engine.multi_pairwise_dev([ixs[0], ixs[1], None, ixs[3], ixs[4]], opts, out[0].data_ptr(), out[1].data_ptr())
        torch.cuda.synchronize()
        holed = [frames[0], frames[1], S.EMPTY, frames[3], frames[4]]
        P.assert_equal([t.cpu().numpy() for t in out], P.pairwise_events(holed, strict, nc), "a NULL index")
        assert not out[0][2].any() and not out[0][:, 2].any()
        with pytest.raises(ValueError, match="one entry per frame"):
            dj.multi_pairwise(sides, strict, nc, indexes=ixs[:3])
        with pytest.raises(ValueError, match="out must hold"):
            dj.multi_pairwise(sides, strict, nc, out=(out[0], out[1][:2]))
        with pytest.raises(_engine.EngineError, match="NULL"):
            dj.engine.multi_pairwise_dev(ixs, opts, out[0].data_ptr(), 0)
    finally:
        for ix in ixs:
            ix.close()


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", ["frames_64", "abutting_chain", "degenerate_mixed"])
def test_every_pair_equals_set_stats(eng, shape, strict):
    """an independent device path: the two-frame walk of the set operations, pair by pair"""
    frames, nc = P.case(shape, strict)
    bases, runs = eng.multi_pairwise(frames, strict, nc)
    for i in range(len(frames)):
        for j in range(i, len(frames)):
            _only_a, _only_b, both, n_int = eng.set_stats(frames[i], frames[j], strict, nc)
            assert (int(bases[i, j]), int(runs[i, j])) == (both, n_int), (i, j)


def test_the_library_refuses_what_the_binding_refuses(eng):
    """the C entry's own argument checks (the binding's checks are bypassed)"""
    import ctypes as C
    frames, nc = P.case("two_frames", True)
    sides = (_engine._Side * 2)()
    keep = []
    for f, frame in enumerate(frames):
        sides[f], arrays = _engine._host_side(*frame)
        keep.append(arrays)
    o = _engine.make_opts(True, nc)
    out = np.full((2, 4), -7, np.int64)
    for n_frames in (0, 65, -1):
        assert eng.L.ivj_multi_pairwise(eng.h, sides, n_frames, C.byref(o), out[0].ctypes.data, out[1].ctypes.data) == -1, n_frames
    assert eng.L.ivj_multi_pairwise(eng.h, None, 2, C.byref(o), out[0].ctypes.data, out[1].ctypes.data) == -1
    assert eng.L.ivj_multi_pairwise(eng.h, sides, 2, C.byref(o), out[0].ctypes.data, None) == -1
    assert (out == -7).all()


def test_two_calls_return_identical_bytes(eng):
    frames, nc = P.case("frames_64", True)
    x = eng.multi_pairwise(frames, True, nc)
    y = eng.multi_pairwise(frames, True, nc)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y))
    assert x[0][63].any() and x[1][:, 63].any(), "frame 63 takes part"
