"""multi_intersect / consensus on the GPU, compared exactly with the event form of tests/_multi_util.py through the host entry
(Engine.multi_inter) and the device entry (ivj_multi_inter_dev via device_api, capacity protocol included), Strict and Weak,
for every min_frames of {1, 2, F}.  The shapes sit around the walk's merged-sequence tile (U.T = MI_TILE of
polars-bio_amd/csrc/multi.hip.h); the run boundary events of a frame set come in pairs, so 3 T and 3 T + 2 stand for the odd
count 3 T + 1."""
import numpy as np
import pytest

from polars_bio_amd import _engine
import _multi_util as U

S = U.S
pytestmark = pytest.mark.gpu

MODES = [pytest.param(True, id="strict"), pytest.param(False, id="weak")]
KINDS = [pytest.param(False, id="segments"), pytest.param(True, id="consensus")]
SEG, CONS = _engine.MULTI_SEGMENTS, _engine.MULTI_CONSENSUS


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


def _host(tensors):
    return [t.cpu().numpy() for t in tensors]


@pytest.mark.parametrize("consensus", KINDS)
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", list(U.SHAPES))
def test_host_entry(eng, shape, strict, consensus):
    frames, nc = U.case(shape, strict)
    for k in U.min_frames_of(len(frames)):
        exp = U.expected(shape, strict, k, consensus)
        got = eng.multi_inter(frames, k, CONS if consensus else SEG, strict, nc)
        assert all(x.dtype == np.int32 for x in got[:3])
        assert (got[3] is None) if consensus else (got[3].dtype == np.uint64)
        U.assert_equal(got, exp, f"{shape} k={k}")


@pytest.mark.parametrize("consensus", KINDS)
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", list(U.SHAPES))
def test_device_entry(dj, shape, strict, consensus):
    """frames without rows reach the entry as NULL indexes; caller buffers of exactly n work, buffers of n - 1 return the total
    and stay untouched"""
    import torch
    from polars_bio_amd.device_api import DeviceSide
    frames, nc = U.case(shape, strict)
    sides = [DeviceSide(*(_t(x) for x in f)) for f in frames]
    dtypes = (torch.int32,) * 3 + (() if consensus else (torch.int64,))
    for k in U.min_frames_of(len(frames)):
        exp = U.expected(shape, strict, k, consensus)
        got = dj.multi_inter(sides, k, strict, nc, consensus=consensus)
        assert len(got) == len(dtypes) and all(t.dtype == d and t.is_cuda for t, d in zip(got, dtypes))
        U.assert_equal(_host(got) + [None] * consensus, exp, f"{shape} k={k}")
        n = len(exp[0])
        out = tuple(torch.full((n,), -7, dtype=d, device="cuda") for d in dtypes)
        got = dj.multi_inter(sides, k, strict, nc, consensus=consensus, out=out)
        U.assert_equal(_host(got) + [None] * consensus, exp, f"{shape} k={k} out=")
        if n > 0:
            small = tuple(torch.full((n - 1,), -7, dtype=d, device="cuda") for d in dtypes)
            with pytest.raises(ValueError, match=f"fewer than {n} regions"):
                dj.multi_inter(sides, k, strict, nc, consensus=consensus, out=small)
            torch.cuda.synchronize()
            assert all(bool((t == -7).all()) for t in small)


@pytest.mark.parametrize("strict", MODES)
def test_device_entry_completes_a_missing_end_order(dj, strict):
    """indexes built without the end order and with the lookup tables are accepted; the capacity protocol at the C entry; the
    mask buffer may be NULL for consensus and may not for segments"""
    import torch
    from polars_bio_amd.device_api import DeviceSide
    frames, nc = U.case(U.EVENTS_IDENTITY, strict)
    opts = _engine.make_opts(strict, nc)
    ixs = [dj.engine.index_build_dev(DeviceSide(*(_t(x) for x in f)).as_c(), opts, False) for f in frames]
    try:
        exp = U.expected(U.EVENTS_IDENTITY, strict, 2, False)
        n = len(exp[0])
        dtypes = (torch.int32,) * 3 + (torch.int64,)
        small = tuple(torch.full((n - 1,), -7, dtype=d, device="cuda") for d in dtypes)
        out = tuple(torch.full((n,), -7, dtype=d, device="cuda") for d in dtypes)
        assert dj.engine.multi_inter_dev(ixs, opts, 2, SEG, n - 1, *(t.data_ptr() for t in small)) == (n, False)
        assert dj.engine.multi_inter_dev(ixs, opts, 2, SEG, n, *(t.data_ptr() for t in out)) == (n, True)
        torch.cuda.synchronize()
        assert all(bool((t == -7).all()) for t in small)
        U.assert_equal(_host(out), exp)
        with pytest.raises(_engine.EngineError, match="NULL"):
            dj.engine.multi_inter_dev(ixs, opts, 2, SEG, n, *(t.data_ptr() for t in out[:3]), 0)
        cexp = U.expected(U.EVENTS_IDENTITY, strict, 2, True)
        cout = tuple(torch.full((len(cexp[0]),), -7, dtype=torch.int32, device="cuda") for _ in range(3))
        assert dj.engine.multi_inter_dev(ixs, opts, 2, CONS, len(cexp[0]), *(t.data_ptr() for t in cout), 0) == (len(cexp[0]), True)
        torch.cuda.synchronize()
        U.assert_equal(_host(cout) + [None], cexp)
        # a NULL index in the middle = an empty frame: bit 1 never appears, the other bits keep their places
        got = tuple(torch.empty(4 * U.T, dtype=d, device="cuda") for d in dtypes)
        m, fits = dj.engine.multi_inter_dev([ixs[0], None, ixs[2]], opts, 1, SEG, 4 * U.T, *(t.data_ptr() for t in got))
        torch.cuda.synchronize()
        assert fits
        U.assert_equal([t[:m] for t in _host(got)], U.multi_events([frames[0], S.EMPTY, frames[2]], strict, nc, 1, False))
    finally:
        for ix in ixs:
            ix.close()


def test_the_library_refuses_what_the_binding_refuses(eng):
    """the C entry's own argument checks (the binding's checks are bypassed)"""
    import ctypes as C
    frames, nc = U.case("two_frames", True)
    sides = (_engine._Side * 2)()
    keep = []
    for f, frame in enumerate(frames):
        sides[f], arrays = _engine._host_side(*frame)
        keep.append(arrays)
    o = _engine.make_opts(True, nc)
    for n_frames, k, mode in ((0, 1, 0), (65, 1, 0), (2, 0, 0), (2, 3, 0), (2, 1, 2)):
        out = _engine._Segments()
        assert eng.L.ivj_multi_inter(eng.h, sides, n_frames, C.byref(o), k, mode, C.byref(out)) == -1, (n_frames, k, mode)
        assert out.n == 0


@pytest.mark.parametrize("strict", MODES)
def test_identities_against_the_existing_operations(eng, strict):
    frames, nc = U.case(U.EVENTS_IDENTITY, strict)
    a, b = frames[0], frames[1]
    # two frames: consensus(1) = union, consensus(2) = intersection
    for k, op in ((1, "union"), (2, "intersection")):
        got = eng.multi_inter([a, b], k, CONS, strict, nc)
        S.assert_regions_equal(got[:3], [x.astype(np.int64) for x in eng.setop(a, b, op, strict, nc)], op)
    # one frame: its segments are merge's intervals (the rows of a frame of this shape neither overlap nor touch)
    c, s, e, mask = eng.multi_inter([a], 1, SEG, strict, nc)
    mc, ms, me, _n = eng.merge(a, strict, nc)
    assert (mask == 1).all()
    S.assert_regions_equal((c, s, e), [x.astype(np.int64) for x in (mc, ms, me)], "merge")
    # per frame: the summed length of the segments that carry its bit = the positions it covers
    c, s, e, mask = eng.multi_inter(frames, 1, SEG, strict, nc)
    length = U.lengths(s, e, strict)
    for f, frame in enumerate(frames):
        covered = eng.set_stats(frame, S.EMPTY, strict, nc)[0]
        assert int(length[(mask >> np.uint64(f)) & np.uint64(1) == 1].sum()) == covered, f"frame {f}"
    # consensus(k) = the segments with n_frames >= k, merged where they touch
    for k in (1, 2, 3):
        keep = U.popcount(mask) >= k
        exp = U.merge_touching(c[keep], s[keep], e[keep], strict)
        S.assert_regions_equal(eng.multi_inter(frames, k, CONS, strict, nc)[:3], exp, f"consensus {k}")
        seg_k = eng.multi_inter(frames, k, SEG, strict, nc)
        U.assert_equal(seg_k, (c[keep].astype(np.int64), s[keep].astype(np.int64), e[keep].astype(np.int64), mask[keep]), f"segments {k}")


def test_two_calls_return_identical_arrays(eng):
    frames, nc = U.case("frames_64", True)
    x = eng.multi_inter(frames, 2, SEG, True, nc)
    y = eng.multi_inter(frames, 2, SEG, True, nc)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(x, y))
    assert (x[3] >> np.uint64(63)).any(), "bit 63 survives"
