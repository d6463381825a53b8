"""depth_profile on the GPU, compared exactly (int64) with the explicit-bin expectation of tests/_depth_profile_util.py -- which
tests/test_depth_profile_cpu.py holds against the pair form -- in both coordinate systems, every case through the host entry
(Engine.depth_profile) and the device entry (ivj_depth_profile_dev via device_api: caller's buffer, prebuilt index without the end
order).  The cases sit on the kernel's paths: edge counts around its tile and workgroup sizes, rows that straddle wavefronts,
items and workgroups, empty bins, windows over all of int32 (the 64-bit product), both metadata forms (CM_LDS), the joint grid's
narrow, wide and crowded bins, the flag path of an index with a start > end row, sums beyond 32 bits, the reversal."""
import numpy as np
import pytest

from polars_bio_amd import _engine
import _depth_profile_util as P
import _depth_sum_util as S

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


def _side(cols):
    import torch
    from polars_bio_amd.device_api import DeviceSide
    return DeviceSide(*(torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in cols))


def _check_both_entries(eng, dj, windows, build, strict, nc, n_bins, reverse, exp, what, flags_as=bool):
    """host entry; device entry on a prebuilt index without the end order into the caller's buffer, twice; the device entry takes
    the flags as a bool or (flags_as=np.uint8) a uint8 tensor"""
    import torch
    n = len(windows[0])
    P.assert_profile_equal(eng.depth_profile(windows, reverse, n_bins, build, strict, nc), exp, f"{what}: host entry")
    w, b = _side(windows), _side(build)
    rev = None if reverse is None else torch.from_numpy(np.asarray(reverse, bool).astype(flags_as)).cuda()
    out = torch.full((n, n_bins), -7, dtype=torch.int64, device="cuda")
    opts = _engine.make_opts(strict, nc)
    ix = dj.engine.index_build_dev(b.as_c(), opts, False)
    try:
        assert dj.depth_profile(w, b, strict, nc, n_bins, reverse=rev, index=ix, out=out) is out
        first = out.cpu().numpy()
        P.assert_profile_equal(first, exp, f"{what}: device entry, first call on the index")
        out.fill_(-7)
        dj.depth_profile(w, b, strict, nc, n_bins, reverse=rev, index=ix, out=out)
        assert out.cpu().numpy().tobytes() == first.tobytes(), f"{what}: two calls differ"
    finally:
        ix.close()


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", P.SHAPES)
def test_shapes(eng, dj, shape, strict):
    windows, build, nc, _ = S.expected(shape, strict)
    reverse = P.mixed_flags(len(windows[0]))
    exp = P.expected_bases(windows, build, strict, nc, P.SHAPE_BINS, reverse)
    _check_both_entries(eng, dj, windows, build, strict, nc, P.SHAPE_BINS, reverse, exp, shape)


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("n_bins", P.N_BINS)
def test_n_bins_and_window_lengths(eng, dj, n_bins, strict):
    """L = 0, 1, B - 1, B, B + 1, primes, no position -- and ordinary windows -- at every bin count"""
    build, nc = P.small_build()
    lw = P.length_windows(n_bins, strict)
    rw = P.random_windows(31 + n_bins, 40, nc)
    windows = tuple(np.concatenate([a, b]) for a, b in zip(lw, rw))
    exp = P.expected_bases(windows, build, strict, nc, n_bins)
    assert (exp > 0).any() and (P.bin_lengths(windows, n_bins, strict) == 0).any()
    _check_both_entries(eng, dj, windows, build, strict, nc, n_bins, None, exp, f"n_bins={n_bins}")
    if n_bins == 1:
        S.assert_bases_equal(eng.overlap_bases(windows, build, strict, nc), exp[:, 0], "n_bins=1 is overlap_bases")


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("n, n_bins", P.BOUNDARIES)
def test_edge_counts_around_the_tile_and_workgroup_sizes(eng, dj, n, n_bins, strict):
    build, nc = P.small_build()
    windows = P.random_windows(1000 * n + n_bins, n, nc, max_len=3000)
    reverse = P.mixed_flags(n, seed=n)
    exp = P.expected_bases(windows, build, strict, nc, n_bins, reverse)
    _check_both_entries(eng, dj, windows, build, strict, nc, n_bins, reverse, exp, f"{n} x ({n_bins} + 1) edges")


@pytest.mark.parametrize("strict", MODES)
def test_rows_straddle_every_boundary(eng, dj, strict):
    """5000 rows of 101 edges over 494 workgroups: rows start at every offset of a wavefront, an item and a workgroup"""
    build, nc = P.small_build(n=20_000)
    windows = P.random_windows(77, 5000, nc)
    exp = P.expected_bases(windows, build, strict, nc, 100)
    _check_both_entries(eng, dj, windows, build, strict, nc, 100, None, exp, "5000 x 100")


@pytest.mark.parametrize("strict", MODES)
def test_windows_over_all_of_int32(eng, dj, strict):
    windows = P.whole_range_windows(strict)
    _, build, nc, _ = S.expected("int32_limits", strict)
    assert P.bin_lengths(windows, P.MAX_BINS, strict).sum(axis=1)[0] == 2 ** 32 - (1 if strict else 0)
    exp = P.expected_bases(windows, build, strict, nc, P.MAX_BINS)
    assert (exp > 0).any()
    _check_both_entries(eng, dj, windows, build, strict, nc, P.MAX_BINS, None, exp, "whole range")


@pytest.mark.parametrize("strict", MODES)
def test_reversal(eng, dj, strict):
    windows, build, nc, _ = S.expected("crowded_bins", strict)
    n, n_bins = len(windows[0]), 9
    plain = P.expected_bases(windows, build, strict, nc, n_bins)
    assert (plain != plain[:, ::-1]).any()
    none = eng.depth_profile(windows, None, n_bins, build, strict, nc)
    P.assert_profile_equal(none, plain, "reverse=None")
    # every form of the flags through both entries, checked against the unreversed call
    _check_both_entries(eng, dj, windows, build, strict, nc, n_bins, None, none, "reverse=None")
    _check_both_entries(eng, dj, windows, build, strict, nc, n_bins, np.zeros(n, bool), none, "no flag set", flags_as=np.uint8)
    _check_both_entries(eng, dj, windows, build, strict, nc, n_bins, np.ones(n, bool), np.ascontiguousarray(none[:, ::-1]), "all set")
    _check_both_entries(eng, dj, windows, build, strict, nc, n_bins, np.ones(n, bool), np.ascontiguousarray(none[:, ::-1]), "all set, uint8",
                        flags_as=np.uint8)
    flags = P.mixed_flags(n)
    mixed = np.where(flags[:, None], none[:, ::-1], none)
    _check_both_entries(eng, dj, windows, build, strict, nc, n_bins, flags, mixed, "mixed")
    _check_both_entries(eng, dj, windows, build, strict, nc, n_bins, flags, mixed, "mixed, uint8", flags_as=np.uint8)


@pytest.mark.parametrize("strict", MODES)
def test_deep_window_in_seven_bins(eng, dj, strict):
    probe, build, nc, bases = S.expected("deep_70k", strict)
    windows = tuple(a[:1] for a in probe)                    # [0, 99 000) under 70 000 rows
    exp = P.expected_bases(windows, build, strict, nc, 7)
    assert (exp > 2 ** 29).all() and exp.sum() == bases[0] > 2 ** 32
    _check_both_entries(eng, dj, windows, build, strict, nc, 7, None, exp, "deep_70k")


def test_bad_bin_counts_are_refused_and_leave_the_output_alone(dj):
    import torch
    windows, build, nc, _ = S.expected("three_rows", True)
    w, b = _side(windows), _side(build)
    opts = _engine.make_opts(True, nc)
    out = torch.full((len(windows[0]) * 8,), -7, dtype=torch.int64, device="cuda")
    ix = dj.engine.index_build_dev(b.as_c(), opts, False)
    try:
        for bad in (0, P.MAX_BINS + 1, -1):
            with pytest.raises(_engine.EngineError, match=f"n_bins must be in .*got {bad}") as err:
                dj.engine.depth_profile_dev(ix, w.as_c(), 0, bad, opts, out.data_ptr())
            assert err.value.code == -1                      # IVJ_EINVAL
            assert (out == -7).all()
        with pytest.raises(_engine.EngineError, match="bases is NULL"):
            dj.engine.depth_profile_dev(ix, w.as_c(), 0, 5, opts, 0)
    finally:
        ix.close()
    for bad in (0, P.MAX_BINS + 1, 10 ** 9):                 # the host entry: refused by the library, and no matrix is allocated first
        with pytest.raises(_engine.EngineError, match=f"n_bins must be in .*got {bad}"):
            dj.engine.depth_profile(windows, None, bad, build, True, nc)
