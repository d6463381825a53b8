"""overlap_bases on the GPU, compared exactly (int64) with the prefix form of tests/_depth_sum_util.py -- which
tests/test_depth_sum_cpu.py holds against the pair form and the depth-block form -- through the host entry
(Engine.overlap_bases) and the device entry (ivj_overlap_bases_dev via device_api: caller's buffer, prebuilt index without the
end order).  The shapes sit on the kernel's paths: both metadata forms (CM_LDS), the joint grid's narrow and wide bins, crowded
bins, the flag path of an index with a start > end row, the tiles of the position-sum scan, sums beyond 32 bits, int32 limits."""
import numpy as np
import pytest

from polars_bio_amd import _engine
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


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_host_entry(eng, shape, strict):
    probe, build, nc, exp = S.expected(shape, strict)
    S.assert_bases_equal(eng.overlap_bases(probe, build, strict, nc), exp, shape)


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_device_entry(dj, shape, strict):
    import torch
    probe, build, nc, exp = S.expected(shape, strict)
    p, b = _side(probe), _side(build)
    got = dj.overlap_bases(p, b, strict, nc)
    assert got.dtype == torch.int64 and got.is_cuda
    S.assert_bases_equal(got.cpu().numpy(), exp, shape)
    # the caller's buffer, and an index built without the end order: completed on demand, position sums on its first call only
    out = torch.full((len(exp),), -7, dtype=torch.int64, device="cuda")
    opts = _engine.make_opts(strict, nc)
    ix = dj.engine.index_build_dev(b.as_c(), opts, False)
    try:
        assert dj.overlap_bases(p, b, strict, nc, index=ix, out=out) is out
        S.assert_bases_equal(out.cpu().numpy(), exp, f"{shape}: out=, first call on the index")
        out.fill_(-7)
        dj.overlap_bases(p, b, strict, nc, index=ix, out=out)
        S.assert_bases_equal(out.cpu().numpy(), exp, f"{shape}: out=, second call on the index")
    finally:
        ix.close()


def test_null_output_is_refused(dj):
    probe, build, nc, _ = S.expected("three_rows", True)
    p, b = _side(probe), _side(build)
    opts = _engine.make_opts(True, nc)
    ix = dj.engine.index_build_dev(b.as_c(), opts, False)
    try:
        with pytest.raises(Exception, match="bases is NULL"):
            dj.engine.overlap_bases_dev(ix, p.as_c(), opts, 0)
    finally:
        ix.close()


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", ["contigs_24", "contigs_cm_lds_plus", "degenerate_build", "scan_300k", "deep_70k", "int32_limits"])
def test_partition_modes_return_identical_arrays(eng, shape, strict):
    probe, build, nc, exp = S.expected(shape, strict)
    got = [eng.overlap_bases(probe, build, strict, nc, partition_mode=m) for m in (0, 1, 2)]
    S.assert_bases_equal(got[0], exp, shape)
    assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes()


def test_two_calls_return_identical_arrays(eng):
    rng = np.random.default_rng(2025)
    build = S.U.random_rows(rng, 100_000, 24, 40_000, max_len=300)
    probe = S.U.random_rows(rng, 100_000, 24, 40_000, max_len=3000)
    a = eng.overlap_bases(probe, build, True, 24)
    b = eng.overlap_bases(probe, build, True, 24)
    assert a.tobytes() == b.tobytes()
    S.assert_bases_equal(a, S.prefix_form(probe, build, True, 24))


def test_scan_wide_tiles(eng):
    """S.SCAN_WIDE_FROM build rows: the one size at which the position sums take the scan's other tile form"""
    probe, build, nc = S.scan_wide_case()
    assert len(build[0]) + 1 >= S.SCAN_WIDE_FROM
    S.assert_bases_equal(eng.overlap_bases(probe, build, True, nc), S.prefix_form(probe, build, True, nc))


@pytest.mark.parametrize("seed", range(30))
def test_random_sweep(eng, seed):
    probe, build, nc, strict = S.sweep_case(seed)
    S.assert_bases_equal(eng.overlap_bases(probe, build, strict, nc), S.prefix_form(probe, build, strict, nc),
                         f"seed {seed}: probes={len(probe[0])} build={len(build[0])} contigs={nc} strict={strict}")
