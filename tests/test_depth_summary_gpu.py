"""depth_summary on the GPU, compared exactly with the block form of tests/_depth_summary_util.py -- which
tests/test_depth_summary_cpu.py holds against the per-base form and the identities -- through the host entry
(Engine.depth_summary) and the device entry (ivj_depth_summary_dev via device_api: caller's buffers, a prebuilt index without the
end order, called twice).  The shapes sit on the kernel's paths: no block / one block / block boundaries under a probe, the tree
of depth maxima over one to three levels with partial 16-blocks, 0 / 1 / 3 / 4 / 8 thresholds, both metadata forms (CM_LDS), the
joint grid's narrow, wide and crowded bins, the flag path of depth_core, depths beyond 16 bits, the int32 limits, both tile forms
of the scan, the depth kernel's tile edge."""
import numpy as np
import pytest

from polars_bio_amd import _engine
import _depth_sum_util as S
import _depth_summary_util as D

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
@pytest.mark.parametrize("shape", list(D.SHAPES))
def test_host_entry(eng, shape, strict):
    probe, build, nc, thr, md, bg = D.expected(shape, strict)
    D.assert_summary_equal(eng.depth_summary(probe, build, strict, nc, thr), (md, bg), shape)


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", list(D.SHAPES))
def test_device_entry(dj, shape, strict):
    import torch
    probe, build, nc, thr, md, bg = D.expected(shape, strict)
    p, b = _side(probe), _side(build)
    gm, gb = dj.depth_summary(p, b, strict, nc, thr)
    assert gm.dtype == torch.int32 and gb.dtype == torch.int64 and gm.is_cuda and gb.is_cuda
    D.assert_summary_equal((gm.cpu().numpy(), gb.cpu().numpy()), (md, bg), shape)
    # the caller's buffers, prefilled, and an index built without the end order (completed on demand), twice
    om = torch.full((len(md),), -7, dtype=torch.int32, device="cuda")
    ob = torch.full(bg.shape, -7, dtype=torch.int64, device="cuda")
    opts = _engine.make_opts(strict, nc)
    ix = dj.engine.index_build_dev(b.as_c(), opts, False)
    try:
        for call in ("first", "second"):
            rm, rb = dj.depth_summary(p, b, strict, nc, thr, index=ix, out_max=om, out_bases=ob)
            assert rm is om and rb is ob
            D.assert_summary_equal((om.cpu().numpy(), ob.cpu().numpy()), (md, bg), f"{shape}: caller buffers, {call} call on the index")
            om.fill_(-7)
            ob.fill_(-7)
    finally:
        ix.close()


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("thr", [(), (2,), (1, 4, 7), (1, 2, 3, 4, 5, 6, 7, 50), (60,), (7, 1, 7, 4, 1)],
                         ids=["none", "one", "three", "eight", "above_every_depth", "repeated_unsorted"])
def test_threshold_counts(eng, thr, strict):
    probe, build, nc, _thr, _md, _bg = D.expected("blocks_5000_deepest_alone", strict)
    md, bg = D.block_form(probe, build, strict, nc, thr)
    if thr == (60,):
        assert (bg == 0).all() and md.max() == 50
    D.assert_summary_equal(eng.depth_summary(probe, build, strict, nc, thr), (md, bg), f"thresholds {thr}")


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", ["small_edges", "blocks_5000", "contigs_cm_lds_plus"])
def test_thresholds_only(eng, shape, strict):
    probe, build, nc, thr, md, bg = D.expected(shape, strict)
    thr = thr or (1, 2)
    _, bg = D.block_form(probe, build, strict, nc, thr)
    gm, gb = eng.depth_summary(probe, build, strict, nc, thr, want_max=False)
    assert gm is None
    D.assert_summary_equal((None, gb), (md, bg), f"{shape}: max_depth = NULL")


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", ["contigs_24", "contigs_cm_lds_plus", "degenerate_build", "blocks_5000", "deep_70k", "whole_range"])
def test_partition_modes_return_identical_arrays(eng, shape, strict):
    probe, build, nc, thr, md, bg = D.expected(shape, strict)
    got = [eng.depth_summary(probe, build, strict, nc, thr, partition_mode=m) for m in (0, 1, 2)]
    D.assert_summary_equal(got[0], (md, bg), shape)
    assert got[0][0].tobytes() == got[1][0].tobytes() == got[2][0].tobytes()
    assert got[0][1].tobytes() == got[1][1].tobytes() == got[2][1].tobytes()


def test_two_calls_return_identical_arrays(eng):
    rng = np.random.default_rng(2026)
    build = S.U.random_rows(rng, 50_000, 24, 20_000, max_len=300)
    probe = S.U.random_rows(rng, 50_000, 24, 20_000, max_len=3000)
    thr = (1, 10, 20, 30)
    a = eng.depth_summary(probe, build, True, 24, thr)
    b = eng.depth_summary(probe, build, True, 24, thr)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    D.assert_summary_equal(a, D.block_form(probe, build, True, 24, thr))


def test_the_whole_range_probe(eng):
    probe, build, nc, thr, md, bg = D.expected("whole_range", False)
    gm, gb = eng.depth_summary(probe, build, False, nc, thr)
    assert gb[0, 0] == 2 ** 32 == bg[0, 0] and gm[0] == md[0]


def test_scan_wide_tiles(eng):
    """more than S.SCAN_WIDE_FROM blocks: the one size at which the threshold table's scans take their other tile form"""
    probe, build, nc, thr = D.scan_wide_case()
    kc = D.U.depth_events(*build, True, nc)[0]
    assert len(kc) + 1 >= S.SCAN_WIDE_FROM
    D.assert_summary_equal(eng.depth_summary(probe, build, True, nc, thr), D.block_form(probe, build, True, nc, thr))


@pytest.mark.parametrize("seed", range(30))
def test_random_sweep(eng, seed):
    probe, build, nc, strict, thr = D.sweep_case(seed)
    D.assert_summary_equal(eng.depth_summary(probe, build, strict, nc, thr), D.block_form(probe, build, strict, nc, thr),
                           f"seed {seed}: probes={len(probe[0])} build={len(build[0])} contigs={nc} strict={strict} thresholds={thr}")


def test_bad_arguments_are_refused(eng, dj):
    probe, build, nc, _thr, _md, _bg = D.expected("small_edges", True)
    with pytest.raises(_engine.EngineError, match=r"thresholds\[1\] must be >= 1"):
        eng.depth_summary(probe, build, True, nc, (1, 0))
    with pytest.raises(_engine.EngineError, match=r"thresholds\[0\] must be >= 1"):
        eng.depth_summary(probe, build, True, nc, (-3,))
    with pytest.raises(_engine.EngineError, match=r"n_thresholds must be in 0 \.\. 8"):
        eng.depth_summary(probe, build, True, nc, tuple(range(1, 10)))
    with pytest.raises(_engine.EngineError, match="max_depth and bases_ge are both NULL"):
        eng.depth_summary(probe, build, True, nc, (), want_max=False)
    # the output checks do not depend on the number of probe rows
    with pytest.raises(_engine.EngineError, match="max_depth and bases_ge are both NULL"):
        eng.depth_summary(D.S.EMPTY, build, True, nc, (), want_max=False)
    p, b = _side(probe), _side(build)
    opts = _engine.make_opts(True, nc)
    ix = dj.engine.index_build_dev(b.as_c(), opts, False)
    try:
        import torch
        none = _side(D.S.EMPTY)
        with pytest.raises(_engine.EngineError, match="bases_ge is NULL"):
            dj.engine.depth_summary_dev(ix, none.as_c(), opts, (1,), torch.zeros(1, dtype=torch.int32, device="cuda").data_ptr(), 0)
        with pytest.raises(_engine.EngineError, match="max_depth and bases_ge are both NULL"):
            dj.engine.depth_summary_dev(ix, none.as_c(), opts, (1,), 0, 0)
        om = torch.zeros(p.n, dtype=torch.int32, device="cuda")
        with pytest.raises(_engine.EngineError, match="bases_ge is NULL"):
            dj.engine.depth_summary_dev(ix, p.as_c(), opts, (1, 2), om.data_ptr(), 0)
        with pytest.raises(_engine.EngineError, match="max_depth and bases_ge are both NULL"):
            dj.engine.depth_summary_dev(ix, p.as_c(), opts, (1, 2), 0, 0)
        with pytest.raises(_engine.EngineError, match="max_depth and bases_ge are both NULL"):
            dj.engine.depth_summary_dev(ix, p.as_c(), opts, (), 0, 0)
        with pytest.raises(_engine.EngineError, match=r"n_thresholds must be in 0 \.\. 8"):
            dj.engine.depth_summary_dev(ix, p.as_c(), opts, tuple(range(1, 10)), 0, 0)
    finally:
        ix.close()
