"""depth_hist on the GPU, compared exactly with the block form of tests/_depth_hist_util.py -- which tests/test_depth_hist_cpu.py
holds against the per-base form and the identities -- through the host entries (Engine.depth_hist, Engine.depth_hist_contigs) and
the device entries (ivj_depth_hist_dev / ivj_depth_hist_contigs_dev via device_api: caller's buffers prefilled, a prebuilt index
without the end order, called twice).  The shapes of depth_summary sit on the paths the two share (the block range, both metadata
forms, the joint grid's bins, depth_core's flag path, depths beyond 16 bits, the int32 limits); the new ones sit on the kernel's
own edges: the workgroup's tile of P probes, a range over several 2048-item chunks, every lane on one LDS address, the clamp at
max_depth, dead probes among live ones, no probes, no blocks; a tile of the contig form across a contig boundary, tiny contigs."""
import ctypes as C

import numpy as np
import pytest

from polars_bio_amd import _engine
import _depth_sum_util as S
import _depth_summary_util as D
import _depth_hist_util as H

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
@pytest.mark.parametrize("shape", list(H.SHAPES))
def test_host_entry(eng, shape, strict):
    probe, build, nc, md, hist = H.expected(shape, strict)
    H.assert_hist_equal(eng.depth_hist(probe, build, strict, nc, md), hist, f"{shape}, max_depth {md}")


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", list(H.SHAPES))
def test_device_entry(dj, shape, strict):
    import torch
    probe, build, nc, md, hist = H.expected(shape, strict)
    p, b = _side(probe), _side(build)
    got = dj.depth_histogram(p, b, strict, nc, md)
    assert got.dtype == torch.int64 and got.is_cuda and tuple(got.shape) == hist.shape
    H.assert_hist_equal(got.cpu().numpy(), hist, shape)
    # the caller's buffer, prefilled, and an index built without the end order (completed on demand), twice
    out = torch.full(hist.shape, -7, dtype=torch.int64, device="cuda")
    opts = _engine.make_opts(strict, nc)
    ix = dj.engine.index_build_dev(b.as_c(), opts, False)
    try:
        for call in ("first", "second"):
            res = dj.depth_histogram(p, b, strict, nc, md, index=ix, out=out)
            assert res is out
            H.assert_hist_equal(out.cpu().numpy(), hist, f"{shape}: caller buffer, {call} call on the index")
            out.fill_(-7)
    finally:
        ix.close()


def test_an_output_off_the_16_byte_grid(dj):
    """an odd number of bins under an odd tile, into a buffer that starts 8 bytes off a 16-byte boundary: heads and tails of the stores"""
    import torch
    md = 682                                                     # 683 bins
    assert H.tile(md) * (md + 1) % 2 == 1                        # the second tile's block starts on an odd 8-byte word
    rng = np.random.default_rng(6500)
    probe, build = H.U.random_rows(rng, 3 * H.tile(md) + 2, 2, 5000, 300), H.U.random_rows(rng, 4000, 2, 5000, 80)
    hist = H.block_form(probe, build, True, 2, md)
    flat = torch.full((hist.size + 1,), -7, dtype=torch.int64, device="cuda")
    for off in (0, 1):
        out = flat[off:off + hist.size].view(hist.shape)
        dj.depth_histogram(_side(probe), _side(build), True, 2, md, out=out)
        H.assert_hist_equal(out.cpu().numpy(), hist, f"offset {off}")
        assert int(flat[hist.size if off == 0 else 0]) == -7
        flat.fill_(-7)


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", list(H.CONTIG_SHAPES))
def test_contig_form_both_entries(eng, dj, shape, strict):
    import torch
    frame, nc, md = H.CONTIG_SHAPES[shape](strict)
    exp = H.contig_form(frame, strict, nc, md)
    H.assert_hist_equal(eng.depth_hist_contigs(frame, strict, nc, md), exp, f"{shape}: host entry")
    f = _side(frame)
    out = torch.full(exp.shape, -7, dtype=torch.int64, device="cuda")
    opts = _engine.make_opts(strict, nc)
    ix = dj.engine.index_build_dev(f.as_c(), opts, False)
    try:
        for call in ("first", "second"):
            assert dj.depth_histogram_contigs(f, strict, nc, md, index=ix, out=out) is out
            H.assert_hist_equal(out.cpu().numpy(), exp, f"{shape}: caller buffer, {call} call on the index")
            out.fill_(-7)
    finally:
        ix.close()
    H.assert_hist_equal(dj.depth_histogram_contigs(f, strict, nc, md).cpu().numpy(), exp, f"{shape}: own index")


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", ["contigs_24", "contigs_cm_lds_plus", "degenerate_build", "blocks_5000", "deep_70k", "whole_range"])
def test_partition_modes_return_identical_arrays(eng, shape, strict):
    probe, build, nc, md, hist = H.expected(shape, strict)
    got = [eng.depth_hist(probe, build, strict, nc, md, partition_mode=m) for m in (0, 1, 2)]
    H.assert_hist_equal(got[0], hist, shape)
    assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes()


def test_two_calls_return_identical_arrays(eng):
    rng = np.random.default_rng(2027)
    build = S.U.random_rows(rng, 50_000, 24, 20_000, max_len=300)
    probe = S.U.random_rows(rng, 50_000, 24, 20_000, max_len=3000)
    a = eng.depth_hist(probe, build, True, 24, 40)
    b = eng.depth_hist(probe, build, True, 24, 40)
    assert a.tobytes() == b.tobytes()
    H.assert_hist_equal(a, H.block_form(probe, build, True, 24, 40))
    ca = eng.depth_hist_contigs(build, True, 24, 40)
    cb = eng.depth_hist_contigs(build, True, 24, 40)
    assert ca.tobytes() == cb.tobytes()
    H.assert_hist_equal(ca, H.contig_form(build, True, 24, 40))


def test_the_whole_range_probe(eng):
    probe, build, nc, md, hist = H.expected("whole_range", False)
    got = eng.depth_hist(probe, build, False, nc, md)
    assert got[0].sum() == 2 ** 32 == hist[0].sum() and (got[0] == hist[0]).all()


@pytest.mark.parametrize("seed", range(20))
def test_random_sweep(eng, seed):
    probe, build, nc, strict, md = H.sweep_case(seed)
    H.assert_hist_equal(eng.depth_hist(probe, build, strict, nc, md), H.block_form(probe, build, strict, nc, md),
                        f"seed {seed}: probes={len(probe[0])} build={len(build[0])} contigs={nc} strict={strict} max_depth={md}")
    H.assert_hist_equal(eng.depth_hist_contigs(build, strict, nc, md), H.contig_form(build, strict, nc, md), f"seed {seed}: contig form")


def test_bad_arguments_are_refused(eng, dj):
    import torch
    probe, build, nc, _md, _hist = H.expected("small_edges", True)
    for bad in (0, -1, H.MAX_HIST_DEPTH + 1):
        for side in (probe, S.EMPTY):                            # the checks do not depend on the number of probe rows
            with pytest.raises(_engine.EngineError, match=r"max_depth must be in 1 \.\. 1023"):
                eng.depth_hist(side, build, True, nc, bad)
            with pytest.raises(_engine.EngineError, match=r"max_depth must be in 1 \.\. 1023"):
                eng.depth_hist_contigs(side, True, nc, bad)
    # a NULL hist on the host entries
    opts = _engine.make_opts(True, nc)
    for cols in (probe, S.EMPTY):
        ps, keep_p = _engine._host_side(*cols)
        bs, keep_b = _engine._host_side(*build)
        with pytest.raises(_engine.EngineError, match="hist is NULL"):
            _engine._check(eng.L, eng.L.ivj_depth_hist(eng.h, C.byref(ps), C.byref(bs), C.byref(opts), 5, None), "ivj_depth_hist")
        with pytest.raises(_engine.EngineError, match="hist is NULL"):
            _engine._check(eng.L, eng.L.ivj_depth_hist_contigs(eng.h, C.byref(ps), C.byref(opts), 5, None), "ivj_depth_hist_contigs")
        del keep_p, keep_b
    p, b, none = _side(probe), _side(build), _side(S.EMPTY)
    ix = dj.engine.index_build_dev(b.as_c(), opts, False)
    try:
        buf = torch.zeros((p.n, 6), dtype=torch.int64, device="cuda")
        for side in (p, none):
            for bad in (0, -1, H.MAX_HIST_DEPTH + 1):
                with pytest.raises(_engine.EngineError, match=r"max_depth must be in 1 \.\. 1023"):
                    dj.engine.depth_hist_dev(ix, side.as_c(), opts, bad, buf.data_ptr())
                with pytest.raises(_engine.EngineError, match=r"max_depth must be in 1 \.\. 1023"):
                    dj.engine.depth_hist_contigs_dev(ix, opts, bad, buf.data_ptr())
            with pytest.raises(_engine.EngineError, match="hist is NULL"):
                dj.engine.depth_hist_dev(ix, side.as_c(), opts, 5, 0)
        with pytest.raises(_engine.EngineError, match="hist is NULL"):
            dj.engine.depth_hist_contigs_dev(ix, opts, 5, 0)
    finally:
        ix.close()
