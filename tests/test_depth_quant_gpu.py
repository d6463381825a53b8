"""depth_quantiles on the GPU, compared exactly with the block form of tests/_depth_quant_util.py -- which
tests/test_depth_quant_cpu.py holds against the per-base form -- through the host entry (Engine.depth_quantiles) and the device
entry (ivj_depth_quantiles_dev via device_api: caller's buffer prefilled, a prebuilt index without the end order, called twice).
The shapes of depth_summary sit on the paths the kernel shares with depth_hist (the block range, both metadata forms, the joint
grid's bins, depths beyond 16 bits, the int32 limits) with K cycling over 1, 3 and 16; the new ones sit on the kernel's own edges:
the workgroup's tile of P probes at the largest and the smallest P, the pass count (piles of 2^B - 1, 2^B, 2^2B - 1, 2^2B and
70 000 rows, a shallow tile in the same call), ranks on a cumulative boundary, the uncovered mass, diverging and shared prefixes,
a range over three chunks, every lane on one address, dead probes and dead ranks, no probes, no blocks."""
import ctypes as C

import numpy as np
import pytest

from polars_bio_amd import _engine
import _depth_sum_util as S
import _depth_summary_util as D
import _depth_hist_util as H
import _depth_quant_util as Q

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
@pytest.mark.parametrize("shape", list(Q.SHAPES))
def test_host_entry(eng, shape, strict):
    probe, build, nc, ranks, val = Q.expected(shape, strict)
    Q.assert_quant_equal(eng.depth_quantiles(probe, build, strict, nc, ranks), val, f"{shape}, K {ranks.shape[1]}")


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", list(Q.SHAPES))
def test_device_entry_equals_the_host_entry(eng, dj, shape, strict):
    import torch
    probe, build, nc, ranks, val = Q.expected(shape, strict)
    p, b, r = _side(probe), _side(build), torch.from_numpy(np.array(ranks)).cuda()
    got = dj.depth_quantiles(p, b, strict, nc, r)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == val.shape
    Q.assert_quant_equal(got.cpu().numpy(), val, shape)
    assert got.cpu().numpy().tobytes() == eng.depth_quantiles(probe, build, strict, nc, ranks).tobytes()
    # the caller's buffer, prefilled, and an index built without the end order (completed on demand), twice
    out = torch.full(val.shape, -7, dtype=torch.int32, device="cuda")
    opts = _engine.make_opts(strict, nc)
    ix = dj.engine.index_build_dev(b.as_c(), opts, False)
    try:
        for call in ("first", "second"):
            assert dj.depth_quantiles(p, b, strict, nc, r, index=ix, out=out) is out
            Q.assert_quant_equal(out.cpu().numpy(), val, f"{shape}: caller buffer, {call} call on the index")
            out.fill_(-7)
    finally:
        ix.close()


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", ["small_edges", "blocks_5000", "contigs_24", "contigs_cm_lds_plus", "degenerate_build", "deep_70k", "whole_range",
                                   "int32_limits", "pile_256"])
def test_the_last_rank_is_depth_summary_s_max_depth(eng, shape, strict):
    probe, build, nc, _ranks, _val = Q.expected(shape, strict)
    L = Q.positions(probe, strict, nc)
    got = eng.depth_quantiles(probe, build, strict, nc, (L - 1)[:, None])
    md, _ = eng.depth_summary(probe, build, strict, nc, thresholds=())
    assert (got[:, 0] == np.where(L > 0, md, -1)).all()


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", ["small_edges", "blocks_5000", "contigs_24", "depth_tile", "degenerate_build", "uncovered_mass", "pile_255",
                                   "long_range_three_chunks"])
def test_equals_the_search_of_depth_hist_s_cumulative_row(eng, shape, strict):
    probe, build, nc, ranks, _val = Q.expected(shape, strict)
    hist = eng.depth_hist(probe, build, strict, nc, H.MAX_HIST_DEPTH)
    assert (hist[:, H.MAX_HIST_DEPTH] == 0).all()              # no depth reaches the clamp
    cum = np.cumsum(hist, axis=1)
    valid = (ranks >= 0) & (ranks < Q.positions(probe, strict, nc)[:, None])
    first = np.stack([(cum <= np.where(valid[:, j], ranks[:, j], 0)[:, None]).sum(axis=1) for j in range(ranks.shape[1])], axis=1)
    got = eng.depth_quantiles(probe, build, strict, nc, ranks)
    assert (got[valid] == first[valid]).all() and (got[~valid] == -1).all()


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", ["contigs_24", "contigs_cm_lds_plus", "degenerate_build", "blocks_5000", "deep_70k", "whole_range",
                                   "pile_70000_and_a_far_tile"])
def test_partition_modes_return_identical_arrays(eng, shape, strict):
    probe, build, nc, ranks, val = Q.expected(shape, strict)
    got = [eng.depth_quantiles(probe, build, strict, nc, ranks, partition_mode=m) for m in (0, 1, 2)]
    Q.assert_quant_equal(got[0], val, shape)
    assert got[0].tobytes() == got[1].tobytes() == got[2].tobytes()


def test_two_calls_return_identical_arrays(eng):
    rng = np.random.default_rng(2028)
    build = S.U.random_rows(rng, 50_000, 24, 20_000, max_len=300)
    probe = S.U.random_rows(rng, 50_000, 24, 20_000, max_len=3000)
    ranks = Q.ranks_for(probe, True, 24, 5, 1)
    a = eng.depth_quantiles(probe, build, True, 24, ranks)
    b = eng.depth_quantiles(probe, build, True, 24, ranks)
    assert a.tobytes() == b.tobytes()
    Q.assert_quant_equal(a, Q.block_form(probe, build, True, 24, ranks))


def test_no_rows_and_an_empty_build(eng, dj):
    import torch
    probe, build, nc, ranks, val = Q.expected("no_probes", True)
    assert eng.depth_quantiles(probe, build, True, nc, ranks).shape == (0, 3)
    got = dj.depth_quantiles(_side(probe), _side(build), True, nc, torch.zeros((0, 3), dtype=torch.int64, device="cuda"))
    assert tuple(got.shape) == (0, 3)
    probe, build, nc, ranks, val = Q.expected("empty_build", True)
    got = eng.depth_quantiles(probe, build, True, nc, ranks)
    live = Q.positions(probe, True, nc) > 0
    assert (got[live] == 0).all() and (got[~live] == -1).all()


@pytest.mark.parametrize("seed", range(12))
def test_random_sweep(eng, seed):
    probe, build, nc, strict, ranks = Q.sweep_case(seed)
    Q.assert_quant_equal(eng.depth_quantiles(probe, build, strict, nc, ranks), Q.block_form(probe, build, strict, nc, ranks),
                         f"seed {seed}: probes={len(probe[0])} build={len(build[0])} contigs={nc} strict={strict} K={ranks.shape[1]}")


def test_bad_arguments_are_refused(eng, dj):
    import torch
    probe, build, nc, _ranks, _val = Q.expected("small_edges", True)
    n = len(probe[0])
    with pytest.raises(_engine.EngineError, match=r"n_ranks must be in 1 \.\. 16"):
        eng.depth_quantiles(probe, build, True, nc, np.zeros((n, 17), np.int64))
    with pytest.raises(_engine.EngineError, match=r"n_ranks must be in 1 \.\. 16"):
        eng.depth_quantiles(probe, build, True, nc, np.zeros((n, 0), np.int64))
    with pytest.raises(ValueError, match="one row per probe row"):
        eng.depth_quantiles(probe, build, True, nc, np.zeros((n + 1, 2), np.int64))
    opts = _engine.make_opts(True, nc)
    some = np.zeros((n, 2), np.int64)
    res = np.zeros((n, 2), np.int32)
    for cols in (probe, S.EMPTY):                                # the checks do not depend on the number of probe rows
        ps, keep_p = _engine._host_side(*cols)
        bs, keep_b = _engine._host_side(*build)
        with pytest.raises(_engine.EngineError, match="ranks is NULL"):
            _engine._check(eng.L, eng.L.ivj_depth_quantiles(eng.h, C.byref(ps), C.byref(bs), C.byref(opts), 2, None, res.ctypes.data), "q")
        with pytest.raises(_engine.EngineError, match="out is NULL"):
            _engine._check(eng.L, eng.L.ivj_depth_quantiles(eng.h, C.byref(ps), C.byref(bs), C.byref(opts), 2, some.ctypes.data, None), "q")
        del keep_p, keep_b
    p, b = _side(probe), _side(build)
    ix = dj.engine.index_build_dev(b.as_c(), opts, False)
    try:
        r = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
        o = torch.zeros((n, 2), dtype=torch.int32, device="cuda")
        for bad in (0, -1, 17):
            with pytest.raises(_engine.EngineError, match=r"n_ranks must be in 1 \.\. 16"):
                dj.engine.depth_quantiles_dev(ix, p.as_c(), opts, bad, r.data_ptr(), o.data_ptr())
        with pytest.raises(_engine.EngineError, match="ranks is NULL"):
            dj.engine.depth_quantiles_dev(ix, p.as_c(), opts, 2, 0, o.data_ptr())
        with pytest.raises(_engine.EngineError, match="out is NULL"):
            dj.engine.depth_quantiles_dev(ix, p.as_c(), opts, 2, r.data_ptr(), 0)
        with pytest.raises(ValueError, match="ranks must be a contiguous int64 tensor"):
            dj.depth_quantiles(p, b, True, nc, r.to(torch.int32))
        with pytest.raises(ValueError, match="out must be a contiguous int32 tensor"):
            dj.depth_quantiles(p, b, True, nc, r, out=torch.zeros((n, 3), dtype=torch.int32, device="cuda"))
    finally:
        ix.close()
