"""The expected values of depth_quantiles (tests/_depth_quant_util.py) held against each other without a GPU: the block form against
the per-base form on every small-span shape, our quantile formula on the per-base windows against np.quantile, quantile_ranks
against exact rational arithmetic, the identity with the cumulative bins of depth_hist's block form, and the tile formula."""
from fractions import Fraction
import math

import numpy as np
import pytest

from polars_bio_amd import _engine, range_op
import _depth_hist_util as H
import _depth_quant_util as Q

MODES = [pytest.param(True, id="strict"), pytest.param(False, id="weak")]
DENSE_ROWS = 300                                 # rows of a shape the per-base form sorts


def _sample(n, seed):
    return np.arange(n) if n <= DENSE_ROWS else np.sort(np.random.default_rng(seed).choice(n, DENSE_ROWS, replace=False))


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", Q.SMALL_SPAN)
def test_block_form_equals_dense_form(shape, strict):
    probe, build, nc, ranks, val = Q.expected(shape, strict)
    idx = _sample(len(probe[0]), 1)
    dense = Q.dense_form(probe, build, strict, nc, ranks, idx)
    bad = np.argwhere(dense != val[idx])
    assert bad.size == 0, f"{shape}: first (sampled row, rank) {tuple(bad[0])}: dense {dense[tuple(bad[0])]} != block {val[idx][tuple(bad[0])]}"


@pytest.mark.parametrize("method", range_op.QUANTILE_METHODS)
@pytest.mark.parametrize("shape", ["small_edges", "blocks_5000", "contigs_24", "degenerate_probe", "uncovered_mass", "pile_16"])
def test_our_formula_equals_numpy_quantile_on_the_windows(shape, method):
    probe, build, nc, _ranks, _val = Q.expected(shape, True)
    qs = np.array([0.0, 0.1, 0.25, 1 / 3, 0.5, 0.75, 0.999, 1.0])
    seen = 0
    for _i, v in Q.windows(probe, build, True, nc, _sample(len(probe[0]), 2)[:120]):
        if v is None:
            continue
        lo, hi, g = range_op.quantile_ranks(np.full(len(qs), v.size), qs)
        ours = Q.quantiles(v[lo], v[hi], g, method)
        ref = np.quantile(v, qs, method=method)
        if method in ("lower", "higher"):
            assert ours.dtype == np.int64 and (ours == ref).all()
        else:                                                  # the same formula up to the order of the roundings
            assert ours.dtype == np.float64 and np.allclose(ours, ref, rtol=1e-12, atol=0.0)
        seen += 1
    assert seen > 20


def test_quantile_ranks_against_exact_rationals():
    for L in (1, 2, 3, 2 ** 31, 2 ** 32 - 1):
        for q in (0.0, 0.25, 0.5, 1.0, 1 / 3):
            # q (L - 1) in IEEE float64 = the exact product of the two float64 operands, rounded once
            h = float(Fraction(q) * (L - 1))
            lo, hi, g = range_op.quantile_ranks(np.array([L], np.int64), q)
            assert lo.dtype == np.int64 and hi.dtype == np.int64 and g.dtype == np.float64
            assert (int(lo[0]), int(hi[0])) == (math.floor(Fraction(h)), math.ceil(Fraction(h))), (L, q)
            assert Fraction(float(g[0])) == Fraction(h) - math.floor(Fraction(h)), (L, q)      # exact: h and floor(h) share a binade or g is h itself
            assert 0 <= lo[0] <= hi[0] <= L - 1 and hi[0] - lo[0] <= 1 and 0.0 <= g[0] < 1.0
    # vectorised, broadcast, and rows without a position
    lo, hi, g = range_op.quantile_ranks(np.array([[5], [0], [-3], [4]]), np.array([[0.0, 0.5, 1.0]]))
    assert lo.tolist() == [[0, 2, 4], [-1, -1, -1], [-1, -1, -1], [0, 1, 3]]
    assert hi.tolist() == [[0, 2, 4], [-1, -1, -1], [-1, -1, -1], [0, 2, 3]]
    assert g.tolist() == [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.5, 0.0]]
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="must lie in"):
            range_op.quantile_ranks(np.array([3]), bad)


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", ["small_edges", "blocks_5000", "contigs_24", "depth_tile", "degenerate_build", "uncovered_mass", "pile_255"])
def test_identity_with_the_cumulative_bins_of_the_histogram(shape, strict):
    """where no depth reaches the clamp, the value at rank k is the first bin whose cumulative count exceeds k"""
    probe, build, nc, ranks, val = Q.expected(shape, strict)
    top = max(int(val.max()), 1) + 1
    md = Q.block_form(probe, build, strict, nc, np.maximum(Q.positions(probe, strict, nc) - 1, 0)[:, None]).max()
    assert md < top or md <= 0
    top = max(top, int(md) + 1)
    cum = np.cumsum(H.block_form(probe, build, strict, nc, top), axis=1)
    assert (cum[:, top] == cum[:, top - 1]).all()              # the clamped bin is empty
    valid = (ranks >= 0) & (ranks < Q.positions(probe, strict, nc)[:, None])
    first = (cum[:, None, :] <= np.where(valid, ranks, 0)[:, :, None]).sum(axis=2)
    assert (first[valid] == val[valid]).all() and (val[~valid] == -1).all()


def test_the_tile_formula_and_the_constants():
    assert Q.MAX_QUANT_RANKS == 16 and Q.QUANT_LDS_BYTES == 65536 and Q.QUANT_MAX_TILE == 512 and 4 <= Q.QUANT_BITS <= 8
    for k in range(1, 17):
        assert Q.tile(k) == _engine.depth_quant_tile(k), k
        assert Q.tile(k) * k * (1 << Q.QUANT_BITS) * 8 <= Q.QUANT_LDS_BYTES
    if Q.QUANT_BITS == 4:
        assert Q.tile(1) == 512 and Q.tile(3) == 170 and Q.tile(16) == 32


def test_the_edge_shapes_sit_on_the_kernel_s_edges():
    probe, build, _nc, ranks, val = Q.expected("rank_on_a_boundary", True)
    assert ranks.shape[1] == 16 and set(range(0, 400, 8)) <= set(ranks.ravel().tolist())
    flat = dict(zip(ranks.ravel().tolist(), val.ravel().tolist()))
    assert [flat[k] for k in (79, 80, 143, 144, 399)] == [0, 1, 1, 2, 5]
    probe, build, _nc, ranks, val = Q.expected("uncovered_mass", True)
    assert (val[:-1, 0] == 0).all() and (val[:-1, 1] >= 1).all() and (val[:-1, 1] == val[:-1, 2]).all() and val[-1].tolist() == [0, -1, 0]
    probe, build, _nc, ranks, val = Q.expected("pile_70000_and_a_far_tile", True)
    assert val[0].tolist() == [0, 70_000, 70_000] and val[2].tolist() == [0, 70_000, -1] and len(probe[0]) > 2 * Q.tile(3)
    assert val[Q.tile(3):].max() < 16                          # the later tiles never see the pile
    probe, build, _nc, ranks, val = Q.expected("diverging_and_shared_prefixes", True)
    assert val[0, 0] == 0 and val[0, 15] == 5000 and len(set(val[0].tolist())) == 16 and len(set(val[1].tolist())) == 1 and (val[2] == 5000).all()
    probe, build, nc, ranks, val = Q.expected("dead_probes_and_ranks", True)
    live = Q.positions(probe, True, nc) > 0
    even = np.arange(len(live)) % 2 == 0                       # the odd rows' middle rank lies far beyond the row
    assert (val[:, 0] == -1).all() and (val[:, 2] == -1).all() and (val[~live] == -1).all()
    assert (val[live & even, 1] >= 0).all() and (val[live & ~even, 1] == -1).all()
    probe, build, nc, ranks, val = Q.expected("empty_build", True)
    live = Q.positions(probe, True, nc) > 0
    assert (val[live] == 0).all() and (val[~live] == -1).all() and (~live).any()
