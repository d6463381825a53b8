"""The expected values of depth_hist (tests/_depth_hist_util.py) held against each other without a GPU: the block form (differences
of _depth_summary_util.block_form's thresholds 1 .. D) against the per-base form on every small-span shape, the row sums, the
collapse to the values of pb.coverage / pb.mean_depth, the contig form against the summed region form, and the tile formula."""
import numpy as np
import pytest

from polars_bio_amd import _engine
import _depth_sum_util as S
import _depth_summary_util as D
import _depth_hist_util as H

MODES = [pytest.param(True, id="strict"), pytest.param(False, id="weak")]


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", H.SMALL_SPAN)
def test_block_form_equals_dense_form(shape, strict):
    probe, build, nc, md, hist = H.expected(shape, strict)
    H.assert_hist_equal(H.dense_form(probe, build, strict, nc, md), hist, shape)


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", list(H.SHAPES))
def test_rows_sum_to_their_positions(shape, strict):
    probe, _build, nc, _md, hist = H.expected(shape, strict)
    assert (hist >= 0).all()
    assert (hist.sum(axis=1) == H.positions(probe, strict, nc)).all()


def test_the_whole_range_probe_holds_two_to_the_32_positions():
    probe, _build, nc, _md, hist = H.expected("whole_range", False)
    assert hist[0].sum() == 2 ** 32 == H.positions(probe, False, nc)[0]


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", ["small_edges", "blocks_5000", "contigs_24", "depth_tile", "degenerate_build"])
def test_collapses_to_coverage_and_mean_depth(shape, strict):
    probe, build, nc, _thr = D.SHAPES[shape](strict)
    md, bg = D.block_form(probe, build, strict, nc, (1,))
    top = int(md.max()) + 1                                    # above every depth: the last bin is empty
    hist = H.block_form(probe, build, strict, nc, top)
    assert (hist[:, top] == 0).all()
    assert (hist[:, 1:].sum(axis=1) == bg[0]).all()            # pb.coverage
    assert ((hist * np.arange(top + 1)).sum(axis=1) == S.block_form(probe, build, strict, nc)).all()      # pb.mean_depth's bases
    # a smaller max_depth folds the deeper bins into its last one
    low = H.block_form(probe, build, strict, nc, 2)
    assert (low[:, :2] == hist[:, :2]).all() and (low[:, 2] == hist[:, 2:].sum(axis=1)).all()


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", list(H.CONTIG_SHAPES))
def test_contig_form_is_the_region_form_of_contig_wide_probes(shape, strict):
    frame, nc, md = H.CONTIG_SHAPES[shape](strict)
    hist = H.contig_form(frame, strict, nc, md)
    assert (hist[:, 0] == 0).all()
    # Strict rows end at INT32_MAX at the latest and never cover that position: [INT32_MIN, INT32_MAX) sees all they cover
    whole = H.as_i32(np.arange(nc), np.full(nc, H.U.I32_MIN), np.full(nc, H.U.I32_MAX))
    region = H.block_form(whole, frame, strict, nc, md)
    assert (region[:, 1:] == hist[:, 1:]).all()


def test_the_tile_formula():
    assert H.MAX_HIST_DEPTH == 1023 and H.HIST_LDS_BYTES in (65536, 131072) and H.HIST_MAX_TILE == 512
    for md in (1, 2, 7, 15, 16, 63, 64, 255, 682, 1023):
        assert H.tile(md) == _engine.depth_hist_tile(md), md
    assert H.tile(1) == 512 and H.tile(1023) == H.HIST_LDS_BYTES // 8192


def test_the_edge_shapes_sit_on_the_kernel_s_edges():
    probe, build, _nc, md, hist = H.expected("long_range_three_chunks", True)
    assert len(probe[0]) == 301 and hist[150, 1:].sum() == 8 * D.N_BLOCKS and 150 + D.N_BLOCKS > 2 * H.CHUNK
    probe, build, _nc, md, hist = H.expected("one_address", True)
    assert md == 1 and hist[0, 1] == 8 * 2 * H.CHUNK and hist[0, 0] == 2 * 2 * H.CHUNK
    probe, build, _nc, md, hist = H.expected("clamp_boundary", True)
    assert (hist[:, md - 1] > 0).any() and (hist[:, md] > 0).any()
    probe, build, nc, md, hist = H.expected("empty_build", True)
    assert (hist[:, 1:] == 0).all() and (hist[:, 0] == H.positions(probe, True, nc)).all() and (hist[:, 0] == 0).any()
    probe, build, nc, md, hist = H.expected("dead_probes", True)
    dead = H.positions(probe, True, nc) == 0
    assert dead.sum() > len(dead) // 2 and (hist[dead] == 0).all() and (hist[~dead].sum(axis=1) > 0).all()
    frame, nc, md = H.CONTIG_SHAPES["tile_straddles_two_contigs"](True)
    kc = H.U.depth_events(*frame, True, nc)[0]
    assert len(kc) == H.CHUNK + 5 and kc[2039] == 0 and kc[2040] == 1
    frame, nc, md = H.CONTIG_SHAPES["tiny_contigs_300"](True)
    kc = H.U.depth_events(*frame, True, nc)[0]
    assert (np.bincount(kc) == 3).all() and len(kc) == 900
