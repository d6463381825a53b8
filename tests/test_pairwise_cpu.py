"""The two numpy forms of pb.pairwise_jaccard (tests/_pairwise_util.py) against each other on every small-universe shape, against
the two-frame reference of the set operations, and the shapes against what their names say."""
import numpy as np
import pytest

import _pairwise_util as P

U, S = P.U, P.S
MODES = [pytest.param(True, id="strict"), pytest.param(False, id="weak")]


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", P.SMALL_UNIVERSE)
def test_the_two_references_agree(shape, strict):
    frames, nc = P.case(shape, strict)
    exp = P.expected(shape, strict)
    assert all(x.dtype == np.int64 and x.shape == (len(frames), len(frames)) for x in exp)
    P.assert_equal(P.pairwise_brute(frames, strict, nc), exp, shape)
    assert (exp[0] == exp[0].T).all() and (exp[1] == exp[1].T).all()


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", P.TWO_FRAMES + ["int32_limits", "full_span_next_to_int32_min"])
def test_pairs_equal_the_two_frame_reference(shape, strict):
    """every pair (the shapes with more than two frames: pair by pair) against setop_events' totals and its intersection regions"""
    frames, nc = P.case(shape, strict)
    bases, runs = P.expected(shape, strict)
    for i in range(len(frames)):
        for j in range(len(frames)):
            regions, (only_a, _only_b, both) = S.setop_events(frames[i], frames[j], strict, nc, "intersection")
            assert (int(bases[i, j]), int(runs[i, j])) == (both, len(regions[0])), (i, j)
            assert int(bases[i, i]) == only_a + both


def test_shapes_hold_what_their_names_say():
    for strict in (True, False):
        for n in (P.STEP - 1, P.STEP, P.STEP + 1, 3 * P.STEP + 1, P.TILE - 1, P.TILE, P.TILE + 1, 3 * P.TILE + 1):
            frames, nc = P.case(f"segments_{n}", strict)
            assert len(frames) == 5 and len(U.multi_events(frames, strict, nc, 1, False)[0]) == n
        frames, nc = P.case("abutting_chain", strict)
        c, s, e, mask = U.multi_events(frames, strict, nc, 1, False)
        e1 = e if strict else e + 1
        abut = (c[1:] == c[:-1]) & (e1[:-1] == s[1:])
        assert len(c) > 3 * P.TILE and abut.sum() == len(c) - nc
        seams = np.arange(P.STEP, len(c), P.STEP)
        assert abut[seams - 1].sum() >= len(seams) - nc and abut[np.arange(P.TILE, len(c), P.TILE) - 1].all()
        assert (mask[1:] & mask[:-1])[abut].any(), "a frame stays in across an abutting boundary"
        frames, nc = P.case("equal_coordinates_on_two_contigs", strict)
        c, s, e, mask = U.multi_events(frames, strict, nc, 1, False)
        e1 = e if strict else e + 1
        seam = np.flatnonzero(c[1:] != c[:-1])
        assert len(seam) == 1 and e1[seam[0]] == s[seam[0] + 1] and mask[seam[0]] == mask[seam[0] + 1] == 3
        assert P.expected("equal_coordinates_on_two_contigs", strict)[1][0, 1] == 3      # one run on contig 0, two on contig 1
        frames, nc = P.case("full_masks_64", strict)
        assert len(frames) == U.MAX_FRAMES and (U.multi_events(frames, strict, nc, 1, False)[3] == np.uint64(2 ** 64 - 1)).all()
        assert len(U.multi_events(*P.case("two_segments", strict)[:1], strict, 1, 1, False)[0]) == 2
    frames, nc = P.case("full_span_next_to_int32_min", False)
    bases, runs = P.expected("full_span_next_to_int32_min", False)
    assert bases[0, 1] == 2 ** 32 + 11 + 2 ** 31 and bases[0, 0] == 2 * 2 ** 32 + 11
    c, s, e, _ = U.multi_events(frames, False, nc, 1, False)
    seam = np.flatnonzero(c[1:] != c[:-1])[0]
    assert np.int32(e[seam]) == P.I32_MAX and s[seam + 1] == P.I32_MIN, "in 32 bits the end + 1 wraps onto the next start"
    assert runs[0, 1] == 3
