"""The two numpy forms of the set operations (tests/_setop_util.py) against each other and against the set identities, on every
shape the GPU tests use.  No device."""
import numpy as np
import pytest

import _setop_util as U

MODES = [pytest.param(True, id="strict"), pytest.param(False, id="weak")]


def _positions(regions, strict):
    c, s, e = regions
    return int((e - s + (0 if strict else 1)).sum())


def _no_touching(regions, strict):
    c, s, e = regions
    e1 = e if strict else e + 1
    assert (s < e1).all()
    same = c[1:] == c[:-1]
    assert (np.diff(c) >= 0).all()
    assert (s[1:][same] > e1[:-1][same]).all()       # a gap of at least one position: neither adjacent nor overlapping


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("op", U.OPS)
@pytest.mark.parametrize("shape", U.SMALL_SPAN)
def test_dense_and_event_forms_agree(shape, op, strict):
    a, b, nc = U.SHAPES[shape](strict)
    dense, dt = U.setop_dense(a, b, strict, nc, op)
    events, et = U.setop_events(a, b, strict, nc, op)
    U.assert_regions_equal(events, dense, f"{shape} {op}")
    assert dt == et


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", list(U.SHAPES))
def test_identities(shape, strict):
    a, b, nc = U.SHAPES[shape](strict)
    res = {op: U.setop_events(a, b, strict, nc, op) for op in U.OPS}
    for op in U.OPS:
        _no_touching(res[op][0], strict)
    only_a, only_b, both = res["union"][1]
    n = {op: _positions(res[op][0], strict) for op in U.OPS}
    size_a = _positions(U.setop_events(a, U.EMPTY, strict, nc, "union")[0], strict)
    size_b = _positions(U.setop_events(U.EMPTY, b, strict, nc, "union")[0], strict)
    assert (size_a, size_b) == (only_a + both, only_b + both)
    assert n["intersection"] == both and n["difference"] == only_a and n["symmetric_difference"] == only_a + only_b
    assert n["union"] == size_a + size_b - n["intersection"]
    # difference and intersection are disjoint and make up U(A)
    d, i = res["difference"][0], res["intersection"][0]
    dr, ir = U.as_i32(*d), U.as_i32(*i)
    assert len(U.setop_events(dr, ir, strict, nc, "intersection")[0][0]) == 0
    U.assert_regions_equal(U.setop_events(dr, ir, strict, nc, "union")[0], U.setop_events(a, U.EMPTY, strict, nc, "union")[0], shape)
    # symmetric difference = difference(A, B) | difference(B, A)
    back = U.as_i32(*U.setop_events(b, a, strict, nc, "difference")[0])
    U.assert_regions_equal(U.setop_events(dr, back, strict, nc, "union")[0], res["symmetric_difference"][0], shape)


@pytest.mark.parametrize("strict", MODES)
def test_examples_of_the_definition(strict):
    one = lambda s, e: U.as_i32([0], [s], [e])
    if strict:
        for op in ("union", "symmetric_difference"):
            U.assert_regions_equal(U.setop_events(one(0, 5), one(5, 9), True, 1, op)[0], ([0], [0], [9]), op)
    else:
        U.assert_regions_equal(U.setop_events(one(1, 5), one(6, 9), False, 1, "union")[0], ([0], [1], [9]))
        U.assert_regions_equal(U.setop_events(one(1, 9), one(4, 6), False, 1, "difference")[0], ([0, 0], [1, 7], [3, 9]))


def test_shapes_have_the_event_counts_their_names_promise():
    T = U.T
    for name, n in (("events_2", 2), (f"events_{T - 2}", T - 2), (f"events_{T}", T), (f"events_{T + 2}", T + 2),
                    (f"events_{2 * T + 2}", 2 * T + 2), ("events_unequal", 3 * T // 2 + 2), ("empty_both", 0)):
        for strict in (True, False):
            a, b, nc = U.SHAPES[name](strict)
            assert U.n_events(a, b, strict, nc) == n, name
    for strict in (True, False):
        a, b, nc = U.SHAPES["tie_on_tile_edge"](strict)
        ra, rb = U.union_runs(a, strict, nc), U.union_runs(b, strict, nc)
        lead = T // 2 - 1
        assert ra[2][lead] == rb[1][0] and (ra[1] < rb[1][0]).sum() == lead + 1      # events 0 .. T - 1 are A's, event T is B's first
        a, b, nc = U.SHAPES["contig_on_tile_edge"](strict)
        assert 2 * (U.union_runs(a, strict, nc)[0] == 0).sum() + 2 * (U.union_runs(b, strict, nc)[0] == 0).sum() == T


def test_sweep_cases_are_within_bounds():
    for seed in range(30):
        a, b, nc, strict, op = U.sweep_case(seed)
        assert 1 <= len(a[0]) <= 30_000 and 1 <= len(b[0]) <= 30_000 and 1 <= nc <= 8 and op in U.OPS
