"""depth on the CPU: the two numpy forms of tests/_depth_util.py agree with each other on every small shape of the GPU test,
with the pinned oracle on three invariants, and with hand-written cases (the GPU runs: tests/test_depth_gpu.py)."""
import numpy as np
import pytest

from oracle import oracle as O
import _depth_util as U

MODES = [pytest.param(True, id="strict"), pytest.param(False, id="weak")]


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", U.SMALL_SPAN)
def test_dense_and_event_forms_agree(shape, strict):
    c, s, e, nc = U.SHAPES[shape](strict)
    U.assert_blocks_equal(U.depth_dense(c, s, e, strict, nc), U.depth_events(c, s, e, strict, nc), shape)


@pytest.mark.parametrize("seed", range(4))
def test_dense_and_event_forms_agree_on_the_sweep(seed):
    c, s, e, nc, strict = U.sweep_case(seed)
    U.assert_blocks_equal(U.depth_dense(c, s, e, strict, nc), U.depth_events(c, s, e, strict, nc), f"seed {seed}")


def _blocks_are_maximal(bc, bs, be, bd, strict):
    """neighbouring blocks of one contig that touch differ in depth; blocks are sorted and disjoint"""
    e1 = be if strict else be + 1
    assert (bd >= 1).all() and (e1 > bs).all()
    same = bc[1:] == bc[:-1]
    assert (np.diff(bc) >= 0).all() and (bs[1:][same] >= e1[:-1][same]).all()
    touch = same & (bs[1:] == e1[:-1])
    assert (bd[1:][touch] != bd[:-1][touch]).all()


# the shapes the O(probes x rows) oracle walks in well under a second
ORACLE_SHAPES = [k for k in U.SHAPES if k not in ("bookended_chain", "identical", "nested_thousands")]


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", ORACLE_SHAPES)
def test_event_form_agrees_with_the_oracle(shape, strict):
    c, s, e, nc = U.SHAPES[shape](strict)
    bc, bs, be, bd = U.depth_events(c, s, e, strict, nc)
    _blocks_are_maximal(bc, bs, be, bd, strict)
    inside = (c >= 0) & (c < nc)
    frame = O.Side(c[inside], s[inside], e[inside])
    e1 = be if strict else be + 1                     # half-open block end
    # 1. depth at the first and last position of sampled blocks and one position on either side = count_overlaps of a unit probe
    pick = np.unique(np.linspace(0, max(len(bc) - 1, 0), 120).astype(np.int64)) if len(bc) else np.empty(0, np.int64)
    qc = np.repeat(bc[pick], 4)
    qp = np.stack([bs[pick] - 1, bs[pick], e1[pick] - 1, e1[pick]], axis=1).ravel()
    ok = (qp >= U.I32_MIN) & (qp + (1 if strict else 0) <= U.I32_MAX)
    qc, qp = qc[ok], qp[ok]
    probes = O.Side(qc, qp, qp + (1 if strict else 0))
    got = O.count_overlaps_brute(probes, frame, strict)
    exp = np.zeros(len(qp), np.int64)
    for k in range(len(qp)):                          # depth of position qp[k] according to the blocks
        hit = (bc == qc[k]) & (bs <= qp[k]) & (qp[k] < e1)
        assert hit.sum() <= 1
        exp[k] = bd[hit][0] if hit.any() else 0
    assert (got == exp).all()
    # 2. sum of length x depth = sum of the lengths of the rows that cover something
    cc, cs, ce1 = U._covering(c, s, e, strict, nc)
    assert int(((e1 - bs) * bd).sum()) == int((ce1 - cs).sum())
    # 3. block lengths per contig = coverage of one contig-wide probe
    if shape != "int32_limits":                       # (a contig-wide closed probe has no int32 end there)
        lo, hi = int(cs.min()) if cs.size else 0, int(ce1.max()) if ce1.size else 1
        wide = O.Side(np.arange(nc), np.full(nc, lo), np.full(nc, hi if strict else hi - 1))
        cov = O.np_coverage_brute(wide, frame, strict)
        mine = np.zeros(nc, np.int64)
        np.add.at(mine, bc, e1 - bs)
        assert (cov == mine).all()


def _both(c, s, e, strict, nc=1):
    a = U.depth_dense(c, s, e, strict, nc)
    U.assert_blocks_equal(a, U.depth_events(c, s, e, strict, nc))
    return [tuple(int(x) for x in row) for row in zip(*a)]


def test_hand_written_cases():
    z = lambda n: [0] * n
    # a bookended chain is one block
    assert _both(z(3), [0, 10, 20], [10, 20, 30], True) == [(0, 0, 30, 1)]
    assert _both(z(3), [0, 10, 20], [9, 19, 29], False) == [(0, 0, 29, 1)]
    # identical rows: one block of depth n
    assert _both(z(4), [5] * 4, [9] * 4, True) == [(0, 5, 9, 4)]
    assert _both(z(4), [5] * 4, [9] * 4, False) == [(0, 5, 9, 4)]
    # staircase
    assert _both(z(3), [0, 2, 4], [6, 8, 10], True) == [(0, 0, 2, 1), (0, 2, 4, 2), (0, 4, 6, 3), (0, 6, 8, 2), (0, 8, 10, 1)]
    assert _both(z(3), [0, 2, 4], [6, 8, 10], False) == [(0, 0, 1, 1), (0, 2, 3, 2), (0, 4, 6, 3), (0, 7, 8, 2), (0, 9, 10, 1)]
    # nested
    assert _both(z(2), [0, 3], [10, 5], True) == [(0, 0, 3, 1), (0, 3, 5, 2), (0, 5, 10, 1)]
    # a zero-length row and an inverted row contribute nothing
    assert _both(z(3), [0, 4, 8], [10, 4, 2], True) == [(0, 0, 10, 1)]
    assert _both(z(3), [0, 4, 8], [10, 3, 2], False) == [(0, 0, 10, 1)]
    # Weak adjacency: closed [1,5] and [6,9] are one block
    assert _both(z(2), [1, 6], [5, 9], False) == [(0, 1, 9, 1)]
    assert _both(z(2), [1, 6], [5, 9], True) == [(0, 1, 5, 1), (0, 6, 9, 1)]
    # a gap and a contig boundary keep equal depths apart; ids outside the dictionary are dropped
    assert _both([0, 0, 1, 2, -1], [0, 7, 0, 0, 0], [5, 9, 5, 5, 5], True, nc=2) == [(0, 0, 5, 1), (0, 7, 9, 1), (1, 0, 5, 1)]
    # the int32 limits (event form only)
    lim = U.depth_events([0, 0], [U.I32_MIN, U.I32_MAX], [U.I32_MAX, U.I32_MAX], False, 1)
    assert [tuple(int(x) for x in r) for r in zip(*lim)] == [(0, U.I32_MIN, U.I32_MAX - 1, 1), (0, U.I32_MAX, U.I32_MAX, 2)]
