"""The two numpy forms of depth_summary (tests/_depth_summary_util.py) against each other on every shape the GPU tests use, and the
identities that tie max_depth / bases_ge to coverage, overlap_bases and count_overlaps.  No GPU: these pin the reference the GPU
tests compare with."""
import numpy as np
import pytest

from oracle import oracle as O
import _depth_sum_util as S
import _depth_summary_util as D

MODES = [pytest.param(True, id="strict"), pytest.param(False, id="weak")]


def _dense_sample(probe, build):
    return S.sample(len(probe[0]), 2000, cells=6_000_000)          # dense_form costs a slice per probe, whatever the build side


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", D.SMALL_SPAN)
def test_two_forms_agree(shape, strict):
    probe, build, nc, thr, md, bg = D.expected(shape, strict)
    assert md.dtype == np.int64 and bg.dtype == np.int64 and bg.shape == (len(thr), len(probe[0]))
    assert (md >= 0).all() and (bg >= 0).all()
    idx = _dense_sample(probe, build)
    dm, db = D.dense_form(probe, build, strict, nc, thr, idx)
    D.assert_summary_equal((None, db), (md[idx], bg[:, idx]), f"{shape}: dense form")
    assert (dm == md[idx]).all(), f"{shape}: dense form, max_depth"


def test_a_hand_worked_case():
    # build [10,20) [15,30) [40,50), [100,200) x 3, [120,150): blocks [10,15) 1, [15,20) 2, [20,30) 1, [40,50) 1, [100,120) 3, [120,150) 4, [150,200) 3
    probe, build, nc, thr, md, bg = D.expected("small_edges", True)
    assert thr == (1, 2, 3, 4)
    rows = {tuple(r): i for i, r in enumerate(zip(probe[1].tolist(), probe[2].tolist()))}
    def at(s, e):
        i = rows[(s, e)]
        return [int(md[i])] + bg[:, i].tolist()
    assert at(30, 40) == [0, 0, 0, 0, 0]                 # inside the gap
    assert at(16, 19) == [2, 3, 3, 0, 0]                 # strictly inside one block
    assert at(10, 30) == [2, 20, 5, 0, 0]                # edges on block boundaries
    assert at(5, 10) == [0, 0, 0, 0, 0]                  # touches [10,20) only
    assert at(0, 300) == [4, 130, 105, 100, 30]
    assert at(119, 151) == [4, 32, 32, 32, 30]
    assert at(25, 25) == [0, 0, 0, 0, 0] and at(60, 50) == [0, 0, 0, 0, 0]
    # closed rows: the touching rows share one position
    probe, build, nc, thr, md, bg = D.expected("small_edges", False)
    i = rows[(5, 10)]
    assert int(md[i]) == 1 and bg[:, i].tolist() == [1, 0, 0, 0]
    i = rows[(30, 40)]                                    # [30,30] of [15,30] and [40,40] of [40,50]
    assert int(md[i]) == 1 and bg[:, i].tolist() == [2, 0, 0, 0]


def test_the_whole_range_probe_has_2_to_the_32_positions():
    probe, build, nc, thr, md, bg = D.expected("whole_range", False)
    assert (int(probe[1][0]), int(probe[2][0])) == (D.I32_MIN, D.I32_MAX)
    assert bg[0, 0] == 2 ** 32 and md[0] >= 2
    probe, build, nc, thr, md, bg = D.expected("whole_range", True)
    assert bg[0, 0] == 2 ** 32 - 1


def test_the_deep_shape_is_deeper_than_16_bits():
    for strict in (True, False):
        _, _, _, thr, md, bg = D.expected("deep_70k", strict)
        assert md.max() == 70_000 > 2 ** 16
        assert (bg[thr.index(70_001)] == 0).all() and bg[thr.index(70_000)].max() > 0


def test_the_many_blocks_shape_has_three_tree_levels():
    for deepest in ("", "_deepest_first", "_deepest_last", "_deepest_alone"):
        probe, build, nc, thr, md, bg = D.expected("blocks_5000" + deepest, True)
        kc, ks, ke, kd = D.U.depth_events(*build, True, nc)
        assert len(kc) == D.N_BLOCKS > 16 ** 3
        if deepest:
            assert kd.max() == 50 and (kd == 50).sum() == 1 and md.max() == 50 and 0 < (md == 50).sum() < len(md)


def test_touching_rows_differ_between_the_modes():
    probe, build = D.as_i32([0], [5], [10]), D.as_i32([0], [10], [20])
    assert D.block_form(probe, build, True, 1, (1,))[1].tolist() == [[0]]
    assert D.block_form(probe, build, False, 1, (1,))[1].tolist() == [[1]]


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", D.CLEAN)
def test_identities(shape, strict):
    probe, build, nc, _thr, _md, _bg = D.expected(shape, strict)
    idx = S.sample(len(probe[0]), len(build[0]), cells=400_000)
    sub = tuple(a[idx] for a in probe)
    p, b = O.Side(*sub), O.Side(*build)
    cov = O.np_coverage_brute(p, b, strict)
    cnt = O.np_count_overlaps(p, b, strict)
    bases = S.prefix_form(sub, build, strict, nc)
    md, one = D.block_form(sub, build, strict, nc, (1,))
    assert (one[0] == cov).all()                                     # bases_ge[1] == coverage
    assert (md <= cnt).all()                                         # max_depth <= count_overlaps
    assert ((md == 0) == (cov == 0)).all()                           # max_depth == 0 exactly when coverage == 0
    top = int(md.max())
    # every threshold up to the deepest pile and one beyond it (a shape deeper than 256 takes a spread of them: the sum identity
    # needs them all and is then left to the shallower shapes)
    ts = list(range(1, top + 2)) if top <= 256 else sorted({1, 2, 3, top // 2, top - 1, top, top + 1})
    _, bg = D.block_form(sub, build, strict, nc, ts)
    if top <= 256:
        assert (bg.sum(axis=0) == bases).all()                       # sum over T of bases_ge[T] == overlap_bases
    assert (np.diff(bg, axis=0) <= 0).all()                          # non-increasing in T
    for k, t in enumerate(ts):
        assert ((bg[k] > 0) == (t <= md)).all()                      # positive exactly when T <= max_depth


@pytest.mark.parametrize("seed", range(6))
def test_sweep_cases_agree(seed):
    probe, build, nc, strict, thr = D.sweep_case(seed)
    md, bg = D.block_form(probe, build, strict, nc, thr)
    idx = _dense_sample(probe, build)
    dm, db = D.dense_form(probe, build, strict, nc, thr, idx)
    D.assert_summary_equal((None, db), (md[idx], bg[:, idx]), f"seed {seed}: dense form")
    assert (dm == md[idx]).all()
