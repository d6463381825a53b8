"""The three numpy forms of overlap_bases (tests/_depth_sum_util.py) against each other on every shape the GPU tests use, and the
identities coverage <= bases <= count x length.  No GPU: these pin the references the GPU tests compare with."""
import numpy as np
import pytest

from oracle import oracle as O
import _depth_sum_util as S

MODES = [pytest.param(True, id="strict"), pytest.param(False, id="weak")]


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", list(S.SHAPES))
def test_three_forms_agree(shape, strict):
    probe, build, nc, exp = S.expected(shape, strict)
    assert exp.dtype == np.int64 and (exp >= 0).all()
    idx = S.sample(len(probe[0]), len(build[0]))
    S.assert_bases_equal(S.pair_form(probe, build, strict, nc, idx), exp[idx], f"{shape}: pair form")
    S.assert_bases_equal(S.block_form(probe, build, strict, nc, idx), exp[idx], f"{shape}: block form")


def test_a_hand_worked_case():
    # build [10,20) [15,30) [30,40): the window [0,50) holds all 35 positions x rows, [12,13) one, [29,31) two, [5,5) none
    probe, build, nc, _ = S.expected("three_rows", True)
    assert S.prefix_form(probe, build, True, nc).tolist() == [35, 15, 1, 2, 10, 0, 0]
    # closed rows [10,20] [15,30] [30,40]: one position more per row, and the bookended pair shares position 30
    assert S.prefix_form(probe, build, False, nc).tolist() == [38, 17, 2, 4, 12, 0, 1]


def test_the_deep_window_exceeds_32_bits():
    for strict in (True, False):
        _, _, _, exp = S.expected("deep_70k", strict)
        assert exp[0] == 70_000 * 99_000 > 2 ** 32


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", S.CLEAN)
def test_identities(shape, strict):
    probe, build, nc, exp = S.expected(shape, strict)
    idx = S.sample(len(probe[0]), len(build[0]), cells=400_000)
    p = O.Side(*(a[idx] for a in probe))
    b = O.Side(*build)
    cov = O.np_coverage_brute(p, b, strict)
    cnt = O.np_count_overlaps(p, b, strict)
    L = S.length(probe, strict)[idx]
    assert (L > 0).all()
    assert (cov <= exp[idx]).all() and (exp[idx] <= cnt * L).all()


@pytest.mark.parametrize("seed", range(6))
def test_sweep_cases_agree(seed):
    probe, build, nc, strict = S.sweep_case(seed)
    exp = S.prefix_form(probe, build, strict, nc)
    idx = S.sample(len(probe[0]), len(build[0]), cells=1_000_000)
    S.assert_bases_equal(S.pair_form(probe, build, strict, nc, idx), exp[idx], f"seed {seed}: pair form")
    S.assert_bases_equal(S.block_form(probe, build, strict, nc, idx), exp[idx], f"seed {seed}: block form")
