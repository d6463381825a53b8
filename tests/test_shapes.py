"""CPU checks of the real-shaped generators (tests/_shapes.py) and of the oracle on them; no GPU needed.

1. The generators are deterministic (pinned sha256 of 100 k-row draws).
2. The sides tests/test_full_size_shapes.py draws meet that module's conditions.  The statistics are functions of the row
   density and the length parameters, not of n (the scaling rule of _shapes: n * scale rows over contigs of scale x the
   length), so they are computed here once at scale 0.02 .. 0.1; sides that are cheap to draw are checked at full size.
3. The oracle is right on these shapes: its three overlap algorithms agree, nearest_fast == nearest_brute, and
   count_overlaps_fast == the two-rank formula #{s2 < e1} - #{e2 <= s1}, which has no prefix-max structure to be fooled.
"""
import hashlib

import numpy as np
import pytest

import _shapes as S
from oracle import oracle as O


def _sha(side):
    h = hashlib.sha256()
    for a in side:
        assert a.dtype == np.int32
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


DRAWS = {
    "chain": lambda: S.chain_side(100_000, 1, hot=0.2, scale=0.02),
    "tail": lambda: S.tail_side(100_000, 2, 1e-3, wide=3, scale=0.1),
    "pileup": lambda: S.pileup_side(100_000, 3, hot=0.3, absent=0.03, degenerate=0.02, scale=0.02),
    "uniform": lambda: S.uniform_side(100_000, 4, scale=0.02),
}
PINNED = {
    "chain": "77ea7224c21076a6df686df3cd7a44d4a375cbced6021e37170f27ab6d83cc70",
    "tail": "0a5be25ac189c09dbe37eda9ed58152a865ca971a2659653d99b9195f57b96bc",
    "pileup": "24afeedac26ee4e5c5ea170f003a99d97f046a4fb4533f514eb5c33fec4661a3",
    "uniform": "b55938dfd6eff2c0c30808b006b6eecc8b45dc62236ff87b863c0d597ae933e3",
}


@pytest.mark.parametrize("name", sorted(DRAWS))
def test_generators_are_deterministic(name):
    a, b = DRAWS[name](), DRAWS[name]()
    assert len(a[0]) == 100_000 and _sha(a) == _sha(b)
    assert _sha(a) == PINNED[name]


def test_shape_stats_on_hand_made_rows():
    # contig 0: 14 rows, row 0 spans all of them -> rows 12 and 13 see a prefix max (CS_WIN rows back) beyond their start
    s = np.arange(14, dtype=np.int32) * 10
    e = s + 5
    e[0] = 1000
    side = (np.zeros(14, np.int32), s, e)
    st = S.shape_stats(side, 1)
    assert st["far_share"] == 2 / 14
    assert abs(st["mean_depth"] - (1000 + 13 * 5) / 1000) < 1e-12
    flat = (np.zeros(14, np.int32), s, s + 5)
    st = S.shape_stats(flat, 1)
    assert st["far_share"] == 0 and st["mean_depth"] == 1.0
    # buckets: 8 build rows in slices of 4 rows; probes ending behind rows 0..3 / 4..7
    build = (np.zeros(8, np.int32), np.arange(8, dtype=np.int32) * 100, np.arange(8, dtype=np.int32) * 100 + 10)
    probe = (np.zeros(4, np.int32), np.array([0, 50, 120, 700], np.int32), np.array([60, 90, 130, 710], np.int32))
    st = S.shape_stats(probe, 1, build=build, rows_per_slice=4)
    assert st["n_buckets"] == 2 and st["bucket_share"] == 0.75


def test_conditions_of_the_full_size_cases_at_reduced_scale():
    sc = 0.05
    kw = dict(S.CASE_A_BUILD, n=int(S.CASE_A_BUILD["n"] * sc), scale=sc)
    build = S.chain_side(**kw)
    st = S.shape_stats(build, 24)
    assert st["far_share"] >= 100 * S.CS_FAR_LIMIT and st["mean_depth"] >= 4, st          # case A
    R = S.slice_rows(S.CASE_A_BUILD["n"])
    ix = O.Index(O.Side(*build), 25)
    kw = dict(S.CASE_A_PROBES, n=int(S.CASE_A_PROBES["n"] * sc), scale=sc)
    pa = S.uniform_side(**kw)
    sides = {"A": pa, "C": S.stretch_between_samples(pa, by=int(8_000_000 * sc))}
    for name, pk in S.CASE_B_PROBES.items():
        if name == "one_bucket":
            continue                                         # (its window is a slice of the full-size build side: checked there)
        kw = dict(pk, n=int(pk["n"] * sc), scale=sc)
        sides[name] = S.pileup_side(**kw)
        bs = S.shape_stats(sides[name], 25, build=build, rows_per_slice=int(R * sc))        # as many buckets as at full size
        assert bs["bucket_share"] * bs["n_buckets"] >= 8, (name, bs)
    for name, probe in sides.items():
        for strict in (True, False):
            c = O.count_overlaps_fast(ix, O.Side(*probe), strict)
            some = float((c > 0).mean())
            if name in ("A", "C"):      # (what a hot window of 1 / 500 of a contig holds depends on the draw, not on the density:
                assert some >= 0.25 and 1 - some >= 0.20, (name, strict, some)     # case B asserts its shares at full size)
            assert c.sum() / sc <= 3e8, (name, strict, c.sum() / sc)
    # case D: >= 16 pairs per probe, pair total within the limit
    dsc = 0.1
    kw = dict(S.CASE_D_BUILD, n=int(S.CASE_D_BUILD["n"] * dsc), scale=S.CASE_D_BUILD["scale"] * dsc)
    db = S.with_wide_rows(S.chain_side(**kw), S.CASE_D_WIDE, scale=kw["scale"])
    kw = dict(S.CASE_D_PROBES, n=int(S.CASE_D_PROBES["n"] * dsc), scale=S.CASE_D_PROBES["scale"] * dsc)
    dp = S.uniform_side(**kw)
    c = O.count_overlaps_fast(O.Index(O.Side(*db), 24), O.Side(*dp), True)
    assert 16 * len(dp[0]) <= c.sum() <= 3e8 * dsc, c.sum() / len(dp[0])


def test_tail_sides_bracket_the_far_limit():
    far = {k: S.shape_stats(S.tail_side(**kw), 24)["far_share"] for k, kw in S.CASE_E_BUILD.items()}      # full size: 1 M rows
    assert S.CS_FAR_LIMIT < far["above"] <= 3 * S.CS_FAR_LIMIT, far
    assert S.CS_FAR_LIMIT / 3 <= far["below"] < S.CS_FAR_LIMIT, far
    # the default-looking tail (genes among exons) sits between the limit and 1e-2: both join kernels are one knob apart
    mid = S.shape_stats(S.tail_side(1_000_000, 5, 2e-4), 24)["far_share"]
    assert S.CS_FAR_LIMIT < mid < 1e-2, mid
    # one contig-wide row makes every later row of its contig far
    wide = S.shape_stats(S.tail_side(200_000, 5, 0.0, wide=24, scale=0.2), 24)["far_share"]
    assert wide > 0.99, wide


def test_pileup_has_duplicates_sorted_runs_and_depth():
    c, s, e = S.pileup_side(200_000, 9, hot=0.3, absent=0.05, run=8192, scale=0.02)
    key = (c.astype(np.int64) << 32) | s
    for lo in range(0, len(c), 8192):
        assert (np.diff(key[lo:lo + 8192]) >= 0).all()
    assert (np.diff(key) < 0).any()                          # ... but not sorted as a whole
    rows, n_copies = np.unique(np.stack([c, s, e]), axis=1, return_counts=True)
    assert rows.shape[1] < 0.3 * len(c) and n_copies.max() > 100
    assert 0.03 < float((c == 24).mean()) < 0.07
    assert (e > s).all()
    hc, lo, hi = S.hot_window(24, 0.02)
    assert float(((c == hc) & (s >= lo) & (s < hi)).mean()) > 0.25
    full = S.pileup_side(50_000, 9, run=1 << 40, scale=0.02)
    assert (np.diff((full[0].astype(np.int64) << 32) | full[1]) >= 0).all()
    dg = S.pileup_side(50_000, 9, degenerate=0.1, scale=0.02)
    assert 0.03 < float((dg[2] == dg[1]).mean()) < 0.07 and 0.03 < float((dg[2] < dg[1]).mean()) < 0.07


def _small_shapes():
    sc = 0.001
    builds = {
        "chain": S.chain_side(5_000, 31, scale=sc),
        "chain_hot": S.chain_side(5_000, 32, hot=0.3, scale=sc),
        "tail": S.tail_side(5_000, 33, 5e-3, wide=3, scale=sc),
        "pileup": S.pileup_side(5_000, 34, hot=0.2, scale=sc),                 # (inverted BUILD rows: nearest does not define them)
    }
    probes = {
        "uniform": S.uniform_side(20_000, 41, scale=sc),
        "pileup": S.pileup_side(20_000, 42, hot=0.3, absent=0.03, degenerate=0.04, scale=sc),
        "chain": S.chain_side(20_000, 43, hot=0.2, scale=sc),
        "stretched": S.stretch_between_samples(S.uniform_side(20_000, 44, scale=sc), by=20_000),
    }
    return [(f"{pn}-x-{bn}", p, b) for bn, b in builds.items() for pn, p in probes.items()]


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "weak"])
def test_oracle_algorithms_agree_on_every_shape(strict):
    for name, probe, build in _small_shapes():
        ps, bs = O.Side(*probe), O.Side(*build)
        ix = O.Index(bs, 25)
        fp, fb = O.overlap_fast(ix, ps, strict)
        tp, tb = O.overlap_tree(ix, ps, strict)
        assert (fp == tp).all() and (fb == tb).all(), name
        bp, bb = O.overlap_brute(ps, bs, strict)
        of, ob = np.lexsort((fb, fp)), np.lexsort((bb, bp))
        assert len(fp) == len(bp) > 0 and (fp[of] == bp[ob]).all() and (fb[of] == bb[ob]).all(), name
        assert (O.count_overlaps_fast(ix, ps, strict) == O.count_overlaps_brute(ps, bs, strict)).all(), name
        for k, incl in ((1, True), (1, False), (3, True), (3, False)):
            fi, fd, fn = O.nearest_fast(ix, ps, strict, k, incl)
            bi, bd, bn = O.nearest_brute(ps, bs, strict, k, incl)
            assert (fn == bn).all() and (fd == bd).all(), (name, k, incl)
            if not name.endswith("-x-pileup"):              # (a build side of exact duplicates: equal distances, either row)
                assert (fi == bi).all(), (name, k, incl)


@pytest.mark.parametrize("strict", [True, False], ids=["strict", "weak"])
def test_oracle_counts_equal_the_two_rank_formula_at_4M_x_1M(strict):
    sc = 0.2
    builds = {"chain": S.chain_side(1_000_000, 51, scale=sc), "tail": S.tail_side(1_000_000, 52, 2e-4, wide=2, scale=sc)}
    probes = {"pileup": S.pileup_side(4_000_000, 53, hot=0.3, absent=0.03, scale=sc),
              "chain": S.chain_side(4_000_000, 54, hot=0.2, scale=sc)}
    for bn, build in builds.items():
        ix = O.Index(O.Side(*build), 25)
        for pn, probe in probes.items():
            ps = O.Side(*probe)
            c = O.count_overlaps_fast(ix, ps, strict)
            assert c.sum() > len(probe[0]) // 4, (bn, pn)
            assert (c == O.np_count_overlaps(ps, O.Side(*build), strict)).all(), (bn, pn)
