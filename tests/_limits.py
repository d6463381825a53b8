"""Interval sets that hug the int32 coordinate limits (test helper; numpy only).

The ABI takes any int32 as a start or an end, and the kernels use INT32_MAX / INT32_MIN as in-band pad values (LDS slice pads,
"rows past the segment" keys).  The generators here put real rows on exactly those values: rows that start or end at a limit,
rows one or two positions away from it, zero-length rows at both limits, the whole-range row, and rows whose length needs 32
bits -- next to rows drawn uniformly over the whole range, so that per-contig grids span all of int32.
"""
import numpy as np

MIN = int(np.iinfo(np.int32).min)
MAX = int(np.iinfo(np.int32).max)

# (start, end) rows that every limit_rows side holds on each of its first contigs
PLANTED = ((MIN, MIN), (MAX, MAX), (MIN, MAX), (MAX - 1, MAX), (MIN, MIN + 1))
ANCHORS = (MIN, MIN + 1, MIN + 2, -1, 0, 1, MAX - 2, MAX - 1, MAX)
LENGTHS = (0, 0, 1, 2, 5, (1 << 31) - 1, (1 << 32) - 1)


def _clip32(a):
    return np.clip(a, MIN, MAX)


def limit_rows(rng, n, n_contigs, inverted=False, outside=False):
    """n limit-hugging rows -> (contig, start, end) int32 columns.

    70 % of the rows start at an anchor (MIN, MIN + 1, MIN + 2, -1, 0, 1, MAX - 2, MAX - 1, MAX) moved by up to 3 positions and
    have a length from LENGTHS (clipped to int32: a row of 2^32 - 1 positions from MIN is the whole range); 30 % start anywhere
    in int32 and are shorter than 2^20.  The PLANTED rows sit on each of the first min(n_contigs, n // 10) contigs, at the head
    of the side.  inverted: 5 % of the other rows have start and end swapped.  outside (the probe side): three rows carry the
    contig id n_contigs, which no dictionary of n_contigs holds."""
    n = int(n)
    s = _clip32(rng.choice(np.array(ANCHORS, np.int64), n) + rng.integers(-3, 4, n))
    e = _clip32(s + rng.choice(np.array(LENGTHS, np.int64), n))
    u = rng.random(n) < 0.3
    us = rng.integers(MIN, MAX + 1, n, dtype=np.int64)
    s = np.where(u, us, s)
    e = np.where(u, _clip32(us + rng.integers(0, 1 << 20, n)), e)
    c = rng.integers(0, n_contigs, n).astype(np.int64)
    if inverted:
        f = rng.random(n) < 0.05
        s, e = np.where(f, e, s), np.where(f, s, e)
    k = min(n_contigs, max(1, n // 10))
    planted = [(cc, ps, pe) for cc in range(k) for ps, pe in PLANTED][:n]
    for i, (cc, ps, pe) in enumerate(planted):
        c[i], s[i], e[i] = cc, ps, pe
    if outside:
        c[len(planted):len(planted) + 3] = n_contigs
    return c.astype(np.int32), s.astype(np.int32), e.astype(np.int32)


def far_contig(rng, n_probe, n_build):
    """Two contigs whose two sides lie at opposite ends of int32 -> (probe, build), n_contigs = 2.  Contig 0: every build row
    within 1000 positions of MAX, every probe within 1000 of MIN; contig 1 the other way round.  No pair overlaps and every
    nearest distance is about 2^32, which neither an int32 nor a uint32 difference of two coordinates holds."""
    def near(lo, n):
        s = lo + rng.integers(0, 990, n)
        return s, s + rng.integers(0, 10, n)
    pc = (np.arange(n_probe) % 2).astype(np.int32)
    bc = (np.arange(n_build) % 2).astype(np.int32)
    ps_lo, pe_lo = near(MIN, n_probe)
    ps_hi, pe_hi = near(MAX - 1000, n_probe)
    bs_lo, be_lo = near(MIN, n_build)
    bs_hi, be_hi = near(MAX - 1000, n_build)
    probe = (pc, np.where(pc == 0, ps_lo, ps_hi).astype(np.int32), np.where(pc == 0, pe_lo, pe_hi).astype(np.int32))
    build = (bc, np.where(bc == 0, bs_hi, bs_lo).astype(np.int32), np.where(bc == 0, be_hi, be_lo).astype(np.int32))
    # the extremes themselves, on both contigs
    probe[1][:2], probe[2][:2] = (MIN, MAX), (MIN, MAX)
    build[1][:2], build[2][:2] = (MAX, MIN), (MAX, MIN)
    return probe, build


def embed(big_side, planted, rng, positions=None):
    """The rows of `planted` written over rows of `big_side` at random positions (or at `positions`) -> the side, as new int32
    columns.  The kernels of the large paths then meet the limit rows inside ordinary tiles, buckets and slices."""
    n, m = len(big_side[0]), len(planted[0])
    pos = rng.choice(n, size=m, replace=False) if positions is None else np.asarray(positions)[:m]
    assert len(pos) == m and len(np.unique(pos)) == m
    out = tuple(np.array(a, np.int32) for a in big_side)
    for col, rows in zip(out, planted):
        col[pos] = rows
    return out


def unsampled_positions(rng, n, m, group=8, every=512):
    """m distinct rows of a side of n rows that a sample of the first `group` rows of every `every` rows never reads."""
    cand = np.nonzero(np.arange(n) % every >= group)[0]
    return rng.choice(cand, size=m, replace=False)


def touches(ep, eb, probe, build):
    """How many expected pairs touch each extreme -> dict; `whole_x_max`: the whole-range probe with the (MAX, MAX) build row."""
    ps, pe, bs, be = probe[1][ep], probe[2][ep], build[1][eb], build[2][eb]
    return {"probe_end_max": int((pe == MAX).sum()), "build_start_max": int((bs == MAX).sum()),
            "probe_start_min": int((ps == MIN).sum()), "build_end_min": int((be == MIN).sum()),
            "whole_x_max": int(((ps == MIN) & (pe == MAX) & (bs == MAX) & (be == MAX)).sum())}


def assert_touches(ep, eb, probe, build, strict):
    """The non-vacuity bar of every limit case, from the reference's own pairs.  Under Weak every extreme occurs in an expected
    pair.  Under Strict a build row with start == MAX cannot match (it needs start < probe end <= MAX) and neither can a build row
    with end == MIN (it needs MIN <= probe start < end): there the bar is that such rows are present on a contig the other side
    uses and that the reference pairs hold none of them -- a kernel that lets a pad or sentinel comparison admit them fails."""
    t = touches(ep, eb, probe, build)
    assert t["probe_end_max"] > 0 and t["probe_start_min"] > 0, t
    if strict:
        used = np.unique(probe[0])
        assert np.isin(build[0][build[1] == MAX], used).any() and np.isin(build[0][build[2] == MIN], used).any()
        assert t["build_start_max"] == 0 and t["whole_x_max"] == 0, t
        assert t["build_end_min"] == 0, t
    else:
        assert t["build_start_max"] > 0 and t["build_end_min"] > 0 and t["whole_x_max"] > 0, t
    return t
