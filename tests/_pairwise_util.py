"""Expected values of pb.pairwise_jaccard without the engine, and the shapes its tests share.

F frames (1 <= F <= 64) read as position sets U(frame), as tests/_multi_util.py reads them.  For every ordered pair (i, j):
  bases[i, j] = |U(i) & U(j)|                       (the diagonal: what frame i covers)
  runs[i, j]  = the maximal runs of U(i) & U(j)     (set_stats' n_intersections; the diagonal: the union runs of frame i)
Two independent numpy forms, both -> (bases, runs) as (F, F) int64:

  pairwise_brute   one boolean array per frame over the universe [0, UNIVERSE] of every contig, pair by pair: &, .sum(), and the
                   run starts by diff: for shapes whose coordinates lie in that universe only
  pairwise_events  the segments of U.multi_events(.., k = 1, consensus = False) and the two sums of the kernel's header
                   (polars-bio_amd/csrc/pairwise.hip.h) in int64: works at the int32 limits"""
import numpy as np

import _multi_util as U

S = U.S
I32_MIN, I32_MAX = S.I32_MIN, S.I32_MAX

# the kernel's geometry, polars-bio_amd/csrc/pairwise.hip.h: PW_STEP segments a wavefront step (one per lane), PW_TILE segments a
# workgroup tile
STEP = 64
TILE = 1024


def pairwise_brute(frames, strict, n_contigs):
    n = len(frames)
    bases, runs = np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
    for ct in range(n_contigs):
        cover = []
        for frame in frames:
            c, s, e = (np.asarray(a).astype(np.int64) for a in frame)
            e1 = e if strict else e + 1
            sel = (c == ct) & (s < e1)
            assert (s[sel] >= 0).all() and (e1[sel] <= U.UNIVERSE).all(), "pairwise_brute is for coordinates in [0, UNIVERSE)"
            diff = np.zeros(U.UNIVERSE + 2, np.int64)
            np.add.at(diff, s[sel], 1)
            np.add.at(diff, e1[sel], -1)
            cover.append(np.cumsum(diff)[:U.UNIVERSE + 1] > 0)
        for i in range(n):
            if not cover[i].any():
                continue
            for j in range(i, n):
                both = cover[i] & cover[j]
                bases[i, j] += int(both.sum())
                runs[i, j] += int((np.diff(np.concatenate([[False], both]).astype(np.int8)) == 1).sum())
    upper = np.triu_indices(n, 1)
    bases.T[upper], runs.T[upper] = bases[upper], runs[upper]
    return bases, runs


def _bits(mask, n):
    mask = np.ascontiguousarray(mask, np.uint64)
    return ((mask[:, None] >> np.arange(n, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.int64)


def pairwise_events(frames, strict, n_contigs):
    n = len(frames)
    c, s, e, mask = U.multi_events(frames, strict, n_contigs, 1, False)
    if c.size == 0:
        return np.zeros((n, n), np.int64), np.zeros((n, n), np.int64)
    length = U.lengths(s, e, strict)
    e1 = e if strict else e + 1                                          # int64: INT32_MAX + 1 does not wrap
    abut = np.concatenate([[False], (c[1:] == c[:-1]) & (e1[:-1] == s[1:])])
    kept = np.where(abut, mask & np.concatenate([[np.uint64(0)], mask[:-1]]).astype(np.uint64), np.uint64(0))
    m, p = _bits(mask, n), _bits(kept, n)
    return m.T @ (m * length[:, None]), m.T @ m - p.T @ p


def jaccard_of(bases):
    """(union, jaccard) of a bases matrix: NaN where the union is empty"""
    own = np.diagonal(bases)
    union = own[:, None] + own[None, :] - bases
    jac = np.full(bases.shape, np.nan)
    np.divide(bases, union, out=jac, where=union != 0)
    return union, jac


# ---- shapes beyond U.SHAPES: name -> builder(strict) -> (frames, n_contigs) -----------------------------------------------------

def _segments(total, n_frames=5):
    """exactly `total` segments of n_frames frames, half of them on each of two contigs: 1 or 2 positions long, every mask a
    random non-empty one that differs from its neighbour's; most segments abut the one before, every seventh follows a gap"""
    def build(strict):
        rng = np.random.default_rng(6000 + total)
        rows = [([], [], []) for _ in range(n_frames)]
        for ct, count in ((0, total - total // 2), (1, total // 2)):
            x, prev = 3, 0
            for k in range(count):
                if k % 7 == 6:
                    x += 1
                m = int(rng.integers(1, 1 << n_frames))
                while m == prev:
                    m = int(rng.integers(1, 1 << n_frames))
                length = int(rng.integers(1, 3))
                for f in range(n_frames):
                    if (m >> f) & 1:
                        rows[f][0].append(ct); rows[f][1].append(x); rows[f][2].append(x + length)
                x, prev = x + length, m
            assert x <= U.UNIVERSE
        return [S.side(*r, strict) for r in rows], 2
    return build


def _abutting_chain(strict):
    """U.SHAPES["touching_runs"] without its gaps and scaled up: 3 segments per period of 12 positions, 900 segments on each of
    four contigs, every one abutting the one before it: a_t = 1 lies on every wavefront-step and tile seam (64 and 1024 are no
    multiples of 3, so the seams meet every phase of the period)"""
    i = np.arange(300, dtype=np.int64)
    frames = [[], [], []]
    for ct in range(4):
        z = np.full(300, ct, np.int64)
        frames[0].append((z, 12 * i, 12 * i + 5))
        frames[1].append((z, 12 * i + 5, 12 * i + 12))
        frames[2] += [(z, 12 * i, 12 * i + 3), (z, 12 * i + 3, 12 * i + 7)]
    return [S.side(*S.cat(*f), strict) for f in frames], 4


def _equal_coordinates_on_two_contigs(strict):
    """both frames end a run at position P on contig 0 and start one at P on contig 1: consecutive segments with equal masks whose
    coordinates say "abutting" and whose contigs differ"""
    P = 500
    f0 = ([0, 0, 1, 1], [P - 40, P - 10, P, P + 30], [P - 30, P, P + 10, P + 40])
    f1 = ([0, 1], [P - 20, P], [P, P + 35])
    return [S.side(*f, strict) for f in (f0, f1)], 2


def _full_span(strict):
    """[INT32_MIN, INT32_MAX] on contig 0 (Weak: 2^32 positions, its end + 1 is 2^31) next to runs that start at INT32_MIN on
    contig 1: in 32 bits the end + 1 of the first would equal the start of the second"""
    f0 = [(0, I32_MIN, I32_MAX), (1, I32_MIN, I32_MIN + 10), (2, I32_MIN, I32_MAX)]
    f1 = [(0, I32_MIN, I32_MAX), (1, I32_MIN, 5), (2, 0, I32_MAX)]
    f2 = [(1, I32_MIN, I32_MAX), (2, I32_MIN, 0)]
    return [S.as_i32(*zip(*f)) for f in (f0, f1, f2)], 3


def _full_masks(strict):
    """64 frames with the same rows: every mask is full, bit 63 is in every pair"""
    rows = ([0, 0, 1], [100, 300, 0], [200, 350, 50])
    return [S.side(*rows, strict) for _ in range(U.MAX_FRAMES)], 2


def _two_segments(strict):
    return [S.side([0], [10], [30], strict), S.side([0], [20], [30], strict)], 1


EXTRA = {f"segments_{n}": _segments(n) for n in (STEP - 1, STEP, STEP + 1, 3 * STEP + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 1)}
EXTRA.update({
    "abutting_chain": _abutting_chain, "equal_coordinates_on_two_contigs": _equal_coordinates_on_two_contigs,
    "full_span_next_to_int32_min": _full_span, "full_masks_64": _full_masks, "two_segments": _two_segments,
})
SHAPES = {**U.SHAPES, **EXTRA}
SMALL_UNIVERSE = [k for k in SHAPES if k not in ("int32_limits", "full_span_next_to_int32_min")]     # what pairwise_brute can hold
TWO_FRAMES = ["two_frames", "equal_coordinates_on_two_contigs", "two_segments"]

_cases = {}


def case(shape, strict):
    """the frames of a shape, built once and shared (read-only)"""
    if shape in U.SHAPES:
        return U.case(shape, strict)
    key = (shape, strict)
    if key not in _cases:
        frames, nc = EXTRA[shape](strict)
        frames = [S.as_i32(*f) for f in frames]
        for f in frames:
            for x in f:
                x.setflags(write=False)
        _cases[key] = (frames, nc)
    return _cases[key]


_expected = {}


def expected(shape, strict):
    """the event-form reference of a case, computed once and shared by the tests of every entry (read-only)"""
    key = (shape, strict)
    if key not in _expected:
        frames, nc = case(shape, strict)
        res = pairwise_events(frames, strict, nc)
        for x in res:
            x.setflags(write=False)
        _expected[key] = res
    return _expected[key]


def assert_equal(got, exp, what=""):
    for name, g, x in zip(("bases", "runs"), got, exp):
        g = np.asarray(g)
        assert g.shape == x.shape, f"{what}: {name} has shape {g.shape}, expected {x.shape}"
        bad = np.argwhere(g != x)
        assert bad.size == 0, f"{what}: {name} differs first at {tuple(bad[0])}: {g[tuple(bad[0])]} != {x[tuple(bad[0])]}"
