"""Expected values of depth_summary (per probe row the maximum depth of the build side and the positions covered at least T deep)
without the engine, and the shapes its tests share.

d(c, x) = the number of build rows of contig c that cover position x: Strict rows cover [start, end), Weak rows [start, end]; a row
that covers no position contributes nothing; contig ids outside [0, n_contigs) contribute and receive nothing.  For a probe row
with position set Q:  max_depth = max over Q of d (0 when Q is empty),  bases_ge[T] = |{x in Q : d(c, x) >= T}|.
Two independent numpy forms of that definition, both -> (max_depth int64[n], bases_ge int64[K, n]):

  dense_form   a per-base difference array per contig (np.add.at +-1, cumsum), then per probe a slice, .max() and (>= T).sum():
               small spans only; `idx` picks the probe rows it is run on
  block_form   the run-length depth blocks of the build side (_depth_util.depth_events), then per probe np.searchsorted over the
               block bounds, 64-bit threshold prefix sums with int64 edge clips and np.maximum.reduceat: works at the int32 limits"""
import numpy as np

import _depth_util as U
import _depth_sum_util as S
import _limits

I32_MIN, I32_MAX = U.I32_MIN, U.I32_MAX
MAX_THRESHOLDS = 8               # include/ivjoin.h: IVJ_MAX_THRESHOLDS
as_i32 = U.as_i32


def _cols(side):
    return tuple(np.asarray(a).astype(np.int64) for a in side)


def dense_form(probe, build, strict, n_contigs, thresholds, idx=None):
    pc, ps, pe = _cols(probe)
    idx = np.arange(len(pc)) if idx is None else np.asarray(idx)
    w = 0 if strict else 1
    bc, bs, be1 = U._covering(*build, strict, n_contigs)
    md = np.zeros(len(idx), np.int64)
    bg = np.zeros((len(thresholds), len(idx)), np.int64)
    per_base = {}
    for ct in np.unique(bc):
        m = bc == ct
        lo, hi = int(bs[m].min()), int(be1[m].max())
        assert hi - lo < 50_000_000, "dense_form is for small spans"
        diff = np.zeros(hi - lo + 1, np.int64)
        np.add.at(diff, bs[m] - lo, 1)
        np.add.at(diff, be1[m] - lo, -1)
        per_base[int(ct)] = (lo, hi, np.cumsum(diff)[:hi - lo])
    for j, i in enumerate(idx):
        qs, qe = int(ps[i]), int(pe[i]) + w
        if qe <= qs or int(pc[i]) not in per_base:
            continue
        lo, hi, d = per_base[int(pc[i])]
        a, b = max(qs, lo), min(qe, hi)
        if b <= a:
            continue
        win = d[a - lo:b - lo]
        md[j] = int(win.max())
        for k, t in enumerate(thresholds):
            bg[k, j] = int((win >= t).sum())
    return md, bg


def block_form(probe, build, strict, n_contigs, thresholds):
    pc, ps, pe = _cols(probe)
    n = len(pc)
    w = 0 if strict else 1
    md = np.zeros(n, np.int64)
    bg = np.zeros((len(thresholds), n), np.int64)
    kc, ks, ke, kd = U.depth_events(*build, strict, n_contigs)
    if kc.size == 0 or n == 0:
        return md, bg
    ke = ke + w                                        # half-open
    qs, qe = ps, pe + w
    span = np.int64(1) << 34
    ok = (pc >= 0) & (pc < n_contigs) & (qs < qe)
    cq = np.where(ok, pc, 0)
    # blocks are disjoint and sorted: one global order serves both bounds
    i0 = np.searchsorted(kc * span + (ke - I32_MIN), cq * span + (qs - I32_MIN), "right")       # blocks that end at or before qs
    i1 = np.searchsorted(kc * span + (ks - I32_MIN), cq * span + (qe - I32_MIN), "left")        # blocks that start before qe
    live = np.flatnonzero(ok & (i1 > i0))
    if live.size == 0:
        return md, bg
    a, b = i0[live], i1[live]
    lclip = np.maximum(qs[live] - ks[a], 0)
    rclip = np.maximum(ke[b - 1] - qe[live], 0)
    length = ke - ks
    for k, t in enumerate(thresholds):
        P = np.concatenate([[0], np.cumsum(np.where(kd >= t, length, 0))])
        bg[k, live] = P[b] - P[a] - np.where(kd[a] >= t, lclip, 0) - np.where(kd[b - 1] >= t, rclip, 0)
    # reduceat over [a0, b0, a1, b1, ...]: the even results are the maxima over [a_j, b_j) (a_j < b_j); a 0 behind the last block
    # makes b_j = number of blocks a legal index
    pairs = np.empty(2 * live.size, np.int64)
    pairs[0::2], pairs[1::2] = a, b
    md[live] = np.maximum.reduceat(np.concatenate([kd, [0]]), pairs)[0::2]
    return md, bg


# ---- the shapes: name -> builder(strict) -> (probe, build, n_contigs, thresholds) -------------------------------------------------

# threshold lists the reused shapes cycle through: 1, 3 (padded to 4), 4, 8 thresholds, none, repeated and unsorted, 2
THRESHOLD_SETS = [(1,), (1, 2, 5), (1, 10, 20, 30), (1, 2, 3, 4, 5, 6, 7, 8), (), (3, 1, 3, 2, 1), (2, 1)]


def _reused(name, k):
    def build(strict):
        probe, b, nc = S.SHAPES[name](strict)
        return probe, b, nc, THRESHOLD_SETS[k % len(THRESHOLD_SETS)]
    return build


def _small(strict):
    """blocks [10,15) d1, [15,20) d2, [20,30) d1, gap, [40,50) d1, and a nest of identical rows [100,200) x 3 with [120,150) inside;
    probes: inside the gap (no block), strictly inside one block, edges exactly on block boundaries, rows that only touch a block
    (Strict shares nothing, Weak one position), over everything, outside everything, empty"""
    bs = [10, 15, 40, 100, 100, 100, 120]
    be = [20, 30, 50, 200, 200, 200, 150]
    rows = [(30, 40), (32, 38), (16, 19), (41, 42), (15, 20), (10, 15), (20, 30), (10, 30), (5, 10), (50, 60), (30, 41), (0, 300),
            (100, 200), (120, 150), (119, 151), (121, 149), (150, 200), (-50, 0), (300, 400), (25, 25), (26, 25), (60, 50), (199, 200),
            (200, 201), (99, 100)]
    ps, pe = zip(*rows)
    return as_i32(np.zeros(len(rows)), ps, pe), as_i32(np.zeros(len(bs)), bs, be), 1, (1, 2, 3, 4)


N_BLOCKS = 5000


def _many_blocks(deepest):
    """N_BLOCKS blocks on one contig (block j = 8 positions from 10 j, depth 1 .. 7 by repeated rows, a gap of 2 before the next
    one: nothing merges) -- a tree of three levels above the depths -- under probes that span 1, 2, 3, 15 .. 17, 31 .. 33,
    255 .. 257, 4095 .. 4097 and all blocks from random first blocks: the range maximum crosses one, two and three levels with
    partial 16-blocks at both ends.  deepest: the block of depth 50 sits first, last, or in the middle of an otherwise depth-1
    16-block; None: no such block."""
    def build(strict):
        rng = np.random.default_rng(4100 + {None: 0, "first": 1, "last": 2, "alone": 3}[deepest])
        j = np.arange(N_BLOCKS)
        depth = 1 + (j * 2654435761 % 7)
        where = {None: None, "first": 0, "last": N_BLOCKS - 1, "alone": 2064 + 7}[deepest]
        if where is not None:
            g = where & ~15
            depth[g:g + 16] = 1
            depth[where] = 50
        bs = np.repeat(10 * j, depth)
        be = bs + (8 if strict else 7)
        spans = np.array([1, 2, 3, 15, 16, 17, 31, 32, 33, 255, 256, 257, 300, 4095, 4096, 4097, N_BLOCKS])
        sp = np.concatenate([np.tile(spans, 40), rng.integers(1, N_BLOCKS + 1, 1500)])
        first = (rng.integers(0, N_BLOCKS, sp.size) % (N_BLOCKS - sp + 1))
        ps = 10 * first + rng.integers(-2, 8, sp.size)                          # from the gap before the first block to its last position
        pe = 10 * (first + sp - 1) + rng.integers(1, 11, sp.size)               # from its first position to the gap behind the last block
        # the whole contig and beyond, every block alone
        ps = np.concatenate([ps, [-5, 0], 10 * j])
        pe = np.concatenate([pe, [10 * N_BLOCKS + 5, 10 * N_BLOCKS], 10 * j + (8 if strict else 7)])
        return as_i32(np.zeros(ps.size), ps, pe), as_i32(np.zeros(bs.size), bs, be), 1, (1, 4, 7, 50)
    return build


def _depth_tile(n):
    """a build side of n rows = 2 n merged events of the depth kernel (tile U.T)"""
    def build(strict):
        c, s, e, nc = U.SHAPES[f"rows_{n}"](strict)
        rng = np.random.default_rng(4200 + n)
        return U.random_rows(rng, 1500, nc, max(n // 2, 4), 90), (c, s, e), nc, (1, 2, 3)
    return build


def _deep(strict):
    probe, build, nc = S.SHAPES["deep_70k"](strict)
    return probe, build, nc, (1, 65_536, 65_537, 70_000, 70_001)            # the last one is above every depth: a column of zeros


def _whole_range(strict):
    """the build rows of _depth_util's int32_limits shape (contig 0 and 2 covered from INT32_MIN to INT32_MAX) under limit-hugging
    probes; probe 0 is [INT32_MIN, INT32_MAX] on contig 0: 2^32 positions under Weak"""
    c, s, e, nc = U.SHAPES["int32_limits"](strict)
    rng = np.random.default_rng(4300)
    pc, ps, pe = _limits.limit_rows(rng, 1500, nc, outside=True)
    pc[0], ps[0], pe[0] = 0, I32_MIN, I32_MAX
    return (pc, ps, pe), (c, s, e), nc, (1, 2, 3, 4)


def _outside_build(strict):
    c, s, e, nc = U.SHAPES["outside_dictionary"](strict)
    rng = np.random.default_rng(4400)
    return U.random_rows(rng, 2000, 6, 1200, 150), (c, s, e), nc, (1, 3)


SHAPES = {name: _reused(name, k) for k, name in enumerate(n for n in S.SHAPES if n != "deep_70k")}
SHAPES.update({
    "small_edges": _small,
    "blocks_5000": _many_blocks(None), "blocks_5000_deepest_first": _many_blocks("first"), "blocks_5000_deepest_last": _many_blocks("last"),
    "blocks_5000_deepest_alone": _many_blocks("alone"),
    "depth_tile_half": _depth_tile(U.T // 2), "depth_tile": _depth_tile(U.T), "depth_tile_plus": _depth_tile(U.T + 1),
    "deep_70k": _deep, "whole_range": _whole_range, "outside_dictionary_build": _outside_build,
})
# what dense_form can hold (spans below 5 x 10^7 positions per contig)
SMALL_SPAN = [k for k in SHAPES if k not in ("wide_grid", "int32_limits", "int32_limits_inverted", "whole_range")]
# build sides and probes without a row that covers nothing: where O.np_count_overlaps' two-rank formula holds
CLEAN = [k for k in S.CLEAN] + ["blocks_5000", "depth_tile"]


def scan_wide_case():
    """S.scan_wide_case's build side: more than SCAN_WIDE_FROM rows, and more blocks than rows"""
    probe, build, nc = S.scan_wide_case()
    return probe, build, nc, (1, 5, 10)


def sweep_case(seed):
    """one case of the randomised sweep: sizes up to 50 000 rows, a random contig count, mode and threshold list"""
    rng = np.random.default_rng(9500 + seed)
    nb, npr = int(rng.integers(1, 50_001)), int(rng.integers(1, 50_001))
    nc = int(rng.choice([1, 2, 5, 24, 300]))
    strict = bool(rng.integers(0, 2))
    span = max(nb // int(rng.integers(2, 40)), 3)
    build = U.random_rows(rng, nb, nc, span, max_len=int(rng.integers(1, 300)))
    probe = U.random_rows(rng, npr, nc, span, max_len=int(rng.integers(1, 2000)))
    if seed % 3 == 1:
        build = S._degenerate(*build, rng, strict, share=int(rng.integers(4, 40)))
    if seed % 3 == 2:
        probe = S._degenerate(*probe, rng, strict, share=int(rng.integers(4, 40)))
    k = int(rng.integers(0, MAX_THRESHOLDS + 1))
    thresholds = tuple(int(t) for t in rng.integers(1, 40, k))              # any order, repeats allowed
    return probe, build, nc, strict, thresholds


_expected = {}


def expected(shape, strict):
    """(probe, build, n_contigs, thresholds, max_depth, bases_ge by the block form) of a shape, computed once and shared; read-only"""
    key = (shape, strict)
    if key not in _expected:
        probe, build, nc, thr = SHAPES[shape](strict)
        md, bg = block_form(probe, build, strict, nc, thr)
        md.setflags(write=False)
        bg.setflags(write=False)
        _expected[key] = (probe, build, nc, thr, md, bg)
    return _expected[key]


def assert_summary_equal(got, exp, what=""):
    """got = (max_depth or None, bases_ge) of the engine; exp = (max_depth, bases_ge) int64"""
    gm, gb = got
    em, eb = exp
    if gm is not None:
        gm = np.asarray(gm)
        assert gm.dtype == np.int32 and gm.shape == em.shape, f"{what}: max_depth {gm.dtype} {gm.shape}"
        bad = np.flatnonzero(gm.astype(np.int64) != em)
        assert bad.size == 0, f"{what}: max_depth, {bad.size} rows differ, first row {bad[0]}: {gm[bad[0]]} != {em[bad[0]]}"
    gb = np.asarray(gb)
    assert gb.dtype == np.int64 and gb.shape == eb.shape, f"{what}: bases_ge {gb.dtype} {gb.shape} != {eb.shape}"
    bad = np.argwhere(gb != eb)
    assert bad.size == 0, f"{what}: bases_ge, {len(bad)} values differ, first (column, row) {tuple(bad[0])}: {gb[tuple(bad[0])]} != {eb[tuple(bad[0])]}"
