"""Expected values of depth_hist (per probe row, or per contig, the number of positions at each depth 0 .. D of the build side, the
last bin holding depth >= D) without the engine, and the shapes its tests share.

d(c, x), the modes and Q as in _depth_summary_util.  Region form, for a probe row with position set Q and bins = D + 1:
hist[d] = |{x in Q : d(c, x) == d}| for d < D, hist[D] = |{x in Q : d(c, x) >= D}|; a probe that covers nothing or lies outside
the dictionary gets zeros.  Two independent numpy forms, both -> int64 (n, D + 1):

  block_form   _depth_summary_util.block_form with thresholds 1 .. D (no 8-threshold limit there): hist[d] = ge[d] - ge[d + 1],
               hist[D] = ge[D], hist[0] = |Q| - ge[1]: works at the int32 limits
  dense_form   a per-base difference array per contig, a cumulative sum, then per probe np.bincount(np.minimum(window, D)):
               small spans only

Contig form -> int64 (n_contigs, D + 1): np.add.at of the block lengths of _depth_util.depth_events at [contig, min(depth, D)];
bin 0 stays 0."""
import numpy as np

from polars_bio_amd import _engine
import _depth_util as U
import _depth_sum_util as S
import _depth_summary_util as D

MAX_HIST_DEPTH = _engine.MAX_HIST_DEPTH          # include/ivjoin.h: IVJ_MAX_HIST_DEPTH
HIST_LDS_BYTES = _engine.HIST_LDS_BYTES          # include/ivjoin.h: IVJ_HIST_LDS_BYTES
HIST_MAX_TILE = _engine.HIST_MAX_TILE            # include/ivjoin.h: IVJ_HIST_MAX_TILE
CHUNK = 2048                     # depth_hist.hip.h: DH_CH, items (blocks under probes, or blocks) per chunk / tile
as_i32 = U.as_i32


def tile(max_depth):
    """probe rows one workgroup of k_depth_hist owns: floor(LDS budget / (bins * 8)) clamped to [1, HIST_MAX_TILE]"""
    return min(max(HIST_LDS_BYTES // ((max_depth + 1) * 8), 1), HIST_MAX_TILE)


def positions(probe, strict, n_contigs):
    """|Q| of every probe row (int64); 0 for a row that covers nothing or lies outside the dictionary"""
    pc, ps, pe = D._cols(probe)
    ln = pe - ps + (0 if strict else 1)
    return np.where((pc >= 0) & (pc < n_contigs) & (ln > 0), ln, 0)


def block_form(probe, build, strict, n_contigs, max_depth):
    _, ge = D.block_form(probe, build, strict, n_contigs, range(1, max_depth + 1))
    n = len(probe[0])
    hist = np.zeros((n, max_depth + 1), np.int64)
    hist[:, 1:max_depth] = (ge[:-1] - ge[1:]).T
    hist[:, max_depth] = ge[max_depth - 1]
    hist[:, 0] = positions(probe, strict, n_contigs) - ge[0]
    return hist


def dense_form(probe, build, strict, n_contigs, max_depth):
    pc, ps, pe = D._cols(probe)
    w = 0 if strict else 1
    bc, bs, be1 = U._covering(*build, strict, n_contigs)
    hist = np.zeros((len(pc), max_depth + 1), np.int64)
    per_base = {}
    for ct in np.unique(bc):
        m = bc == ct
        lo, hi = int(bs[m].min()), int(be1[m].max())
        assert hi - lo < 50_000_000, "dense_form is for small spans"
        diff = np.zeros(hi - lo + 1, np.int64)
        np.add.at(diff, bs[m] - lo, 1)
        np.add.at(diff, be1[m] - lo, -1)
        per_base[int(ct)] = (lo, hi, np.cumsum(diff)[:hi - lo])
    for i in range(len(pc)):
        qs, qe = int(ps[i]), int(pe[i]) + w
        if qe <= qs or not 0 <= int(pc[i]) < n_contigs:
            continue
        covered = 0
        if int(pc[i]) in per_base:
            lo, hi, d = per_base[int(pc[i])]
            a, b = max(qs, lo), min(qe, hi)
            if b > a:
                hist[i] = np.bincount(np.minimum(d[a - lo:b - lo], max_depth), minlength=max_depth + 1)
                covered = b - a
        hist[i, 0] += (qe - qs) - covered
    return hist


def contig_form(build, strict, n_contigs, max_depth):
    kc, ks, ke, kd = U.depth_events(*build, strict, n_contigs)
    hist = np.zeros((n_contigs, max_depth + 1), np.int64)
    np.add.at(hist, (kc, np.minimum(kd, max_depth)), ke - ks + (0 if strict else 1))
    return hist


# ---- the shapes: name -> builder(strict) -> (probe, build, n_contigs, max_depth) ------------------------------------------------

DEPTHS = [1, 2, 7, 63, 64, 255, 1023]          # the reused shapes cycle through these


def _reused(name, k):
    def build(strict):
        probe, b, nc, _thr = D.SHAPES[name](strict)
        return probe, b, nc, DEPTHS[k % len(DEPTHS)]
    return build


def _tile_edge(max_depth, count):
    """`count` probes around the workgroup's tile of P rows, over a pile deep enough for the clamp of max_depth = 1"""
    def build(strict):
        rng = np.random.default_rng(6100 + max_depth + count)
        return U.random_rows(rng, count, 2, 9000, 400), U.random_rows(rng, 3000, 2, 9000, 60), 2, max_depth
    return build


def _blocks(n, depth, strict):
    """n blocks on contig 0: block j = 8 positions from 10 j at depth[j] (repeated rows), a gap of 2 behind it"""
    bs = np.repeat(10 * np.arange(n), depth)
    return as_i32(np.zeros(bs.size), bs, bs + (8 if strict else 7))


def _one_block_probes(first, count, strict):
    j = first + np.arange(count)
    return 10 * j + 1, 10 * j + (6 if strict else 5)


def _long_range(strict):
    """one probe over all 5000 blocks amid 300 one-block probes: its range starts at item 150 of the tile's first chunk and
    spans three chunks"""
    n = D.N_BLOCKS
    build = _blocks(n, 1 + (np.arange(n) * 2654435761 % 7), strict)
    s0, e0 = _one_block_probes(0, 150, strict)
    s1, e1 = _one_block_probes(2000, 150, strict)
    ps = np.concatenate([s0, [-5], s1])
    pe = np.concatenate([e0, [10 * n + 5], e1])
    return as_i32(np.zeros(ps.size), ps, pe), build, 1, 5


def _one_address(strict):
    """4096 blocks of depth 1 under one probe, max_depth 1: every lane of two chunks adds to one LDS address"""
    build = _blocks(2 * CHUNK, np.ones(2 * CHUNK, np.int64), strict)
    return as_i32([0, 0], [0, 3], [10 * 2 * CHUNK, 10 * CHUNK + 4]), build, 1, 1


def _clamp_boundary(strict):
    """blocks alternating between depth D - 1, D and D + 1 with D = 4"""
    n, md = 3000, 4
    build = _blocks(n, md - 1 + np.arange(n) % 3, strict)
    rng = np.random.default_rng(6200)
    first = rng.integers(0, n - 40, 700)
    ps = 10 * first + rng.integers(-2, 8, 700)
    pe = 10 * (first + rng.integers(0, 40, 700)) + rng.integers(1, 11, 700)
    return as_i32(np.zeros(700), ps, pe), build, 1, md


def _dead_probes(strict):
    """empty and inverted probes, and probes outside the dictionary, interleaved with live ones"""
    probe, build, nc, _ = D.SHAPES["blocks_5000"](strict)
    pc, ps, pe = (a.copy() for a in probe)
    k = np.arange(pc.size) % 5
    pe = np.where(k == 1, ps - (0 if strict else 1), pe)          # no position
    pe = np.where(k == 2, ps - 7, pe)                             # inverted
    pc = np.where(k == 3, np.where(np.arange(pc.size) % 2 == 0, -1, nc), pc)
    return as_i32(pc, ps, pe), build, nc, 3


def _no_probes(strict):
    return S.EMPTY, U.random_rows(np.random.default_rng(6300), 500, 2, 3000, 60), 2, 9


def _empty_build(strict):
    probe = U.random_rows(np.random.default_rng(6400), 700, 3, 3000, 400)
    return (np.where(np.arange(700) % 9 == 0, 5, probe[0]).astype(np.int32), probe[1], probe[2]), S.EMPTY, 3, 6


SHAPES = {name: _reused(name, k) for k, name in enumerate(D.SHAPES)}
EDGE_SHAPES = {f"tile_d{md}_{what}": _tile_edge(md, n)
               for md in (1, MAX_HIST_DEPTH) for what, n in (("P_minus_1", tile(md) - 1), ("P", tile(md)), ("P_plus_1", tile(md) + 1),
                                                              ("2P_plus_1", 2 * tile(md) + 1))}
EDGE_SHAPES.update({"long_range_three_chunks": _long_range, "one_address": _one_address, "clamp_boundary": _clamp_boundary,
                    "dead_probes": _dead_probes, "no_probes": _no_probes, "empty_build": _empty_build})
SHAPES.update(EDGE_SHAPES)
# what dense_form can hold
SMALL_SPAN = [k for k in SHAPES if k not in ("wide_grid", "int32_limits", "int32_limits_inverted", "whole_range")]


def _straddle(strict):
    """2048 + 5 blocks, the contig changes at block 2040: the first tile's last 8 blocks lie on the next contig"""
    c0 = _blocks(2040, 1 + np.arange(2040) % 3, strict)
    c1 = _blocks(CHUNK + 5 - 2040, 1 + np.arange(CHUNK + 5 - 2040) % 4, strict)
    return as_i32(np.concatenate([c0[0], c1[0] + 1]), np.concatenate([c0[1], c1[1]]), np.concatenate([c0[2], c1[2]])), 2, 2


def _tiny_contigs(strict):
    """300 contigs of 3 blocks each: all but the first contig of a tile take the global-atomic route"""
    one = _blocks(3, np.array([2, 1, 3]), strict)
    c = np.repeat(np.arange(300), one[0].size)
    return as_i32(c, np.tile(one[1], 300) + c, np.tile(one[2], 300) + c), 300, 2


def _contig_reused(name, k):
    def build(strict):
        _p, b, nc, _thr = D.SHAPES[name](strict)
        return b, nc, DEPTHS[k % len(DEPTHS)]
    return build


# name -> builder(strict) -> (frame, n_contigs, max_depth)
CONTIG_SHAPES = {name: _contig_reused(name, k) for k, name in enumerate(D.SHAPES)}
CONTIG_SHAPES.update({"tile_straddles_two_contigs": _straddle, "tiny_contigs_300": _tiny_contigs})


def sweep_case(seed):
    """one case of the randomised sweep: _depth_summary_util.sweep_case with a random max_depth in 1 .. 300"""
    probe, build, nc, strict, _thr = D.sweep_case(seed)
    return probe, build, nc, strict, int(np.random.default_rng(9700 + seed).integers(1, 301))


_expected = {}


def expected(shape, strict):
    """(probe, build, n_contigs, max_depth, hist by the block form) of a shape, computed once and shared; read-only"""
    key = (shape, strict)
    if key not in _expected:
        probe, build, nc, md = SHAPES[shape](strict)
        hist = block_form(probe, build, strict, nc, md)
        hist.setflags(write=False)
        _expected[key] = (probe, build, nc, md, hist)
    return _expected[key]


def assert_hist_equal(got, exp, what=""):
    got = np.asarray(got)
    assert got.dtype == np.int64 and got.shape == exp.shape, f"{what}: hist {got.dtype} {got.shape} != {exp.shape}"
    bad = np.argwhere(got != exp)
    assert bad.size == 0, f"{what}: {len(bad)} values differ, first (row, bin) {tuple(bad[0])}: {got[tuple(bad[0])]} != {exp[tuple(bad[0])]}"
