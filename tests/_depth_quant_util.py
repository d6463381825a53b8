"""Expected values of depth_quantiles (per probe row and per rank the order statistic of the build side's depth over the row's
positions) without the engine, and the shapes its tests share.

d(c, x), the modes and Q as in _depth_summary_util.  For a probe row with L = |Q| >= 1 and v[0] <= ... <= v[L - 1] the depths of
its positions, sorted (uncovered positions at depth 0): out[k] = v[k] for 0 <= k < L, -1 for any other rank and for a row that
covers nothing or lies outside the dictionary.  Two independent numpy forms, both ranks int64 (n, K) -> int64 (n, K):

  block_form   per row the depth blocks of _depth_util.depth_events under it, clipped, plus the uncovered mass at depth 0, sorted
               by depth, their cumulative lengths and a searchsorted for the rank: works at the int32 limits
  dense_form   a per-base difference array per contig, a cumulative sum, then per probe np.sort of its window and an index:
               small spans only; `idx` picks the probe rows it is run on

quantiles(v_lo, v_hi, g, method) is the front door's arithmetic on two order statistics."""
import numpy as np

from polars_bio_amd import _engine
import _depth_util as U
import _depth_summary_util as D
import _depth_hist_util as H

MAX_QUANT_RANKS = _engine.MAX_QUANT_RANKS        # include/ivjoin.h: IVJ_MAX_QUANT_RANKS
QUANT_BITS = _engine.QUANT_BITS                  # include/ivjoin.h: IVJ_QUANT_BITS
QUANT_LDS_BYTES = _engine.QUANT_LDS_BYTES        # include/ivjoin.h: IVJ_QUANT_LDS_BYTES
QUANT_MAX_TILE = _engine.QUANT_MAX_TILE          # include/ivjoin.h: IVJ_QUANT_MAX_TILE
I32_MIN = U.I32_MIN
as_i32 = U.as_i32
positions = H.positions


def tile(n_ranks):
    """probe rows one workgroup of k_depth_quant owns: floor(LDS budget / (K * 2^B * 8)) clamped to [1, QUANT_MAX_TILE]"""
    return min(max(QUANT_LDS_BYTES // (n_ranks * (1 << QUANT_BITS) * 8), 1), QUANT_MAX_TILE)


def block_form(probe, build, strict, n_contigs, ranks):
    pc, ps, pe = D._cols(probe)
    ranks = np.asarray(ranks, np.int64)
    n = len(pc)
    out = np.full(ranks.shape, -1, np.int64)
    if n == 0:
        return out
    w = 0 if strict else 1
    L = positions(probe, strict, n_contigs)
    kc, ks, ke, kd = U.depth_events(*build, strict, n_contigs)
    ke = ke + w                                        # half-open
    qs, qe = ps, pe + w
    span = np.int64(1) << 34
    ok = L > 0
    cq = np.where(ok, pc, 0)
    i0 = np.searchsorted(kc * span + (ke - I32_MIN), cq * span + (qs - I32_MIN), "right")       # blocks that end at or before qs
    i1 = np.searchsorted(kc * span + (ks - I32_MIN), cq * span + (qe - I32_MIN), "left")        # blocks that start before qe
    cnt = np.where(ok, np.maximum(i1 - i0, 0), 0)
    # every (row, block) incidence, flat
    row = np.repeat(np.arange(n), cnt)
    first = np.cumsum(cnt) - cnt
    blk = i0[row] + (np.arange(row.size) - first[row])
    ln = np.minimum(ke[blk], qe[row]) - np.maximum(ks[blk], qs[row])
    assert (ln > 0).all()
    covered = np.zeros(n, np.int64)
    np.add.at(covered, row, ln)
    # one entry of depth 0 per row in front: the uncovered mass
    rows = np.concatenate([np.arange(n), row])
    depth = np.concatenate([np.zeros(n, np.int64), kd[blk]])
    mass = np.concatenate([L - covered, ln])
    order = np.lexsort((depth, rows))
    rows, depth, mass = rows[order], depth[order], mass[order]
    cum = np.cumsum(mass)                              # non-decreasing over all rows
    base = np.concatenate([[0], np.cumsum(L)])[:-1]    # the mass in front of a row
    valid = (ranks >= 0) & (ranks < L[:, None])
    at = np.searchsorted(cum, base[:, None] + np.where(valid, ranks, 0), "right")               # the first entry whose cumulative count exceeds the rank
    at = np.minimum(at, cum.size - 1)
    assert (rows[at] == np.arange(n)[:, None])[valid].all()
    out[valid] = depth[at][valid]
    return out


def windows(probe, build, strict, n_contigs, idx=None):
    """(row, its per-position depths SORTED, or None for a row without a position) for the rows of idx; small spans only"""
    pc, ps, pe = D._cols(probe)
    idx = np.arange(len(pc)) if idx is None else np.asarray(idx)
    w = 0 if strict else 1
    bc, bs, be1 = U._covering(*build, strict, n_contigs)
    per_base = {}
    for ct in np.unique(bc):
        m = bc == ct
        lo, hi = int(bs[m].min()), int(be1[m].max())
        assert hi - lo < 50_000_000, "dense_form is for small spans"
        diff = np.zeros(hi - lo + 1, np.int64)
        np.add.at(diff, bs[m] - lo, 1)
        np.add.at(diff, be1[m] - lo, -1)
        per_base[int(ct)] = (lo, hi, np.cumsum(diff)[:hi - lo])
    for i in idx:
        qs, qe = int(ps[i]), int(pe[i]) + w
        if qe <= qs or not 0 <= int(pc[i]) < n_contigs:
            yield int(i), None
            continue
        assert qe - qs < 50_000_000, "dense_form is for small spans"
        win = np.zeros(qe - qs, np.int64)
        if int(pc[i]) in per_base:
            lo, hi, d = per_base[int(pc[i])]
            a, b = max(qs, lo), min(qe, hi)
            if b > a:
                win[a - qs:b - qs] = d[a - lo:b - lo]
        yield int(i), np.sort(win)


def dense_form(probe, build, strict, n_contigs, ranks, idx=None):
    ranks = np.asarray(ranks, np.int64)
    idx = np.arange(len(probe[0])) if idx is None else np.asarray(idx)
    out = np.full((len(idx), ranks.shape[1]), -1, np.int64)
    for j, (i, v) in enumerate(windows(probe, build, strict, n_contigs, idx)):
        if v is None:
            continue
        k = ranks[i]
        ok = (k >= 0) & (k < v.size)
        out[j, ok] = v[k[ok]]
    return out


def quantiles(v_lo, v_hi, g, method):
    """the value of a quantile from its two order statistics, as the issue's table states it"""
    v_lo, v_hi = np.asarray(v_lo), np.asarray(v_hi)
    if method == "lower":
        return v_lo.astype(np.int64)
    if method == "higher":
        return v_hi.astype(np.int64)
    if method == "midpoint":
        return (v_lo.astype(np.float64) + v_hi.astype(np.float64)) / 2.0
    assert method == "linear"
    return v_lo.astype(np.float64) + (v_hi.astype(np.float64) - v_lo.astype(np.float64)) * g


def ranks_for(probe, strict, n_contigs, k, seed):
    """k ranks per row, all inside [0, |Q|) (0 for a row without a position, which has no valid rank): column 0 the lower median,
    the last column (k > 1) the maximum, the rest drawn at random"""
    L = positions(probe, strict, n_contigs)
    rng = np.random.default_rng(7100 + seed)
    r = np.floor(rng.random((len(L), k)) * L[:, None]).astype(np.int64)
    r = np.minimum(r, np.maximum(L - 1, 0)[:, None])
    r[:, 0] = np.maximum(L - 1, 0) // 2
    if k > 1:
        r[:, k - 1] = np.maximum(L - 1, 0)
    return r


# ---- the shapes: name -> builder(strict) -> (probe, build, n_contigs, ranks) ------------------------------------------------------

KS = [1, 3, 16]                                  # the reused shapes cycle through these


def _reused(name, k):
    def build(strict):
        probe, b, nc, _thr = D.SHAPES[name](strict)
        return probe, b, nc, ranks_for(probe, strict, nc, KS[k % len(KS)], k)
    return build


def _tile_edge(k, count):
    """`count` probes around the workgroup's tile of P rows"""
    def build(strict):
        rng = np.random.default_rng(7200 + 16 * count + k)
        probe, b = U.random_rows(rng, count, 2, 9000, 400), U.random_rows(rng, 3000, 2, 9000, 60)
        return probe, b, 2, ranks_for(probe, strict, 2, k, count)
    return build


def _pile(depth, far=200):
    """one contig whose deepest pile is `depth` identical rows over [1000, 1100), shallow rows (depth <= a few) from 2000 on;
    probes: three that straddle the pile's first position (ranks just below, at and just above it), two that straddle its last,
    one inside, one over everything, then `far` rows over the shallow part only"""
    def build(strict):
        rng = np.random.default_rng(7300 + depth % 1000)
        w = 0 if strict else 1
        sh = U.random_rows(rng, 1500, 1, 40_000, 60)
        bs = np.concatenate([np.full(depth, 1000), sh[1] + 2000])
        be = np.concatenate([np.full(depth, 1100 - w), sh[2] + 2000])
        near = [(990, 1010), (999, 1002), (900, 1001), (1090, 1110), (1099, 1101), (1010, 1090), (0, 43_000)]
        fp = U.random_rows(rng, far, 1, 39_000, 400)
        ps = np.concatenate([[a for a, _ in near], fp[1] + 2500])
        pe = np.concatenate([[b - w for _, b in near], fp[2] + 2500])
        probe = as_i32(np.zeros(ps.size), ps, pe)
        ranks = ranks_for(probe, strict, 1, 3, depth)
        for i, (a, _b) in enumerate(near[:3]):
            u = 1000 - a                               # the uncovered positions in front of the pile
            ranks[i] = [u - 1, u, u + 1]
        return probe, as_i32(np.zeros(bs.size), bs, be), 1, ranks
    return build


def _rank_on_a_boundary(strict):
    """3000 blocks of 8 positions, a gap of 2 behind each, depths cycling through 1 .. 5; one probe over 40 blocks and their gaps
    (400 positions: 80 uncovered, 64 at each depth), repeated so that every multiple of 8 and its two neighbours is asked once,
    16 ranks per row: wherever the rank is a multiple of 8 the cumulative count below some depth equals it exactly"""
    build = H._blocks(3000, 1 + np.arange(3000) % 5, strict)
    want = np.unique(np.clip(np.concatenate([np.arange(0, 401, 8) + o for o in (-1, 0, 1)]), 0, 399))
    want = np.concatenate([want, np.full(-want.size % 16, 399)]).reshape(-1, 16)
    m = len(want)
    probe = as_i32(np.zeros(m), np.full(m, 10 * 1200), np.full(m, 10 * 1240 - (0 if strict else 1)))
    return probe, build, 1, want


def _uncovered_mass(strict):
    """blocks of 100 positions with gaps of 100; probes half over a gap (50 uncovered, 50 covered), ranks uncovered - 1, uncovered
    and L - 1; the last probe lies wholly in a gap: its three ranks are L - 1, L (dead) and 0"""
    n, w = 600, 0 if strict else 1
    j = np.arange(n)
    bs = np.repeat(200 * j, 1 + j % 3)
    build = as_i32(np.zeros(bs.size), bs, bs + 100 - w)
    ps = np.concatenate([200 * j + 50, [200 * 7 + 110]])
    pe = np.concatenate([200 * j + 150 - w, [200 * 7 + 190 - w]])
    ranks = np.tile(np.array([49, 50, 99], np.int64), (n + 1, 1))
    ranks[n] = [79, 80, 0]
    return as_i32(np.zeros(ps.size), ps, pe), build, 1, ranks


def _prefixes(strict):
    """one long row over a build side whose depth climbs from 1 to 5000 and falls back, one step per position: 16 ranks spread
    evenly (their prefixes diverge pass by pass), then the same row with all 16 ranks equal, and with all at the maximum"""
    n = 5000
    i = np.arange(n)
    build = as_i32(np.zeros(n), i, 2 * n + 5 - i - (0 if strict else 1))
    L = 2 * n + 205
    probe = as_i32(np.zeros(3), np.full(3, -100), np.full(3, -100 + L - (0 if strict else 1)))
    ranks = np.stack([np.linspace(0, L - 1, 16).astype(np.int64), np.full(16, L // 2), np.full(16, L - 1)])
    return probe, build, 1, ranks


def _from_hist(name, k):
    def build(strict):
        probe, b, nc, _md = H.EDGE_SHAPES[name](strict)
        return probe, b, nc, ranks_for(probe, strict, nc, k, 3)
    return build


def _dead(strict):
    """_depth_hist_util's dead probes among live ones; of the live rows' three ranks the first is -1 and the last |Q|"""
    probe, b, nc, _md = H.EDGE_SHAPES["dead_probes"](strict)
    ranks = ranks_for(probe, strict, nc, 3, 4)
    ranks[:, 2] = positions(probe, strict, nc)
    ranks[:, 0] = -1
    ranks[:, 1] = np.where(np.arange(len(ranks)) % 2 == 0, ranks[:, 1], 2 ** 40)
    return probe, b, nc, ranks


def _no_probes(strict):
    return H.S.EMPTY, U.random_rows(np.random.default_rng(7400), 500, 2, 3000, 60), 2, np.zeros((0, 3), np.int64)


def _empty_build(strict):
    probe, b, nc, _md = H.EDGE_SHAPES["empty_build"](strict)
    return probe, b, nc, ranks_for(probe, strict, nc, 3, 5)


B = QUANT_BITS
SHAPES = {name: _reused(name, k) for k, name in enumerate(D.SHAPES)}
EDGE_SHAPES = {f"tile_k{k}_{what}": _tile_edge(k, n)
               for k in (1, MAX_QUANT_RANKS) for what, n in (("P_minus_1", tile(k) - 1), ("P", tile(k)), ("P_plus_1", tile(k) + 1),
                                                             ("2P_plus_1", 2 * tile(k) + 1))}
EDGE_SHAPES.update({f"pile_{d}": _pile(d) for d in ((1 << B) - 1, 1 << B, (1 << 2 * B) - 1, 1 << 2 * B)})
EDGE_SHAPES.update({"pile_70000_and_a_far_tile": _pile(70_000, far=2 * tile(3) + 5), "rank_on_a_boundary": _rank_on_a_boundary,
                    "uncovered_mass": _uncovered_mass, "diverging_and_shared_prefixes": _prefixes,
                    "long_range_three_chunks": _from_hist("long_range_three_chunks", 3), "one_address": _from_hist("one_address", 2),
                    "dead_probes_and_ranks": _dead, "no_probes": _no_probes, "empty_build": _empty_build})
SHAPES.update(EDGE_SHAPES)
# what dense_form can hold
SMALL_SPAN = [k for k in SHAPES if k not in ("wide_grid", "int32_limits", "int32_limits_inverted", "whole_range")]


def sweep_case(seed):
    """one case of the randomised sweep: _depth_summary_util.sweep_case with a random K in 1 .. 16 and random valid ranks"""
    probe, build, nc, strict, _thr = D.sweep_case(seed)
    k = int(np.random.default_rng(9800 + seed).integers(1, MAX_QUANT_RANKS + 1))
    return probe, build, nc, strict, ranks_for(probe, strict, nc, k, 100 + seed)


_expected = {}


def expected(shape, strict):
    """(probe, build, n_contigs, ranks, values by the block form) of a shape, computed once and shared; read-only"""
    key = (shape, strict)
    if key not in _expected:
        probe, build, nc, ranks = SHAPES[shape](strict)
        val = block_form(probe, build, strict, nc, ranks)
        val.setflags(write=False)
        ranks.setflags(write=False)
        _expected[key] = (probe, build, nc, ranks, val)
    return _expected[key]


def assert_quant_equal(got, exp, what=""):
    got = np.asarray(got)
    assert got.dtype == np.int32 and got.shape == exp.shape, f"{what}: {got.dtype} {got.shape} != {exp.shape}"
    bad = np.argwhere(got.astype(np.int64) != exp)
    assert bad.size == 0, f"{what}: {len(bad)} values differ, first (row, rank) {tuple(bad[0])}: {got[tuple(bad[0])]} != {exp[tuple(bad[0])]}"
