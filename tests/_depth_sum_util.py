"""Expected values of overlap_bases (the per-row numerator of mean_depth) without the engine, and the shapes its tests share.

bases[i] = sum over the build rows of probe row i's contig of the positions the two rows share: Strict rows cover [start, end),
Weak rows [start, end]; a row that covers no position shares nothing; contig ids outside [0, n_contigs) match nothing.
Three independent numpy forms of that definition:

  pair_form    O.np_overlap_pairs, then the clipped length of every pair summed per probe (np.add.at, int64)
  block_form   the run-length depth blocks of the build side (_depth_util.depth_events), clipped to the window, times depth
  prefix_form  G(e') - G(s) with G(x) = x (ra - rb) - PA[ra] + PB[rb] over the sorted starts / half-open ends of the contig
               (np.searchsorted ranks, np.cumsum prefix sums, uint64 with wrap-around): the only one cheap enough for 10^5 rows

pair_form and block_form cost O(probes x build rows); `sample` picks the probe rows they are run on for the larger shapes."""
import numpy as np

from oracle import oracle as O
import _depth_util as U
import _limits

I32_MIN, I32_MAX = U.I32_MIN, U.I32_MAX

# constants of the code under test that the shapes are sized by
CM_LDS = 256                     # index_view.hip.h: per-contig grid metadata in LDS up to this many contigs
SCAN_TILE = 1024 * 8             # onesweep.hip.h: OS_THREADS * LB_ITEMS entries per workgroup of the look-back sum scan
SCAN_WIDE_FROM = 4 << 20         # host_core.hip.h, device_scan: from this many entries on the scan takes tiles of 1024 * 32
                                 # (the scan is one look-back pass: it has no levels, these are its two tile forms)


def _cols(side):
    return tuple(np.asarray(a).astype(np.int64) for a in side)


def _valid(c, n_contigs):
    return (c >= 0) & (c < n_contigs)


def sample(n_probe, n_build, cells=2_000_000):
    """probe rows the quadratic forms are run on: all of them while probes x build rows stays small, else an even spread"""
    if n_probe * max(n_build, 1) <= cells:
        return np.arange(n_probe)
    k = max(8, min(n_probe, cells // max(n_build, 1)))
    return np.unique(np.linspace(0, n_probe - 1, k).astype(np.int64))


def pair_form(probe, build, strict, n_contigs, idx=None):
    pc, ps, pe = _cols(probe)
    bc, bs, be = _cols(build)
    idx = np.arange(len(pc)) if idx is None else idx
    out = np.zeros(len(idx), np.int64)
    if len(idx) == 0 or len(bc) == 0:
        return out
    p, b = O.np_overlap_pairs(O.Side(pc[idx], ps[idx], pe[idx]), O.Side(bc, bs, be), strict)
    keep = _valid(pc[idx][p], n_contigs)
    p, b = p[keep], b[keep]
    w = 0 if strict else 1
    shared = np.minimum(pe[idx][p], be[b]) - np.maximum(ps[idx][p], bs[b]) + w
    np.add.at(out, p, np.maximum(shared, 0))
    return out


def block_form(probe, build, strict, n_contigs, idx=None):
    pc, ps, pe = _cols(probe)
    idx = np.arange(len(pc)) if idx is None else idx
    w = 0 if strict else 1
    kc, ks, ke, kd = U.depth_events(*build, strict, n_contigs)
    ke = ke + w                                        # half-open
    out = np.zeros(len(idx), np.int64)
    for j, i in enumerate(idx):
        qs, qe = int(ps[i]), int(pe[i]) + w
        if qe <= qs or not (0 <= pc[i] < n_contigs):
            continue
        m = kc == pc[i]
        out[j] = int((np.maximum(np.minimum(ke[m], qe) - np.maximum(ks[m], qs), 0) * kd[m]).sum())
    return out


def prefix_form(probe, build, strict, n_contigs):
    pc, ps, pe = _cols(probe)
    bc, bs, be = _cols(build)
    w = 0 if strict else 1
    be = be + w
    keep = _valid(bc, n_contigs) & (bs < be)           # rows that cover no position share nothing
    bc, bs, be = bc[keep], bs[keep], be[keep]
    out = np.zeros(len(pc), np.int64)
    xs_all, xe_all = (ps - I32_MIN).astype(np.uint64), (pe + w - I32_MIN).astype(np.uint64)
    for c in np.unique(pc[_valid(pc, n_contigs)]):
        pm = np.flatnonzero((pc == c) & (xs_all < xe_all))
        bm = bc == c
        if pm.size == 0 or not bm.any():
            continue
        A = np.sort((bs[bm] - I32_MIN).astype(np.uint64))
        B = np.sort((be[bm] - I32_MIN).astype(np.uint64))
        PA = np.concatenate([[np.uint64(0)], np.cumsum(A, dtype=np.uint64)])
        PB = np.concatenate([[np.uint64(0)], np.cumsum(B, dtype=np.uint64)])

        def G(x):
            ra, rb = np.searchsorted(A, x, "left"), np.searchsorted(B, x, "left")
            with np.errstate(over="ignore"):
                return x * (ra.astype(np.int64) - rb.astype(np.int64)).astype(np.uint64) - PA[ra] + PB[rb]
        with np.errstate(over="ignore"):
            out[pm] = (G(xe_all[pm]) - G(xs_all[pm])).view(np.int64)
    return out


def length(probe, strict):
    """positions of every probe row, int64 (<= 0: none)"""
    _, ps, pe = _cols(probe)
    return pe - ps + (0 if strict else 1)


# ---- the shapes: name -> builder(strict) -> (probe, build, n_contigs) ------------------------------------------------------------

as_i32 = U.as_i32
EMPTY = as_i32([], [], [])


def _windows(rng, n, n_contigs, span, max_len):
    return U.random_rows(rng, n, n_contigs, span, max_len)


def _empty_probe(strict):
    return EMPTY, U.random_rows(np.random.default_rng(1), 500, 2, 1000), 2


def _empty_build(strict):
    return U.random_rows(np.random.default_rng(2), 500, 2, 1000), EMPTY, 2


def _one_sided_contigs(strict):
    rng = np.random.default_rng(3)
    pc, ps, pe = _windows(rng, 900, 3, 2000, 300)      # probes on contigs 0, 2, 4; build rows on contigs 2, 3
    bc, bs, be = U.random_rows(rng, 700, 2, 2000, 200)
    return as_i32(pc * 2, ps, pe), as_i32(bc + 2, bs, be), 5


def _three_rows(strict):
    probe = as_i32([0] * 7, [0, 10, 12, 29, 30, 5, 40], [50, 20, 13, 31, 40, 5, 45])
    return probe, as_i32([0, 0, 0], [10, 15, 30], [20, 30, 40]), 1


def _crowded_bins(strict):
    """a few hot positions hold all the rows: bins of the joint grid with dozens of rows whose keys are equal or one or two apart
    (the rank inside such a bin gallops over the key array)"""
    rng = np.random.default_rng(4)
    hot = rng.integers(0, 1_000_000, 40)
    bs = rng.choice(hot, 6000) + rng.integers(0, 3, 6000)
    be = bs + rng.integers(5, 8, 6000)
    ps = rng.choice(hot, 4000) + rng.integers(-6, 9, 4000)
    pe = ps + rng.integers(1, 12, 4000)
    return as_i32(rng.integers(0, 2, 4000), ps, pe), as_i32(rng.integers(0, 2, 6000), bs, be), 2


def _wide_grid(strict):
    """200 rows over nearly all of int32: two bins per row make a bin wider than 2^16 positions (the grid's wide form); the rows
    come in tight groups so that a bin holds several"""
    rng = np.random.default_rng(5)
    centre = rng.integers(I32_MIN + 1000, I32_MAX - 1000, 40)
    bs = np.repeat(centre, 5) + rng.integers(0, 4, 200)
    be = bs + rng.integers(1, 500, 200)
    ps = np.concatenate([rng.choice(centre, 1500) + rng.integers(-300, 300, 1500), rng.integers(I32_MIN, I32_MAX - 600, 500)])
    pe = ps + rng.integers(1, 600, 2000)
    bs[0], be[0] = I32_MIN + 5, I32_MAX - 5                 # the contig spans the whole range
    return as_i32(np.zeros(2000), ps, pe), as_i32(np.zeros(200), bs, be), 1


def _contigs(nc):
    def build(strict):
        rng = np.random.default_rng(600 + nc)
        used = np.arange(0, nc, 3) if nc > 3 else np.arange(nc)          # two of three contigs hold no build row
        bc = rng.choice(used, 5000)
        bs = rng.integers(0, 3000, 5000)
        pc = rng.integers(0, nc, 6000)
        ps = rng.integers(0, 3000, 6000)
        pc[:50] = nc - 1                                     # the last contig id on both sides: the end of the metadata table
        bc[:20] = nc - 1
        return as_i32(pc, ps, ps + rng.integers(1, 400, 6000)), as_i32(bc, bs, bs + rng.integers(1, 200, 5000)), nc
    return build


def _scan_rows(n, n_probe=3000):
    def build(strict):
        rng = np.random.default_rng(7000 + n % 9973)
        bc, bs, be = U.random_rows(rng, n, 3, max(n // 3, 8), 120)
        return _windows(rng, n_probe, 3, max(n // 3, 8), 700), (bc, bs, be), 3
    return build


def _deep(strict):
    """70 000 rows of 100 000 positions that all cover the window [0, 99 000): its bases = 6.93 x 10^9 > 2^32; the same build
    side under 1-position windows"""
    j = np.arange(70_000)
    bs = -(j % 1000)
    be = bs + (100_000 if strict else 99_999)
    one = np.concatenate([np.arange(-1002, 100_003, 97), [-1000, -999, -1, 0, 1, 98_999, 99_000, 99_001, 99_999, 100_000]])
    ps = np.concatenate([[0], one])
    pe = np.concatenate([[99_000 if strict else 98_999], one + (1 if strict else 0)])
    return as_i32(np.zeros(ps.size), ps, pe), as_i32(np.zeros(j.size), bs, be), 1


def _limit_rows(inverted):
    def build(strict):
        rng = np.random.default_rng(88 + inverted)
        return _limits.limit_rows(rng, 2500, 3, outside=True), _limits.limit_rows(rng, 2000, 3, inverted=inverted), 3
    return build


def _degenerate(c, s, e, rng, strict, share=4):
    """a share of the rows made zero-length, start = end + 1 or start > end"""
    kind = rng.integers(0, share, c.size)
    s64, e64 = s.astype(np.int64), e.astype(np.int64)
    e64 = np.where(kind == 0, s64, e64)
    e64 = np.where(kind == 1, s64 - 1, e64)
    e64 = np.where(kind == 2, s64 - rng.integers(2, 60, c.size), e64)
    return as_i32(c, s64, e64)


def _degenerate_build(strict):
    rng = np.random.default_rng(9)
    build = _degenerate(*U.random_rows(rng, 5000, 4, 1500, 90), rng, strict)
    return _windows(rng, 4000, 4, 1500, 200), build, 4


def _zero_length_build(strict):
    """a third of the rows with start == end (Strict: they cover nothing; Weak: one position), none with start > end: the
    index's flag stays clear"""
    rng = np.random.default_rng(10)
    c, s, e = U.random_rows(rng, 4000, 3, 900, 60)
    e = np.where(rng.integers(0, 3, c.size) == 0, s, e)
    return _windows(rng, 3000, 3, 900, 150), as_i32(c, s, e), 3


def _degenerate_probe(strict):
    rng = np.random.default_rng(11)
    probe = _degenerate(*_windows(rng, 4000, 4, 1500, 200), rng, strict)
    return probe, U.random_rows(rng, 5000, 4, 1500, 90), 4


def _touching_nested(strict):
    """a bookended chain, nests around one centre, and windows that end exactly on the rows' bounds"""
    i = np.arange(2000)
    bs = np.concatenate([10 * i, 30_000 - i])
    be = np.concatenate([10 * i + (10 if strict else 9), 30_000 + i + 1])
    ps = np.concatenate([10 * i + 10, 10 * i - 5, 30_000 - 2 * i, np.full(2000, 30_000)])
    pe = np.concatenate([10 * i + 20, 10 * i, 30_000 + 2 * i + 1, 30_000 + i + 1])
    if not strict:
        pe = pe - 1
    return as_i32(np.zeros(ps.size), ps, pe), as_i32(np.zeros(bs.size), bs, be), 1


SHAPES = {
    "empty_probe": _empty_probe, "empty_build": _empty_build, "one_sided_contigs": _one_sided_contigs, "three_rows": _three_rows,
    "crowded_bins": _crowded_bins, "wide_grid": _wide_grid,
    "contigs_1": _contigs(1), "contigs_24": _contigs(24), "contigs_cm_lds": _contigs(CM_LDS), "contigs_cm_lds_plus": _contigs(CM_LDS + 1),
    # the scan runs over build rows + 1 entries: one tile exactly, one entry more, several tiles
    "scan_one_tile": _scan_rows(SCAN_TILE - 1), "scan_two_tiles": _scan_rows(SCAN_TILE), "scan_tiles_3": _scan_rows(3 * SCAN_TILE + 5),
    "scan_300k": _scan_rows(300_000, 100_000),
    "deep_70k": _deep, "int32_limits": _limit_rows(False), "int32_limits_inverted": _limit_rows(True),
    "degenerate_build": _degenerate_build, "zero_length_build": _zero_length_build, "degenerate_probe": _degenerate_probe,
    "touching_nested": _touching_nested,
}
# build sides without a row that covers nothing, probes likewise: where O.np_count_overlaps' two-rank formula holds
CLEAN = ["one_sided_contigs", "crowded_bins", "wide_grid", "contigs_24", "scan_two_tiles", "deep_70k", "touching_nested"]


def scan_wide_case():
    """the one case beyond the other shapes' sizes: SCAN_WIDE_FROM build rows, so that the position sums take the scan's wide tiles"""
    rng = np.random.default_rng(12)
    n = SCAN_WIDE_FROM + 77
    bs = rng.integers(0, 50_000_000, n)
    build = as_i32(rng.integers(0, 2, n), bs, bs + rng.integers(1, 150, n))
    ps = rng.integers(0, 50_000_000, 20_000)
    return as_i32(rng.integers(0, 2, 20_000), ps, ps + rng.integers(1, 5000, 20_000)), build, 2


def sweep_case(seed):
    """one case of the randomised sweep: up to 10^5 rows per side, a span small enough that ties are common, a random mode and
    contig count, and in two cases of three a share of rows that cover nothing on either side"""
    rng = np.random.default_rng(9000 + seed)
    nb, npr = int(rng.integers(1, 100_001)), int(rng.integers(1, 100_001))
    nc = int(rng.choice([1, 2, 5, 24, 300]))
    strict = bool(rng.integers(0, 2))
    span = max(nb // int(rng.integers(2, 40)), 3)
    build = U.random_rows(rng, nb, nc, span, max_len=int(rng.integers(1, 300)))
    probe = U.random_rows(rng, npr, nc, span, max_len=int(rng.integers(1, 2000)))
    if seed % 3 == 1:
        build = _degenerate(*build, rng, strict, share=int(rng.integers(4, 40)))
    if seed % 3 == 2:
        probe = _degenerate(*probe, rng, strict, share=int(rng.integers(4, 40)))
        c, s, e = build
        build = as_i32(c, s, np.where(rng.integers(0, 20, nb) == 0, s, e))          # zero-length rows only: no flag
    return probe, build, nc, strict


_expected = {}


def expected(shape, strict):
    """(probe, build, n_contigs, bases by the prefix form) of a shape, computed once and shared; read-only"""
    key = (shape, strict)
    if key not in _expected:
        probe, build, nc = SHAPES[shape](strict)
        exp = prefix_form(probe, build, strict, nc)
        exp.setflags(write=False)
        _expected[key] = (probe, build, nc, exp)
    return _expected[key]


def assert_bases_equal(got, exp, what=""):
    got = np.asarray(got)
    assert got.dtype == np.int64 and got.shape == exp.shape, f"{what}: {got.dtype} {got.shape}"
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"{what}: {bad.size} rows differ, first row {bad[0]}: {got[bad[0]]} != {exp[bad[0]]}"
