"""The yardstick of the distance-window join (test helper; numpy only) and the shapes the GPU tests run it on.

``brute`` is a brute force over all probe x build pairs of one contig, 256 probe rows at a time, that evaluates the LITERAL
definitions of include/ivjoin.h in int64 --

    gap_right = b.start - a.end      gap_left = a.start - b.end
    d(a, b)   = 0 if the rows overlap under the frame's predicate, else max(gap_right, gap_left)
    kept iff  both rows cover a position  and  d >= min_distance  and
              (overlap  or  (b after a and d <= R(a))  or  (b before a and d <= L(a)))

-- with "b after a" = not (b.start (<) a.end) and "b before a" = not (a.start (<) b.end).  Contig ids outside [0, n_contigs) never
pair.  The signed distance is -d for a build row before the probe row."""
import os
import re

import numpy as np

MIN = int(np.iinfo(np.int32).min)
MAX = int(np.iinfo(np.int32).max)
U32 = (1 << 32) - 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _const(name):
    src = open(os.path.join(ROOT, "polars-bio_amd", "csrc", "window.hip.h")).read()
    return int(re.search(name + r"\s*=\s*(\d+)", src).group(1))


def kernel_tile():
    """Probes per workgroup of the window kernel, from its header."""
    return _const("WIN_THREADS") * _const("WIN_ITEMS")


def kernel_chunk():
    """Candidates per chunk of the window kernel, from its header."""
    return _const("WIN_CH")


def brute(probe, build, n_contigs, strict, left, right, min_distance, probe_left=None, probe_right=None, rows=256):
    """-> (probe_idx, build_idx, signed distance) sorted by (probe row, build row), and the per-probe counts (int64)."""
    pc, ps, pe = (np.asarray(a, np.int64) for a in probe)
    bc, bs, be = (np.asarray(a, np.int64) for a in build)
    n = len(pc)
    L = np.full(n, int(left), np.int64) if probe_left is None else np.asarray(probe_left, np.uint32).astype(np.int64)
    R = np.full(n, int(right), np.int64) if probe_right is None else np.asarray(probe_right, np.uint32).astype(np.int64)
    lt = (lambda x, y: x < y) if strict else (lambda x, y: x <= y)
    outp, outb, outd = [np.empty(0, np.int64)], [np.empty(0, np.int64)], [np.empty(0, np.int64)]
    for c in np.unique(pc):
        if c < 0 or c >= n_contigs:
            continue
        P, B = np.nonzero(pc == c)[0], np.nonzero(bc == c)[0]
        if len(B) == 0:
            continue
        for lo in range(0, len(P), rows):
            p = P[lo:lo + rows]
            a_s, a_e, b_s, b_e = ps[p][:, None], pe[p][:, None], bs[B][None, :], be[B][None, :]
            covers = lt(a_s, a_e) & lt(b_s, b_e)
            ov = lt(b_s, a_e) & lt(a_s, b_e)
            after, before = ~lt(b_s, a_e), ~lt(a_s, b_e)
            d = np.where(ov, 0, np.maximum(b_s - a_e, a_s - b_e))
            keep = covers & (d >= int(min_distance)) & (ov | (after & (d <= R[p][:, None])) | (before & (d <= L[p][:, None])))
            i, j = np.nonzero(keep)
            outp.append(p[i])
            outb.append(B[j])
            outd.append(np.where(before[i, j] & ~ov[i, j], -d[i, j], d[i, j]))
    qp, qb, qd = np.concatenate(outp), np.concatenate(outb), np.concatenate(outd)
    o = np.lexsort((qb, qp))
    qp, qb, qd = qp[o].astype(np.int32), qb[o].astype(np.int32), qd[o].astype(np.int64)
    return qp, qb, qd, np.bincount(qp, minlength=n).astype(np.int64)


def sort_pairs(p, b, d=None):
    p, b = np.asarray(p), np.asarray(b)
    o = np.lexsort((b, p))
    return (p[o], b[o]) if d is None else (p[o], b[o], np.asarray(d)[o])


def assert_order(p, b, build):
    """The output contract: the pairs of one probe are contiguous and ordered by (build.start, build row)."""
    p, b = np.asarray(p, np.int64), np.asarray(b, np.int64)
    if len(p) < 2:
        return
    change = np.nonzero(p[1:] != p[:-1])[0]
    assert len(np.unique(p)) == len(change) + 1, "the pairs of one probe row are not contiguous"
    same = p[1:] == p[:-1]
    s = np.asarray(build[1], np.int64)[b]
    ok = (s[1:] > s[:-1]) | ((s[1:] == s[:-1]) & (b[1:] > b[:-1]))
    assert ok[same].all(), "the pairs of a probe row are not ordered by (build.start, build row)"


def side(rows, contig=0):
    """[(start, end), ...] or [(contig, start, end), ...] -> int32 columns."""
    rows = [((contig,) + tuple(r)) if len(r) == 2 else tuple(r) for r in rows]
    return tuple(np.array([r[k] for r in rows], np.int64).astype(np.int32) for k in range(3))


def _random_side(rng, n, nc, span, max_len, empty=True):
    c = rng.integers(0, nc, n).astype(np.int32)
    s = rng.integers(0, span, n).astype(np.int64)
    ln = rng.integers(1, max_len + 1, n).astype(np.int64)
    if empty:
        ln[rng.random(n) < 0.05] = 0
        ln[rng.random(n) < 0.02] = -3
    return c, s.astype(np.int32), (s + ln).astype(np.int32)


def W(left=0, right=0, min_distance=0, probe_left=None, probe_right=None):
    return dict(left=left, right=right, min_distance=min_distance, probe_left=probe_left, probe_right=probe_right)


# ---- the shapes: name -> () -> dict(probe, build, nc, windows=[W(...), ...]) ------------------------------------------------

def small_edges():
    """One contig; build rows at gap w - 1, w, w + 1 on each side of a probe for w in {0, 1, 1000}; bookended, contained,
    containing and identical rows."""
    a = (100_000, 100_100)
    rows = [a, (a[0] + 10, a[1] - 10), (a[0] - 50, a[1] + 50), (a[1], a[1] + 5), (a[0] - 5, a[0])]
    for w in (0, 1, 1000):
        for g in (w - 1, w, w + 1):
            rows += [(a[1] + g, a[1] + g + 7), (a[0] - g - 7, a[0] - g)]
    probe = side([a, (a[0], a[0] + 1), (a[1] + 1000, a[1] + 1001)])
    return dict(probe=probe, build=side(rows), nc=1, windows=[W(w, w) for w in (0, 1, 2, 999, 1000, 1001)])


def asymmetric():
    rng = np.random.default_rng(7)
    probe, build = _random_side(rng, 700, 2, 60_000, 200), _random_side(rng, 900, 2, 60_000, 150)
    pl = rng.choice(np.array([0, 0, 1, 50, 700, 5000], np.uint32), 700)
    pr = rng.choice(np.array([0, 0, 3, 90, 1000, 4000], np.uint32), 700)
    return dict(probe=probe, build=build, nc=2,
                windows=[W(0, 800), W(800, 0), W(probe_left=pl, probe_right=pr), W(left=300, probe_right=pr), W(right=300, probe_left=pl)])


def min_distance():
    """Gaps at m - 1 and m; overlapping rows with m = 0 and m = 1; m above both extents."""
    a = (50_000, 50_200)
    m = 40
    rows = [(a[0] + 20, a[0] + 30), a, (a[1], a[1] + 9), (a[0] - 9, a[0])]
    for g in (m - 1, m, m + 1):
        rows += [(a[1] + g, a[1] + g + 5), (a[0] - g - 5, a[0] - g)]
    return dict(probe=side([a]), build=side(rows), nc=1,
                windows=[W(100, 100, 0), W(100, 100, 1), W(100, 100, m), W(100, 100, m + 1), W(100, 100, 101), W(10, 100, 50), W(0, 0, 1)])


def int32_limits():
    """Rows at INT32_MIN and INT32_MAX with extents 1, 2^31 and 2^32 - 1 (pads that overflow int32 on either side); a closed row of
    length 2^31; a pair at distance 2^32 - 1."""
    rows_p = [(MIN, MIN + 1), (MAX - 1, MAX), (MIN, MIN), (MAX, MAX), (0, MAX), (MIN, -1), (0, 10), (MIN, MAX), (MAX, MIN)]
    rows_b = [(MIN, MIN + 1), (MAX - 1, MAX), (MIN, MIN), (MAX, MAX), (-1, MAX), (MIN, 0), (-5, 5), (MIN + 1, MIN + 2), (MAX - 2, MAX - 1),
              (MIN, MAX), (7, 3)]
    ws = [W(e, e) for e in (0, 1, 1 << 31, U32)] + [W(U32, 0), W(0, U32), W(U32, U32, U32), W(U32, U32, U32 - 1), W(1 << 31, 1, 1 << 31)]
    return dict(probe=side(rows_p), build=side(rows_b), nc=1, windows=ws)


def tile_edges():
    """511, 512, 513 and 1025 probes (the 512-probe tile)."""
    T = kernel_tile()
    rng = np.random.default_rng(11)
    build = _random_side(rng, 1500, 2, 40_000, 120)
    out = []
    for n in (T - 1, T, T + 1, 2 * T + 1):
        out.append(_random_side(rng, n, 2, 40_000, 100))
    return dict(probe=out, build=build, nc=2, windows=[W(150, 90, 5)])


def chunks():
    """One probe with 5 000 build rows inside its window (three chunks); a tile whose ranges start and end on chunk boundaries
    (a probe over 2047, 2048 and 2049 build rows -- the loose range may add a row or two -- followed by probes whose ranges begin
    where it ends); every probe of a tile on one range."""
    CH, T = kernel_chunk(), kernel_tile()
    i = np.arange(5000)
    dense = (np.zeros(5000, np.int32), (10_000 + 2 * i).astype(np.int32), (10_001 + 2 * i).astype(np.int32))
    one = side([(15_000, 15_010)])
    cases = [dict(probe=one, build=dense, nc=1, windows=[W(6000, 6000), W(6000, 6000, 100), W(10, 6000)])]
    for n in (CH - 1, CH, CH + 1):
        j = np.arange(n)
        b = (np.zeros(n, np.int32), (1000 + 3 * j).astype(np.int32), (1002 + 3 * j).astype(np.int32))
        # two probes: the first one's range takes all n rows, the second one's starts where it ends
        cases.append(dict(probe=side([(1000, 1000 + 3 * n), (1000 + 3 * n + 50, 1000 + 3 * n + 60), (900, 950)]), build=b, nc=1,
                          windows=[W(0, 0), W(40, 40), W(3 * n + 100, 3 * n + 100)]))
    same = (np.zeros(T, np.int32), np.full(T, 12_000, np.int32), np.full(T, 12_050, np.int32))
    cases.append(dict(probe=same, build=(dense[0][:300], dense[1][:300] + 1500, dense[2][:300] + 1500), nc=1, windows=[W(700, 400, 3)]))
    return cases


def long_row():
    """A contig-wide build row keeps every range open: candidates far outnumber matches."""
    n = 4000
    starts = 100 * np.arange(n, dtype=np.int64) + 100
    build = (np.zeros(n + 1, np.int32), np.concatenate([[0], starts]).astype(np.int32), np.concatenate([[500_000], starts + 50]).astype(np.int32))
    ps = np.concatenate([100 + 97 * np.arange(15), 390_000 + 97 * np.arange(15)])
    probe = (np.zeros(30, np.int32), ps.astype(np.int32), (ps + 180).astype(np.int32))
    return dict(probe=probe, build=build, nc=1, windows=[W(250, 250), W(250, 250, 1), W(0, 1000, 60)])


def _contigs(nc):
    rng = np.random.default_rng(nc)
    probe, build = _random_side(rng, 1100, nc, max(200_000 // nc, 3000), 150), _random_side(rng, 1600, nc, max(200_000 // nc, 3000), 150)
    build[0][build[0] == 1] = 0                            # contig 1: the build side lacks it
    probe[0][::17] = -1                                    # a null chrom
    probe[0][5::29] = nc + 3                               # an id outside the dictionary
    build[0][::23] = -1
    build[0][7::31] = nc
    return dict(probe=probe, build=build, nc=nc, windows=[W(200, 500, 2), W(0, 0)])


def contigs_24():
    return _contigs(24)


def contigs_300():
    return _contigs(300)


def degenerate():
    """Zero-length and inverted rows on both sides; no probes; no build rows."""
    rng = np.random.default_rng(3)
    rp, rb = _random_side(rng, 300, 2, 3000, 40), _random_side(rng, 300, 2, 3000, 40)
    planted_p = side([(10, 10), (20, 12), (10, 20), (30, 30), (2999, 2990)])
    planted_b = side([(10, 10), (25, 15), (20, 30), (15, 15), (21, 21), (9, 5)])
    probe = tuple(np.concatenate([planted_p[k], rp[k]]) for k in range(3))
    build = tuple(np.concatenate([planted_b[k], rb[k]]) for k in range(3))
    none = tuple(np.empty(0, np.int32) for _ in range(3))
    ws = [W(0, 0), W(30, 30), W(30, 30, 1)]
    return [dict(probe=probe, build=build, nc=2, windows=ws), dict(probe=none, build=build, nc=2, windows=ws),
            dict(probe=probe, build=none, nc=2, windows=ws)]


def random_2000():
    rng = np.random.default_rng(2000)
    probe, build = _random_side(rng, 2000, 3, 150_000, 300), _random_side(rng, 2000, 3, 150_000, 300)
    ws = [W(int(rng.integers(0, 3000)), int(rng.integers(0, 3000)), int(rng.integers(0, 200))) for _ in range(3)]
    ws.append(W(min_distance=int(rng.integers(0, 100)), probe_left=rng.integers(0, 4000, 2000).astype(np.uint32),
                probe_right=rng.integers(0, 4000, 2000).astype(np.uint32)))
    return dict(probe=probe, build=build, nc=3, windows=ws)


SHAPES = {f.__name__: f for f in (small_edges, asymmetric, min_distance, int32_limits, tile_edges, chunks, long_row, contigs_24, contigs_300,
                                  degenerate, random_2000)}


def cases(name):
    """The (probe, build, nc, window) cases of a shape, flattened."""
    got = SHAPES[name]()
    out = []
    for g in (got if isinstance(got, list) else [got]):
        probes = g["probe"] if isinstance(g["probe"], list) else [g["probe"]]
        for p in probes:
            for w in g["windows"]:
                if w["probe_left"] is not None and len(w["probe_left"]) != len(p[0]):
                    continue
                out.append((p, g["build"], g["nc"], w))
    return out


def no_empty_rows(seed, n_probe, n_build, nc, span=80_000):
    """Random sides in which every row covers a position in both modes (for the comparisons with nearest)."""
    rng = np.random.default_rng(seed)
    return _random_side(rng, n_probe, nc, span, 200, empty=False), _random_side(rng, n_build, nc, span, 200, empty=False)
