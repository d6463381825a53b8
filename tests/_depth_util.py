"""Expected values of depth (run-length coverage blocks) without the engine, and the shapes its tests share.

Two independent numpy forms of the same definition -- the maximal runs of positions covered by the same number (>= 1) of
rows, per contig, Strict rows covering [start, end) and Weak rows [start, end]; blocks in the mode's own convention:

  depth_dense   (a) a difference array over the coordinate span (np.add.at +-1, cumsum, run-length encode): small spans only
  depth_events  (b) an event sort over the unique positions in int64: works at the int32 limits

Both return (contig, start, end, depth) int64 arrays in (contig, start) order."""
import numpy as np

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1

# merged-sequence tile of the kernel: DP_TILE = DP_THREADS * DP_ITEMS in polars-bio_amd/csrc/depth.hip.h (starts + ends per
# workgroup); a frame of n rows is 2 n events
T = 2048


def _covering(contig, start, end, strict, n_contigs):
    c, s, e = (np.asarray(a).astype(np.int64) for a in (contig, start, end))
    e1 = e if strict else e + 1                      # half-open end
    keep = (c >= 0) & (c < n_contigs) & (s < e1)
    return c[keep], s[keep], e1[keep]


def _out(c, s, e1, d, strict):
    cols = [np.asarray(x, np.int64) for x in (c, s, e1, d)]
    if not strict:
        cols[2] = cols[2] - 1
    return tuple(cols)


def depth_dense(contig, start, end, strict, n_contigs):
    c, s, e1 = _covering(contig, start, end, strict, n_contigs)
    oc, os_, oe, od = [], [], [], []
    for ct in np.unique(c):
        m = c == ct
        lo, hi = int(s[m].min()), int(e1[m].max())
        assert hi - lo < 50_000_000, "depth_dense is for small spans"
        diff = np.zeros(hi - lo + 2, np.int64)
        np.add.at(diff, s[m] - lo, 1)
        np.add.at(diff, e1[m] - lo, -1)
        per_base = np.cumsum(diff)[:hi - lo]         # depth of position lo + k
        if per_base.size == 0:
            continue
        edge = np.flatnonzero(np.diff(per_base)) + 1
        first = np.concatenate([[0], edge])
        last = np.concatenate([edge, [per_base.size]])
        dd = per_base[first]
        nz = dd != 0
        oc.append(np.full(int(nz.sum()), ct)); os_.append(first[nz] + lo); oe.append(last[nz] + lo); od.append(dd[nz])
    if not oc:
        return _out([], [], [], [], strict)
    return _out(np.concatenate(oc), np.concatenate(os_), np.concatenate(oe), np.concatenate(od), strict)


def depth_events(contig, start, end, strict, n_contigs):
    c, s, e1 = _covering(contig, start, end, strict, n_contigs)
    if c.size == 0:
        return _out([], [], [], [], strict)
    span = np.int64(1) << 34
    key = np.concatenate([c * span + (s - I32_MIN), c * span + (e1 - I32_MIN)])
    delta = np.concatenate([np.ones(c.size, np.int64), -np.ones(c.size, np.int64)])
    pos, inv = np.unique(key, return_inverse=True)
    net = np.zeros(pos.size, np.int64)
    np.add.at(net, inv, delta)
    after = np.cumsum(net)
    before = after - net
    assert (after >= 0).all()
    b = np.flatnonzero(net != 0)                      # boundaries: the depth changes
    opens = b[after[b] != 0]
    closes = b[before[b] != 0]
    assert opens.size == closes.size
    return _out(pos[opens] // span, pos[opens] % span + I32_MIN, pos[closes] % span + I32_MIN, after[opens], strict)


def as_i32(*cols):
    return tuple(np.ascontiguousarray(a, np.int32) for a in cols)


def random_rows(rng, n, n_contigs, span, max_len=50):
    c = rng.integers(0, max(n_contigs, 1), n)
    s = rng.integers(0, max(span, 1), n)
    return as_i32(c, s, s + rng.integers(1, max_len + 1, n))


# ---- the shapes: name -> builder(strict) -> (contig, start, end, n_contigs) ------------------------------------------------------

def _tile_rows(n):
    def build(strict):
        rng = np.random.default_rng(1000 + n)
        return (*random_rows(rng, n, 3, max(n // 2, 4)), 3)
    return build


def _long_group(lead):
    """1.5 T rows that start at X, 1.5 T rows whose half-open end is X (netting across tile edges and across the two streams),
    behind `lead` rows at smaller positions so that the group begins mid-tile."""
    def build(strict):
        m, X = 3 * T // 2, 5000
        j = np.arange(m)
        ls = np.arange(lead) * 2
        s = np.concatenate([ls, X - 100 - j % 50, np.full(m, X)])
        e = np.concatenate([ls + 3, np.full(m, X), X + 1 + j % 70])
        if not strict:
            e = e - 1                                 # the same positions covered, closed
        return (*as_i32(np.zeros(s.size), s, e), 1)
    return build


def _contig_edge(k):
    """contig 0 holds k rows (2 k events: k = T / 2 puts the contig boundary on a tile edge), contig 1 one row, contig 2 none,
    contig 3 a random lot, contig 4 (the last) none"""
    def build(strict):
        rng = np.random.default_rng(k)
        c0 = random_rows(rng, k, 1, 300)
        c3 = random_rows(rng, T // 2 + 1, 1, 300)
        c = np.concatenate([c0[0], [1], c3[0] + 3])
        s = np.concatenate([c0[1], [7], c3[1]])
        e = np.concatenate([c0[2], [9], c3[2]])
        o = rng.permutation(c.size)
        return (*as_i32(c[o], s[o], e[o]), 5)
    return build


def _identical(strict):
    n = 5000
    return (*as_i32(np.full(n, 1), np.full(n, 100), np.full(n, 200)), 2)


def _nested(strict):
    n = 3000                                          # depth climbs to n and falls back, one step per position
    i = np.arange(n)
    return (*as_i32(np.zeros(n), i, 2 * n + 5 - i), 1)


def _staircase(strict):
    n = 1500
    i = np.arange(n)
    return (*as_i32(i % 2, 3 * i, 3 * i + 40), 2)


def _chain(strict):
    n = 50_000                                        # bookended: every row ends where the next one starts
    i = np.arange(n // 2)
    s = np.concatenate([10 * i, 10 * i + 3])
    e = s + (10 if strict else 9)
    return (*as_i32(np.repeat([0, 1], n // 2), s, e), 2)


def _degenerate(strict):
    rng = np.random.default_rng(77)
    c, s, e = random_rows(rng, 3000, 4, 900)
    kind = rng.integers(0, 4, c.size)
    e = np.where(kind == 0, s, e)                     # zero-length (Strict) / one position (Weak)
    e = np.where(kind == 1, s - rng.integers(1, 30, c.size), e)     # inverted
    return (*as_i32(c, s, e), 4)


def _zero_length_only(strict):
    rng = np.random.default_rng(78)
    c, s, e = random_rows(rng, 2500, 3, 700)
    e = np.where(rng.integers(0, 3, c.size) == 0, s - (0 if strict else 1), e)      # rows that cover nothing, none with start > end + 1
    return (*as_i32(c, s, e), 3)


def _outside_dictionary(strict):
    rng = np.random.default_rng(79)
    c, s, e = random_rows(rng, 4000, 6, 1200)
    c = np.where(rng.integers(0, 5, c.size) == 0, -1, c)
    c = np.where(rng.integers(0, 5, c.size) == 0, rng.integers(4, 40, c.size), c)   # n_contigs = 4: ids 4 .. 39 are outside
    return (*as_i32(c, s, e), 4)


def _many_contigs(strict):
    rng = np.random.default_rng(80)
    c = np.repeat(np.arange(300), 3)
    s = rng.integers(0, 40, c.size)
    o = rng.permutation(c.size)
    return (*as_i32(c[o], s[o], s[o] + rng.integers(1, 30, c.size)), 300)


def _limits(strict):
    rows = [(0, I32_MIN, I32_MAX), (0, I32_MIN, 0), (0, 5, I32_MAX), (0, I32_MAX - 3, I32_MAX), (0, I32_MIN, I32_MIN + 1),
            (1, I32_MAX, I32_MAX), (1, I32_MAX - 1, I32_MAX), (1, I32_MIN, I32_MIN), (2, I32_MIN, I32_MAX), (2, I32_MIN, I32_MAX),
            (2, -1, 1)]
    c, s, e = (np.array(x) for x in zip(*rows))
    return (*as_i32(c, s, e), 3)


SHAPES = {f"rows_{n}": _tile_rows(n) for n in (0, 1, 2, T // 2 - 1, T // 2, T // 2 + 1, T, T + 1, 3 * T // 2 + 1)}
SHAPES.update({
    "long_group_mid_tile": _long_group(500), "long_group_at_start": _long_group(0),
    "contig_edge_minus": _contig_edge(T // 2 - 1), "contig_edge": _contig_edge(T // 2), "contig_edge_plus": _contig_edge(T // 2 + 1),
    "identical": _identical, "nested_thousands": _nested, "staircase": _staircase, "bookended_chain": _chain,
    "degenerate_mixed": _degenerate, "zero_length": _zero_length_only, "outside_dictionary": _outside_dictionary,
    "contigs_300x3": _many_contigs, "int32_limits": _limits,
})
SMALL_SPAN = [k for k in SHAPES if k != "int32_limits"]           # what depth_dense can hold


def sweep_case(seed):
    """one case of the randomised sweep: size 1 .. 60 000, a span small enough that ties are common, a random mode"""
    rng = np.random.default_rng(5000 + seed)
    n = int(rng.integers(1, 60_001))
    nc = int(rng.integers(1, 9))
    strict = bool(rng.integers(0, 2))
    c, s, e = random_rows(rng, n, nc, max(n // int(rng.integers(2, 40)), 3), max_len=int(rng.integers(1, 200)))
    return c, s, e, nc, strict


def assert_blocks_equal(got, exp, what=""):
    got = tuple(np.asarray(a).astype(np.int64) for a in got)
    assert len(got[0]) == len(exp[0]), f"{what}: {len(got[0])} blocks, expected {len(exp[0])}"
    for name, g, x in zip(("contig", "start", "end", "depth"), got, exp):
        bad = np.flatnonzero(g != x)
        assert bad.size == 0, f"{what}: {name} differs first at block {bad[0]}: {g[bad[0]]} != {x[bad[0]]}"
