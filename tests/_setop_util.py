"""Expected values of the set operations on two interval frames without the engine, and the shapes their tests share.

U(F) = the (contig, position) pairs at least one row of F covers: Strict rows cover [start, end), Weak rows [start, end]; rows
that cover nothing and rows outside the dictionary [0, n_contigs) contribute nothing.  An operation returns the maximal runs of
op(U(A), U(B)) in (contig, start) order, bounds in the mode's own convention.  Two independent numpy forms:

  setop_dense   (a) one boolean array per contig and side over the coordinate span, combined with & | &~ ^, run-length
                    encoded: small spans only
  setop_events  (b) union runs of each side by a sort + running maximum, then an int64 event sort over the run boundaries with
                    an XOR of the two membership bits: works at the int32 limits

Both return ((contig, start, end) int64 arrays, (only_a, only_b, both) position totals as Python ints)."""
import numpy as np

I32_MIN, I32_MAX = -(2 ** 31), 2 ** 31 - 1

# merged-sequence tile of the kernel: SO_TILE = SO_THREADS * SO_ITEMS in polars-bio_amd/csrc/setop.hip.h (boundary events per
# workgroup); after the union step the sides hold 2 * runs(A) + 2 * runs(B) events
T = 2048
ITEMS = 8

OPS = ("intersection", "union", "difference", "symmetric_difference")
# membership of the state in-A | in-B << 1 in the result
_TABLE = {"intersection": (0, 0, 0, 1), "union": (0, 1, 1, 1), "difference": (0, 1, 0, 0), "symmetric_difference": (0, 1, 1, 0)}
_SPAN = np.int64(1) << 34


def _covering(side, strict, n_contigs):
    c, s, e = (np.asarray(a).astype(np.int64) for a in side)
    e1 = e if strict else e + 1                      # half-open end
    keep = (c >= 0) & (c < n_contigs) & (s < e1)
    return c[keep], s[keep], e1[keep]


def _out(c, s, e1, strict):
    cols = [np.asarray(x, np.int64).reshape(-1) for x in (c, s, e1)]
    if not strict:
        cols[2] = cols[2] - 1
    return tuple(cols)


def union_runs(side, strict, n_contigs):
    """maximal runs of U(side) -> (contig, start, half-open end) int64, (contig, start) order; rows that touch are one run"""
    c, s, e1 = _covering(side, strict, n_contigs)
    if c.size == 0:
        z = np.empty(0, np.int64)
        return z, z, z
    ks, ke = c * _SPAN + (s - I32_MIN), c * _SPAN + (e1 - I32_MIN)
    o = np.argsort(ks, kind="stable")
    ks, ke = ks[o], ke[o]
    reach = np.maximum.accumulate(ke)
    first = np.concatenate([[True], ks[1:] > reach[:-1]])
    idx = np.flatnonzero(first)
    last = np.concatenate([idx[1:] - 1, [ks.size - 1]])
    return ks[idx] // _SPAN, ks[idx] % _SPAN + I32_MIN, reach[last] % _SPAN + I32_MIN


def union_rows(side, strict, n_contigs):
    """the union runs of a side as int32 rows in the mode's own convention (probe rows of a cross-check)"""
    return as_i32(*_out(*union_runs(side, strict, n_contigs), strict))


def n_events(a, b, strict, n_contigs):
    return 2 * len(union_runs(a, strict, n_contigs)[0]) + 2 * len(union_runs(b, strict, n_contigs)[0])


def setop_events(a, b, strict, n_contigs, op):
    ra, rb = union_runs(a, strict, n_contigs), union_runs(b, strict, n_contigs)
    keys, bits = [], []
    for (c, s, e1), bit in ((ra, 1), (rb, 2)):
        keys += [c * _SPAN + (s - I32_MIN), c * _SPAN + (e1 - I32_MIN)]
        bits += [np.full(2 * c.size, bit, np.int64)]
    key, bit = np.concatenate(keys), np.concatenate(bits)
    if key.size == 0:
        return _out([], [], [], strict), (0, 0, 0)
    pos, inv = np.unique(key, return_inverse=True)
    net = np.zeros(pos.size, np.int64)
    np.bitwise_xor.at(net, inv, bit)
    after = np.bitwise_xor.accumulate(net)
    before = after ^ net
    assert after[-1] == 0
    f = np.array(_TABLE[op], bool)
    opens = np.flatnonzero(~f[before] & f[after])
    closes = np.flatnonzero(f[before] & ~f[after])
    assert opens.size == closes.size
    p = pos % _SPAN
    totals = tuple(int(p[(before == k) & (after != k)].sum()) - int(p[(after == k) & (before != k)].sum()) for k in (1, 2, 3))
    return _out(pos[opens] // _SPAN, p[opens] + I32_MIN, p[closes] + I32_MIN, strict), totals


def setop_dense(a, b, strict, n_contigs, op):
    ca, sa, ea = _covering(a, strict, n_contigs)
    cb, sb, eb = _covering(b, strict, n_contigs)
    oc, os_, oe = [], [], []
    totals = [0, 0, 0]
    for ct in np.unique(np.concatenate([ca, cb])):
        ma, mb = ca == ct, cb == ct
        lo = int(min(sa[ma].min(initial=2 ** 40), sb[mb].min(initial=2 ** 40)))
        hi = int(max(ea[ma].max(initial=-2 ** 40), eb[mb].max(initial=-2 ** 40)))
        assert hi - lo < 50_000_000, "setop_dense is for small spans"
        masks = []
        for s, e1, m in ((sa, ea, ma), (sb, eb, mb)):
            diff = np.zeros(hi - lo + 1, np.int64)
            np.add.at(diff, s[m] - lo, 1)
            np.add.at(diff, e1[m] - lo, -1)
            masks.append(np.cumsum(diff)[:hi - lo] > 0)
        ua, ub = masks
        totals[0] += int((ua & ~ub).sum()); totals[1] += int((ub & ~ua).sum()); totals[2] += int((ua & ub).sum())
        r = {"intersection": ua & ub, "union": ua | ub, "difference": ua & ~ub, "symmetric_difference": ua ^ ub}[op]
        edge = np.diff(np.concatenate([[False], r, [False]]).astype(np.int8))
        st, en = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
        oc.append(np.full(st.size, ct)); os_.append(st + lo); oe.append(en + lo)
    if not oc:
        return _out([], [], [], strict), (0, 0, 0)
    return _out(np.concatenate(oc), np.concatenate(os_), np.concatenate(oe), strict), tuple(totals)


def as_i32(*cols):
    return tuple(np.ascontiguousarray(a, np.int32) for a in cols)


EMPTY = as_i32([], [], [])


def side(c, s, e1, strict):
    """rows given with half-open ends -> the same positions in the mode's convention"""
    c, s, e1 = (np.asarray(x, np.int64).reshape(-1) for x in (c, s, e1))
    return as_i32(c, s, e1 if strict else e1 - 1)


def random_rows(rng, n, n_contigs, span, max_len=50):
    c = rng.integers(0, max(n_contigs, 1), n)
    s = rng.integers(0, max(span, 1), n)
    return as_i32(c, s, s + rng.integers(1, max_len + 1, n))


def separate_runs(rng, k, contig=0, origin=0):
    """k rows of one contig that are k runs: row i lies inside [20 i, 20 i + 13) (+ origin); few distinct offsets, so two
    sides built this way tie often"""
    i = np.arange(k, dtype=np.int64)
    s = origin + 20 * i + rng.integers(0, 4, k)
    return np.full(k, contig, np.int64), s, s + rng.integers(1, 10, k)


def cat(*sides):
    return tuple(np.concatenate([x[k] for x in sides]) for k in range(3))


# ---- the shapes: name -> builder(strict) -> (a, b, n_contigs), a / b = (contig, start, end) int32 ------------------------------------

def _events(total, runs_a=None):
    """total boundary events: runs_a runs in A (default: half of them), the rest in B"""
    def build(strict):
        rng = np.random.default_rng(3000 + total)
        runs = total // 2
        ka = runs // 2 if runs_a is None else runs_a
        return side(*separate_runs(rng, ka), strict), side(*separate_runs(rng, runs - ka), strict), 1
    return build


def _empty(which):
    def build(strict):
        rng = np.random.default_rng(3100)
        rows = side(*separate_runs(rng, 700), strict)
        return (EMPTY if "a" in which else rows), (EMPTY if "b" in which else rows), 2
    return build


def _identical(strict):
    rows = side(*separate_runs(np.random.default_rng(3200), T // 2 + 37), strict)
    return rows, tuple(x.copy() for x in rows), 1


def _tie_split(lead):
    """`lead` runs of A alone, then A = [X, X + 5) and B = [X + 5, X + 9): the stream-1 event X + 5 is merged event
    2 lead + 1 and the equal stream-2 event is 2 lead + 2 -- lead = T / 2 - 1 splits the pair over a tile edge, lead = 3 over a
    thread's edge.  More runs follow on both sides."""
    def build(strict):
        rng = np.random.default_rng(3300 + lead)
        X = 20 * lead + 40
        tail_a, tail_b = separate_runs(rng, 300, origin=X + 100), separate_runs(rng, 300, origin=X + 100)
        a = cat(separate_runs(rng, lead), ([0], [X], [X + 5]), tail_a)
        b = cat(([0], [X + 5], [X + 9]), tail_b)
        return side(*a, strict), side(*b, strict), 1
    return build


def _wide_run(strict):
    rng = np.random.default_rng(3400)
    b = separate_runs(rng, 2 * T, origin=100)
    return side([0], [0], [20 * 2 * T + 500], strict), side(*b, strict), 1


def _chains(strict):
    i = np.arange(3000, dtype=np.int64)
    c = np.concatenate([np.zeros(1500, np.int64), np.ones(1500, np.int64)])
    return side(c, 10 * i, 10 * i + 5, strict), side(c, 10 * i + 5, 10 * i + 10, strict), 2


def _contig_layout(strict):
    """contig 0 both, 1 A only, 2 B only, 3 neither, 4 both, 5 neither, 6 (the last) B only"""
    rng = np.random.default_rng(3500)
    a = cat(*(separate_runs(rng, 400, contig=c) for c in (0, 1, 4)))
    b = cat(*(separate_runs(rng, 400, contig=c) for c in (0, 2, 4, 6)))
    oa, ob = rng.permutation(a[0].size), rng.permutation(b[0].size)
    return side(*(x[oa] for x in a), strict), side(*(x[ob] for x in b), strict), 7


def _contig_edge(strict):
    """contig 0 holds exactly T events (T / 4 runs a side): the contig boundary lies on a tile edge"""
    rng = np.random.default_rng(3600)
    a = cat(separate_runs(rng, T // 4, contig=0), separate_runs(rng, 333, contig=1))
    b = cat(separate_runs(rng, T // 4, contig=0), separate_runs(rng, 444, contig=1))
    return side(*a, strict), side(*b, strict), 3


def _many_contigs(strict):
    rng = np.random.default_rng(3700)
    def rows():
        c = np.repeat(np.arange(300), 3)
        s = rng.integers(0, 40, c.size)
        o = rng.permutation(c.size)
        return side(c[o], s[o], s[o] + rng.integers(1, 30, c.size), strict)
    return rows(), rows(), 300


def _degenerate(strict):
    def rows(seed):
        rng = np.random.default_rng(seed)
        c, s, e = random_rows(rng, 3000, 6, 900)
        kind = rng.integers(0, 6, c.size)
        e = np.where(kind == 0, s - (0 if strict else 1), e)            # zero-length: covers nothing
        e = np.where(kind == 1, s - rng.integers(2, 30, c.size), e)     # inverted (the index is built again without them)
        c = np.where(kind == 2, -1, c)
        c = np.where(kind == 3, rng.integers(4, 40, c.size), c)         # n_contigs = 4: ids 4 .. 39 are outside
        return as_i32(c, s, e)
    return rows(3801), rows(3802), 4


def _nothing_side(strict):
    rng = np.random.default_rng(3900)
    a = random_rows(rng, 2000, 3, 700)
    c, s, e = random_rows(rng, 1500, 3, 700)
    kind = rng.integers(0, 3, c.size)
    e = np.where(kind == 0, s - (0 if strict else 1), s - 5)            # zero-length or inverted
    c = np.where(kind == 2, -1, c)
    return a, as_i32(c, s, e), 3


def _limits(strict):
    a = [(0, I32_MIN, I32_MAX), (1, I32_MAX - 1, I32_MAX), (2, I32_MIN, I32_MIN + 1), (3, I32_MIN, I32_MAX), (4, I32_MIN, 0)]
    b = [(0, I32_MAX - 1, I32_MAX), (0, I32_MIN, I32_MIN + 1), (1, I32_MIN, I32_MAX), (2, I32_MIN, I32_MAX), (4, 0, I32_MAX),
         (4, -5, 5)]
    if not strict:
        b.append((3, I32_MAX, I32_MAX))                                 # one position, the last one, against a contig-wide row
    return as_i32(*zip(*a)), as_i32(*zip(*b)), 5


SHAPES = {"empty_a": _empty("a"), "empty_b": _empty("b"), "empty_both": _empty("ab"), "events_2": _events(2, 1)}
SHAPES.update({f"events_{n}": _events(n) for n in (T - 2, T, T + 2, 2 * T + 2)})
SHAPES.update({
    "events_unequal": _events(3 * T // 2 + 2, 3), "identical": _identical,
    "tie_on_tile_edge": _tie_split(T // 2 - 1), "tie_on_thread_edge": _tie_split(3), "tie_on_thread_edge_tile_1": _tie_split(T // 2 + 3),
    "wide_run": _wide_run, "bookended_chains": _chains, "contig_layout": _contig_layout, "contig_on_tile_edge": _contig_edge,
    "contigs_300x3": _many_contigs, "degenerate_mixed": _degenerate, "nothing_side": _nothing_side, "int32_limits": _limits,
})
SMALL_SPAN = [k for k in SHAPES if k != "int32_limits"]           # what setop_dense can hold


def sweep_case(seed):
    """one case of the randomised sweep: 1 .. 30 000 rows a side, spans small enough that ties are common"""
    rng = np.random.default_rng(7000 + seed)
    nc = int(rng.integers(1, 9))
    strict = bool(rng.integers(0, 2))
    op = OPS[int(rng.integers(0, 4))]
    sides = []
    for _ in range(2):
        n = int(rng.integers(1, 30_001))
        sides.append(random_rows(rng, n, nc, max(n * int(rng.integers(2, 30)), 3), max_len=int(rng.integers(1, 40))))
    return sides[0], sides[1], nc, strict, op


def assert_regions_equal(got, exp, what=""):
    got = tuple(np.asarray(a).astype(np.int64) for a in got)
    assert len(got[0]) == len(exp[0]), f"{what}: {len(got[0])} regions, expected {len(exp[0])}"
    for name, g, x in zip(("contig", "start", "end"), got, exp):
        bad = np.flatnonzero(g != x)
        assert bad.size == 0, f"{what}: {name} differs first at region {bad[0]}: {g[bad[0]]} != {x[bad[0]]}"
