"""Inputs, references and runners of tests/test_permutation_matrix.py (test helper).  Every generator takes the sizes as arguments, so
that the CPU group runs a scaled-down copy of exactly the recipe the GPU tests run.  Numbers come from numpy and from the constants
of the kernel's headers, never from the code under test."""
import os
import re

import numpy as np

import _join_ops_util as J
import _limits
import _map_select_util as S
import _permutation_util as U
import _position_ops_util as P
from test_permutation_gpu import _frames, _offsets

I32 = np.int32
BRUTE_MAX = 400_000                    # (df1 rows x permutations) up to which the literal brute force is the reference
TILE, WAVE_ROWS, BLOCK, CHUNK = U.kernel_geometry()
CSRC = os.path.join(U.ROOT, "polars-bio_amd", "csrc")
MAXI = 2 ** 31 - 1


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def scan_tile():
    """rows per tile of device_scan (scan.hip.h), read the way kernel_geometry() reads the permutation kernel's constants"""
    src = _src("scan.hip.h")
    get = lambda name: int(re.search(rf"constexpr int {name}\s*=\s*(\d+)", src).group(1))
    assert "SCAN_TILE = SCAN_THREADS * SCAN_ITEMS" in src
    return get("SCAN_THREADS") * get("SCAN_ITEMS")


def partial_bytes():
    """PERM_PARTIAL_BYTES of host_permute.hip.h"""
    m = re.search(r"PERM_PARTIAL_BYTES\s*=\s*\(size_t\)(\d+)\s*<<\s*(\d+)", _src("host_permute.hip.h"))
    return int(m.group(1)) << int(m.group(2))


def per_launch(n_rows, n_perm):
    """permutations per launch as permute_plan computes them"""
    tiles = (n_rows + TILE - 1) // TILE
    per = partial_bytes() // (tiles * 16) // BLOCK * BLOCK
    return min(max(per, BLOCK), CHUNK, n_perm)


def piece_rows(nc, n_perm):
    """permutations per offset piece of the host entry (ivjoin.hip, ivj_permute_overlaps)"""
    assert "((size_t)64 << 20) / row_bytes" in _src("ivjoin.hip")
    return min(max((64 << 20) // (4 * nc), 1), n_perm)


def contig_shift(build, c, bins_per_row=2):
    """the joint grid's shift of contig c by k_contig_meta_joint's formula (index_build.hip.h), keys in the frame's coordinates"""
    on = np.asarray(build[0]) == c
    s, e = np.asarray(build[1], np.int64)[on], np.asarray(build[2], np.int64)[on]
    if len(s) == 0:
        return 0
    span = max(s.max(), e.max()) - min(s.min(), e.min())
    cap = max(bins_per_row * len(s), 2)
    shift = 0
    while (span >> shift) + 1 > cap:
        shift += 1
    return shift


def no_position(build, strict):
    """perm_no_position of permute.hip.h on a whole side"""
    s, e = np.asarray(build[1], np.int64), np.asarray(build[2], np.int64)
    return s >= e if strict else s > e


def z_prefixes(build, strict):
    """(zs, ze): rows without a position before position p of the (contig, start) order / of the (contig, end) order, p = 0 .. n"""
    nop = no_position(build, strict)
    c = np.asarray(build[0], np.int64)
    out = []
    for key in (build[1], build[2]):
        order = np.lexsort((np.asarray(key, np.int64), c))
        out.append(np.concatenate([[0], np.cumsum(nop[order])]))
    return out[0], out[1], nop[np.lexsort((np.asarray(build[1], np.int64), c))]


def eligible(probe, nc, strict, lengths):
    one = 0 if strict else 1
    pc, ps, pe = (np.asarray(a, np.int64) for a in probe)
    inside = (pc >= 0) & (pc < nc)
    L = np.where(inside, np.asarray(lengths, np.int64)[np.clip(pc, 0, nc - 1)], 0)
    return inside & (0 <= ps - one) & (ps - one < pe) & (pe <= L)


class Case:
    def __init__(self, name, probe, build, nc, lengths, off, **note):
        as_i32 = lambda side: tuple(np.array(a, dtype=I32) for a in side)          # noqa: E731
        self.name, self.probe, self.build, self.nc = name, as_i32(probe), as_i32(build), int(nc)
        self.lengths = np.ascontiguousarray(lengths, dtype=I32)
        self.off = np.ascontiguousarray(off, dtype=I32).reshape(len(off), self.nc)
        self.note = note
        for a in self.probe + self.build + (self.lengths, self.off):
            a.setflags(write=False)

    @property
    def args(self):
        return self.probe, self.build, self.nc, self.lengths, self.off


_cases, _refs = {}, {}


def once(key, build):
    if key not in _cases:
        _cases[key] = build()
    return _cases[key]


def reference(case, strict, probe=None):
    """brute force up to BRUTE_MAX (rows x permutations), the rank identity above; ``probe``: the df1 rows to take instead of all"""
    p = case.probe if probe is None else probe
    fn = U.expected if len(p[0]) * len(case.off) <= BRUTE_MAX else U.ranks
    return fn(p, case.build, case.nc, strict, case.lengths, case.off)


def reference_once(case, strict):
    key = (case.name, bool(strict))
    if key not in _refs:
        _refs[key] = reference(case, strict)
    return _refs[key]


def assert_stats(got, exp, what):
    for k, stat in enumerate(("n_pairs", "n_rows")):
        g = np.asarray(got[k])
        assert g.dtype == np.int64 and g.shape == exp[k].shape, (what, stat, g.dtype, g.shape)
        bad = np.flatnonzero(g != exp[k])
        assert len(bad) == 0, f"{what}: {stat}: {len(bad)} permutations differ, first {bad[0]}: {g[bad[0]]} != {exp[k][bad[0]]}"


def blob(got):
    return b"|".join(np.ascontiguousarray(np.asarray(a)).tobytes() for a in got)


# ---- runners --------------------------------------------------------------------------------------------------------------------------

def dev_tables(case, shift=0):
    lengths, off = J.dev_cols([case.lengths, case.off.reshape(-1)], shift)
    return lengths, off.view(len(case.off), case.nc)


def run_host(eng, case, strict, **kw):
    return eng.permute_overlaps(case.probe, case.build, strict, case.nc, case.lengths, case.off, **kw)


def run_dev(dj, case, strict, probe_row_id=None, build_row_id=None, shift=0, index=None, **kw):
    dp, db = J.dev_side(case.probe, probe_row_id, shift), J.dev_side(case.build, build_row_id, shift)
    lengths, off = dev_tables(case, shift)
    pairs, rows = dj.permute_overlaps(dp, db, strict, case.nc, lengths, off, index=index, **kw)
    return pairs.cpu().numpy(), rows.cpu().numpy()


def check_both(eng, dj, case, strict, exp=None, what=None):
    exp = reference_once(case, strict) if exp is None else exp
    what = what or case.name
    got = {}
    if eng is not None:
        got["host"] = run_host(eng, case, strict)
        assert_stats(got["host"], exp, what + ": host entry")
    if dj is not None:
        got["device"] = run_dev(dj, case, strict)
        assert_stats(got["device"], exp, what + ": device entry")
    return exp, got


# ---- generators -------------------------------------------------------------------------------------------------------------------------

def _inside(rng, k, contigs, lengths, w, one):
    """k rows inside their contigs, which are drawn from ``contigs``"""
    lengths = np.asarray(lengths, np.int64)
    c = np.asarray(contigs, np.int64)[rng.integers(0, len(contigs), k)]
    ln = np.minimum(rng.integers(1, w + 1, k), lengths[c])
    hs = (rng.random(k) * (lengths[c] - ln + 1)).astype(np.int64)
    return c, hs + one, hs + ln


def _cat(*sides):
    return tuple(np.concatenate([np.asarray(s[k], np.int64) for s in sides]) for k in range(3))


def _shuffled(rng, side):
    o = rng.permutation(len(side[0]))
    return tuple(a[o] for a in side)


def _clip(side):
    return side[0], np.clip(side[1], -2 ** 31, MAXI), np.clip(side[2], -2 ** 31, MAXI)


Z_LEN = [60_000, 20_000, 777, 90_000]


def z_case(strict, m, n=2 * TILE + 3, n_perm=9, share=0.4):
    """Z: m df2 rows, ``share`` of them without a position -- dense in the first third of contig 0, absent from contig 1, dense at
    the end of the last contig; every second one inverted by 25 000 positions or more, so that it sorts far earlier by end than by
    start (on contig 0, which holds most of the other rows, ahead of every row that covers a position)"""
    def build():
        rng = np.random.default_rng(7000 + m)
        one = 0 if strict else 1
        probe, _ = _frames(rng, n, 0, 4, Z_LEN, strict, width=3000)
        k = int(m * share)
        k0 = k // 2
        good = _inside(rng, m - k, [0] * 7 + [1, 2, 3], Z_LEN, 4000, one)
        hs = np.concatenate([rng.integers(16_000, Z_LEN[0] // 3, k0), Z_LEN[3] - 1 - rng.integers(0, Z_LEN[3] // 20, k - k0)])
        d = np.where(np.arange(k) % 2 == 1, rng.integers(25_000, 40_000, k), 0)
        bad = (np.concatenate([np.zeros(k0, np.int64), np.full(k - k0, 3)]), hs + one, hs - d)
        return Case(f"z_{m}_{n}_{strict}", probe, _shuffled(rng, _cat(good, bad)), 4, Z_LEN, _offsets(rng, n_perm, Z_LEN))
    return once(("z", strict, m, n, n_perm, share), build)


def z_edge_case(strict, which, m=3000, n=2 * TILE + 3, n_perm=9):
    """Z: exactly one df2 row without a position -- the last row of the start order (entry n of the prefix arrays), or the first"""
    def build():
        rng = np.random.default_rng(7100 + m + len(which))
        one = 0 if strict else 1
        probe, _ = _frames(rng, n, 0, 4, Z_LEN, strict, width=3000)
        good = _inside(rng, m - 1, [0, 1, 2, 3], [Z_LEN[0], Z_LEN[1], Z_LEN[2], Z_LEN[3] - 100], 4000, one)
        if which == "last":                                  # above every start of the last contig, still inside it: wrapped pieces end above it
            bad = ([3], [Z_LEN[3] - 50 + one], [Z_LEN[3] - 59])
        else:
            bad = ([0], [-5], [-9])
        return Case(f"z_{which}_{m}_{n}_{strict}", probe, _shuffled(rng, _cat(good, bad)), 4, Z_LEN, _offsets(rng, n_perm, Z_LEN))
    return once(("z_edge", strict, which, m, n, n_perm), build)


def o_case(strict, L, n, m, n_perm=12, width=300, bwidth=200):
    """O: contig 0 of length L (contig 1: 1000), df2 rows across either end of contig 0, across both, entirely outside it, and limit rows"""
    def build():
        rng = np.random.default_rng(7200 + L % 9973 + n)
        one = 0 if strict else 1
        lengths = [L, 1000]
        probe, build = _frames(rng, n, m, 2, lengths, strict, width=width, bwidth=bwidth)
        build = _limits.embed(build, _limits.limit_rows(rng, max(10, m // 10), 2), rng)
        lo = -2 ** 31 + 1
        half_open = [(-50, 10), (-1, 1), (lo, 5), (L - 10, L + 50), (L - 1, L + 1), (-100, L + 100), (lo, MAXI), (-500, -3), (lo, lo + 5), (-1, 0),
                     (L, L + 40), (L + 5, L + 6)]
        hs, he = np.array(half_open, np.int64).T
        planted = _clip((np.zeros(len(hs), np.int64), hs + one, he))
        build = _shuffled(rng, _cat(build, planted, planted))
        off = _offsets(rng, n_perm, lengths)
        off[0], off[1], off[2] = 0, 1 % 1000, [L - 1, 999]
        # two df1 rows of contig 0: an offset that ends the row exactly at L (one piece), and one more that leaves [0, 1) as its second piece
        ok = np.flatnonzero(eligible(probe, 2, strict, lengths) & (probe[0] == 0) & (probe[2].astype(np.int64) - probe[1] + one >= 2))
        i, j = int(ok[0]), int(ok[1])
        ends_at = lambda r, e: (e - int(probe[2][r])) % L     # noqa: E731  (s' + len == e  <=>  off == e - he  mod L)
        off[3, 0], off[4, 0] = ends_at(i, L), ends_at(j, L + 1)
        off[1, 0] = 1 % L
        return Case(f"o_{L}_{n}_{strict}", probe, build, 2, lengths, off, ends_at_L=(i, 3), second_piece_0_1=(j, 4), planted=half_open)
    return once(("o", strict, L, n, m, n_perm, width, bwidth), build)


R1_L, R1_X, R1_Y = 200_000, 190_000, 199_000


def r1_case(strict, cluster=3000, n=900, background=300, second=200):
    """R1: the last `cluster` rows of contig 0's start order share the start X; the last `cluster` of its end order but one share the
    end Y (the one row after them ends at L, so that targets just above Y lie inside the grid and are searched); contig 1 follows
    directly with coordinates below both"""
    def build():
        rng = np.random.default_rng(7300 + cluster)
        one = 0 if strict else 1
        lengths = [R1_L, 20_000]
        xs = (np.zeros(cluster, np.int64), np.full(cluster, R1_X + one), R1_X + rng.integers(1, 5001, cluster))
        ys = (np.zeros(cluster, np.int64), 150_000 + rng.integers(0, 40_000, cluster) + one, np.full(cluster, R1_Y))
        back = _inside(rng, background, [0], [149_000], 200, one)
        # one row that ends at L: it lifts the grid's upper edge above Y (a target above the edge takes the segment's end without
        # a search), and is the only row after the Y cluster in the end order
        # ... and one row at position 0, which fixes the grid's lower edge and with it the clusters' places inside their bins
        back = _cat(back, ([0, 0], [170_000 + one, one], [R1_L, 50]))
        other =_inside(rng, second, [1], [0, 5000], 300, one)
        k = n // 8
        near_x = (np.zeros(k, np.int64), R1_X - rng.integers(1, 300, k) + one, R1_X + rng.integers(1, 17, k))      # ends just above X
        dy = np.where(np.arange(k) % 3 == 0, rng.integers(0, 2, k), rng.integers(0, 17, k))     # (a third at Y and Y + 1: the cluster's own bin)
        near_y = (np.zeros(k, np.int64), R1_Y + dy + one, R1_Y + 17 + rng.integers(1, 300, k))                       # starts at / just above Y
        rest = _inside(rng, n - 2 * k, [0, 0, 1], lengths, 400, one)
        off = _offsets(rng, 8, lengths)
        off[0] = 0
        return Case(f"r1_{cluster}_{n}_{strict}", _shuffled(rng, _cat(near_x, near_y, rest)), _shuffled(rng, _cat(xs, ys, back, other)), 2, lengths, off)
    return once(("r1", strict, cluster, n, background, second), build)


R2_MID = 2 ** 30


def r2_case(strict, window_rows=5000, n=800, side_rows=300):
    """R2: contig 1 of length 2^31 - 1 with one df2 row near 0, one near L and `window_rows` inside 1000 positions around 2^30 (a grid
    wider than 2^16 per bin); populated contigs before and after it"""
    def build():
        rng = np.random.default_rng(7400 + window_rows)
        one = 0 if strict else 1
        L = MAXI
        lengths = [10_000, L, 10_000]
        ws = R2_MID - 500 + rng.integers(0, 990, window_rows)
        window = (np.ones(window_rows, np.int64), ws + one, np.minimum(ws + rng.integers(1, 200, window_rows), R2_MID + 500))
        ends = (np.ones(2, np.int64), np.array([5, L - 20]) + one, np.array([9, L - 3]))
        sides = _inside(rng, 2 * side_rows, [0, 2], lengths, 300, one)
        k = n // 8
        ps = R2_MID - 2000 + rng.integers(0, 4000, 5 * k)
        near = (np.ones(5 * k, np.int64), ps + one, ps + rng.integers(1, 300, 5 * k))
        at_l = L - 40 + rng.integers(0, 20, 30)
        tips = (np.ones(60, np.int64), np.concatenate([rng.integers(0, 8, 30), at_l]) + one, np.concatenate([rng.integers(8, 30, 30), at_l + rng.integers(1, 21, 30)]))
        wide = _inside(rng, k, [1], lengths, 2 ** 29, one)
        rest = _inside(rng, n - 6 * k - 60, [0, 2], lengths, 400, one)
        off = _offsets(rng, 8, lengths)
        off[:, 1] = [0, 700, 1500, L - 700, L - 1500, 400_000, L - 400_000, 2 ** 30]
        return Case(f"r2_{window_rows}_{n}_{strict}", _shuffled(rng, _cat(near, tips, wide, rest)), _shuffled(rng, _cat(window, ends, sides)), 3, lengths, off)
    return once(("r2", strict, window_rows, n, side_rows), build)


def r3_case(strict, n=1000, third=300):
    """R3: contig 0 holds a single df2 row, contig 1 two identical rows, contig 2 a uniform set"""
    def build():
        rng = np.random.default_rng(7500 + n)
        one = 0 if strict else 1
        lengths = [5000, 5000, 5000]
        few = ([0, 1, 1], [2000 + one, 3000 + one, 3000 + one], [2400, 3100, 3100])
        probe, _ = _frames(rng, n, 0, 3, lengths, strict, width=600)
        return Case(f"r3_{n}_{strict}", probe, _shuffled(rng, _cat(few, _inside(rng, third, [2], lengths, 300, one))), 3, lengths, _offsets(rng, 8, lengths))
    return once(("r3", strict, n, third), build)


A_NC = 24


def a_case(strict, n=3 * TILE + 17, m=5000, n_perm=9):
    """A: df1 in random order on 24 contigs, every ineligible kind planted"""
    def build():
        rng = np.random.default_rng(7600 + n + n_perm)
        lengths = rng.integers(5000, 40_000, A_NC)
        probe, build = _frames(rng, n, m, A_NC, lengths, strict, width=400, bwidth=300)
        return Case(f"a_{n}_{m}_{n_perm}_{strict}", probe, build, A_NC, lengths, _offsets(rng, n_perm, lengths))
    return once(("a", strict, n, m, n_perm), build)


def sweep_lengths(probe, nc):
    """max probe end + slack per contig; every 5th contig shortened to the 80th percentile of its df1 ends (below the largest end in
    any case), which makes part of its df1 rows ineligible"""
    L = np.full(nc, 1000, np.int64)
    inside = P.inside(probe, nc)
    pc, pe = probe[0][inside], probe[2][inside].astype(np.int64)
    np.maximum.at(L, pc, pe + 10)
    for c in range(0, nc, 5):
        ends = pe[pc == c]
        if len(ends):
            L[c] = max(1, min(int(np.quantile(ends, 0.8)), int(ends.max()) - 1))
    return L


def sweep_case(strict, nc, rows=None, n_perm=5):
    """B: the sides of _map_select_util.sweep_sides (every OUTSIDE id on both sides); rows: a random subset of that many rows per side"""
    def build():
        probe, build = S.sweep_sides(nc)
        if rows is not None:
            probe, build = J.scaled(probe, rows, 1), J.scaled(build, rows, 2)
        lengths = sweep_lengths(probe, nc)
        return Case(f"sweep_{nc}_{rows}", probe, build, nc, lengths, _offsets(np.random.default_rng(7700 + nc), n_perm, lengths))
    return once(("sweep", nc, rows, n_perm), build)


SPARSE_L = 1_004_000


def sparse_case(strict, rows=None, n_perm=3):
    """B: 2^24 + 1 ids; one offset row per piece of the host entry: no shift, a shift by a few positions, a shift anywhere"""
    def build():
        probe, build = S.sparse_sides()
        if rows is not None:
            probe, build = J.scaled(probe, rows, 1), J.scaled(build, rows, 2)
        nc = P.SPARSE_NC
        rng = np.random.default_rng(7800)
        off = np.zeros((n_perm, nc), I32)
        for p in range(1, n_perm):
            off[p] = rng.integers(0, 300 if p == 1 else SPARSE_L, nc, dtype=I32)
        return Case(f"sparse_{rows}", probe, build, nc, np.full(nc, SPARSE_L, I32), off)
    return once(("sparse", rows, n_perm), build)


PIECES_NC = 262_145


def pieces_case(strict, n=4000, m=4000, occupied=300, n_perm=70):
    """B: 70 permutations x 262 145 contigs: two offset pieces of 63 and 7 permutations on the host entry"""
    def build():
        rng = np.random.default_rng(7900 + n)
        one = 0 if strict else 1
        nc = PIECES_NC
        occ = np.unique(np.concatenate([[0, nc - 1], rng.choice(nc, occupied, replace=False)]))
        lengths = np.full(nc, 5000, np.int64)
        probe, build = _inside(rng, n, occ, lengths, 300, one), _inside(rng, m, occ, lengths, 300, one)
        return Case(f"pieces_{n}_{n_perm}_{strict}", probe, build, nc, lengths, rng.integers(0, 5000, (n_perm, nc), dtype=I32))
    return once(("pieces", strict, n, m, occupied, n_perm), build)


def auto_case(strict, rows=None, n_perm=4):
    """C: df1 = the 140 000 rows on 24 contigs that take the balanced build by the automatic rule; df2 = 20 000 rows"""
    def build():
        case = P.auto_case()
        probe, build = case.frame, P.rows(case.probe, np.arange(20_000))
        if rows is not None:
            probe, build = J.scaled(probe, rows, 1), J.scaled(build, rows, 2)
        lengths = np.full(case.nc, 400_400, np.int64)
        return Case(f"auto_{rows}", probe, build, case.nc, lengths, _offsets(np.random.default_rng(8000), n_perm, lengths))
    return once(("auto", rows, n_perm), build)


def handover_case(strict, rows=None, n_perm=4):
    """C: df1 = 140 000 rows inside one narrow window plus two far rows (the balanced build hands over to the LSD sort)"""
    def build():
        df2, df1, nc = J.handover_sides()
        if rows is not None:
            df1, df2 = P.rows(df1, np.arange(len(df1[0]) - rows, len(df1[0]))), J.scaled(df2, rows, 2)      # (the tail: the two far rows with it)
        lengths = [(1 << 30) + 100]
        off = _offsets(np.random.default_rng(8100), n_perm, lengths)
        off[0], off[1] = 0, 17
        return Case(f"handover_{rows}", df1, df2, nc, lengths, off)
    return once(("handover", rows, n_perm), build)


def sequence_case(strict, rows=None, n_perm=16):
    """D: 30 000 df1 rows (contig 24 = outside among them) x 50 000 df2 rows on 24 contigs"""
    def build():
        probe, build, nc = J.sequence_sides()
        if rows is not None:
            probe, build = J.scaled(probe, rows, 1), J.scaled(build, rows, 2)
        lengths = np.full(nc, 61_000, np.int64)             # some df1 rows (up to 2000 long from starts below 60 000) end beyond it
        return Case(f"sequence_{rows}", probe, build, nc, lengths, _offsets(np.random.default_rng(8200), n_perm, lengths))
    return once(("sequence", rows, n_perm), build)


def sized_case(strict, n, seed, rows=None, n_perm=4):
    """D: the large (n df2 rows, n // 2 + 1 df1 rows) and small inputs that alternate on one context"""
    def build():
        probe, build, nc = S.sized_sides(n, seed)
        if rows is not None:
            probe, build = J.scaled(probe, rows, 1), J.scaled(build, rows, 2)
        top = int(max(probe[2].max(), build[2].max())) + 10
        lengths = np.full(nc, top, np.int64)
        return Case(f"sized_{n}_{seed}_{rows}", probe, build, nc, lengths, _offsets(np.random.default_rng(8300 + seed), n_perm, lengths))
    return once(("sized", n, seed, rows, n_perm), build)


def p_case(strict, tile=TILE, tiles=4096, extra=501, hot=3000, m=4000, n_perm=961):
    """P: tiles * tile + extra df1 rows, all but ``hot`` of them on contig 1, where df2 has no row; the hot rows on contigs 0 and 2, so
    that the (contig, start) order puts them into the first and the last tiles"""
    def build():
        rng = np.random.default_rng(8400 + tile)
        one = 0 if strict else 1
        n = tiles * tile + extra
        lengths = [50_000, 50_000, 50_000]
        probe = _shuffled(rng, _cat(_inside(rng, hot // 2, [0], lengths, 400, one), _inside(rng, hot - hot // 2, [2], lengths, 400, one),
                                    _inside(rng, n - hot, [1], lengths, 400, one)))
        off = _offsets(rng, n_perm, lengths)
        off[0] = 0
        return Case(f"p_{tile}_{tiles}_{strict}", probe, _inside(rng, m, [0, 2], lengths, 300, one), 3, lengths, off, tile=tile)
    return once(("p", strict, tile, tiles, extra, hot, m, n_perm), build)


def hot_rows(case):
    return P.rows(case.probe, case.probe[0] != 1)


SCALED = {
    "z": lambda s: z_case(s, 300, n=200, n_perm=5),
    "z_last": lambda s: z_edge_case(s, "last", m=200, n=200, n_perm=5),
    "z_first": lambda s: z_edge_case(s, "first", m=200, n=200, n_perm=5),
    "o_small": lambda s: o_case(s, 77, 200, 60, n_perm=7),
    "o_medium": lambda s: o_case(s, 300_000, 300, 300, n_perm=7, width=40_000, bwidth=20_000),
    "o_large": lambda s: o_case(s, MAXI, 300, 200, n_perm=7, width=2 ** 30, bwidth=2 ** 28),
    "r1": lambda s: r1_case(s, cluster=120, n=240, background=40, second=30),
    "r2": lambda s: r2_case(s, window_rows=200, n=320, side_rows=30),
    "r3": lambda s: r3_case(s, n=200, third=40),
    "a": lambda s: a_case(s, n=300, m=300, n_perm=5),
    "sweep_64": lambda s: sweep_case(s, 64, rows=300),
    "sweep_1025": lambda s: sweep_case(s, 1025, rows=400),
    "sparse": lambda s: sparse_case(s, rows=300, n_perm=2),
    "pieces": lambda s: pieces_case(s, n=300, m=300, occupied=30, n_perm=3),
    "auto": lambda s: auto_case(s, rows=400),
    "handover": lambda s: handover_case(s, rows=300),
    "sequence": lambda s: sequence_case(s, rows=400, n_perm=4),
    "sized_large": lambda s: sized_case(s, 150_000, 900, rows=400),
    "sized_small": lambda s: sized_case(s, J.SMALL_ROWS, 901),
    "p": lambda s: p_case(s, tile=40, tiles=8, extra=6, hot=30, m=60, n_perm=5),
}
