"""Inputs, references and runners of tests/test_depth_profile_matrix.py (test helper).  Every generator takes the sizes as arguments, so
that the CPU group runs a scaled-down copy of exactly the recipe the GPU tests run.  The expected matrix is always
_depth_profile_util.expected_bases (explicit bins through the prefix form, int64, engine-free); numbers come from numpy and from the
constants of the kernel's headers, never from the code under test.

A Case is (name, windows, build, nc): the window side of a case of _position_ops_util / _permutation_matrix_util is its ``probe``, the
build side its ``frame`` (``build``).  Windows and build rows are in the mode's own convention -- Strict rows cover [start, end), Weak
rows [start, end] -- and "position space" below means the half-open form of either: [start, end + w), w = 0 Strict / 1 Weak."""
import os
import re

import numpy as np

import _depth_profile_util as DP
import _depth_sum_util as S
import _depth_util as U
import _join_ops_util as J
import _map_select_util as MS
import _permutation_matrix_util as M
import _position_ops_util as P

I32 = np.int32
SENTINEL = MS.SENTINEL
BINS = 7                               # the small odd bin count of every group that names no other
CSRC = M.CSRC


def chunk_bytes():
    """DPROF_CHUNK_BYTES of host_depth_profile.hip.h"""
    src = open(os.path.join(CSRC, "host_depth_profile.hip.h")).read()
    m = re.search(r"DPROF_CHUNK_BYTES\s*=\s*\(size_t\)(\d+)\s*<<\s*(\d+)", src)
    assert "DPROF_CHUNK_BYTES / row_bytes" in src and "row_bytes = (size_t)n_bins * 8" in src
    return int(m.group(1)) << int(m.group(2))


def chunk_rows(n_bins, n=None):
    """rows per chunk of the host entry as depth_profile_host computes them"""
    rows = chunk_bytes() // (8 * n_bins)
    return max(1, rows if n is None else min(n, rows))


class Case:
    def __init__(self, name, windows, build, nc, **note):
        self.name, self.nc, self.note = name, int(nc), note
        self.windows, self.build = U.as_i32(*windows), U.as_i32(*build)
        for a in self.windows + self.build:
            a.setflags(write=False)

    @property
    def n(self):
        return len(self.windows[0])


_cases, _refs = {}, {}


def once(key, build):
    if key not in _cases:
        _cases[key] = build()
    return _cases[key]


def flags_of(case, seed=5):
    """the mixed reverse flags of a case (_depth_profile_util.mixed_flags), or its own where the generator fixes them (H)"""
    return case.note["flags"] if "flags" in case.note else DP.mixed_flags(case.n, seed)


def reference(case, strict, n_bins, reverse=None):
    if "period" in case.note:
        return h_reference(case, strict, n_bins, reverse)
    return DP.expected_bases(case.windows, case.build, strict, case.nc, n_bins, reverse)


def reference_once(case, strict, n_bins=BINS, reverse="mixed"):
    """the expected matrix of a case, computed once and shared by the tests that run it (read-only); reverse: "mixed" = flags_of(case)"""
    key = (case.name, bool(strict), n_bins, reverse if isinstance(reverse, str) or reverse is None else reverse.tobytes())
    if "period" in case.note:                                # (H: hundreds of megabytes at full size -- computed for its one user, not kept)
        return reference(case, strict, n_bins, flags_of(case) if isinstance(reverse, str) else reverse)
    if key not in _refs:
        exp = reference(case, strict, n_bins, flags_of(case) if isinstance(reverse, str) else reverse)
        exp.setflags(write=False)
        _refs[key] = exp
    return _refs[key]


def pair_reference(case, strict, n_bins, reverse=None, cells=3_000_000):
    """(sampled flat bin indices, the pair form of those bins in the UNREVERSED layout, the same entries of the expectation)"""
    bins = DP.explicit_bins(case.windows, n_bins, strict)
    idx = S.sample(len(bins[0]), len(case.build[0]), cells=cells)
    plain = DP.expected_bases(case.windows, case.build, strict, case.nc, n_bins)
    return idx, S.pair_form(bins, case.build, strict, case.nc, idx), plain.reshape(-1)[idx]


def fill(case, strict, n_bins, exp=None):
    """(share of non-zero bins among the windows inside the dictionary, number of empty bins, number of windows inside)"""
    exp = reference_once(case, strict, n_bins, None) if exp is None else exp
    inside = P.inside(case.windows, case.nc)
    empty = int((DP.bin_lengths(case.windows, n_bins, strict)[inside] == 0).sum())
    return (float((exp[inside] != 0).mean()) if inside.any() else 0.0), empty, int(inside.sum())


def blob(a):
    return np.ascontiguousarray(np.asarray(a)).tobytes()


# ---- runners --------------------------------------------------------------------------------------------------------------------------

def run_host(eng, case, strict, n_bins=BINS, reverse=None):
    return eng.depth_profile(case.windows, reverse, n_bins, case.build, strict, case.nc)


def dev_flags(reverse, offset=0):
    """the flags as a uint8 tensor in HBM; offset: a view that starts that many bytes into a larger tensor"""
    import torch
    if reverse is None:
        return None
    r = torch.from_numpy(np.asarray(reverse, bool).astype(np.uint8))
    big = torch.full((len(r) + offset + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    big[offset:offset + len(r)] = r.cuda()
    out = big[offset:offset + len(r)]
    assert out.is_contiguous() and (len(r) == 0 or out.data_ptr() % 2 == offset % 2), "an odd offset is an odd address"
    return out


def dev_out(n, n_bins, offset=0, pad=5):
    """(the whole sentinel-filled int64 tensor, its contiguous (n, n_bins) view that starts ``offset`` elements in)"""
    import torch
    whole = torch.full((offset + n * n_bins + pad,), SENTINEL, dtype=torch.int64, device="cuda")
    out = whole[offset:offset + n * n_bins].view(n, n_bins)
    assert out.is_contiguous()
    return whole, out


def run_dev(dj, case, strict, n_bins=BINS, reverse=None, index=None, shift=0, window_row_id=None, build_row_id=None, partition_mode=None,
            flag_offset=0, out_offset=0, whole=False):
    """the device entry into a caller's buffer pre-filled with a sentinel -> the matrix (numpy); whole=True: (matrix, the whole
    buffer around it as numpy, the offset of the matrix inside it).  partition_mode: through the raw entry with that opts field."""
    from polars_bio_amd import _engine
    w = J.dev_side(case.windows, window_row_id, shift)
    b = J.dev_side(case.build, build_row_id, shift)
    rev = dev_flags(reverse, flag_offset)
    buf, out = dev_out(case.n, n_bins, out_offset)
    if partition_mode is None:
        assert dj.depth_profile(w, b, strict, case.nc, n_bins, reverse=rev, index=index, out=out) is out
    else:
        opts = _engine.make_opts(strict, case.nc, partition_mode=partition_mode)
        ix = dj.engine.index_build_dev(b.as_c(), opts, False) if index is None else index
        try:
            dj.engine.depth_profile_dev(ix, w.as_c(), rev.data_ptr() if rev is not None and case.n else 0, n_bins, opts,
                                        out.data_ptr() if out.numel() else 0)
        finally:
            if index is None:
                ix.close()
    got = out.cpu().numpy()
    return (got, buf.cpu().numpy(), out_offset) if whole else got


def check_both(eng, dj, case, strict, n_bins=BINS, reverse="mixed", exp=None, what=None):
    """both entries against the expectation -> (exp, {"host": ..., "device": ...}); reverse: "mixed" = flags_of(case), or None"""
    flags = flags_of(case) if isinstance(reverse, str) else reverse
    exp = reference_once(case, strict, n_bins, reverse) if exp is None else exp
    what = what or f"{case.name}, {n_bins} bins"
    got = {}
    if eng is not None:
        got["host"] = run_host(eng, case, strict, n_bins, flags)
        DP.assert_profile_equal(got["host"], exp, what + ": host entry")
    if dj is not None:
        got["device"] = run_dev(dj, case, strict, n_bins, flags)
        DP.assert_profile_equal(got["device"], exp, what + ": device entry")
    return exp, got


# ---- generators -------------------------------------------------------------------------------------------------------------------------

def _cat(*sides):
    return tuple(np.concatenate([np.asarray(s[k], np.int64) for s in sides]) for k in range(3))


def short_windows(contigs, start, n_bins, strict):
    """per contig a window of L = 0 and one of L = n_bins - 1 positions: the bins that hold no position"""
    w = 0 if strict else 1
    lens = np.array([0, max(n_bins - 1, 0)] * len(contigs), np.int64)
    s = np.full(len(lens), start, np.int64)
    return np.repeat(np.asarray(contigs, np.int64), 2), s, s + lens - w


H_PATTERN = np.array([1, 0, 0, 1, 0, 1, 1], bool)


def h_case(n_bins=DP.MAX_BINS, n=None, distinct=61, build_rows=3000, span=60_000, max_len=400):
    """H: ``distinct`` different windows repeated cyclically over n rows (default: one chunk of the host entry + 300), flags of period
    len(H_PATTERN) = 7.  The windows are 2 - 7 n_bins long (one is n_bins / 2 + 1: every second bin empty) over a build side about
    five rows deep, so that most bins are non-zero and two windows differ in most bins."""
    n = chunk_rows(n_bins) + 300 if n is None else n

    def build():
        rng = np.random.default_rng(8800 + n_bins)
        frame = U.random_rows(rng, build_rows, 2, span, max_len)
        length = rng.integers(2 * n_bins, 7 * n_bins, distinct)
        length[distinct // 2] = n_bins // 2 + 1
        assert len(set(length.tolist())) > distinct // 2 and length.max() < span
        ws = (rng.random(distinct) * (span - length)).astype(np.int64)
        wc = np.arange(distinct) % 2
        i = np.arange(n)
        flags = H_PATTERN[i % len(H_PATTERN)]
        # (Strict and Weak read the same arrays: a Weak window is one position longer)
        return Case(f"h_{n_bins}_{n}", (wc[i % distinct], ws[i % distinct], (ws + length)[i % distinct]), frame, 2,
                    flags=flags, period=(distinct, len(H_PATTERN)))
    return once(("h", n_bins, n, distinct, build_rows, span, max_len), build)


def h_reference(case, strict, n_bins, reverse, shift_windows=0, shift_flags=0):
    """expected_bases of the distinct (window, flag) rows -- one period of both -- indexed out to the case's n rows.  shift_*: the
    reference of the input with its windows / flags moved by that many rows (what a wrong chunk offset would compute)."""
    d, p = case.note["period"]
    period = d * p
    i = np.arange(case.n)
    if reverse is not None:
        assert np.array_equal(reverse, case.note["flags"])
    k = np.arange(period)
    head = tuple(np.ascontiguousarray(a[:d][(k + shift_windows) % d]) for a in case.windows)
    rev = None if reverse is None else H_PATTERN[(k + shift_flags) % p]
    exp = DP.expected_bases(head, case.build, strict, case.nc, n_bins, rev)
    return exp[i % period]


T_LAYERS = [(1, 0.0, 1.0), (2, 0.0, 1.0), (3, 0.0, 1.0), (5, 0.25, 0.75), (7, 1 / 3, 1.0)]       # (cells per row, from, to) of a layer
T_ORIGIN = [0, -3500]


def t_case(strict, n_bins, pitch=5, cells=896, starts=12):
    """T: on each of 2 contigs a lattice of ``cells`` cells of ``pitch`` positions; the build rows tile it in layers (rows of 1, 2 and 3
    cells over all of it, of 5 and 7 cells over parts: depth 3 - 5), so that every lattice point is a build start and a build end
    (the first only a start, the last only an end).  Windows of L = n_bins * pitch * k, k = 1 .. 3, from ``starts`` lattice points per
    contig: every edge on the lattice; the same windows moved by -1 and by +1; one window per contig from its smallest key to its
    largest; windows with bins that hold no position; one window half beyond the largest key."""
    def build():
        w = 0 if strict else 1
        assert cells % n_bins == 0 and pitch >= 3
        rows = []
        for c, origin in enumerate(T_ORIGIN):
            for length, lo, hi in T_LAYERS:
                lo, hi = int(lo * cells), int(hi * cells)
                a = np.arange(lo, hi, length)
                rows.append((np.full(len(a), c), origin + a * pitch, origin + np.minimum(a + length, hi) * pitch - w))
        rng = np.random.default_rng(8900 + n_bins)
        frame = _cat(*rows)
        order = rng.permutation(len(frame[0]))
        frame = tuple(a[order] for a in frame)
        wins, kind = [], []
        for c, origin in enumerate(T_ORIGIN):
            for k in (1, 2, 3):
                a = np.unique(np.linspace(1, cells - 1 - n_bins * k, starts).astype(np.int64))
                s = origin + a * pitch
                for d in (0, -1, 1):
                    wins.append((np.full(len(s), c), s + d, s + d + n_bins * pitch * k - w))
                    kind += [d] * len(s)
            wins.append(([c], [origin], [origin + cells * pitch - w]))
            kind.append(2)
            wins.append(([c], [origin + (cells - n_bins) * pitch], [origin + (cells + n_bins) * pitch - w]))
            kind.append(3)
        wins.append(short_windows([0, 1], 40 * pitch, n_bins, strict))
        kind += [3] * 4
        return Case(f"t_{n_bins}_{pitch}_{cells}_{strict}", _cat(*wins), frame, 2, kind=np.array(kind), pitch=pitch, cells=cells)
    return once(("t", strict, n_bins, pitch, cells, starts), build)


def keys_of(build, c, strict):
    """(the build starts, the build half-open ends) of contig c in position space, int64"""
    on = np.asarray(build[0]) == c
    return np.asarray(build[1], np.int64)[on], np.asarray(build[2], np.int64)[on] + (0 if strict else 1)


def i_case(n=30_000, span=9000, windows=5000):
    """I: the degenerate frame (a quarter of the rows inverted, a quarter zero-length) under the first ``windows`` of its probes"""
    def build():
        c = P.degenerate_case(n, span)
        return Case(f"i_{n}_{windows}", P.rows(c.probe, np.arange(min(windows, len(c.probe[0])))), c.frame, c.nc)
    return once(("i", n, span, windows), build)


def i_single_case(n=30_000, span=9000, windows=5000, with_row=True):
    """I: the same frame with every inverted row turned round (start < end: ordinary) and ONE row, in the middle of the input,
    inverted by 25 positions inside the populated range; with_row=False: that row removed"""
    def build():
        base = i_case(n, span, windows)
        c, s, e = (np.asarray(a, np.int64) for a in base.build)
        s, e = np.minimum(s, e), np.maximum(s, e)
        at = len(c) // 2
        s[at], e[at] = span // 2 + 25, span // 2
        keep = np.ones(len(c), bool)
        keep[at] = with_row
        return Case(f"i_single_{n}_{windows}_{with_row}", base.windows, (c[keep], s[keep], e[keep]), base.nc, row=at)
    return once(("i_single", n, span, windows, with_row), build)


def shared_keys(build, c, strict, top=1):
    """the ``top`` most frequent start keys and end keys of contig c in position space -> [(key, rows that share it)], starts first"""
    out = []
    for keys in keys_of(build, c, strict):
        v, k = np.unique(keys, return_counts=True)
        best = np.argsort(-k, kind="stable")[:top]
        out += [(int(v[i]), int(k[i])) for i in best]
    return out


def key_windows(keys, c, n_bins, strict):
    """windows of contig c laid so that edge j falls on key + d, d = -1, 0, 1: just below, on and just above the key -- for the
    first edge, the second, a middle one and the last, with bins of q = 1, 3, 50 and 7 positions (edge j = start + j q exactly)"""
    w = 0 if strict else 1
    s, e = [], []
    for key in keys:
        for d in (-1, 0, 1):
            for j, q in ((0, 1), (min(1, n_bins), 3), (n_bins // 2, 50), (n_bins, 7)):
                s.append(key + d - j * q)
                e.append(key + d - j * q + n_bins * q - w)
    return np.full(len(s), c, np.int64), np.array(s, np.int64), np.array(e, np.int64)


R_CONTIG = {"r1": 0, "r2": 1, "r3": None}


def r_case(which, strict, n_bins, **sizes):
    """R: the build side of r1_case / r2_case / r3_case of _permutation_matrix_util under its probes and under key_windows of its
    most shared keys (r3: of the single row's and of the two identical rows' keys)"""
    def build():
        base = {"r1": M.r1_case, "r2": M.r2_case, "r3": M.r3_case}[which](strict, **sizes)
        extra = []
        for c in ([0, 1] if which == "r3" else [R_CONTIG[which]]):
            extra.append(key_windows([k for k, _ in shared_keys(base.build, c, strict)], c, n_bins, strict))
        extra.append(short_windows([0, 1], 2000, n_bins, strict))
        # (most probes of these recipes lie beside the clusters or in the empty reaches of the grid: as many windows on build rows)
        extra.append(cover_windows(base.build, base.nc, len(base.probe[0]), 9400 + n_bins, n_bins))
        wins = _cat(base.probe, *extra)
        assert wins[1].min() >= DP.I32_MIN and wins[2].max() <= DP.I32_MAX
        return Case(f"{base.name}_{n_bins}", wins, base.build, base.nc, own=len(base.probe[0]))
    return once(("r", which, strict, n_bins, tuple(sorted(sizes.items()))), build)


def of_position_case(case, windows=None, rows=None):
    """a Case of _position_ops_util as a Case of this module: windows = its probe (the first ``windows`` of them), build = its frame;
    rows: a random subset of that many rows per side (the scaled-down copies of the CPU group)"""
    def build():
        probe = case.probe if windows is None else P.rows(case.probe, np.arange(min(windows, len(case.probe[0]))))
        frame = case.frame
        if rows is not None:
            probe, frame = J.scaled(probe, rows, 1), J.scaled(frame, rows, 2)
        return Case(f"{case.name}_{windows}_{rows}", probe, frame, case.nc)
    return once(("pos", case.name, windows, rows), build)


def sweep_case(nc, rows=None):
    """B: P.sweep_case(nc) with as many cover_windows as it has probes: from about 1000 contigs on its 30 000 build rows of at most
    100 positions lie over nc x 5000 positions, and the probes alone leave most bins zero"""
    def build():
        base = of_position_case(P.sweep_case(nc), rows=rows)
        wins = _cat(base.windows, cover_windows(base.build, nc, base.n, 9300 + nc))
        return Case(f"{base.name}_covered", wins, base.build, nc, own=base.n)
    return once(("sweep_covered", nc, rows), build)


def sparse_case(rows=None):
    return of_position_case(P.sparse_case(), rows=rows)


def bare_case(case):
    """the case without its out-of-dictionary rows on either side, and the mask of the windows it keeps (P.without_outside's rule)"""
    keep = P.inside(case.windows, case.nc)
    return Case(case.name + " (dictionary rows only)", P.rows(case.windows, keep), P.rows(case.build, P.inside(case.build, case.nc)), case.nc), keep


def brief_windows(contigs, at):
    """per contig a window of -1 and one of 3 positions Strict / 0 and 4 Weak, the same arrays for both modes: bins without a position
    under 7 bins for the cases whose own windows are all longer"""
    c = np.repeat(np.asarray(contigs, np.int64), 2)
    s = np.tile(np.array([at, at + 100], np.int64), len(contigs))
    return c, s, s + np.tile(np.array([-1, 3], np.int64), len(contigs))


def cover_windows(build, nc, k, seed, n_bins=BINS):
    """k windows that ARE a build row of the dictionary (even ones) or that row less its first and last position (odd ones), taken
    from the rows at least n_bins (+ 2) long where the side has such rows: every bin holds a position under a build row.  The
    same arrays serve both modes (a row and a window with the same start and end cover the same positions in either)."""
    rng = np.random.default_rng(seed)
    c, s, e = (np.asarray(a, np.int64)[P.inside(build, nc)] for a in build)
    long_enough = np.flatnonzero(e - s >= n_bins + 2)
    pool = long_enough if len(long_enough) else np.flatnonzero(e > s)
    r = pool[rng.integers(0, len(pool), k)]
    d = (np.arange(k) % 2) * (e[r] - s[r] >= n_bins + 2)
    return c[r], s[r] + d, e[r] - d


def v3_case(entry, rows=None):
    """C: a shape of test_gpu_parity._v3_cases(): its probes and 5/4 as many cover_windows of its build side, at least 1500 (the
    probes of the one-row, the one-bucket and the 33-bit shapes on their own share next to nothing with it)"""
    def build():
        base = of_position_case(P.v3_case(entry), rows=rows)
        k = max(1500 if rows is None else 0, 5 * base.n // 4)
        wins = _cat(base.windows, cover_windows(base.build, base.nc, k, len(entry[0])), brief_windows([0], int(base.build[1][0])))
        return Case(f"v3: {entry[0]}_{rows}", wins, base.build, base.nc, own=base.n)
    return once(("v3", entry[0], rows), build)


def auto_case(windows=20_000, rows=None):
    return of_position_case(P.auto_case(), windows=windows, rows=rows)


def sequence_case(rows=None):
    return of_position_case(P.sequence_case(), rows=rows)


def sized_case(n, seed, rows=None):
    """D: P.sized_case with four brief_windows (its probes are 1 .. 1500 long: at 300 rows none may be shorter than the 7 bins)"""
    def build():
        base = of_position_case(P.sized_case(n, seed), rows=rows)
        return Case(f"{base.name}_short", _cat(base.windows, brief_windows([0, 23], 100)), base.build, base.nc)
    return once(("sized_short", n, seed, rows), build)


def a_case(strict, n=3 * DP.TILE + 17, m=5000):
    """A: the windows and the build side of _permutation_matrix_util.a_case (random order, 24 contigs, rows outside and without a
    position planted), with windows that hold empty bins"""
    def build():
        base = M.a_case(strict, n=n, m=m)
        wins = _cat(base.probe, short_windows([0, 23], 1000, 100, strict))
        return Case(f"a_{n}_{m}_{strict}", wins, base.build, base.nc)
    return once(("a", strict, n, m), build)


def v3_entries():
    """test_gpu_parity._v3_cases(), generated once"""
    from test_gpu_parity import _v3_cases
    return once("v3_entries", _v3_cases)


# name -> (strict -> a scaled-down copy of the generator above, the bin count it runs with)
SCALED = {
    "h": (lambda s: h_case(n_bins=64, n=61 * 7 + 61, build_rows=300, span=2000, max_len=60), 64),
    "t_7": (lambda s: t_case(s, 7, cells=56, starts=4), 7),
    "t_64": (lambda s: t_case(s, 64, cells=256, starts=4), 64),
    "t_1": (lambda s: t_case(s, 1, cells=56, starts=4), 1),
    "i": (lambda s: i_case(2000, 900, 300), 100),
    "i_single": (lambda s: i_single_case(2000, 900, 300), 100),
    "i_single_without": (lambda s: i_single_case(2000, 900, 300, with_row=False), 100),
    "r1": (lambda s: r_case("r1", s, 7, cluster=120, n=240, background=40, second=30), 7),
    "r2": (lambda s: r_case("r2", s, 64, window_rows=200, n=320, side_rows=30), 64),
    "r3": (lambda s: r_case("r3", s, 7, n=200, third=40), 7),
    "sweep_64": (lambda s: sweep_case(64, rows=300), BINS),
    "sweep_1025": (lambda s: sweep_case(1025, rows=400), BINS),
    "sparse": (lambda s: sparse_case(rows=300), BINS),
    "auto": (lambda s: auto_case(rows=400), BINS),
    "sequence": (lambda s: sequence_case(rows=400), BINS),
    "sized_large": (lambda s: sized_case(150_000, 900, rows=400), BINS),
    "sized_small": (lambda s: sized_case(J.SMALL_ROWS, 901), BINS),
    "a": (lambda s: a_case(s, n=300, m=300), 100),
}
V3_SHAPES = 6                          # shapes of _v3_cases(): generated on first use, not on import
for _k in range(V3_SHAPES):
    SCALED[f"v3_{_k}"] = (lambda s, _k=_k: v3_case(v3_entries()[_k], rows=300), BINS)
