"""Inputs, references and runners of tests/test_depth_dist_matrix.py (test helper): depth_histogram (region and contig form) and
depth_quantiles across the project's cross-cutting matrices.  A Case is _depth_profile_matrix_util's (name, windows, build, nc): the
``windows`` are the probe rows.  Most generators are that module's, with a pile on top (``deepened``): a few build rows that climb
to PILE_DEPTH and fall back over 2 PILE_DEPTH positions, and probes over them, so that the clamp bin of max_depth 6 is reached and
a row has many distinct order statistics whatever the dictionary size thins the random rows down to.

The expected values are always _depth_hist_util.block_form / contig_form and _depth_quant_util.block_form (int64, engine-free);
numbers come from numpy and from the constants of the kernels' headers, never from the code under test."""
import zlib

import numpy as np

import _depth_hist_util as H
import _depth_profile_matrix_util as X
import _depth_quant_util as Q
import _depth_util as U
import _join_ops_util as J
import _position_ops_util as P

MAX_DEPTH = 6                          # 7 bins: every group that names no other
SENTINEL = X.SENTINEL                  # int64 outputs
SENTINEL32 = 0x5A5A5A5A                # int32 outputs
Case, once, blob = X.Case, X.once, X.blob
PILE_DEPTH = 9
PILE_PROBES = 4


def k_of(case):
    """the number of ranks a case runs with: 1, 3 or 16 by its name"""
    return case.note.get("k", Q.KS[zlib.crc32(case.name.encode()) % len(Q.KS)])


def md_of(case):
    return case.note.get("md", MAX_DEPTH)


# ---- references, computed once per (case, mode) and shared (read-only) ------------------------------------------------------------------

_refs = {}


def _keep(key, make):
    if key not in _refs:
        out = make()
        for a in (out if isinstance(out, tuple) else (out,)):
            a.setflags(write=False)
        _refs[key] = out
    return _refs[key]


def hist_ref(case, strict, md=None):
    md = md_of(case) if md is None else md
    return _keep(("hist", case.name, bool(strict), md), lambda: H.block_form(case.windows, case.build, strict, case.nc, md))


def contig_ref(case, strict, md=None):
    md = md_of(case) if md is None else md
    return _keep(("contigs", case.name, bool(strict), md), lambda: H.contig_form(case.build, strict, case.nc, md))


def contig_rows(build, strict, nc, md):
    """the contig form through its non-zero rows -> (the contigs that hold a block, ascending; their (len, md + 1) rows): what a
    dictionary of 2^24 + 1 ids is compared through"""
    kc, ks, ke, kd = U.depth_events(*build, strict, nc)
    ids, inv = np.unique(kc, return_inverse=True)
    rows = np.zeros((len(ids), md + 1), np.int64)
    np.add.at(rows, (inv, np.minimum(kd, md)), ke - ks + (0 if strict else 1))
    return ids, rows


def ranks_of(case, strict, k=None):
    """the ranks of a case: its own where the generator fixes them (T), else _depth_quant_util.ranks_for"""
    k = k_of(case) if k is None else k
    if "ranks" in case.note and k == case.note["ranks"].shape[1]:
        return case.note["ranks"]
    return _keep(("ranks", case.name, bool(strict), k), lambda: Q.ranks_for(case.windows, strict, case.nc, k, k + len(case.name)))


def quant_ref(case, strict, k=None):
    ranks = ranks_of(case, strict, k)
    return _keep(("quant", case.name, bool(strict), ranks.shape[1]), lambda: Q.block_form(case.windows, case.build, strict, case.nc, ranks))


def n_blocks(build, strict, nc):
    return len(U.depth_events(*build, strict, nc)[0])


def blocks_side(build, strict, nc):
    """the depth blocks as a side, in the mode's own convention: what depth_blocks_build indexes"""
    kc, ks, ke, _ = U.depth_events(*build, strict, nc)
    return U.as_i32(kc, ks, ke)


def bars(case, strict):
    """the non-blind figures of a case among its probes inside the dictionary: (share of rows with a non-zero bin above bin 0, sum
    of the clamp bin, share of the valid ranks that answer above 0, number of distinct answers)"""
    md = md_of(case)
    hist, val = hist_ref(case, strict), quant_ref(case, strict)
    inside = P.inside(case.windows, case.nc)
    L = H.positions(case.windows, strict, case.nc)
    ranks = ranks_of(case, strict)
    valid = (ranks >= 0) & (ranks < L[:, None]) & inside[:, None]
    return (float((hist[inside][:, 1:] != 0).any(axis=1).mean()), int(hist[inside][:, md].sum()), float((val[valid] > 0).mean()),
            len(np.unique(val[valid])))


# ---- runners ------------------------------------------------------------------------------------------------------------------------------

def host_hist(eng, case, strict, md=None, partition_mode=0):
    return eng.depth_hist(case.windows, case.build, strict, case.nc, md_of(case) if md is None else md, partition_mode=partition_mode)


def host_contigs(eng, case, strict, md=None):
    return eng.depth_hist_contigs(case.build, strict, case.nc, md_of(case) if md is None else md)


def host_quant(eng, case, strict, ranks=None, partition_mode=0):
    return eng.depth_quantiles(case.windows, case.build, strict, case.nc, ranks_of(case, strict) if ranks is None else ranks,
                               partition_mode=partition_mode)


def sentinel_of(dtype):
    """the fill of a caller's buffer of that torch or numpy dtype"""
    return SENTINEL if str(dtype).endswith("int64") else SENTINEL32


def dev_buffer(shape, dtype, offset=0, pad=5):
    """(the whole sentinel-filled tensor, its contiguous view of ``shape`` that starts ``offset`` elements in)"""
    import torch
    count = int(np.prod(shape))
    whole = torch.full((offset + count + pad,), sentinel_of(dtype), dtype=dtype, device="cuda")
    out = whole[offset:offset + count].view(*shape)
    assert out.is_contiguous() and out.data_ptr() == whole.data_ptr() + offset * whole.element_size()
    return whole, out


def dev_ranks(ranks, offset=0):
    """the ranks as an int64 tensor in HBM; offset: a view that starts that many int64 elements into a larger tensor"""
    import torch
    r = np.ascontiguousarray(ranks, np.int64)
    big = torch.full((r.size + offset + 3,), -(1 << 40), dtype=torch.int64, device="cuda")
    big[offset:offset + r.size] = torch.from_numpy(r.reshape(-1).copy()).cuda()
    out = big[offset:offset + r.size].view(*r.shape)
    assert out.is_contiguous()
    return out


def _result(out, buf, offset, whole):
    got = out.cpu().numpy()
    return (got, buf.cpu().numpy(), offset) if whole else got


def dev_hist(dj, case, strict, md=None, index=None, shift=0, probe_row_id=None, build_row_id=None, partition_mode=0, out_offset=0, whole=False):
    """the device entry into a caller's buffer pre-filled with a sentinel -> the histogram rows (numpy); whole=True: (rows, the
    whole buffer around them as numpy, their offset inside it)"""
    md = md_of(case) if md is None else md
    p, b = J.dev_side(case.windows, probe_row_id, shift), J.dev_side(case.build, build_row_id, shift)
    buf, out = dev_buffer((case.n, md + 1), dj.torch.int64, out_offset)
    assert dj.depth_histogram(p, b, strict, case.nc, md, index=index, out=out, partition_mode=partition_mode) is out
    return _result(out, buf, out_offset, whole)


def dev_contigs(dj, case, strict, md=None, index=None, shift=0, build_row_id=None, out_offset=0, whole=False):
    md = md_of(case) if md is None else md
    b = J.dev_side(case.build, build_row_id, shift)
    buf, out = dev_buffer((case.nc, md + 1), dj.torch.int64, out_offset)
    assert dj.depth_histogram_contigs(b, strict, case.nc, md, index=index, out=out) is out
    return _result(out, buf, out_offset, whole)


def dev_quant(dj, case, strict, ranks=None, index=None, shift=0, probe_row_id=None, build_row_id=None, partition_mode=0, rank_offset=0,
              out_offset=0, whole=False):
    ranks = ranks_of(case, strict) if ranks is None else ranks
    p, b = J.dev_side(case.windows, probe_row_id, shift), J.dev_side(case.build, build_row_id, shift)
    buf, out = dev_buffer(ranks.shape, dj.torch.int32, out_offset)
    assert dj.depth_quantiles(p, b, strict, case.nc, dev_ranks(ranks, rank_offset), index=index, out=out, partition_mode=partition_mode) is out
    return _result(out, buf, out_offset, whole)


def check_all(eng, dj, case, strict, what=None, index=None, contigs=True):
    """the three host entries (eng) and the three device entries (dj; index: a DeviceIndex of the build side) against the references
    -> {"host_hist": ..., "dev_quant": ...}"""
    what = what or case.name
    got = {}
    if eng is not None:
        got["host_hist"], got["host_quant"] = host_hist(eng, case, strict), host_quant(eng, case, strict)
        if contigs:
            got["host_contigs"] = host_contigs(eng, case, strict)
    if dj is not None:
        got["dev_hist"], got["dev_quant"] = dev_hist(dj, case, strict, index=index), dev_quant(dj, case, strict, index=index)
        if contigs:
            got["dev_contigs"] = dev_contigs(dj, case, strict, index=index)
    for key, g in got.items():
        w = f"{what}: {key}"
        if key.endswith("_hist"):
            H.assert_hist_equal(g, hist_ref(case, strict), w)
        elif key.endswith("_quant"):
            Q.assert_quant_equal(g, quant_ref(case, strict), w)
        else:
            H.assert_hist_equal(g, contig_ref(case, strict), w)
    return got


# ---- generators ---------------------------------------------------------------------------------------------------------------------------

def pile(contigs, at, strict):
    """(build rows, probes) of a pile per contig: row j covers [at + j, at + 2 PILE_DEPTH - j), j < PILE_DEPTH -- the depth climbs by
    one per position to PILE_DEPTH and falls back; PILE_PROBES probes: over all of it and 10 positions either side, over its
    rising half, over its two deepest positions, and over its last position and the 5 behind it"""
    w = 0 if strict else 1
    j = np.arange(PILE_DEPTH)
    top = 2 * PILE_DEPTH
    probes = [(-10, top + 10), (0, PILE_DEPTH), (PILE_DEPTH - 1, PILE_DEPTH + 1), (top - 1, top + 5)]
    assert len(probes) == PILE_PROBES
    bc, bs, be, pc, ps, pe = [], [], [], [], [], []
    for c, a in zip(contigs, at):
        bc.append(np.full(PILE_DEPTH, c)); bs.append(a + j); be.append(a + top - j - w)
        pc.append(np.full(PILE_PROBES, c)); ps.append(a + np.array([p[0] for p in probes])); pe.append(a + np.array([p[1] for p in probes]) - w)
    cat = lambda xs: np.concatenate(xs).astype(np.int64)          # noqa: E731
    return (cat(bc), cat(bs), cat(be)), (cat(pc), cat(ps), cat(pe))


def deepened(case, strict, piles=2, copies=1):
    """the case with a pile on the first and the last contig its build side holds rows on (piles=2), at the start of a build row
    there, behind its own rows on either side; copies: the piles' probes that many times"""
    def build():
        inside = P.inside(case.build, case.nc)
        ids = np.unique(case.build[0][inside])
        contigs = [int(ids[0]), int(ids[-1])][:piles]
        first = lambda c: int(case.build[1][inside][case.build[0][inside] == c][0])                    # noqa: E731
        at = [min(max(first(c), -2 ** 30), 2 ** 30) for c in contigs]
        rows, probes = pile(contigs, at, strict)
        probes = tuple(np.tile(a, copies) for a in probes)
        note = dict(case.note, piled=len(probes[0]))
        return Case(f"{case.name}_piled_{strict}", X._cat(case.windows, probes), X._cat(case.build, rows), case.nc, **note)
    return once(("piled", case.name, strict, piles, copies), build)


def sweep_case(nc, strict, rows=None):
    return deepened(X.sweep_case(nc, rows=rows), strict)


def sparse_case(strict, rows=None):
    """B: the sparse dictionary with as many cover windows as probes (its probes lie mostly beside its 2000-position rows)"""
    def build():
        base = X.sparse_case(rows=rows)
        wins = X._cat(base.windows, X.cover_windows(base.build, base.nc, base.n, 9500))
        return Case(f"{base.name}_covered", wins, base.build, base.nc, own=base.n)
    return deepened(once(("sparse_covered", rows), build), strict)


def bare_case(case):
    """the case without its out-of-dictionary rows on either side, and the mask of the probes it keeps (its ranks: ranks[keep])"""
    bare, keep = X.bare_case(case)
    return bare, keep


def v3_case(entry, strict, rows=None):
    """C: X.v3_case; the one-row shape stays one row (max_depth 1: its only depth is the clamp bin), every other shape is piled"""
    base = X.v3_case(entry, rows=rows)
    if len(base.build[0]) == 1:
        return once(("v3_one_row", base.name), lambda: Case(base.name + "_md1", base.windows, base.build, base.nc, md=1, k=3, **base.note))
    return deepened(base, strict)


def auto_case(strict, rows=None):
    return deepened(X.auto_case(rows=rows), strict)


def inner_auto_case(strict, pairs=50_000, nc=24):
    """C: 2 x pairs short rows, row 2 i over [10 i, 10 i + 5) and row 2 i + 1 over [10 i + 3, 10 i + 8) of a contig (Weak: the same
    arrays, each row one position longer) -- pairs of rows that share 2 (3) positions and lie at least one position from the next
    pair: 3 blocks per pair in either mode.  At 50 000 pairs the build side has 100 000 rows (+ the piles' 18), below the
    automatic rule's 131 072, and 150 000 blocks, above it.  Probes: 6000 random ones of up to 300 positions, 6000 that are a
    build row, and the piles' (the pairs alone are 2 deep: the clamp bin of max_depth 6 needs the piles)."""
    def build():
        rng = np.random.default_rng(5100 + pairs)
        i = np.arange(pairs)
        c = np.repeat(i % nc, 2)
        s = np.stack([10 * (i // nc), 10 * (i // nc) + 3], axis=1).reshape(-1)
        frame = (c, s, s + 5)
        order = rng.permutation(2 * pairs)
        frame = tuple(a[order] for a in frame)
        n = min(6000, pairs)
        span = 10 * (pairs // nc)
        ps = rng.integers(-50, span, n)
        wins = X._cat((rng.integers(0, nc + 1, n), ps, ps + rng.integers(1, 300, n)), X.cover_windows(frame, nc, n, 5200, n_bins=1))
        return Case(f"inner_auto_{pairs}", wins, frame, nc)
    return deepened(once(("inner_auto", pairs, nc), build), strict, copies=8)


def sequence_case(rows=None):
    """D: X.sequence_case as it is (50 000 rows about five deep: no pile needed), so that the references of the other calls of
    the sequence are those of test_position_ops_matrix"""
    return X.sequence_case(rows=rows)


def rank_form(case, strict, md, ranks):
    """(hist, order statistics) by a third route, row by row, with no block list: the build rows of the probe's contig clipped to
    the probe; between two neighbouring clip points p the depth is #(starts <= p) - #(ends <= p) by two searchsorted calls; the
    histogram is a weighted bincount and a rank is looked up in the cumulative lengths of the pieces sorted by depth.  Works at
    any span (the per-base forms need small ones)."""
    pc, ps, pe = (np.asarray(a, np.int64) for a in case.windows)
    bc, bs, be1 = U._covering(*case.build, strict, case.nc)
    w = 0 if strict else 1
    hist = np.zeros((case.n, md + 1), np.int64)
    val = np.full(ranks.shape, -1, np.int64)
    for i in range(case.n):
        qs, qe = int(ps[i]), int(pe[i]) + w
        if qe <= qs or not 0 <= pc[i] < case.nc:
            continue
        on = (bc == pc[i]) & (bs < qe) & (be1 > qs)
        a, b = np.sort(np.maximum(bs[on], qs)), np.sort(np.minimum(be1[on], qe))
        pts = np.unique(np.concatenate([[qs, qe], a, b]))
        ln = np.diff(pts)
        depth = np.searchsorted(a, pts[:-1], "right") - np.searchsorted(b, pts[:-1], "right")
        hist[i] = np.bincount(np.minimum(depth, md), weights=ln, minlength=md + 1).astype(np.int64)
        order = np.argsort(depth, kind="stable")
        cum = np.cumsum(ln[order])
        ok = (ranks[i] >= 0) & (ranks[i] < qe - qs)
        val[i, ok] = depth[order][np.searchsorted(cum, ranks[i][ok], "right")]
    return hist, val


def dense_fits(case, strict, limit=20_000_000):
    """whether the per-base forms can hold the case: the contigs' spans together, and every probe, below `limit` positions"""
    bc, bs, be1 = U._covering(*case.build, strict, case.nc)
    total = sum(int(be1[bc == c].max() - bs[bc == c].min()) for c in np.unique(bc))
    return total < limit and int((case.windows[2].astype(np.int64) - case.windows[1]).max()) < limit


def sized_case(n, seed, strict, rows=None):
    """D: X.sized_case piled, and -- at 300 rows over 24 x 2000 positions, where most probes lie beside the rows -- as many cover
    windows as it has probes"""
    def build():
        base = X.sized_case(n, seed, rows=rows)
        return Case(f"{base.name}_covered", X._cat(base.windows, X.cover_windows(base.build, base.nc, base.n, 9600 + seed, n_bins=1)), base.build, base.nc)
    return deepened(once(("sized_covered", n, seed, rows), build), strict, copies=8 if n <= J.SMALL_ROWS else 1)


def a_case(strict, n=None, m=5000):
    base = X.a_case(strict, m=m) if n is None else X.a_case(strict, n=n, m=m)
    return deepened(base, strict, copies=8)


T_SINGLE, T_PAIR = 2, 3                # contigs of the T case: one block; two abutting blocks
T_BLOCKS = {T_SINGLE: [(1000, 1100, 1)], T_PAIR: [(1000, 1100, 2), (1100, 1250, 5)]}       # (start, half-open end, depth)
T_REACH = 37


def boundary_ranks(hist, L, k=Q.MAX_QUANT_RANKS):
    """k ranks per row around the row's cumulative boundaries: for the first (k - 1) // 3 depths the row holds, the number of
    positions below-or-at it (`covered-below`) - 1, itself and + 1, clipped to [0, L - 1]; the rest is the lower median.  hist:
    the row's histogram with no depth clamped."""
    n = len(L)
    ranks = np.repeat((np.maximum(L - 1, 0) // 2)[:, None], k, axis=1)
    for r in range(n):
        if L[r] <= 0:
            ranks[r] = 0
            continue
        cum = np.cumsum(hist[r])[hist[r] > 0][:(k - 1) // 3]
        want = np.clip(np.concatenate([cum - 1, cum, cum + 1]), 0, L[r] - 1)
        ranks[r, :len(want)] = want
    return ranks


def t_case(strict, cells=896, starts=12):
    """T: X.t_case(strict, 1) -- probes whose start and half-open end are points of a lattice on 2 contigs, the same probes one
    position off either way, one probe per contig from its smallest key to its largest -- over that case's 3 - 5-deep layers plus
    TWO identical rows on every even cell: the depth changes at every lattice point (by 2, which no layer's own edge cancels),
    so every lattice point is a block's start and the half-open end of the block before it, and the depth runs from 3 to 7.
    Contig T_SINGLE holds exactly one block, contig T_PAIR two abutting blocks of depth 2 and 5 (T_BLOCKS); probes of T_REACH
    positions end, and others start, just below, on and just above each of their boundaries.  Ranks (16 per row): around the
    cumulative boundaries of the row's own histogram (boundary_ranks)."""
    def build():
        w = 0 if strict else 1
        base = X.t_case(strict, 1, cells=cells, starts=starts)
        pitch = base.note["pitch"]
        rows, wins = [base.build], [base.windows]
        kind = list(base.note["kind"])
        even = np.arange(0, cells, 2)
        for c, origin in enumerate(X.T_ORIGIN):
            for _ in range(2):
                rows.append((np.full(len(even), c), origin + even * pitch, origin + (even + 1) * pitch - w))
        for c, blocks in T_BLOCKS.items():
            for s, e, d in blocks:
                rows.append((np.full(d, c), np.full(d, s), np.full(d, e - w)))
            for b in sorted({x for s, e, _ in blocks for x in (s, e)}):
                for d in (-1, 0, 1):
                    wins.append(([c, c], [b + d - T_REACH, b + d], [b + d - w, b + d + T_REACH - w]))
                    kind += [4, 4]
            wins.append(([c], [blocks[0][0] - 5], [blocks[-1][1] + 5 - w]))
            kind.append(4)
        probes, frame = X._cat(*wins), X._cat(*rows)
        nc = 4
        probes32, frame32 = U.as_i32(*probes), U.as_i32(*frame)
        ranks = boundary_ranks(H.block_form(probes32, frame32, strict, nc, 64), H.positions(probes32, strict, nc))
        ranks.setflags(write=False)
        return Case(f"t_dist_{cells}_{starts}_{strict}", probes, frame, nc, kind=np.array(kind), pitch=pitch, cells=cells, ranks=ranks, k=ranks.shape[1])
    return once(("t_dist", strict, cells, starts), build)


def lds_tile(max_depth, budget):
    """_depth_hist_util.tile generalised to a budget: the probe rows of one workgroup of k_depth_hist under IVJ_HIST_LDS_KB"""
    return min(max(budget // ((max_depth + 1) * 8), 1), H.HIST_MAX_TILE)


# name -> strict -> a scaled-down copy (at most 2000 rows per side) of the generator above
SCALED = {
    "t": lambda s: t_case(s, cells=56, starts=4),
    "sweep_64": lambda s: sweep_case(64, s, rows=300),
    "sweep_1025": lambda s: sweep_case(1025, s, rows=400),
    "sparse": lambda s: sparse_case(s, rows=300),
    "auto": lambda s: auto_case(s, rows=400),
    "inner_auto": lambda s: inner_auto_case(s, pairs=600),
    "sequence": lambda s: sequence_case(rows=400),
    "sized_large": lambda s: sized_case(150_000, 900, s, rows=400),
    "sized_small": lambda s: sized_case(J.SMALL_ROWS, 901, s),
    "a": lambda s: a_case(s, n=300, m=300),
}
for _k in range(X.V3_SHAPES):
    SCALED[f"v3_{_k}"] = lambda s, _k=_k: v3_case(X.v3_entries()[_k], s, rows=300)
