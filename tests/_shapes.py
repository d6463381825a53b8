"""Deterministic real-shaped interval sets for the parity tests (test helper; numpy only).

polars_bio_amd.synth draws flat sets: short rows, uniform positions.  Real interval sets are nested (alignment chains), have a
thin tail of long rows (genes among exons), arrive sorted by (contig, start) in runs, pile up at hot loci and repeat rows
exactly.  The generators here draw such sets from ``Generator(PCG64(seed))`` over the same 24 GRCh38 contigs as synth and
return ``(contig, start, end)`` int32 columns, unsorted unless stated.  Nothing is copied from published interval sets.

Scaling rule: every generator takes ``scale``; the contig lengths are multiplied by it.  Far share, mean depth and pairs per
probe are functions of the row DENSITY (rows per base) and of the length parameters, not of n: ``n * scale`` rows drawn with
``scale`` have the statistics of n rows drawn with scale 1 (tests/test_shapes.py checks the full-size parameters at scale
0.02 .. 0.1 that way).
"""
import numpy as np

from polars_bio_amd.synth import CONTIG_LENGTHS

CS_WIN = 12                 # cslice.hip.h: rows below hi the branch-free window covers
CS_FAR_LIMIT = 5e-4         # host_cslice.hip.h: far share above which the walking join kernel serves an index
CS_MIN_ROWS = 3072          # host_cslice.hip.h::cs_geom
HOT_CONTIG = 3              # chr4: the hot spot of chain_side / pileup_side
HOT_DIV = 500               # ... is 1 / 500 of that contig


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _lengths(n_contigs, scale):
    return np.maximum((CONTIG_LENGTHS[:n_contigs] * float(scale)).astype(np.int64), 10_000)


def _contigs(rng, n, lengths):
    nc = len(lengths)
    if nc == 1:
        return np.zeros(n, np.int64)
    return rng.choice(nc, size=n, p=lengths / lengths.sum()).astype(np.int64)


def hot_window(n_contigs=24, scale=1.0, hot_at=0.37):
    """(contig, lo, hi): 1 / HOT_DIV of one contig, starting at the fraction hot_at of it."""
    lengths = _lengths(n_contigs, scale)
    c = min(HOT_CONTIG, n_contigs - 1)
    w = int(lengths[c]) // HOT_DIV
    lo = int(hot_at * (int(lengths[c]) - w))
    return c, lo, lo + w


def uniform_side(n, seed, len_range=(100, 150), n_contigs=24, scale=1.0):
    """synth.make_side's flat shape (uniform positions, short rows) with this module's ``scale``."""
    rng = _rng(seed)
    lengths = _lengths(n_contigs, scale)
    c = _contigs(rng, n, lengths)
    L = rng.integers(len_range[0], len_range[1] + 1, size=n, dtype=np.int64)
    s = np.floor(rng.random(n) * (lengths[c] - L)).astype(np.int64)
    return c.astype(np.int32), s.astype(np.int32), (s + L).astype(np.int32)


def chain_side(n, seed, levels=4, fan=6, top_len=(5000, 300000), leaf=30, hot=0.0, shrink=(0.08, 0.42), n_contigs=24,
               scale=1.0, hot_at=0.37):
    """Nested "alignment chain" set: top-level blocks of log-uniform length in top_len at uniform positions; every block holds
    ``fan`` children of shrink x its length placed uniformly inside it, recursively down ``levels`` levels (no row shorter than
    ``leaf``); rows shuffled, the first n kept.  ``hot``: that share of the top-level blocks starts inside hot_window()."""
    rng = _rng(seed)
    lengths = _lengths(n_contigs, scale)
    per_top = sum(fan ** l for l in range(levels))
    n_top = -(-n // per_top)
    c = _contigs(rng, n_top, lengths)
    L = np.exp(rng.uniform(np.log(top_len[0]), np.log(top_len[1]), n_top)).astype(np.int64)
    L = np.minimum(L, lengths[c] // 2)
    s = np.floor(rng.random(n_top) * (lengths[c] - L)).astype(np.int64)
    if hot > 0:
        hc, lo, hi = hot_window(n_contigs, scale, hot_at)
        m = rng.random(n_top) < hot
        c[m] = hc
        L[m] = np.minimum(L[m], lengths[hc] // 2)
        s[m] = np.minimum(lo + np.floor(rng.random(int(m.sum())) * (hi - lo)).astype(np.int64), lengths[hc] - L[m])
    cs, ss, es = [c], [s], [s + L]
    for _ in range(1, levels):
        c, s, L = np.repeat(c, fan), np.repeat(s, fan), np.repeat(L, fan)
        cl = np.maximum((L * rng.uniform(shrink[0], shrink[1], len(L))).astype(np.int64), leaf)
        cl = np.minimum(cl, L)
        s = s + np.floor(rng.random(len(L)) * (L - cl + 1)).astype(np.int64)
        L = cl
        cs.append(c); ss.append(s); es.append(s + L)
    c, s, e = np.concatenate(cs), np.concatenate(ss), np.concatenate(es)
    keep = rng.permutation(len(c))[:n]
    return c[keep].astype(np.int32), s[keep].astype(np.int32), e[keep].astype(np.int32)


def tail_side(n, seed, gene_share, short_len=(200, 2000), gene_len=(30_000, 120_000), wide=0, n_contigs=24, scale=1.0):
    """Uniform short rows (exons) with a thin tail of long ones: a share gene_share of the rows gets a length in gene_len, and
    the first ``wide`` contigs get one contig-wide row each.  The far share grows with gene_share (every gene makes the
    rows that start inside it far, beyond the first CS_WIN); a contig-wide row makes EVERY row of its contig far, so the sets
    that sit near CS_FAR_LIMIT are drawn with wide = 0."""
    rng = _rng(seed)
    lengths = _lengths(n_contigs, scale)
    c = _contigs(rng, n, lengths)
    L = rng.integers(short_len[0], short_len[1] + 1, size=n, dtype=np.int64)
    g = rng.random(n) < gene_share
    L[g] = rng.integers(gene_len[0], gene_len[1] + 1, size=int(g.sum()), dtype=np.int64)
    L = np.minimum(L, lengths[c] // 2)
    s = np.floor(rng.random(n) * (lengths[c] - L)).astype(np.int64)
    e = s + L
    if wide > 0:
        rows = rng.choice(n, size=min(wide, n_contigs), replace=False)
        for k, r in enumerate(rows):
            c[r], s[r], e[r] = k, 0, lengths[k]
    return c.astype(np.int32), s.astype(np.int32), e.astype(np.int32)


def pileup_side(n, seed, read_len=(100, 150), loci_per_row=0.25, deep=0.05, deep_depth=200, hot=0.0, run=8192, absent=0.0,
                degenerate=0.0, window=None, n_contigs=24, scale=1.0, hot_at=0.37):
    """Read-like probes.  Rows are draws (with repetition) from n * loci_per_row distinct reads, so most rows have exact
    duplicates; a share ``deep`` of the rows falls on few loci with ~ deep_depth copies each; a share ``hot`` lies inside
    hot_window(); ``window`` = (contig, lo, hi) confines every read to that span (one bucket).  A share ``absent`` sits on
    contig id n_contigs (a contig the other side lacks: pass a dictionary of n_contigs + 1), a share ``degenerate`` is
    zero-length or inverted (half each).  The rows come in runs of ``run`` rows sorted by (contig, start), as from
    concatenated sorted files; run = 0: shuffled, run >= n: fully sorted."""
    rng = _rng(seed)
    lengths = _lengths(n_contigs, scale)
    n_loci = max(1, int(n * loci_per_row))
    n_deep = max(1, int(n * deep / deep_depth))
    lc = _contigs(rng, n_loci, lengths)
    ll = rng.integers(read_len[0], read_len[1] + 1, size=n_loci, dtype=np.int64)
    ls = np.floor(rng.random(n_loci) * (lengths[lc] - ll)).astype(np.int64)
    if hot > 0:
        hc, lo, hi = hot_window(n_contigs, scale, hot_at)
        m = rng.random(n_loci) < hot
        lc[m] = hc
        ls[m] = lo + np.floor(rng.random(int(m.sum())) * (hi - lo - ll[m])).astype(np.int64)
    if window is not None:
        wc, lo, hi = window
        lc[:] = wc
        ls = lo + np.floor(rng.random(n_loci) * max(1, hi - lo)).astype(np.int64)
    pick = rng.integers(0, n_loci, size=n)
    d = rng.random(n) < deep
    pick[d] = rng.integers(0, n_deep, size=int(d.sum()))           # the first n_deep loci are the deep ones
    c, s, e = lc[pick], ls[pick], ls[pick] + ll[pick]
    if absent > 0:
        c[rng.random(n) < absent] = n_contigs
    if degenerate > 0:
        u = rng.random(n)
        z = u < degenerate / 2
        e[z] = s[z]
        iv = (u >= degenerate / 2) & (u < degenerate)
        e[iv] = s[iv] - rng.integers(1, 50, size=int(iv.sum()))
    if run > 0:
        blk = np.arange(n, dtype=np.int64) // run if run < n else np.zeros(n, np.int64)
        o = np.argsort((blk << 40) | (c << 32) | s, kind="stable")          # (contig ids < 256, 0 <= start < 2^31)
        c, s, e = c[o], s[o], e[o]
    return c.astype(np.int32), s.astype(np.int32), e.astype(np.int32)


def slice_rows(n_build):
    """Rows per slice of the contig-aligned slice path for an index of n_build rows (host_cslice.hip.h::cs_geom, auto)."""
    r = max((n_build + 1023) // 1024, CS_MIN_ROWS)
    return (r + 63) // 64 * 64


def shape_stats(side, n_contigs, build=None, rows_per_slice=None):
    """CPU statistics of one side:
      far_share     share of the rows whose prefix max of the ends, CS_WIN sorted rows back inside their contig, is > their
                    start (the rule of cslice.hip.h::k_cs_bins; > CS_FAR_LIMIT: the walking join kernel serves the index)
      mean_depth    sum of the lengths / covered length (non-flatness; 1 = rows never overlap)
    and, with ``build``: ``side`` is a probe side and
      bucket_share  largest share of the probes in one of nb = ceil(n_build / R) equal-row slices of the sorted build side
                    (a probe belongs to the slice of the last build row that starts below its end)
      n_buckets     nb (the average bucket holds 1 / nb of the probes)."""
    c, s, e = (np.asarray(a).astype(np.int64) for a in side)
    n = len(c)
    o = np.lexsort((s, c))
    c, s, e = c[o], s[o], e[o]
    far, length_sum, covered = 0, 0, 0
    for k in np.unique(c):
        lo, hi = np.searchsorted(c, k, "left"), np.searchsorted(c, k, "right")
        ss, pm = s[lo:hi], np.maximum.accumulate(e[lo:hi])
        if hi - lo > CS_WIN:
            far += int((pm[:-CS_WIN] > ss[CS_WIN:]).sum())
        ee = e[lo:hi]
        length_sum += int(np.maximum(ee - ss, 0).sum())
        # union length: a row adds what lies beyond the prefix max of the rows before it
        prev = np.concatenate([[ss[0]], pm[:-1]]) if hi > lo else pm
        covered += int(np.maximum(ee - np.maximum(ss, prev), 0).sum())
    out = {"n": n, "far_share": far / max(n, 1), "mean_depth": length_sum / max(covered, 1)}
    if build is not None:
        bc, bs, _ = (np.asarray(a).astype(np.int64) for a in build)
        R = rows_per_slice or slice_rows(len(bc))
        key = np.sort((bc << 32) | (bs + (1 << 31)))
        heads = key[::R]
        nb = len(heads)
        pk = (np.asarray(side[0]).astype(np.int64) << 32) | (np.asarray(side[2]).astype(np.int64) + (1 << 31))
        b = np.clip(np.searchsorted(heads, pk, "left") - 1, 0, nb - 1)
        out["bucket_share"] = float(np.bincount(b, minlength=nb).max()) / max(n, 1)
        out["n_buckets"] = nb
    return out


# ---- the sides of tests/test_full_size_shapes.py (tests/test_shapes.py checks their statistics at reduced scale) --------------------
N_32MI = 32 << 20
CASE_A_BUILD = dict(n=5_000_000, seed=101)                                     # chain_side defaults: 4 levels, fan 6, 5 .. 300 kbp
CASE_A_PROBES = dict(n=N_32MI + 12_345, seed=102)                              # uniform_side: a ragged last tile beyond 32 Mi
CASE_B_PROBES = {                                                              # pileup_side over the case-A build side
    "sorted": dict(n=N_32MI + 777, seed=103, hot=0.1, absent=0.03, run=1 << 40),
    "hot": dict(n=N_32MI + 4_099, seed=104, hot=0.3, absent=0.03, run=8192),
    "one_bucket": dict(n=N_32MI, seed=105, absent=0.0, run=8192),              # + window = one slice of the build side
}
CASE_D_BUILD = dict(n=2_000_000, seed=106, shrink=(0.2, 0.8), scale=0.4)
CASE_D_PROBES = dict(n=4_000_000, seed=107, scale=0.4)
CASE_D_WIDE = 4                                                                # contig-wide rows added to the first contigs
CASE_E_BUILD = {"above": dict(n=1_000_000, seed=21, gene_share=8e-5), "below": dict(n=1_000_000, seed=21, gene_share=2e-5)}
CASE_E_PROBES = dict(n=10_000_000, seed=108)
CASE_F_BUILD = dict(n=2_000_000, seed=109)
CASE_F_PROBES = dict(n=20_000_000, seed=110, hot=0.1, absent=0.03, run=1 << 20)
CASE_F_COUNT_BUILD = dict(n=200_000, seed=111)
CASE_F_COUNT_PROBES = dict(n=100_000_000, seed=112, hot=0.1, absent=0.02, run=1 << 20)


def one_slice_window(build, k_of=0.4):
    """(contig, lo, hi): the start span of ONE slice of the sorted build side (the slice at the fraction k_of of the rows that
    lies wholly inside one contig) -- probes confined to it fall into one bucket (two at most)."""
    c, s = np.asarray(build[0]).astype(np.int64), np.asarray(build[1]).astype(np.int64)
    key = np.sort((c << 32) | s)
    R = slice_rows(len(c))
    k = int(k_of * (len(c) // R))
    while (key[k * R] >> 32) != (key[(k + 1) * R - 1] >> 32):
        k += 1
    return int(key[k * R] >> 32), int(key[k * R] & 0xffffffff), int(key[(k + 1) * R - 1] & 0xffffffff)


def with_wide_rows(side, n_wide, n_contigs=24, scale=1.0):
    """side + one contig-wide row on each of the first n_wide contigs (appended: rows keep their ids)."""
    lengths = _lengths(n_contigs, scale)
    c = np.concatenate([side[0], np.arange(n_wide, dtype=np.int32)])
    s = np.concatenate([side[1], np.zeros(n_wide, np.int32)])
    e = np.concatenate([side[2], lengths[:n_wide].astype(np.int32)])
    return c, s, e


def stretch_between_samples(probe, by=8_000_000):
    """Copy of a probe side whose every (512 x 37)-th row from row 100 on is stretched by ``by`` positions (more than a slice
    is wide): rows the 1 / 64 sample (8 rows every 512) never sees and an 8-byte record cannot hold."""
    c, s, e = (a.copy() for a in probe)
    idx = np.arange(100, len(c), 512 * 37)
    e[idx] = np.minimum(s[idx].astype(np.int64) + by, np.iinfo(np.int32).max).astype(np.int32)
    return c, s, e
