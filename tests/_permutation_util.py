"""The yardstick of pb.permutation_test (test helper; numpy only, no knowledge of tiles): for every permutation the shifted pieces
of every eligible df1 row are built LITERALLY in Python integers --

    hs = start - (closed ? 1 : 0), he = end;   eligible iff the contig is in the dictionary and 0 <= hs < he <= L
    s' = (hs + off) % L, e' = s' + (he - hs);  e' <= L: the piece [s', e'), otherwise the pieces [s', L) and [0, e' - L)

-- handed back to the frame's own coordinates and matched with _thresholds_util.brute(..., min_overlap=1): n_pairs = matching
(piece, build row) pairs, n_rows = distinct df1 rows among them.  ``ranks`` is the second, fast route for larger cases: the
two-rank identity #{b.hs < q.e} - #{b.he <= q.s} over the build rows that cover a position, with np.searchsorted."""
import os
import re

import numpy as np

import _thresholds_util as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_geometry():
    """(df1 rows per workgroup, rows per wavefront, permutations per block, permutations per launch at most), from the kernel's header."""
    src = open(os.path.join(ROOT, "polars-bio_amd", "csrc", "permute.hip.h")).read()
    get = lambda name: int(re.search(rf"constexpr int {name}\s*=\s*(\d+)", src).group(1))
    threads, items, block, chunk = get("PERM_THREADS"), get("PERM_ITEMS"), get("PERM_BLOCK"), get("PERM_CHUNK")
    assert "PERM_TILE = PERM_THREADS * PERM_ITEMS" in src
    return threads * items, 64 * items, block, chunk


def pieces_of(c, start, end, n_contigs, strict, lengths, off_row):
    """The half-open pieces [(s, e), ...] of ONE df1 row under one permutation's offsets; [] for an ineligible row."""
    c, one = int(c), 0 if strict else 1
    if c < 0 or c >= n_contigs:
        return []
    L, hs, he = int(lengths[c]), int(start) - one, int(end)
    if not (0 <= hs < he <= L):
        return []
    s = (hs + int(off_row[c])) % L
    e = s + (he - hs)
    return [(s, e)] if e <= L else [(s, L), (0, e - L)]


def shifted(probe, n_contigs, strict, lengths, offsets):
    """-> (piece frame (contig, start, end) in the frame's coordinates, permutation of each piece, df1 row of each piece)."""
    one = 0 if strict else 1
    pc, ps, pe = probe
    oc, os_, oe, operm, orow = [], [], [], [], []
    for p, off_row in enumerate(np.asarray(offsets).reshape(len(offsets), -1)):
        for i in range(len(pc)):
            for s, e in pieces_of(pc[i], ps[i], pe[i], n_contigs, strict, lengths, off_row):
                oc.append(int(pc[i])); os_.append(s + one); oe.append(e); operm.append(p); orow.append(i)
    return (np.array(oc, np.int64), np.array(os_, np.int64), np.array(oe, np.int64)), np.array(operm, np.int64), np.array(orow, np.int64)


def expected(probe, build, n_contigs, strict, lengths, offsets):
    """-> (n_pairs int64[n_perm], n_rows int64[n_perm]) by brute force."""
    n_perm, n = len(offsets), len(probe[0])
    frame, perm, row = shifted(probe, n_contigs, strict, lengths, offsets)
    _, _, counts = T.brute(frame, build, n_contigs, strict, min_overlap=1)
    pairs = np.zeros(n_perm, np.int64)
    np.add.at(pairs, perm, counts)
    hit = np.zeros((n_perm, max(n, 1)), bool)
    hit[perm[counts > 0], row[counts > 0]] = True
    return pairs.astype(np.int64), hit.sum(axis=1).astype(np.int64)


def ranks(probe, build, n_contigs, strict, lengths, offsets):
    """The same two arrays by the two-rank identity (vectorised; for cases too large for the brute force)."""
    one = 0 if strict else 1
    pc, ps, pe = (np.asarray(a, np.int64) for a in probe)
    bc, bs, be = (np.asarray(a, np.int64) for a in build)
    lengths, offsets = np.asarray(lengths, np.int64), np.asarray(offsets, np.int64).reshape(len(offsets), -1)
    bs = bs - one
    keep = (bc >= 0) & (bc < n_contigs) & (bs < be)
    bc, bs, be = bc[keep], bs[keep], be[keep]
    hs = ps - one
    inside = (pc >= 0) & (pc < n_contigs)
    L_row = np.where(inside, lengths[np.clip(pc, 0, max(n_contigs - 1, 0))] if n_contigs else 0, 0)
    ok = inside & (0 <= hs) & (hs < pe) & (pe <= L_row)
    n_perm = len(offsets)
    pairs, rows = np.zeros(n_perm, np.int64), np.zeros(n_perm, np.int64)
    for c in np.unique(pc[ok]):
        sel = ok & (pc == c)
        S, E = np.sort(bs[bc == c]), np.sort(be[bc == c])
        h, ln, L = hs[sel][None, :], (pe - hs)[sel][None, :], int(lengths[c])
        s1 = (h + offsets[:, c][:, None]) % L
        e1 = s1 + ln
        wrap = e1 > L
        cnt = lambda qs, qe: np.searchsorted(S, qe, "left") - np.searchsorted(E, qs, "right")
        first = cnt(s1, np.where(wrap, L, e1))
        second = np.where(wrap, cnt(np.zeros_like(s1), np.where(wrap, e1 - L, 1)), 0)
        pairs += (first + second).sum(axis=1)
        rows += ((first + second) > 0).sum(axis=1)
    return pairs, rows
