"""The yardstick of the overlap thresholds (test helper; numpy only): a brute force over all probe x build pairs of one contig,
O(n * m), that evaluates the LITERAL definitions of include/ivjoin.h --

    ov(a, b) = min(a.end, b.end) - max(a.start, b.start)      (+ 1 for 1-based closed frames)
    len(r)   = r.end - r.start                                (+ 1 for 1-based closed frames)
    min_overlap:  ov >= min_overlap
    min_frac1:    ov >= 1 and ov / len(a) >= min_frac1        the division in float64
    min_frac2:    ov >= 1 and ov / len(b) >= min_frac2

-- never the integer minima the front door derives from the fractions.  The engine-level per-row minima (probe_min / build_min:
uint32 base counts, 0 = no requirement, NEVER = the row never matches) are a separate input, tested as ov >= minimum.  Every
threshold that is given must hold, and any of them implies ov >= 1.  Contig ids outside [0, n_contigs) never match."""
import os
import re

import numpy as np

NEVER = 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_tile():
    """Probes per workgroup of the thresholded kernel, from its header."""
    src = open(os.path.join(ROOT, "polars-bio_amd", "csrc", "thresh.hip.h")).read()
    threads = int(re.search(r"THRESH_THREADS\s*=\s*(\d+)", src).group(1))
    items = int(re.search(r"THRESH_ITEMS\s*=\s*(\d+)", src).group(1))
    return threads * items


def brute(probe, build, n_contigs, strict, min_overlap=None, min_frac1=None, min_frac2=None, probe_min=None, build_min=None, rows=256):
    """-> (probe_idx, build_idx) sorted by (probe row, build row), and the per-probe counts (int64)."""
    pc, ps, pe = (np.asarray(a, np.int64) for a in probe)
    bc, bs, be = (np.asarray(a, np.int64) for a in build)
    one = 0 if strict else 1
    plen, blen = pe - ps + one, be - bs + one
    pm = None if probe_min is None else np.asarray(probe_min, np.uint32).astype(np.int64)
    bm = None if build_min is None else np.asarray(build_min, np.uint32).astype(np.int64)
    outp, outb = [np.empty(0, np.int64)], [np.empty(0, np.int64)]
    for c in np.unique(pc):
        if c < 0 or c >= n_contigs:
            continue
        P, B = np.nonzero(pc == c)[0], np.nonzero(bc == c)[0]
        if len(B) == 0:
            continue
        for lo in range(0, len(P), rows):
            p = P[lo:lo + rows]
            ov = np.minimum(pe[p][:, None], be[B][None, :]) - np.maximum(ps[p][:, None], bs[B][None, :]) + one
            keep = ov >= 1
            if min_overlap is not None:
                keep &= ov >= int(min_overlap)
            with np.errstate(divide="ignore", invalid="ignore"):
                if min_frac1 is not None:
                    keep &= (plen[p] > 0)[:, None] & ((ov.astype(np.float64) / plen[p].astype(np.float64)[:, None]) >= float(min_frac1))
                if min_frac2 is not None:
                    keep &= (blen[B] > 0)[None, :] & ((ov.astype(np.float64) / blen[B].astype(np.float64)[None, :]) >= float(min_frac2))
            if pm is not None:
                keep &= (pm[p] != NEVER)[:, None] & (ov >= pm[p][:, None])
            if bm is not None:
                keep &= (bm[B] != NEVER)[None, :] & (ov >= bm[B][None, :])
            i, j = np.nonzero(keep)
            outp.append(p[i])
            outb.append(B[j])
    qp, qb = np.concatenate(outp), np.concatenate(outb)
    o = np.lexsort((qb, qp))
    qp, qb = qp[o].astype(np.int32), qb[o].astype(np.int32)
    return qp, qb, np.bincount(qp, minlength=len(pc)).astype(np.int64)


def sort_pairs(p, b):
    p, b = np.asarray(p), np.asarray(b)
    o = np.lexsort((b, p))
    return p[o], b[o]


def assert_pairs(got, exp, what=""):
    gp, gb = sort_pairs(*got)
    assert len(gp) == len(exp[0]), f"{what}: {len(gp)} pairs, expected {len(exp[0])}"
    assert (gp == exp[0]).all() and (gb == exp[1]).all(), f"{what}: pair sets differ"


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
