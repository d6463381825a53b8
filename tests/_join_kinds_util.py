"""The yardstick of the join kinds (test helper; numpy only): expected semi / anti rows and left outer pairs from the brute
forces the suite already trusts -- oracle.count_overlaps_brute / overlap_brute for the plain predicate, tests/_thresholds_util.brute
for the thresholded one.  The definitions of include/ivjoin.h, literally: with cnt[i] = count_overlaps of probe row i,

    semi = the rows with cnt[i] > 0, ascending        anti = the rows with cnt[i] == 0, ascending
    left = the inner pairs + (i, -1) for every anti row i

Contig ids outside [0, n_contigs) never match (a null chrom or on-value is -1)."""
import os
import re

import numpy as np

from oracle import oracle as O
import _thresholds_util as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEMI, ANTI = 0, 1


def kernel_tile():
    """Probes per workgroup of the selection kernel, from its header."""
    src = open(os.path.join(ROOT, "polars-bio_amd", "csrc", "select.hip.h")).read()
    threads = int(re.search(r"SELECT_THREADS\s*=\s*(\d+)", src).group(1))
    items = int(re.search(r"SELECT_ITEMS\s*=\s*(\d+)", src).group(1))
    return threads * items


def _oracle_sides(probe, build, n_contigs):
    """The C brute force compares contig ids literally: ids outside the dictionary are moved to values the other side lacks."""
    pc, bc = np.array(probe[0], np.int32), np.array(build[0], np.int32)
    pc[(pc < 0) | (pc >= n_contigs)] = np.iinfo(np.int32).min
    bc[(bc < 0) | (bc >= n_contigs)] = np.iinfo(np.int32).min + 1
    return O.Side(pc, probe[1], probe[2]), O.Side(bc, build[1], build[2])


def has_thresholds(thr):
    return any(v is not None for v in thr.values())


def counts(probe, build, n_contigs, strict, **thr):
    """count_overlaps per probe row (int64) under the plain predicate, or the thresholded one when a threshold is given."""
    if len(probe[0]) == 0:
        return np.zeros(0, np.int64)
    if has_thresholds(thr):
        return T.brute(probe, build, n_contigs, strict, **thr)[2]
    ps, bs = _oracle_sides(probe, build, n_contigs)
    return O.count_overlaps_brute(ps, bs, strict)


def inner_pairs(probe, build, n_contigs, strict, **thr):
    """The inner pairs sorted by (probe row, build row)."""
    if len(probe[0]) == 0 or len(build[0]) == 0:
        return np.empty(0, np.int32), np.empty(0, np.int32)
    if has_thresholds(thr):
        return T.brute(probe, build, n_contigs, strict, **thr)[:2]
    ps, bs = _oracle_sides(probe, build, n_contigs)
    return T.sort_pairs(*O.overlap_brute(ps, bs, strict))


def select_rows(cnt, mode):
    cnt = np.asarray(cnt)
    keep = (cnt > 0) if mode in (SEMI, "semi") else (cnt == 0)
    return np.flatnonzero(keep).astype(np.int32)


def expected(probe, build, n_contigs, strict, **thr):
    """-> dict: cnt, semi, anti (ascending rows), inner = (p, b) sorted, left = (p, b) sorted (the (i, -1) pairs sort first within row i)."""
    cnt = counts(probe, build, n_contigs, strict, **thr)
    semi, anti = select_rows(cnt, SEMI), select_rows(cnt, ANTI)
    ip, ib = inner_pairs(probe, build, n_contigs, strict, **thr)
    assert (np.bincount(ip, minlength=len(cnt)) == cnt).all(), "the two brute forces disagree"
    lp, lb = T.sort_pairs(np.concatenate([ip, anti]).astype(np.int32), np.concatenate([ib, np.full(len(anti), -1, np.int32)]).astype(np.int32))
    return dict(cnt=cnt, semi=semi, anti=anti, inner=(ip, ib), left=(lp, lb))


def assert_outer(got, exp, build, what=""):
    """A left outer result against expected(): the pair multiset, every probe row present, the (i, -1) tail ascending and behind
    every inner pair, the inner part under the contiguity / order contract of the inner join."""
    p, b = np.asarray(got[0]), np.asarray(got[1])
    n_inner, anti = len(exp["inner"][0]), exp["anti"]
    assert len(p) == len(b) == n_inner + len(anti), f"{what}: {len(p)} pairs, expected {n_inner + len(anti)}"
    T.assert_pairs((p, b), exp["left"], f"{what} outer pairs")
    assert (b[:n_inner] >= 0).all() and (b[n_inner:] == -1).all(), f"{what}: the unmatched rows do not follow the inner pairs"
    assert (p[n_inner:] == anti).all(), f"{what}: the (row, -1) tail is not the ascending anti rows"
    assert (np.unique(p) == np.arange(len(exp["cnt"]))).all(), f"{what}: a probe row is missing"
    T.assert_order(p[:n_inner], b[:n_inner], build)
