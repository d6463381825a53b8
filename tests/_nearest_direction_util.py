"""Expected answers of the directional nearest (``nearest_ignore``), from the read-only oracle alone.

``oracle.nearest_brute`` with ``k = n_build`` gives every probe's FULL candidate list in the oracle's total order
(distance, class, build.start, build row) -- oracle/ivj_oracle.c:73-108.  The class of each listed row is recomputed here in numpy
from the two predicates that define it; the directional answer is that list with the rows of the ignored classes removed, cut to k
and padded with -1."""
import numpy as np

from oracle import oracle as O

IGNORE_LEFT, IGNORE_RIGHT = 1, 2


def _lt(x, y, strict):
    return x < y if strict else x <= y


def full_lists(probe, build, strict, include_overlaps=True):
    """-> (idx, dist, cls), each n_probe x n_build: the ordered candidate list of every probe, -1 past its end.
    cls: 0 the row overlaps the probe, 1 "left" (build.start (<) probe.end without an overlap), 2 "right" (everything else)."""
    nb = len(build[0])
    idx, dist, _ = O.nearest_brute(O.Side(*probe), O.Side(*build), strict, k=nb, include_overlaps=include_overlaps)
    j = np.maximum(idx, 0)
    qs = np.asarray(probe[1], np.int64)[:, None]
    qe = np.asarray(probe[2], np.int64)[:, None]
    bs, be = np.asarray(build[1], np.int64)[j], np.asarray(build[2], np.int64)[j]
    a = _lt(bs, qe, strict)                    # build.start (<) probe.end
    b = _lt(qs, be, strict)                    # probe.start (<) build.end
    cls = np.where(a & b, 0, np.where(a, 1, 2))
    cls[idx < 0] = -1
    return idx, dist, cls


def directed(lists, mask, k):
    """The first k rows of every list after the classes in ``mask`` (a scalar, or one value per probe) are dropped."""
    idx, dist, cls = lists
    n, nb = idx.shape
    m = np.broadcast_to(np.asarray(mask, np.int64), (n,))[:, None]
    drop = ((cls == 1) & ((m & IGNORE_LEFT) != 0)) | ((cls == 2) & ((m & IGNORE_RIGHT) != 0))
    keep = (idx >= 0) & ~drop
    order = np.argsort(~keep, axis=1, kind="stable")          # kept rows first, their order unchanged
    kept = np.take_along_axis(keep, order, 1)
    oi = np.where(kept, np.take_along_axis(idx, order, 1), -1).astype(np.int32)
    od = np.where(kept, np.take_along_axis(dist, order, 1), -1).astype(np.int64)
    if nb < k:
        oi = np.concatenate([oi, np.full((n, k - nb), -1, np.int32)], 1)
        od = np.concatenate([od, np.full((n, k - nb), -1, np.int64)], 1)
    return np.ascontiguousarray(oi[:, :k]), np.ascontiguousarray(od[:, :k]), np.minimum(keep.sum(1), k).astype(np.int32)


def left_right_ties(lists):
    """Probes whose closest left row and closest right row are equally far (the left one must win)."""
    idx, dist, cls = lists
    big = np.iinfo(np.int64).max
    dl = np.where(cls == 1, dist, big).min(1)
    dr = np.where(cls == 2, dist, big).min(1)
    return (dl == dr) & (dl != big)
