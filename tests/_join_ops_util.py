"""Inputs, fast references and the call lists of tests/test_join_ops_matrix.py: the thresholded join / count (thresh.hip.h) and the
merge aggregates (merge_agg.hip.h) across contig-dictionary sizes, index build forms, partition modes, row ids and call sequences.

The literal yardsticks (_thresholds_util.brute, O(n * m); _merge_agg_util.group_by, one full mask per cluster) are too slow for
matrix sizes, so each gets ONE fast form here, shown equal to the literal one on the CPU (test_join_ops_matrix.py):

  sorted_candidates   per contig the build rows sorted by start; the candidates of a probe are the build rows with
                      start < probe.end (Weak: <=) and start >= probe.start - (longest build row of the contig); on those pairs
                      the literal definitions of _thresholds_util's docstring.  Knows nothing of tiles, chunks or tables.
  group_by_fast       np.lexsort on the oracle's cluster ids, then np.add.reduceat in the column's dtype (int64 wraps),
                      np.fmin.reduceat / np.fmax.reduceat and counts of valid values.

numpy, int64 and float64 only; every comparison is bit-exact."""
import numpy as np

import _depth_util as U
import _merge_agg_util as M
import _position_ops_util as P
import _thresholds_util as T
import test_contig_dictionaries as D
from polars_bio_amd import range_op

NEVER = T.NEVER
I64, F64 = np.int64, np.float64
ALL = list(M.OPS)
THR = dict(min_overlap=3, min_frac1=0.25, min_frac2=0.25)          # the threshold set of the matrix
TILE = T.kernel_tile()
MAGG_TILE = M.kernel_tile()


# ---- thresholds: the sorted-candidate reference -------------------------------------------------------------------------------------

def sorted_candidates(probe, build, n_contigs, strict, min_overlap=None, min_frac1=None, min_frac2=None, probe_min=None, build_min=None,
                      cells=1 << 22):
    """-> (probe_idx, build_idx) int32 sorted by (probe row, build row), and the per-probe counts (int64): what _thresholds_util.brute
    returns, from per-contig sorted candidate ranges instead of the full probe x build matrix."""
    pc, ps, pe = (np.asarray(a, np.int64) for a in probe)
    bc, bs, be = (np.asarray(a, np.int64) for a in build)
    one = 0 if strict else 1
    plen, blen = pe - ps + one, be - bs + one
    pm = None if probe_min is None else np.asarray(probe_min, np.uint32).astype(np.int64)
    bm = None if build_min is None else np.asarray(build_min, np.uint32).astype(np.int64)
    outp, outb = [np.empty(0, np.int64)], [np.empty(0, np.int64)]
    b_order = np.lexsort((bs, bc))                                       # (contig, start), equal keys in row order
    b_keys = bc[b_order]
    p_order = np.argsort(pc, kind="stable")
    p_keys = pc[p_order]
    for c in np.unique(pc):
        if c < 0 or c >= n_contigs:
            continue
        B = b_order[np.searchsorted(b_keys, c, "left"):np.searchsorted(b_keys, c, "right")]
        if len(B) == 0:
            continue
        Pr = p_order[np.searchsorted(p_keys, c, "left"):np.searchsorted(p_keys, c, "right")]
        starts = bs[B]
        longest = int((be[B] - bs[B]).max())
        lo = np.searchsorted(starts, ps[Pr] - longest, "left")
        hi = np.searchsorted(starts, pe[Pr], "left" if strict else "right")
        cn = np.maximum(hi - lo, 0)
        ends = np.cumsum(cn)
        at = 0
        while at < len(Pr):
            base = ends[at - 1] if at else 0
            to = max(int(np.searchsorted(ends, base + cells, "right")), at + 1)
            k = cn[at:to]
            if k.sum():
                rep = np.repeat(np.arange(at, to), k)
                within = np.arange(int(k.sum())) - np.repeat(ends[at:to] - k - base, k)
                p, b = Pr[rep], B[lo[rep] + within]
                ov = np.minimum(pe[p], be[b]) - np.maximum(ps[p], bs[b]) + one
                keep = ov >= 1
                if min_overlap is not None:
                    keep &= ov >= int(min_overlap)
                with np.errstate(divide="ignore", invalid="ignore"):
                    if min_frac1 is not None:
                        keep &= (plen[p] > 0) & ((ov.astype(F64) / plen[p].astype(F64)) >= float(min_frac1))
                    if min_frac2 is not None:
                        keep &= (blen[b] > 0) & ((ov.astype(F64) / blen[b].astype(F64)) >= float(min_frac2))
                if pm is not None:
                    keep &= (pm[p] != NEVER) & (ov >= pm[p])
                if bm is not None:
                    keep &= (bm[b] != NEVER) & (ov >= bm[b])
                outp.append(p[keep])
                outb.append(b[keep])
            at = to
    qp, qb = np.concatenate(outp), np.concatenate(outb)
    o = np.lexsort((qb, qp))
    qp, qb = qp[o].astype(np.int32), qb[o].astype(np.int32)
    return qp, qb, np.bincount(qp, minlength=len(pc)).astype(np.int64)


def lengths(side, strict):
    return side[2].astype(np.int64) - side[1].astype(np.int64) + (0 if strict else 1)


def engine_kw(probe, build, strict, min_overlap=None, min_frac1=None, min_frac2=None, probe_min=None, build_min=None):
    """what the engine receives for a threshold set: the fractions as the minima of range_op.min_bases, ANDed with given minima by
    the maximum (as test_thresholds_gpu._engine_kw)"""
    pm = None if probe_min is None else np.asarray(probe_min, np.uint32)
    bm = None if build_min is None else np.asarray(build_min, np.uint32)
    if min_frac1 is not None:
        f = range_op.min_bases(lengths(probe, strict), min_frac1)
        pm = f if pm is None else np.maximum(pm, f)
    if min_frac2 is not None:
        f = range_op.min_bases(lengths(build, strict), min_frac2)
        bm = f if bm is None else np.maximum(bm, f)
    return dict(min_overlap=int(min_overlap or 0), probe_min=pm, build_min=bm)


def never_mix(rng, n):
    return rng.choice(np.array([0, 3, 40, NEVER], np.uint32), n)


# ---- thresholds: the four entries ------------------------------------------------------------------------------------------------------

def dev_cols(cols, shift=0):
    """int32 columns in HBM; shift: each column is a view that starts `shift` elements into a larger tensor (shift % 4 != 0: not
    16-byte aligned, the kernels' vector loads are off)"""
    import torch
    out = []
    for a in cols:
        a = np.ascontiguousarray(a, np.int32)
        if shift == 0:
            out.append(torch.from_numpy(a.copy()).cuda())
        else:
            big = torch.full((len(a) + shift + 8,), -7, dtype=torch.int32, device="cuda")
            big[shift:shift + len(a)] = torch.from_numpy(a).cuda()
            out.append(big[shift:shift + len(a)])
            assert out[-1].is_contiguous() and out[-1].data_ptr() % 16 == (4 * shift) % 16
    return out


def dev_side(side, row_id=None, shift=0):
    from polars_bio_amd.device_api import DeviceSide
    cols = dev_cols(list(side) + ([row_id] if row_id is not None else []), shift)
    return DeviceSide(*cols)


def dev_min(m):
    import torch
    return None if m is None else torch.from_numpy(np.ascontiguousarray(m, np.uint32).view(np.int32).copy()).cuda()


def thresh_run(eng, dj, probe, build, nc, strict, kw, partition_mode=0, probe_row_id=None, build_row_id=None, index=None, shift=0):
    """the thresholded join and count through the four entries -> dict "host_pairs", "host_counts", "dev_pairs", "dev_counts".
    eng None (or a side with a row id, which the host binding cannot carry): device entries only.  index: a DeviceIndex of the
    build side that both device entries use."""
    got = {}
    if eng is not None and probe_row_id is None and build_row_id is None:
        p, b = eng.overlap_thresh(probe, build, strict, nc, partition_mode=partition_mode, **kw)
        got["host_pairs"] = (np.array(p), np.array(b))
        got["host_counts"] = eng.count_overlaps_thresh(probe, build, strict, nc, partition_mode=partition_mode, **kw)
    dp, db = dev_side(probe, probe_row_id, shift), dev_side(build, build_row_id, shift)
    dkw = dict(min_overlap=kw["min_overlap"], probe_min=dev_min(kw["probe_min"]), build_min=dev_min(kw["build_min"]))
    gp, gb = dj.overlap_thresh(dp, db, strict, nc, index=index, partition_mode=partition_mode, **dkw)
    got["dev_pairs"] = (gp.cpu().numpy(), gb.cpu().numpy())
    got["dev_counts"] = dj.count_overlaps_thresh(dp, db, strict, nc, index=index, partition_mode=partition_mode, **dkw).cpu().numpy()
    return got


def positions_of(ids, reported, what):
    """reported ids -> positions in the column `ids` (an injective map); an id that is no element of `ids` fails"""
    ids = np.asarray(ids, np.int64)
    order = np.argsort(ids, kind="stable")
    r = np.asarray(reported, np.int64)
    at = np.minimum(np.searchsorted(ids[order], r), len(ids) - 1)
    assert len(r) == 0 or (ids[order][at] == r).all(), f"{what}: reported ids that are not in the row_id column"
    return order[at]


def thresh_check(got, exp, build, what, probe_row_id=None, build_row_id=None):
    """every entry of thresh_run against (probe_idx, build_idx, counts) of the reference, the documented pair order included.
    With row ids the pairs are brought back to positions first (they must report ids: a position is no element of the id column);
    the counts always go by position."""
    ep, eb, ecnt = exp
    assert got, what
    for key, g in got.items():
        if key.endswith("pairs"):
            p, b = g
            assert p.dtype == np.int32 and b.dtype == np.int32, f"{what} {key}"
            if probe_row_id is not None:
                p = positions_of(probe_row_id, p, f"{what} {key} probe")
            if build_row_id is not None:
                b = positions_of(build_row_id, b, f"{what} {key} build")
            T.assert_order(p, b, build)
            T.assert_pairs((p, b), (ep, eb), f"{what} {key}")
        else:
            assert g.dtype == np.int64 and len(g) == len(ecnt) and (g == ecnt).all(), f"{what} {key}"


def thresh_blob(got):
    """the results of thresh_run as bytes, pair order included"""
    parts = []
    for key in sorted(got):
        g = got[key]
        parts += [np.ascontiguousarray(a).tobytes() for a in (g if isinstance(g, tuple) else (g,))]
    return b"|".join(parts)


def assert_thresh_same(got, ref, what, keys=None):
    for key in (keys or ref):
        g, r = got[key], ref[key]
        for x, y in zip(g if isinstance(g, tuple) else (g,), r if isinstance(r, tuple) else (r,)):
            assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), f"{what}: {key} differs"


def reindexed(pairs, keep_p, keep_b):
    """pairs on the full sides -> the same pairs on the sides cut to the rows of keep_p / keep_b (every pair must survive the cut)"""
    p, b = pairs
    assert keep_p[p].all() and keep_b[b].all(), "a pair holds a row that the cut removes"
    return (np.cumsum(keep_p) - 1)[p].astype(np.int32), (np.cumsum(keep_b) - 1)[b].astype(np.int32)


def kept_and_removed(probe, build, nc, strict, thr):
    """(pairs the threshold set keeps, pairs the plain predicate keeps)"""
    return len(sorted_candidates(probe, build, nc, strict, **thr)[0]), len(sorted_candidates(probe, build, nc, strict, min_overlap=1)[0])


# ---- merge aggregates: the vectorised group-by ------------------------------------------------------------------------------------------

def group_by_fast(cid, n_clusters, values, valid=None):
    """-> dict op -> array with one entry per cluster, and "has": the clusters with a valid value (min / max / mean are unspecified
    elsewhere: group_by reports None there; sum is 0)"""
    values = np.asarray(values)
    assert values.dtype in (I64, F64)
    cid = np.asarray(cid, np.int64)
    use = np.ones(len(values), bool) if valid is None else np.asarray(valid).astype(bool)
    order = np.lexsort((cid,))                                            # stable: rows of a cluster in input order
    order = order[use[order]]
    v, k = values[order], cid[order]
    count = np.bincount(k, minlength=n_clusters).astype(I64)
    out = {"count": count, "has": count > 0, "sum": np.zeros(n_clusters, values.dtype), "min": np.zeros(n_clusters, values.dtype),
           "max": np.zeros(n_clusters, values.dtype), "mean": np.zeros(n_clusters, F64)}
    if len(v):
        first = np.flatnonzero(np.concatenate([[True], k[1:] != k[:-1]]))
        present = k[first]
        with np.errstate(over="ignore", invalid="ignore"):
            out["sum"][present] = np.add.reduceat(v, first, dtype=values.dtype)
            out["min"][present] = np.fmin.reduceat(v, first)
            out["max"][present] = np.fmax.reduceat(v, first)
            out["mean"][present] = out["sum"][present].astype(F64) / count[present].astype(F64)
    return out


def as_lists(fast):
    """group_by_fast's result in group_by's form (None where the op has no value)"""
    has = fast["has"]
    return {op: [fast[op][k] if (has[k] or op in ("sum", "count")) else None for k in range(len(has))] for op in ALL}


def assert_lists_equal(a, b, dtype, what):
    """two results in group_by's form, bit for bit (a NaN equals a NaN)"""
    for op in ALL:
        kind = I64 if op == "count" else F64 if op == "mean" else dtype
        assert len(a[op]) == len(b[op]), (what, op)
        for k, (x, y) in enumerate(zip(a[op], b[op])):
            assert (x is None) == (y is None), (what, op, k)
            if x is not None and not (kind == F64 and np.isnan(x) and np.isnan(y)):
                assert M.bits(x, kind) == M.bits(y, kind), (what, op, k, x, y)


def assert_agg_equal(got, exp, dtype, what):
    """got: dict op -> array of the engine for one value column; exp: group_by_fast's.  Bit for bit; entries without a valid value
    are unspecified for min / max / mean and skipped; a NaN expected compares as NaN (_merge_agg_util.assert_column, vectorised)."""
    assert set(got) == set(ALL), what
    for op in ALL:
        kind = I64 if op == "count" else F64 if op == "mean" else dtype
        g, x = np.asarray(got[op]), exp[op]
        assert g.dtype == kind and g.shape == x.shape, f"{what} {op}: {g.dtype} {g.shape}, expected {np.dtype(kind)} {x.shape}"
        look = np.ones(len(x), bool) if op in ("sum", "count") else exp["has"]
        same = g.view(np.uint64) == x.view(np.uint64)
        if kind == F64:
            same |= np.isnan(g) & np.isnan(x)
        bad = np.flatnonzero(look & ~same)
        assert len(bad) == 0, f"{what} {op}: {len(bad)} clusters differ, first {bad[0]}: got {g[bad[0]]!r}, expected {x[bad[0]]!r}"


def wide_ints(n, seed):
    """int64 over the full range: the sums of clusters wrap"""
    return np.random.default_rng(seed).integers(np.iinfo(I64).min, np.iinfo(I64).max, n, dtype=I64, endpoint=True)


def whole_doubles(n, seed, nan=0.05):
    """integer-valued doubles (test_merge_agg_gpu.whole_doubles: every summation order is exact) with NaNs among them"""
    rng = np.random.default_rng(seed)
    v = rng.integers(-(1 << 30), 1 << 30, n).astype(F64)
    v[rng.random(n) < nan] = np.nan
    return v


def agg_columns(n, seed):
    """the two value columns of the matrix: int64 over the full range with a validity mask, integer-valued float64 with NaNs"""
    mask = np.random.default_rng(seed + 2).random(n) < 0.8
    return [(wide_ints(n, seed), mask, ALL), (whole_doubles(n, seed + 1), None, ALL)]


_agg_expected = {}


def agg_expected(name, side, nc, strict, min_dist, columns):
    """(merged table, [group_by_fast per column]) of a named input, computed once"""
    key = (name, strict, min_dist)
    if key not in _agg_expected:
        cid, table = M.clusters(side, nc, strict, min_dist)
        _agg_expected[key] = (table, [group_by_fast(cid, len(table[0]), v, m) for v, m, _ in columns])
    return _agg_expected[key]


def agg_dev_call(engine, ix, nc, strict, min_dist, columns, capacity):
    """ivj_merge_agg_dev on a given DeviceIndex -> (table arrays, [dict per column])"""
    import torch
    from polars_bio_amd import _engine
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                     # noqa: E731
    table = [torch.empty(max(capacity, 1), dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.int32, torch.int64)]
    held, cols, outs = [], [], []
    for v, m, ops in columns:
        tv, tm = up(v), None if m is None else up(np.asarray(m).astype(np.uint8))
        held.append((tv, tm))
        cols.append((tv.data_ptr(), 0 if tm is None else tm.data_ptr(), _engine.AGG_I64 if v.dtype == I64 else _engine.AGG_F64,
                     _engine.agg_ops_mask(ops)))
        outs.append({op: torch.empty(max(capacity, 1), dtype=torch.float64 if op == "mean" or (v.dtype == F64 and op != "count") else torch.int64,
                                     device=dev) for op in ops})
    n, fits = engine.merge_agg_dev(ix, _engine.make_opts(strict, nc), min_dist, capacity, *(t.data_ptr() for t in table), len(columns[0][0]), cols,
                                   [{op: t.data_ptr() for op, t in o.items()} for o in outs])
    torch.cuda.synchronize()
    assert fits, (n, capacity)
    return [t[:n].cpu().numpy() for t in table], [{op: t[:n].cpu().numpy() for op, t in o.items()} for o in outs]


def agg_run(eng, dj, side, nc, strict, min_dist, columns):
    """host form and device form -> dict "host" / "device" -> (table, [dict per column])"""
    import torch
    from polars_bio_amd.device_api import DeviceSide
    got = {}
    if eng is not None:
        *table, res = eng.merge_agg(side, strict, nc, columns, min_dist)
        got["host"] = (table, res)
    if dj is not None:
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()                  # noqa: E731
        agg = [(up(v), None if m is None else up(np.asarray(m).astype(np.uint8)), ops) for v, m, ops in columns]
        *table, res = dj.merge(DeviceSide(*map(up, U.as_i32(*side))), strict, nc, min_dist, agg=agg)
        got["device"] = ([t.cpu().numpy() for t in table], [{k: t.cpu().numpy() for k, t in r.items()} for r in res])
    return got


def agg_check(got, exp, columns, what):
    etable, eres = exp
    assert got, what
    for name, (table, res) in got.items():
        for k in range(4):
            assert np.asarray(table[k]).dtype == etable[k].dtype and len(table[k]) == len(etable[k]) and (table[k] == etable[k]).all(), \
                f"{what} {name}: merged table column {k}"
        assert len(res) == len(columns), (what, name)
        for j, (v, _, _) in enumerate(columns):
            assert_agg_equal(res[j], eres[j], v.dtype, f"{what} {name} column {j}")


def agg_blob(got):
    """the results of agg_run as bytes; min / max / mean of clusters without a valid value (unspecified) blanked"""
    parts = []
    for name in sorted(got):
        table, res = got[name]
        parts += [np.ascontiguousarray(a).tobytes() for a in table]
        for r in res:
            has = r["count"] > 0
            for op in ALL:
                a = np.array(r[op]).view(np.uint64)
                if op in ("min", "max", "mean"):
                    a = np.where(has, a, 0)
                parts.append(a.tobytes())
    return b"|".join(parts)


def tiles_crossed(cid_sorted_sizes, tile):
    """how many tile boundaries of the sorted order fall strictly inside a cluster, given the cluster sizes in sorted order"""
    ends = np.cumsum(cid_sorted_sizes)
    inner = np.arange(tile, int(ends[-1]), tile)
    return int((~np.isin(inner, ends)).sum()) if len(inner) else 0


# ---- the inputs ------------------------------------------------------------------------------------------------------------------------

_inputs = {}


def _once(key, build):
    if key not in _inputs:
        sides = build()
        for side in sides[:2]:
            for a in side:
                a.setflags(write=False)
        _inputs[key] = sides
    return _inputs[key]


def partition_sides(n_probe=3 * TILE + 17, n_build=5000, nc=24, seed=61):
    """A1 / A2 / A4: probes in random (not position-sorted) order x 5000 build rows on 24 contigs, and minima with NEVER mixed in"""
    def build():
        rng = np.random.default_rng(seed + n_probe)
        probe, frame = D.random_side(rng, n_probe, nc, 20_000, 300), D.random_side(rng, n_build, nc, 20_000, 400)
        return U.as_i32(*probe), U.as_i32(*frame), dict(min_overlap=2, probe_min=never_mix(rng, n_probe), build_min=never_mix(rng, n_build))
    return _once(("partition", n_probe, n_build, nc, seed), build)


def probe_ids(n, seed=7):
    """a probe row_id that is an injective non-identity map with every value above n: a position used where an id belongs (or the
    reverse) is out of the other's range"""
    return (n + 11 + 3 * np.random.default_rng(seed).permutation(n)).astype(np.int32)


def build_ids(n, seed=8):
    """a build row_id: a permutation of [0, n) with six ids moved outside [0, n) -> (ids, the positions that carry outside ids)"""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(n).astype(np.int64)
    moved = rng.choice(n, 6, replace=False)
    ids[moved] = [-1, -5, n, n + 1000, np.iinfo(np.int32).max, np.iinfo(np.int32).min]
    return ids.astype(np.int32), moved


def sweep_sides(nc, n_build=8000, n_probe=6000):
    """B1 / B2 / B4: test_contig_dictionaries._sweep_sides, smaller: every 7th contig empty on the build side, every OUTSIDE id on
    both sides.  (From 2047 contigs on a contig holds a few rows only: a shorter span keeps hundreds of pairs under the thresholds.)"""
    span = 5000 if nc < 2000 else 1000
    return _once(("sweep", nc, n_build, n_probe),
                 lambda: tuple(U.as_i32(*s) for s in D._sweep_sides(nc, 8100 + nc, n_build=n_build, n_probe=n_probe, span=span)))


def sparse_sides(n_build=12_000, n_probe=8000, occupied=3000):
    """B3: 2^24 + 1 ids, a few heavy contigs, thousands of single-row ones, ids 0 and nc - 1 occupied, every OUTSIDE id on both sides"""
    def build():
        nc, span = P.SPARSE_NC, 1_000_000
        rng = np.random.default_rng(425)
        frame = D.sparse_side(rng, n_build, nc, occupied, span, 2000)
        pc = np.where(rng.random(n_probe) < 0.8, frame[0][rng.integers(0, n_build, n_probe)], rng.integers(0, nc, n_probe)).astype(np.int32)
        ps = rng.integers(0, span, n_probe)
        probe = U.as_i32(pc, ps, ps + rng.integers(0, 3000, n_probe))
        return U.as_i32(*D._plant_outside(rng, probe, nc)), U.as_i32(*D._plant_outside(rng, frame, nc))
    return _once(("sparse", n_build, n_probe, occupied), build)


V3_PROBES = 12_000


def v3_sides(entry):
    """C1: a shape of test_gpu_parity._v3_cases(): (its first V3_PROBES probes and 1500 shifted copies of build rows, its build
    side, n_contigs).  The copies -- a build row moved by up to its own length either way -- give every shape pairs that the
    thresholds keep and pairs they remove: the probes of the one-row and the 33-bit shapes on their own hit next to nothing.
    Where more than 10 000 build rows share one start every hit is 10 000 pairs: 1000 probes and 40 copies there, which keeps the
    result near a million pairs."""
    name, probe, frame, nc, balanced = entry
    rng = np.random.default_rng(len(name))
    stacked = np.unique(frame[0].astype(np.int64) << 32 | frame[1].astype(np.int64) & 0xffffffff, return_counts=True)[1].max() > 10_000
    r = rng.integers(0, len(frame[0]), 40 if stacked else 1500)
    s, e = frame[1][r].astype(np.int64), frame[2][r].astype(np.int64)
    reach = np.maximum(e - s, 8)
    d = rng.integers(-reach, reach + 1)
    lim = np.iinfo(np.int32)
    copies = (frame[0][r], np.clip(s + d, lim.min, lim.max), np.clip(e + d, lim.min, lim.max))
    own = 1000 if stacked else V3_PROBES
    return U.as_i32(*(np.concatenate([a[:own], b]) for a, b in zip(probe, copies))), U.as_i32(*frame), nc


def auto_sides():
    """C2: 140 000 build rows on 24 contigs (no knob: the balanced build by the automatic rule) and 20 000 probes"""
    case = P.auto_case()
    return P.rows(case.probe, np.arange(20_000)), case.frame, case.nc


def handover_sides(n=140_000, n_probe=20_000):
    """C3: every row but two inside one window of n positions, rows 3 long one position apart in shuffled order (one cluster chain
    over every tile), and two far rows (0 and 2^30) that stretch the key span: the window falls into ONE bucket of the balanced
    build, which at this size runs by the automatic rule and hands the index over to the LSD sort"""
    def build():
        rng = np.random.default_rng(143)
        s = 1_000_000 + rng.permutation(n - 2)
        frame = U.as_i32(np.zeros(n, np.int64), np.concatenate([s, [0, 1 << 30]]), np.concatenate([s + 3, [7, (1 << 30) + 9]]))
        ps = 1_000_000 + rng.integers(0, n, n_probe)
        return U.as_i32(np.zeros(n_probe, np.int64), ps, ps + rng.integers(0, 40, n_probe)), frame
    return _once(("handover", n, n_probe), build) + (1,)


def sequence_sides():
    """D1 / D2: 50 000 build rows on 24 contigs and 30 000 probes (contig 24 = outside among them)"""
    case = P.sequence_case()
    return case.probe, case.frame, case.nc


SMALL_ROWS = 300
# D3: (build rows, seed, Strict) of each round on the one context: large and small inputs in turn
D3_ROUNDS = [(150_000, 900, True), (SMALL_ROWS, 901, False), (150_000, 900, False), (SMALL_ROWS, 901, True), (150_000, 900, True)]


def sized_sides(n, seed):
    """D3.  Large: n build rows and n // 2 + 1 probes on 24 contigs (_position_ops_util.sized_case).  Small (SMALL_ROWS): 300 build
    rows and 300 probes on 24 contigs inside 800 positions -- dense enough that the matrix's thresholds still keep more than 100
    pairs of a 300-row input (sized_case's 2000 positions leave about 60)."""
    if n > SMALL_ROWS:
        case = P.sized_case(n, seed)
        return case.probe, case.frame, case.nc

    def build():
        rng = np.random.default_rng(seed)
        frame = U.random_rows(rng, n, 24, 800, max_len=200)
        return U.random_rows(rng, n, 24, 800, max_len=1500), frame
    return _once(("sized", n, seed), build) + (24,)


def chained_frame(side, rows, seed=0):
    """a frame with `rows` more rows on contig 0, two positions apart and five long (each overlaps the next two), mixed in at
    random places: with the contig's other rows under them they are ONE cluster of more than `rows` rows at the head of the
    sorted order"""
    rng = np.random.default_rng(seed)
    s = 2 * np.arange(rows)
    cat = tuple(np.concatenate([a, b]) for a, b in zip(side, (np.zeros(rows, np.int64), s, s + 5)))
    order = rng.permutation(len(cat[0]))
    return U.as_i32(*(a[order] for a in cat))


def sweep_frame(nc):
    """B4: the build side of sweep_sides with a chain of MAGG_TILE + 50 rows on contig 0: at every dictionary size one cluster
    crosses the first tile boundary of the aggregate kernel (from about 1000 contigs on the side's own clusters hold a few rows
    each and no tile boundary falls inside one)"""
    return _once(("sweep_frame", nc), lambda: (chained_frame(sweep_sides(nc)[1], MAGG_TILE + 50, nc),))[0]


def scaled(side, n, seed=0):
    """a random subset of n rows of a side, in input order (the scaled-down copies of the CPU tests)"""
    if len(side[0]) <= n:
        return side
    idx = np.sort(np.random.default_rng(seed).choice(len(side[0]), n, replace=False))
    return P.rows(side, idx)
