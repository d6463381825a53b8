"""References, runners and comparisons of tests/test_map_select_matrix.py: map_overlaps (overlap_agg.hip.h) and the semi / anti / left
outer join kinds (select.hip.h) across the cross-cutting matrices.  The inputs are the generators of _join_ops_util.

The literal yardsticks (_overlap_agg_util.pairs + group_by, _join_kinds_util.expected: brute forces over all probe x build pairs
and one Python loop per probe) are too slow for matrix sizes.  Everything here comes from ONE list of matching pairs,

  reference          thresholded: _join_ops_util.sorted_candidates; the plain predicate -- which is NOT "overlap >= 1": a row that
                     covers no position matches what count_overlaps counts for it -- the oracle's sort + bound search
                     (oracle.overlap_fast), sorted by (probe row, build row),
  map_expected       _join_ops_util.group_by_fast keyed on the probe row over values[b], valid[b] of the matched build rows,
  select_expected    semi = flatnonzero(counts > 0), anti = its complement, outer = the inner pairs followed by (anti, -1),

and is shown equal to the literal forms on the CPU (test_map_select_matrix.py).  numpy, int64 and float64 only; every comparison
is bit-exact."""
import numpy as np

import _join_kinds_util as K
import _join_ops_util as J
import _thresholds_util as T
from oracle import oracle as O

I64, F64 = np.int64, np.float64
ALL = J.ALL
PLAIN = dict(min_overlap=0, probe_min=None, build_min=None)          # what the engines receive for the plain predicate
SENTINEL = 0x5A5A5A5A5A5A5A5A


# ---- the references ----------------------------------------------------------------------------------------------------------------

def reference(probe, build, nc, strict, thr=None):
    """-> (probe_idx, build_idx) int32 sorted by (probe row, build row), and the per-probe counts (int64).  thr: a threshold set of
    sorted_candidates; None or empty = the plain predicate."""
    if thr:
        return J.sorted_candidates(probe, build, nc, strict, **thr)
    n = len(probe[0])
    if n == 0 or len(build[0]) == 0:
        return np.empty(0, np.int32), np.empty(0, np.int32), np.zeros(n, np.int64)
    ox = O.Index(O.Side(*build), nc)
    try:
        p, b = T.sort_pairs(*O.overlap_fast(ox, O.Side(*probe), strict))
    finally:
        ox.close()
    return p.astype(np.int32), b.astype(np.int32), np.bincount(p, minlength=n).astype(np.int64)


def map_expected(ref, n_probe, columns, build_row_id=None, n_values=None):
    """[group_by_fast per value column] over the pairs of `ref`.  The value of a build row is values[row] -- values[id] where the
    build side carries row ids; a row whose id lies outside [0, n_values) is invalid."""
    p, b, _ = ref
    out = []
    for values, valid, _ in columns:
        values = np.asarray(values)
        nv = len(values) if n_values is None else n_values
        rid = b.astype(np.int64) if build_row_id is None else np.asarray(build_row_id, np.int64)[b]
        inside = (rid >= 0) & (rid < nv)
        at = np.where(inside, rid, 0)
        if nv == 0:
            v, ok = np.zeros(len(b), values.dtype), np.zeros(len(b), bool)
        else:
            v = values[at]
            ok = inside if valid is None else inside & np.asarray(valid).astype(bool)[at]
        out.append(J.group_by_fast(p, n_probe, v, ok))
    return out


def select_expected(ref, n_probe):
    """-> dict in the form of _join_kinds_util.expected: cnt, semi, anti, inner = (p, b) sorted, left = (p, b) sorted"""
    p, b, cnt = ref
    assert len(cnt) == n_probe
    semi, anti = np.flatnonzero(cnt > 0).astype(np.int32), np.flatnonzero(cnt == 0).astype(np.int32)
    lp, lb = T.sort_pairs(np.concatenate([p, anti]).astype(np.int32), np.concatenate([b, np.full(len(anti), -1, np.int32)]).astype(np.int32))
    return dict(cnt=cnt, semi=semi, anti=anti, inner=(p, b), left=(lp, lb))


_references = {}


def reference_once(name, probe, build, nc, strict, thr=None):
    """reference() of a named input, computed once and shared by the tests that run it"""
    key = (name, strict, None if not thr else tuple(sorted((k, id(v) if isinstance(v, np.ndarray) else v) for k, v in thr.items())))
    if key not in _references:
        _references[key] = (reference(probe, build, nc, strict, thr), thr)            # (thr kept alive: its ids are part of the key)
    return _references[key][0]


def engine_kw(probe, build, strict, thr=None):
    return J.engine_kw(probe, build, strict, **thr) if thr else dict(PLAIN)


# ---- the comparisons -----------------------------------------------------------------------------------------------------------------

def map_check(got, exp, columns, what):
    """every entry of map_run against map_expected: bit for bit; min / max / mean of a probe without a valid match are skipped"""
    assert got, what
    for name, res in got.items():
        assert len(res) == len(columns) == len(exp), (what, name)
        for j, (v, _, ops) in enumerate(columns):
            assert sorted(res[j]) == sorted(ops), f"{what} {name} column {j}: operations {sorted(res[j])}"
            full = {op: res[j][op] if op in res[j] else _stand_in(exp[j][op]) for op in ALL}
            J.assert_agg_equal(full, exp[j], np.asarray(v).dtype, f"{what} {name} column {j}")


def _stand_in(x):
    return x.copy()                                          # an operation that was not asked for compares with itself


def select_check(got, exp, build, what, probe_row_id=None):
    """every entry of select_run against select_expected.  The device select reports row_id[position] in position order."""
    assert got, what
    for key, g in got.items():
        if key.endswith("outer"):
            K.assert_outer(g, exp, build, f"{what} {key}")
            continue
        want = exp[key.split("_")[1]]
        if key.startswith("dev") and probe_row_id is not None:
            want = np.asarray(probe_row_id, np.int32)[want]
        assert g.dtype == np.int32 and len(g) == len(want) and (g == want).all(), f"{what} {key}: {len(g)} rows, expected {len(want)}"


def map_blob(got):
    """the results of map_run as bytes; min / max / mean of probes without a valid match (unspecified) blanked"""
    parts = []
    for name in sorted(got):
        for r in got[name]:
            has = r["count"] > 0 if "count" in r else None
            for op in sorted(r):
                a = np.array(r[op]).view(np.uint64)
                if op in ("min", "max", "mean"):
                    assert has is not None, "a blob of min / max / mean needs the count column"
                    a = np.where(has, a, 0)
                parts.append(a.tobytes())
    return b"|".join(parts)


def select_blob(got, n_inner=None):
    """the results of select_run as bytes.  The inner part of an outer join is sorted first: the order of the probe rows there
    follows the partition (bucket by bucket where the probes were bucketed), which is the inner join's contract, not the
    selection's; the (row, -1) tail is taken as it is."""
    parts = []
    for key in sorted(got):
        g = got[key]
        if key.endswith("outer"):
            p, b = np.asarray(g[0]), np.asarray(g[1])
            k = int((b >= 0).sum()) if n_inner is None else n_inner
            sp, sb = T.sort_pairs(p[:k], b[:k])
            parts += [sp.tobytes(), sb.tobytes(), p[k:].tobytes(), b[k:].tobytes()]
        else:
            parts.append(np.ascontiguousarray(g).tobytes())
    return b"|".join(parts)


# ---- the runners ---------------------------------------------------------------------------------------------------------------------

def _up(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def dev_agg(columns):
    return [(_up(v), None if m is None else _up(np.asarray(m).astype(np.uint8)), ops) for v, m, ops in columns]


def dev_kw(kw):
    return dict(min_overlap=kw["min_overlap"], probe_min=J.dev_min(kw["probe_min"]), build_min=J.dev_min(kw["build_min"]))


def map_run(eng, dj, probe, build, nc, strict, columns, kw, partition_mode=0, probe_row_id=None, build_row_id=None, index=None, shift=0):
    """map_overlaps through both entries -> dict "host" / "device" -> [dict op -> array per column].  eng None (or a side with a
    row id, which the host binding cannot carry): the device entry only.  index: a DeviceIndex of the build side."""
    got = {}
    if eng is not None and probe_row_id is None and build_row_id is None:
        got["host"] = eng.overlap_agg(probe, build, strict, nc, agg=columns, partition_mode=partition_mode, **kw)
    if dj is not None:
        dp, db = J.dev_side(probe, probe_row_id, shift), J.dev_side(build, build_row_id, shift)
        res = dj.overlap_agg(dp, db, strict, nc, dev_agg(columns), index=index, partition_mode=partition_mode, **dev_kw(kw))
        got["device"] = [{op: t.cpu().numpy() for op, t in r.items()} for r in res]
    return got


def select_run(eng, dj, probe, build, nc, strict, kw, partition_mode=0, probe_row_id=None, build_row_id=None, index=None, shift=0,
               outer=True):
    """semi and anti through both entries, the left outer join through the host entry -> dict "host_semi", "host_anti",
    "host_outer", "dev_semi", "dev_anti".  eng None or a side with a row id: the device entries only."""
    got = {}
    if eng is not None and probe_row_id is None and build_row_id is None:
        for mode in ("semi", "anti"):
            got["host_" + mode] = eng.overlap_select(probe, build, strict, nc, mode, partition_mode=partition_mode, **kw)
        if outer:
            p, b = eng.overlap_outer(probe, build, strict, nc, partition_mode=partition_mode, **kw)
            got["host_outer"] = (np.array(p), np.array(b))
    if dj is not None:
        dp, db = J.dev_side(probe, probe_row_id, shift), J.dev_side(build, build_row_id, shift)
        dkw = dev_kw(kw)
        for mode in ("semi", "anti"):
            got["dev_" + mode] = dj.overlap_select(dp, db, strict, nc, mode, index=index, partition_mode=partition_mode, **dkw).cpu().numpy()
    return got


def map_dev_offset(dj, probe, build, nc, strict, columns, kw, partition_mode=0, offset=1, shift=0):
    """ivj_overlap_agg_dev with every value column, validity column and all five result columns of every value column starting
    `offset` elements (8 bytes each, 1 byte for validity) into sentinel-filled tensors -> [dict op -> array per column]; the
    sentinels before and after every output, and the whole buffer of an operation that was not asked for, must be intact."""
    import torch
    from polars_bio_amd import _engine
    n, nb = len(probe[0]), len(build[0])
    pad = offset + 8
    opts = _engine.make_opts(strict, nc, partition_mode=partition_mode)
    dp, db = J.dev_side(probe, None, shift), J.dev_side(build)
    dkw = dev_kw(kw)
    plain = not kw["min_overlap"] and kw["probe_min"] is None and kw["build_min"] is None
    thr = None if plain else dj._thresholds(dp, db, dkw["min_overlap"], dkw["probe_min"], dkw["build_min"])
    held, cols, bufs = [], [], []
    for v, m, ops in columns:
        v = np.asarray(v)
        tv = torch.full((nb + pad,), SENTINEL, dtype=torch.int64, device="cuda")
        tv[offset:offset + nb] = _up(v.view(np.int64))
        tm = None
        if m is not None:
            tm = torch.full((nb + pad,), 0x5A, dtype=torch.uint8, device="cuda")
            tm[offset:offset + nb] = _up(np.asarray(m).astype(np.uint8))
        held.append((tv, tm))
        vp = tv.data_ptr() + 8 * offset
        assert vp % 16 == (8 * offset) % 16
        cols.append((vp, 0 if tm is None else tm.data_ptr() + offset, _engine.AGG_I64 if v.dtype == I64 else _engine.AGG_F64,
                     _engine.agg_ops_mask(ops)))
        bufs.append({op: torch.full((n + pad,), SENTINEL, dtype=torch.int64, device="cuda") for op in ALL})
    ix = dj.engine.index_build_dev(db.as_c(), opts, plain)
    try:
        dj.engine.overlap_agg_dev(ix, dp.as_c(), opts, thr, nb, cols, [{op: t.data_ptr() + 8 * offset for op, t in b.items()} for b in bufs])
        torch.cuda.synchronize()
    finally:
        ix.close()
    out = []
    for (v, _, ops), b in zip(columns, bufs):
        kinds = {"sum": np.asarray(v).dtype, "min": np.asarray(v).dtype, "max": np.asarray(v).dtype, "mean": F64, "count": I64}
        res = {}
        for op in ALL:
            raw = b[op].cpu().numpy()
            if op in ops:
                assert (raw[:offset] == SENTINEL).all() and (raw[offset + n:] == SENTINEL).all(), f"'{op}': written outside its column"
                res[op] = raw[offset:offset + n].view(kinds[op]).copy()
            else:
                assert (raw == SENTINEL).all(), f"the buffer of '{op}' was written although it was not asked for"
        out.append(res)
    for tv, tm in held:                                      # the inputs are read-only
        assert int(tv[0]) == SENTINEL and (tm is None or int(tm[0]) == 0x5A)
    return out


# ---- the inputs: the generators of _join_ops_util, with one long candidate run where they have none ------------------------------------

RUN = 130                                                    # build rows under one probe: two wavefronts of candidates and two over
_with_run = {}


def with_run(name, probe, build, nc, unmatched_at=None, keep_tail=0):
    """The sides with one long candidate run written into them, which the generators with a few rows per contig (the large
    dictionaries, the one-chain window) do not have: a candidate run longer than one wavefront.

    Build side: the last RUN in-dictionary rows -- not counting the `keep_tail` rows at the very end, which stay -- become rows 40
    long that start within three positions of s0, the start of the side's first in-dictionary row, on that row's contig.
    Probe side: the last three in-dictionary probes become [s0 + 1, s0 + 30), [s0, s0 + 45) and [s0 + 2, s0 + 3) on that contig.
    unmatched_at (for an input whose every probe matches): a position without build rows; the 50 in-dictionary probes before
    those three are moved there.

    Sizes, row positions, every other row and every out-of-dictionary row stay as they were.  Sides too small for it (fewer than
    2 * RUN build rows or 60 probes) are returned unchanged.  The result is built once per name."""
    if name in _with_run:
        return _with_run[name]
    if len(build[0]) >= 2 * RUN and len(probe[0]) >= 60:
        build = tuple(np.array(a, np.int32) for a in build)
        probe = tuple(np.array(a, np.int32) for a in probe)
        build_rows = np.flatnonzero((build[0] >= 0) & (build[0] < nc))
        probe_rows = np.flatnonzero((probe[0] >= 0) & (probe[0] < nc))
        c0 = int(build[0][build_rows[0]])
        s0 = min(int(build[1][build_rows[0]]), np.iinfo(np.int32).max - 100)
        rewritable = build_rows[build_rows < len(build[0]) - keep_tail]
        run, starts = rewritable[-RUN:], s0 + np.arange(RUN) % 3
        build[0][run], build[1][run], build[2][run] = c0, starts, starts + 40
        across = probe_rows[-3:]
        probe[0][across], probe[1][across], probe[2][across] = c0, [s0 + 1, s0, s0 + 2], [s0 + 30, s0 + 45, s0 + 3]
        if unmatched_at is not None:
            far, at = probe_rows[-53:-3], unmatched_at + 7 * np.arange(50)
            probe[0][far], probe[1][far], probe[2][far] = c0, at, at + 5
        for a in probe + build:
            a.setflags(write=False)
    _with_run[name] = (probe, build)
    return _with_run[name]


def sweep_sides(nc, **kw):
    return with_run(("sweep", nc, tuple(sorted(kw.items()))), *J.sweep_sides(nc, **kw), nc)


def sparse_sides(**kw):
    from _position_ops_util import SPARSE_NC
    return with_run(("sparse", tuple(sorted(kw.items()))), *J.sparse_sides(**kw), SPARSE_NC)


def v3_sides(entry):
    probe, build, nc = J.v3_sides(entry)
    return with_run(("v3", entry[0]), probe, build, nc) + (nc,)


def auto_sides():
    probe, build, nc = J.auto_sides()
    return with_run("auto", probe, build, nc) + (nc,)


def handover_sides(**kw):
    probe, build, nc = J.handover_sides(**kw)
    return with_run(("handover", tuple(sorted(kw.items()))), probe, build, nc, unmatched_at=500_000_000, keep_tail=2) + (nc,)


def sized_sides(n, seed):
    probe, build, nc = J.sized_sides(n, seed)
    return with_run(("sized", n, seed), probe, build, nc) + (nc,)
