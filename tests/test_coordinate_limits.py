"""Every operation at the int32 coordinate limits, on every path.

``include/ivjoin.h`` takes any int32 as a start or an end, while the kernels use INT32_MAX / INT32_MIN as in-band pad values:
the LDS slices end in pad rows (start INT32_MAX, end INT32_MIN), the direct-address records carry INT32_MAX keys for "rows past
the segment", the bucket lookups add 1 to a flipped end under Weak, the 8-byte probe record packs end - start.  Real rows on
exactly those values (``_limits.limit_rows``) therefore go through

* the CPU references themselves (brute force == sort + bound search == the int64 numpy forms == literal sweeps in Python ints),
* every host entry and switch on small inputs against brute force,
* each large path (slices, sampled partition, 8-byte records, 12 288-probe tiles, persistent workgroups, round-2 slices, flat
  kernel, 256-bucket window kernels, nearest lines, joint records, fused rows, streaming, per-probe exchange) with the limit rows
  scattered into an ordinary ``synth.make_side`` pair, each with its "this path ran" evidence.

Every case asserts from the reference's own output that the extremes occur in it (``_limits.assert_touches``).  Nearest runs on
rows with start <= end only: over inverted rows the two oracle forms differ and the ABI leaves it unspecified.
"""
import functools

import numpy as np
import pytest

from _limits import MAX, MIN, assert_touches, embed, far_contig, limit_rows, unsampled_positions
from _util import sparse_overlap
from oracle import oracle as O
from polars_bio_amd import _engine, synth
from test_comm import _local_group, _pp_job, _run_ranks
from test_gpu_parity import _canon, _cmp_all, _fused_overlap

gpu = pytest.mark.gpu
SEEDS = range(6)
NEAREST_CFGS = ((1, True), (1, False), (3, True), (4, False))
MIN_DISTS = (0, 1, 37, (1 << 31) - 1, 1 << 33)
NC = 2


@pytest.fixture(scope="module")
def eng():
    return _engine.Engine(0)


def _fresh(monkeypatch, **env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return _engine.Engine(0)


@functools.lru_cache(maxsize=None)
def _small(seed, inverted):
    """700 x 600 limit rows on two contigs; the probe side holds three rows of a contig outside the dictionary."""
    rng = np.random.default_rng(4100 + seed)
    probe = limit_rows(rng, 700, NC, inverted=inverted, outside=True)
    build = limit_rows(rng, 600, NC, inverted=inverted)
    for a in probe + build:
        a.setflags(write=False)
    return probe, build


@functools.lru_cache(maxsize=None)
def _small_pairs(seed, inverted, strict):
    probe, build = _small(seed, inverted)
    ep, eb = O.overlap_brute(O.Side(*probe), O.Side(*build), strict)
    assert_touches(ep, eb, probe, build, strict)
    return ep, eb


@functools.lru_cache(maxsize=None)
def _far(seed):
    probe, build = far_contig(np.random.default_rng(4200 + seed), 900, 700)
    return probe, build


# ---- the references at the limits (CPU) -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("seed", SEEDS)
def test_reference_overlap_and_count_at_the_limits(seed, strict):
    """Brute force == sort + bound search == the sparse int64 numpy reference (independent of the C code), inverted rows
    included; the counts of both C forms agree and are the pairs' multiplicities."""
    probe, build = _small(seed, True)
    ps, bs = O.Side(*probe), O.Side(*build)
    ep, eb = _small_pairs(seed, True, strict)
    ix = O.Index(bs, NC)
    fp, fb = O.overlap_fast(ix, ps, strict)
    assert len(fp) == len(ep) and (fp == ep).all() and (fb == eb).all()
    sp, sb = sparse_overlap(probe, build, NC, strict)
    assert len(sp) == len(ep) and (sp == ep).all() and (sb == eb).all()
    cb = O.count_overlaps_brute(ps, bs, strict)
    assert (cb == O.count_overlaps_fast(ix, ps, strict)).all()
    assert (cb == np.bincount(ep, minlength=ps.n)).all()
    assert len(ep) > 5000


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("seed", SEEDS)
def test_reference_nearest_at_the_limits(seed, strict):
    """nearest_brute == nearest_fast on rows with start <= end, k = 1 distances == the int64 numpy definition; on far_contig
    (the two sides at opposite ends of int32) every distance is above 2^31."""
    for (probe, build), far in ((_small(seed, False), False), (_far(seed), True)):
        ps, bs = O.Side(*probe), O.Side(*build)
        ix = O.Index(bs, NC)
        for k, inc in NEAREST_CFGS:
            bi, bd, bn = O.nearest_brute(ps, bs, strict, k, inc)
            fi, fd, fn = O.nearest_fast(ix, ps, strict, k, inc)
            assert (bn == fn).all() and (bd == fd).all() and (bi == fi).all(), (k, inc, far)
            if far:
                assert (bn == min(k, 350)).all() and int(bd.min()) >= (1 << 32) - 3000, (k, inc)   # every distance is about 2^32
            if (k, inc) == (1, True):
                assert (bd[:, 0] == O.np_nearest_distance(ps, bs, strict)).all()
        if not far:
            _small_pairs(seed, False, strict)                        # non-vacuity of this side pair


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("seed", SEEDS)
def test_reference_coverage_at_the_limits(seed, strict):
    probe, build = _small(seed, True)
    _small_pairs(seed, True, strict)
    fast = O.np_coverage_fast(O.Side(*probe), O.Side(*build), strict)
    assert (fast == O.np_coverage_brute(O.Side(*probe), O.Side(*build), strict)).all()
    whole = (probe[1] == MIN) & (probe[2] == MAX) & (probe[0] < NC)
    assert whole.any() and int(fast[whole].max()) > (1 << 31)       # the whole-range probe is covered beyond 32 bits


def _sweep_subtract(left, right, strict):
    """Literal sequential sweep in Python ints: every left row minus the right rows of its contig, half-open inside."""
    w = 0 if strict else 1
    by_contig = {}
    for c, s, e in zip(*(a.tolist() for a in right)):
        if e + w > s:
            by_contig.setdefault(c, []).append((s, e + w))
    for v in by_contig.values():
        v.sort()
    out = []
    for i, (c, s, e) in enumerate(zip(*(a.tolist() for a in left))):
        cur, le = s, e + w
        if le <= cur:
            continue
        for rs, re in by_contig.get(c, ()):
            if rs >= le:
                break
            if re <= cur:
                continue
            if rs > cur:
                out.append((i, cur, rs - w))
            cur = re
        if cur < le:
            out.append((i, cur, le - w))
    return out


def _sweep_cluster(side, strict, min_dist):
    """Literal sequential sweep in Python ints -> (cluster id per row, merged rows (contig, start, end, n))."""
    c, s, e = (a.tolist() for a in side)
    order = sorted(range(len(c)), key=lambda i: (c[i], s[i], i))
    cid, merged = [0] * len(c), []
    for i in order:
        if merged and merged[-1][0] == c[i] and (s[i] < merged[-1][2] + min_dist if strict else s[i] <= merged[-1][2] + min_dist):
            m = merged[-1]
            m[2], m[3] = max(m[2], e[i]), m[3] + 1
        else:
            merged.append([c[i], s[i], e[i], 1])
        cid[i] = len(merged) - 1
    return cid, merged


def _short(side):
    """The rows of a side shorter than 2^30: without the half-range and whole-range rows the union of a side has gaps, so merge
    keeps many clusters and subtract / complement many pieces next to the limits."""
    keep = np.abs(side[2].astype(np.int64) - side[1]) < (1 << 30)
    return tuple(np.ascontiguousarray(a[keep]) for a in side)


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("seed", SEEDS)
def test_reference_subtract_and_cluster_at_the_limits(seed, strict):
    """np_subtract and np_cluster (every min_dist) == literal sequential sweeps in Python ints, on the limit rows as they are (a
    whole-range row on every contig) and without their long rows."""
    probe, full = _small(seed, True)
    _small_pairs(seed, True, strict)
    for build in (full, _short(full)):
        r, s, e = O.np_subtract(O.Side(*probe), O.Side(*build), strict)
        exp = _sweep_subtract(probe, build, strict)
        assert list(zip(r.tolist(), s.tolist(), e.tolist())) == exp
        for md in MIN_DISTS:
            cid, cs, ce, (mc, ms, me, mn) = O.np_cluster(O.Side(*build), strict, md)
            ecid, merged = _sweep_cluster(build, strict, md)
            assert cid.tolist() == ecid, md
            assert list(zip(mc.tolist(), ms.tolist(), me.tolist(), mn.tolist())) == [tuple(m) for m in merged], md
            assert cs.tolist() == [merged[k][1] for k in ecid] and ce.tolist() == [merged[k][2] for k in ecid], md
        assert len(_sweep_cluster(build, strict, 1 << 33)[1]) == NC      # one cluster per contig: 2^33 bridges every gap of int32
    assert len(exp) > 100 and len(_sweep_cluster(build, strict, 0)[1]) > 20 * NC


# ---- small inputs through every host entry and switch (GPU) -------------------------------------------------------------------

def _check_sortscan(eng, probe, build, frame, nc, strict, min_dists=MIN_DISTS):
    """merge / cluster of `frame` for every min_dist, coverage / subtract / complement of (probe, build) for partition_mode 0, 1,
    2, against the np_* forms.  `frame` holds no row with start > end: the sweep over such rows is not pinned (oracle.py: the
    engine's cluster end is the contig's running maximum, np_cluster's the cluster's own), like nearest over them."""
    bs = O.Side(*build)
    for md in min_dists:
        ecid, ecs, ece, (mc, ms, me, mn) = O.np_cluster(O.Side(*frame), strict, md)
        gc, gs, ge, gn = eng.merge(frame, strict, nc, md)
        assert len(gc) == len(mc), ("merge", md, len(gc), len(mc))
        assert (gc == mc).all() and (gs == ms).all() and (ge == me).all() and (gn == mn).all(), ("merge", md)
        cid, cs, ce, ncl = eng.cluster(frame, strict, nc, md)
        assert ncl == len(mc) and (cid == ecid).all() and (cs == ecs).all() and (ce == ece).all(), ("cluster", md)
    exp = O.np_coverage_fast(O.Side(*probe), bs, strict)
    er, es, ee = O.np_subtract(O.Side(*probe), bs, strict)
    view = (np.array([0, 1, 0, 1, nc], np.int32), np.array([MIN, MIN, MIN + 1, -5, MIN], np.int32), np.array([MAX, MAX, MAX - 1, MAX, MAX], np.int32))
    vc, vs, ve = O.np_complement(bs, O.Side(*view), strict)
    for pm in (0, 1, 2):
        got = eng.coverage(probe, build, strict, nc, partition_mode=pm)
        assert got.dtype == np.int64 and (got == exp).all(), ("coverage", pm, int((got != exp).sum()))
        gr, gs, ge = eng.subtract(probe, build, strict, nc, partition_mode=pm)
        assert len(gr) == len(er), ("subtract", pm, len(gr), len(er))
        assert (gr == er).all() and (gs == es).all() and (ge == ee).all(), ("subtract", pm)
        gr, gs, ge = eng.complement(build, view, strict, nc, partition_mode=pm)
        assert len(gr) == len(vc), ("complement", pm, len(gr), len(vc))
        assert (view[0][gr] == vc).all() and (gs == vs).all() and (ge == ve).all(), ("complement", pm)


@gpu
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("seed", SEEDS)
def test_small_limit_rows_through_every_entry_and_switch(eng, seed, strict):
    probe, build = _small(seed, True)
    _small_pairs(seed, True, strict)
    _cmp_all(eng, probe, build, NC, strict, brute=True, nearest_cfgs=())               # overlap + count, inverted rows included
    probe, build = _small(seed, False)
    _small_pairs(seed, False, strict)
    _cmp_all(eng, probe, build, NC, strict, brute=True, nearest_cfgs=NEAREST_CFGS)
    frame = build
    probe, build = _small(seed, True)
    _check_sortscan(eng, probe, build, frame, NC, strict)
    _check_sortscan(eng, probe, _short(build), _short(frame), NC, strict)


@gpu
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("seed", range(2))
def test_nearest_distances_beyond_2_to_31(eng, seed, strict):
    """far_contig through nearest on every (table_mode, partition_mode) of _cmp_all, the lines included: rows, int64 distances
    (about 2^32) and n_found == brute force."""
    probe, build = _far(seed)
    d = O.nearest_brute(O.Side(*probe), O.Side(*build), strict, 1, True)[1]
    assert int(d.min()) >= (1 << 32) - 3000 and int(d.max()) > (1 << 31)
    _cmp_all(eng, probe, build, NC, strict, brute=True, nearest_cfgs=NEAREST_CFGS)


# ---- the limit rows inside the large paths (GPU) ------------------------------------------------------------------------------

N_LIMIT = 2000


@functools.lru_cache(maxsize=None)
def _big(n_probe, n_build, nc, inverted=True, hidden=False, seed=0):
    """A synth.make_side pair with N_LIMIT limit rows scattered into each side (hidden: the probe side's limit rows sit where the
    1 / 64 sample of the sampled partition never reads)."""
    rng = np.random.default_rng(4300 + seed)
    probe = synth.make_side(n_probe, 42 + seed, synth.PROBE_LEN, min(nc, 24))
    build = synth.make_side(n_build, 43 + seed, synth.BUILD_LEN, min(nc, 24))
    if nc > 24:                                                      # a larger dictionary: the 24 contigs spread over it
        f = (np.arange(24) * (nc // 24) + 1).astype(np.int32)
        probe, build = (f[probe[0]],) + probe[1:], (f[build[0]],) + build[1:]
    lp = limit_rows(rng, N_LIMIT, nc, inverted=inverted, outside=True)
    lb = limit_rows(rng, N_LIMIT, nc, inverted=inverted)
    probe = embed(probe, lp, rng, unsampled_positions(rng, n_probe, N_LIMIT) if hidden else None)
    build = embed(build, lb, rng)
    for a in probe + build:
        a.setflags(write=False)
    return probe, build


@functools.lru_cache(maxsize=None)
def _big_pairs(strict, *key):
    probe, build = _big(*key)
    ep, eb = O.overlap_fast(O.Index(O.Side(*build), key[2]), O.Side(*probe), strict, threads=16)
    assert_touches(ep, eb, probe, build, strict)
    return ep, eb


BASE = (400_000, 80_000, 24)


def _same(p, b, ep, eb, what):
    p, b = _canon(np.asarray(p), np.asarray(b))
    assert len(p) == len(ep), (what, len(p), len(ep))
    bad = np.nonzero((p != ep) | (b != eb))[0]
    assert len(bad) == 0, (what, len(bad), "first mismatch: got", (int(p[bad[0]]), int(b[bad[0]])), "expected", (int(ep[bad[0]]), int(eb[bad[0]])))


@gpu
@pytest.mark.parametrize("strict", [True, False])
def test_limit_rows_in_the_contig_aligned_slice_join_fused(strict, monkeypatch):
    probe, build = _big(*BASE)
    ep, eb = _big_pairs(strict, *BASE)
    e = _fresh(monkeypatch, IVJ_CS="1")
    try:
        e.enable_timing(2)
        for sr in (0, 64):
            e.timings()
            hp, hb = _fused_overlap(e, probe, build, strict, 24, 6, len(ep), slice_rows=sr)
            t = e.timings()
            assert "cs_join_fused" in t, sorted(t)
            _same(hp, hb, ep, eb, ("fused", sr))
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("strict", [True, False])
def test_limit_rows_in_the_slice_count_fill_pair(strict, monkeypatch):
    probe, build = _big(*BASE)
    ep, eb = _big_pairs(strict, *BASE)
    e = _fresh(monkeypatch, IVJ_CS="1")
    try:
        e.enable_timing(2)
        for det in (False, True):
            e.timings()
            p1, b1 = e.overlap(probe, build, strict, 24, partition_mode=6, deterministic=det)
            t = e.timings()
            assert "cs_join_count" in t and ("cs_join_fill" in t or "cs_fill_cached" in t), sorted(t)
            _same(p1, b1, ep, eb, ("pair", det))
            if det:
                p2, b2 = e.overlap(probe, build, strict, 24, partition_mode=6, deterministic=True)
                assert (np.asarray(p1) == np.asarray(p2)).all() and (np.asarray(b1) == np.asarray(b2)).all()
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("strict", [True, False])
def test_limit_rows_in_the_sampled_partition_and_its_fallback(strict, monkeypatch):
    probe, build = _big(*BASE)
    ep, eb = _big_pairs(strict, *BASE)
    monkeypatch.setenv("IVJ_CS", "1")
    for sampled in (True, False):
        if not sampled:
            monkeypatch.setenv("IVJ_CS_SAMPLED", "0")
        e = _engine.Engine(0)
        try:
            e.enable_timing(2)
            hp, hb = _fused_overlap(e, probe, build, strict, 24, 6, len(ep))
            t = e.timings()
            if sampled:
                assert ("cs_sample" in t or "cs_bins_sample" in t) and "cs_hist" not in t, sorted(t)     # sampled, and not redone
            else:
                assert "cs_hist" in t and "cs_sample" not in t and "cs_bins_sample" not in t, sorted(t)
            _same(hp, hb, ep, eb, ("sampled", sampled))
        finally:
            e.close()


@gpu
@pytest.mark.parametrize("strict", [True, False])
def test_limit_rows_in_the_eight_byte_probe_records_and_their_fallback(strict, monkeypatch):
    """64-row slices of an 80 k-row build side span ~ 2.5 Mbp: the sample of a probe side whose limit rows it never reads picks
    the 8-byte records, the limit rows do not fit them (ends about 2^31 above their slice's minimum, lengths up to 2^32 - 1) and
    the call is redone with 12-byte records.  Limit rows on the build side make the first slice of every contig span half of int32:
    the device then picks the 12-byte form itself."""
    key = BASE + (True, True)
    probe, _ = _big(*key)
    plain_build = synth.make_side(BASE[1], 43, synth.BUILD_LEN, 24)
    ep, eb = O.overlap_fast(O.Index(O.Side(*plain_build), 24), O.Side(*probe), strict, threads=16)
    assert int((probe[2][ep] == MAX).sum()) > 0 and int((probe[1][ep] == MIN).sum()) > 0
    e = _fresh(monkeypatch, IVJ_CS="1")
    try:
        e.enable_timing(2)
        e.timings()
        hp, hb = _fused_overlap(e, probe, plain_build, strict, 24, 6, len(ep), slice_rows=64)
        t = e.timings()
        # the 8-byte attempt + the redo with 12-byte records; a region overflow would be redone through the histogram pass instead
        assert t["cs_scatter"]["launches"] == 2 and "cs_hist" not in t, (sorted(t), t.get("cs_scatter"))
        _same(hp, hb, ep, eb, "8-byte attempt, redo")
        _same(*e.overlap(probe, plain_build, strict, 24, partition_mode=6, slice_rows=64), ep, eb, "8-byte attempt, pair")
        probe, build = _big(*BASE)
        ep, eb = _big_pairs(strict, *BASE)
        e.timings()
        hp, hb = _fused_overlap(e, probe, build, strict, 24, 6, len(ep), slice_rows=64)
        t = e.timings()
        assert "cs_scatter12" in t and t["cs_scatter"]["launches"] == 1 and "cs_hist" not in t, sorted(t)
        _same(hp, hb, ep, eb, "12-byte records")
    finally:
        e.close()


TILES12K = ((8 << 20) + 11, 120_000, 128)       # probes, build rows, rows per slice


def _ptrace_headers(path):
    """Headers of the records the scatter of 12 288- / 16 384-probe tiles appends to the IVJ_CS_PTRACE file, one per launch of that
    kernel (host_cslice.hip.h; no other scatter writes the file) -> [(workgroups, probes per workgroup, probes per tile / 1024)]."""
    w = np.fromfile(path, np.uint64)
    out, i = [], 0
    while i < len(w):
        assert int(w[i]) == 0x50545243, hex(int(w[i]))
        out.append((int(w[i + 1]), int(w[i + 2]), int(w[i + 3])))
        i += 4 + 8 * int(w[i + 1])
    return out


@gpu
def test_limit_rows_in_the_12288_probe_scatter_tiles(monkeypatch, tmp_path):
    """8 Mi + 11 probes (the smallest side that takes the 12 288-probe tiles; a ragged last tile) x 120 k build rows in 128-row
    slices: 962 bucket slots, so the staging of the 8192- and of the 12 288-probe tiles fits the LDS, and slices of ~ 3.3 Mbp, so
    the sample picks the 8-byte records.  The scatter of 8-byte records then runs on 12 288-probe tiles -- it alone writes the
    IVJ_CS_PTRACE file, whose header names the tile -- meets the limit rows the sample did not read, flags them, and the call is
    redone with 12-byte records (two scatter launches, no histogram pass: not a region overflow).  With IVJ_CS_PTILE=8192 the same
    call takes the 8192-probe kernel and writes no trace.  Strict and Weak."""
    n_probe, n_build, sr = TILES12K
    probe, _ = _big(n_probe, n_build, 24, True, True)
    build = synth.make_side(n_build, 43, synth.BUILD_LEN, 24)
    ix = O.Index(O.Side(*build), 24)
    exp = {}
    for strict in (True, False):
        ep, eb = O.overlap_fast(ix, O.Side(*probe), strict, threads=16)
        assert int((probe[2][ep] == MAX).sum()) > 0 and int((probe[1][ep] == MIN).sum()) > 0
        exp[strict] = (ep, eb)
    for ptile in ("", "8192"):
        trace = tmp_path / f"ptrace{ptile}.bin"
        monkeypatch.setenv("IVJ_CS_PTRACE", str(trace))
        e = _fresh(monkeypatch, IVJ_CS="1", **({"IVJ_CS_PTILE": ptile} if ptile else {}))
        try:
            e.enable_timing(2)
            for strict in (True, False):
                ep, eb = exp[strict]
                e.timings()
                hp, hb = _fused_overlap(e, probe, build, strict, 24, 6, len(ep), slice_rows=sr)
                t = e.timings()
                assert t["cs_scatter"]["launches"] == 2 and "cs_hist" not in t, (ptile, strict, sorted(t), t.get("cs_scatter"))
                _same(hp, hb, ep, eb, ("12288 tiles", ptile, strict))
        finally:
            e.close()
        if ptile:
            assert not trace.exists()                                           # the 8192-probe kernel ran
        else:
            heads = _ptrace_headers(trace)
            assert len(heads) == 2, heads                                       # one 8-byte attempt per filter; the redo is not offered it
            for wgs, chunk, wide in heads:
                assert wide == 12 and chunk % 12288 == 0 and wgs * chunk >= n_probe, heads


@gpu
@pytest.mark.parametrize("knobs", [{}, {"IVJ_CS_PMAX": "1"}, {"IVJ_CS_PMAX": "16", "IVJ_SLICE_CHUNK": "4096", "IVJ_CS_PGRAIN": "8"}, {"IVJ_CS_PERSIST": "0"}],
                         ids=["default", "pmax1", "pmax16", "persist0"])
def test_limit_rows_under_the_persistent_workgroups(knobs, monkeypatch):
    probe, build = _big(*BASE)
    e = _fresh(monkeypatch, IVJ_CS="1", **knobs)
    try:
        e.enable_timing(2)
        for strict in (True, False):
            ep, eb = _big_pairs(strict, *BASE)
            e.timings()
            hp, hb = _fused_overlap(e, probe, build, strict, 24, 6, len(ep))
            t = e.timings()
            assert "cs_join_fused" in t, sorted(t)
            _same(hp, hb, ep, eb, ("fused", strict))
            _same(*e.overlap(probe, build, strict, 24, partition_mode=6, deterministic=True), ep, eb, ("pair", strict))
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("strict", [True, False])
def test_limit_rows_in_the_round2_slices_above_256_contigs(strict):
    key = (200_000, 80_000, 300)
    probe, build = _big(*key)
    ep, eb = _big_pairs(strict, *key)
    e = _engine.Engine(0)
    try:
        e.enable_timing(2)
        e.timings()
        p, b = e.overlap(probe, build, strict, 300, partition_mode=6)
        t = e.timings()
        assert any(k.startswith("slice_join") for k in t) and not any(k.startswith("cs_") for k in t), sorted(t)
        _same(p, b, ep, eb, "round-2 slices, pair")
        hp, hb = _fused_overlap(e, probe, build, strict, 300, 6, len(ep))
        t = e.timings()
        assert "slice_join_fused" in t and not any(k.startswith("cs_") for k in t), sorted(t)
        _same(hp, hb, ep, eb, "round-2 slices, fused")
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("strict", [True, False])
def test_limit_rows_in_the_flat_kernel(strict):
    probe, build = _big(*BASE)
    ep, eb = _big_pairs(strict, *BASE)
    e = _engine.Engine(0)
    try:
        e.enable_timing(2)
        hp, hb = _fused_overlap(e, probe, build, strict, 24, 5, len(ep))
        t = e.timings()
        assert "overlap_flat" in t, sorted(t)
        _same(hp, hb, ep, eb, "flat")
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("degenerate", [pytest.param(False, id="rank_count"), pytest.param(True, id="sweep_count")])
def test_flat_kernel_tile_of_many_chunks(degenerate):
    """k_overlap_flat (partition_mode 5) on one tile of 200 probes over 3000 build rows stacked on one position range: about 3000
    candidates per probe (below FLAT_MAX_CAND), i.e. some 290 chunks of which the last is partial, and every probe's range begins in
    one chunk and ends in a later one.  The tile's total comes from the two-rank formula, or -- with a probe that covers no position
    in the tile -- from the counting sweep over the chunks; the pairs are then emitted chunk by chunk.  Compared exactly with the
    oracle's brute force of the plain predicate."""
    i = np.arange(3000)
    build = (np.zeros(3000, np.int32), (1000 + i % 7).astype(np.int32), (2000 - i % 5).astype(np.int32))
    j = np.arange(200)
    probe = (np.zeros(200, np.int32), (1000 + j).astype(np.int32), (1500 + 2 * j).astype(np.int32))
    if degenerate:
        probe[2][77] = probe[1][77]                        # start == end: the formula is not exact for it, the brute force still pairs it
    ep, eb = O.overlap_brute(O.Side(*probe), O.Side(*build), True)
    o = np.lexsort((eb, ep))
    ep, eb = ep[o], eb[o]
    assert 199 * 3000 <= len(ep) <= 200 * 3000
    e = _engine.Engine(0)
    try:
        e.enable_timing(2)
        hp, hb = _fused_overlap(e, probe, build, True, 1, 5, len(ep))
        t = e.timings()
        assert "overlap_flat" in t and "overlap_fused" not in t, sorted(t)
        # the pairs of one probe are contiguous and ordered by (build.start, build row)
        assert len(np.unique(hp)) == int((hp[1:] != hp[:-1]).sum()) + 1
        inside = hp[1:] == hp[:-1]
        ks, kb = build[1][hb].astype(np.int64), hb.astype(np.int64)
        assert (((ks[1:] > ks[:-1]) | ((ks[1:] == ks[:-1]) & (kb[1:] > kb[:-1]))) | ~inside).all()
        o = np.lexsort((hb, hp))
        assert (hp[o] == ep).all() and (hb[o] == eb).all(), "flat kernel, many chunks"
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("strict", [True, False])
def test_limit_rows_in_the_256_bucket_window_kernels(strict):
    probe, build = _big(*BASE)
    ep, eb = _big_pairs(strict, *BASE)
    e = _engine.Engine(0)
    try:
        e.enable_timing(2)
        for tm in (1, 2):
            e.timings()
            p, b = e.overlap(probe, build, strict, 24, partition_mode=1, table_mode=tm)
            t = e.timings()
            assert "part_scatter" in t and ("overlap_fill" in t or "overlap_fill_dense" in t), sorted(t)
            _same(p, b, ep, eb, ("window kernels", tm))
    finally:
        e.close()


NEAR = (1_100_000, 131_072 + 5, 24, False)         # >= 128 k build rows and >= 8 x as many probes: the lines by the automatic choice


@gpu
@pytest.mark.parametrize("strict", [True, False])
def test_limit_rows_in_the_nearest_lines_at_their_automatic_size(strict):
    probe, build = _big(*NEAR)
    _big_pairs(strict, *NEAR)
    ei, ed, en = O.nearest_fast(O.Index(O.Side(*build), 24), O.Side(*probe), strict, 1, True, threads=16)
    lim = (probe[1] == MIN) | (probe[2] == MAX)
    assert int(en[lim].sum()) > 100
    e = _engine.Engine(0)
    try:
        e.enable_timing(2)
        i, d, n = e.nearest(probe, build, strict, 24, 1, True)
        t = e.timings()
        assert "nearest_k1_lines" in t, sorted(t)
        assert (n == en).all() and (d == ed).all() and (i == ei).all()
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("strict", [True, False])
def test_limit_rows_in_the_count_overlaps_joint_records(strict):
    probe, build = _big(*BASE)
    ep, eb = _big_pairs(strict, *BASE)
    ec = np.bincount(ep, minlength=len(probe[0]))
    assert (ec == O.count_overlaps_fast(O.Index(O.Side(*build), 24), O.Side(*probe), strict, threads=16)).all()
    e = _engine.Engine(0)
    try:
        e.enable_timing(2)
        got = e.count_overlaps(probe, build, strict, 24)
        t = e.timings()
        assert "joint_records" in t and "count_overlaps" in t, sorted(t)
        assert (got == ec).all(), int((got != ec).sum())
    finally:
        e.close()


def _upload(eng, side, ptrs):
    ps = []
    for col in side:
        p = eng.dev_alloc(max(4 * len(col), 16))
        eng.h2d(p, np.ascontiguousarray(col, np.int32))
        ps.append(p)
    ptrs += ps
    return eng.dev_side(ps[0], ps[1], ps[2], len(side[0]))


@gpu
@pytest.mark.parametrize("strict", [True, False])
def test_fused_rows_carry_the_extremes(eng, strict):
    """ivj_overlap_fused_rows_dev with all seven columns: the gathered start_* / end_* equal the host take of the oracle's pairs."""
    probe, build = _big(*BASE)
    ep, eb = _big_pairs(strict, *BASE)
    total = len(ep)
    for pm in (0, 6):
        ptrs = []
        sp, sb = _upload(eng, probe, ptrs), _upload(eng, build, ptrs)
        opts = _engine.make_opts(strict, 24, partition_mode=pm)
        ix = eng.index_build_dev(sb, opts)
        cols = [eng.dev_alloc(4 * total) for _ in _engine.ROW_COLUMNS]
        n_rows, fits = eng.overlap_fused_rows_dev(ix, sp, opts, total, *cols)
        assert fits and n_rows == total, (pm, n_rows, total)
        h = {}
        for name, ptr in zip(_engine.ROW_COLUMNS, cols):
            h[name] = np.empty(total, np.int32)
            eng.d2h(h[name], ptr)
        ix.close()
        for p in ptrs + cols:
            eng.dev_free(p)
        o = np.argsort(h["probe_idx"], kind="stable")
        assert (h["probe_idx"][o] == ep).all() and (h["build_idx"][o] == eb).all(), pm
        assert (h["contig"][o] == probe[0][ep]).all(), pm
        assert (h["start_1"][o] == probe[1][ep]).all() and (h["end_1"][o] == probe[2][ep]).all(), pm
        assert (h["start_2"][o] == build[1][eb]).all() and (h["end_2"][o] == build[2][eb]).all(), pm
        assert (h["end_1"] == MAX).any() and (h["start_1"] == MIN).any()
        assert strict or ((h["start_2"] == MAX).any() and (h["end_2"] == MIN).any())


@gpu
@pytest.mark.parametrize("strict", [True, False])
def test_fused_join_writes_nothing_past_its_capacity(eng, strict):
    """ivj_overlap_fused_dev with capacity = total // 2: IVJ_ECAPACITY, n_pairs == total, and the words behind the capacity --
    as many as a call that ignored it would write -- keep their pattern."""
    probe, build = _big(*BASE)
    total = len(_big_pairs(strict, *BASE)[0])
    cap = total // 2
    pattern = np.full(total + 4096, 0x5A5A5A5A, np.int32)
    for pm in (0, 1, 2, 5, 6):
        ptrs = []
        sp, sb = _upload(eng, probe, ptrs), _upload(eng, build, ptrs)
        opts = _engine.make_opts(strict, 24, partition_mode=pm)
        ix = eng.index_build_dev(sb, opts)
        op, ob = eng.dev_alloc(4 * len(pattern)), eng.dev_alloc(4 * len(pattern))
        eng.h2d(op, pattern)
        eng.h2d(ob, pattern)
        n_pairs, fits = eng.overlap_fused_dev(ix, sp, opts, op, ob, cap)
        assert not fits and n_pairs == total, (pm, fits, n_pairs, total)
        for ptr in (op, ob):
            h = np.empty(len(pattern), np.int32)
            eng.d2h(h, ptr)
            assert (h[cap:] == 0x5A5A5A5A).all(), (pm, int((h[cap:] != 0x5A5A5A5A).sum()), "words written past the capacity")
        ix.close()
        for p in ptrs + [op, ob]:
            eng.dev_free(p)


@gpu
@pytest.mark.parametrize("strict", [True, False])
def test_probe_stream_batches_with_limit_rows(strict):
    key = (300_000, 60_000, 24, False)
    probe, build = _big(*key)
    _big_pairs(strict, *key)
    ix = O.Index(O.Side(*build), 24)
    rng = np.random.default_rng(5)
    n = len(probe[0])
    bounds = [0] + [k * n // 6 + int(rng.integers(-9000, 9000)) for k in range(1, 6)] + [n]      # ragged batches of ~ 50 k rows
    bounds.insert(3, bounds[3])                            # an empty batch in the middle
    batches = list(zip(bounds[:-1], bounds[1:]))
    for lo, hi in batches:
        assert hi == lo or ((probe[2][lo:hi] == MAX).any() and (probe[1][lo:hi] == MIN).any())
    rows = max(hi - lo for lo, hi in batches)
    e = _engine.Engine(0)
    try:
        for op, k, inc in ((_engine.STREAM_OVERLAP, 1, True), (_engine.STREAM_COUNT, 1, True), (_engine.STREAM_NEAREST, 1, True),
                           (_engine.STREAM_NEAREST, 3, False)):
            got = {}
            with e.probe_stream(build, strict, 24, op, rows, k=k, include_overlaps=inc) as st:
                for lo, hi in batches:
                    r = st.submit(tuple(c[lo:hi] for c in probe))
                    if r is not None:
                        got[r["batch"]] = r
                while True:
                    r = st.flush()
                    if r is None:
                        break
                    got[r["batch"]] = r
            assert sorted(got) == list(range(len(batches)))
            for i, (lo, hi) in enumerate(batches):
                side = O.Side(*(c[lo:hi] for c in probe))
                r = got[i]
                assert r["n_probe"] == hi - lo
                if op == _engine.STREAM_OVERLAP:
                    _same(r["probe_idx"], r["build_idx"], *O.overlap_fast(ix, side, strict), ("stream", i))
                elif op == _engine.STREAM_COUNT:
                    assert (r["counts"] == O.count_overlaps_fast(ix, side, strict)).all(), i
                else:
                    ei, ed, en = O.nearest_fast(ix, side, strict, k, inc)
                    assert (r["n_found"] == en).all() and (r["dist"] == ed).all() and (r["build_idx"] == ei).all(), (i, k, inc)
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("op,k", [("count", 1), ("nearest", 1), ("nearest", 3)])
def test_per_probe_exchange_carries_distances_beyond_2_to_31(op, k):
    """ivj_nearest_allgather_dev / ivj_count_overlaps_allgather_dev over the loopback transport at world 2 on far_contig rows plus
    limit rows: distances of about 2^32 cross the wire format intact.  Strict only: the shared rank job of test_comm pins it."""
    rng = np.random.default_rng(4400)
    fp, fb = far_contig(rng, 3000, 2000)
    lp, lb = limit_rows(rng, 1500, 2, outside=True), limit_rows(rng, 1000, 2)
    nc = 4                                                                      # contigs 0, 1: far_contig; 2, 3: limit rows; 4: outside
    probe = tuple(np.concatenate([a, b]) for a, b in zip(fp, ((lp[0] + 2).astype(np.int32),) + lp[1:]))
    build = tuple(np.concatenate([a, b]) for a, b in zip(fb, ((lb[0] + 2).astype(np.int32),) + lb[1:]))
    ix = O.Index(O.Side(*build), nc)
    if op == "count":
        exp = (O.count_overlaps_fast(ix, O.Side(*probe), True),)
        assert int(exp[0][(probe[2] == MAX) | (probe[1] == MIN)].sum()) > 0
    else:
        ei, ed, en = O.nearest_fast(ix, O.Side(*probe), True, k, True)
        assert int(ed.max()) > (1 << 31) and int((ed > (1 << 31)).sum()) > 1000
        exp = (ei.ravel(), ed.ravel(), en.ravel())
    engines, comms = _local_group(2)
    out = {}
    _run_ranks(_pp_job, [(engines[r], comms[r], probe, build, nc, r, 2, op, k, out) for r in range(2)])
    assert sorted(out) == [0, 1]
    for r in range(2):
        assert not isinstance(out[r], Exception), out[r]
        for g, w in zip(out[r], exp):
            assert (g == w).all(), (r, int((g != w).sum()))
    for c in comms:
        c.close()
    for e in engines:
        e.close()
