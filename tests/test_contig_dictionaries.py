"""Every operation across contig-dictionary sizes and the thresholds the engine chooses kernels and layouts by.

The engine picks its index build, its slice paths and where per-contig metadata lives by ``n_contigs``: 64 (the round-2
slice table), 256 (contig-aligned slices, per-contig metadata in LDS, the balanced index build, nearest lines), 1022-1024
(LDS staging of the sort and the bucketing), 2^11 / 2^13 / 2^24 (LSD passes), 4096 (the front door's own encoder).  These
tests sit on both sides of each, check every operation bit-exact against the CPU oracle (and overlap / count against the
independent sparse numpy reference of ``_util``), and pin by kernel name which implementation ran where that is visible.
Contig ids outside the dictionary (-1, n_contigs, n_contigs + 1, INT32_MIN, INT32_MAX) never match and merge among themselves.
"""
import os

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
from _util import OracleEngine, random_side, sparse_count_overlaps, sparse_overlap, sparse_side
from oracle import oracle as O
from polars_bio_amd import _engine, range_op, synth
from test_gpu_parity import _canon, _cmp_all, _fused_overlap

gpu = pytest.mark.gpu
I32 = np.iinfo(np.int32)
OUTSIDE = lambda nc: [-1, nc, nc + 1, int(I32.min), int(I32.max)]        # noqa: E731


@pytest.fixture(scope="module")
def eng():
    return _engine.Engine(0)


def _fresh(monkeypatch, **env):
    """An Engine created under the given environment (the context reads its knobs once, at creation)."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return _engine.Engine(0)


def _in_dict(side, nc):
    m = (side[0] >= 0) & (side[0] < nc)
    return tuple(np.ascontiguousarray(a[m]) for a in side)


def _plant_outside(rng, side, nc, per_id=2):
    """Rows with every out-of-dictionary id, at random positions of the side."""
    c = side[0].copy()
    ids = np.repeat(np.array(OUTSIDE(nc), np.int64), per_id)
    pos = rng.choice(len(c), size=len(ids), replace=False)
    c[pos] = ids.astype(np.int32)
    return (c, side[1], side[2])


def _sweep_sides(nc, seed, n_build=30_000, n_probe=20_000, span=5000, max_len=100):
    """Build rows on most contigs of the dictionary (ids 0 and nc - 1 occupied, every 7th contig left empty), probes on every
    contig (those the build side lacks included) and on ids past the dictionary; both sides hold every out-of-dictionary id."""
    rng = np.random.default_rng(seed)
    keep = np.array([c for c in range(nc) if c % 7 != 3 or c in (0, nc - 1)], np.int32)
    bc, bs, be = random_side(rng, n_build, nc, span, max_len)
    bc = keep[rng.integers(0, len(keep), n_build)]
    bc[:2] = [0, nc - 1]
    pc, ps, pe = random_side(rng, n_probe, nc, span, max_len)
    pc[:2] = [0, nc - 1]
    build = _plant_outside(rng, (bc.astype(np.int32), bs, be), nc)
    probe = _plant_outside(rng, (pc, ps, pe), nc)
    return probe, build


def _view(nc, ids, hi):
    ids = np.concatenate([np.asarray(ids, np.int64), OUTSIDE(nc)]).astype(np.int32)
    return ids, np.zeros(len(ids), np.int32), np.full(len(ids), hi, np.int32)


def _check_sortscan(eng, probe, build, nc, strict, view_ids=None):
    """coverage / subtract / complement / merge / cluster against the oracle's numpy sweeps.  The numpy sweeps match contig
    ids by equality, so they get the build (right, frame) side without its out-of-dictionary rows; merge and cluster map those
    rows to one pseudo-contig (-1), which the engine orders last (as test_merge_cluster_coverage_parity)."""
    bd = _in_dict(build, nc)
    exp = O.np_coverage_fast(O.Side(*probe), O.Side(*bd), strict)
    for pm in (0, 1, 2):
        got = eng.coverage(probe, build, strict, nc, partition_mode=pm)
        assert (got == exp).all(), ("coverage", pm, int((got != exp).sum()))
    er, es, ee = O.np_subtract(O.Side(*probe), O.Side(*bd), strict)
    for pm in (2, 1):
        gr, gs, ge = eng.subtract(probe, build, strict, nc, partition_mode=pm)
        assert len(gr) == len(er), ("subtract", pm, len(gr), len(er))
        assert (gr == er).all() and (gs == es).all() and (ge == ee).all(), ("subtract", pm)
    hi = int(max(int(build[2].max()), int(probe[2].max()))) + 10 if len(build[0]) else 10
    view = _view(nc, np.arange(nc) if view_ids is None else view_ids, min(hi, int(I32.max)))
    ec, es, ee = O.np_complement(O.Side(*bd), O.Side(*view), strict)
    for pm in (0, 1):
        gr, gs, ge = eng.complement(build, view, strict, nc, partition_mode=pm)
        assert len(gr) == len(ec), ("complement", pm, len(gr), len(ec))
        assert (view[0][gr] == ec).all() and (gs == es).all() and (ge == ee).all(), ("complement", pm)
    c = np.where((build[0] >= 0) & (build[0] < nc), build[0], -1).astype(np.int32)
    for md in (0, 37):
        ecid, ecs, ece, (mc, ms, me, mn) = O.np_cluster(O.Side(c, build[1], build[2]), strict, md)
        gc, gs, ge, gn = eng.merge(build, strict, nc, md)
        eo = np.lexsort((ms, np.where(mc < 0, nc, mc)))
        assert len(gc) == len(mc), ("merge", md, len(gc), len(mc))
        assert (gc == mc[eo]).all() and (gs == ms[eo]).all() and (ge == me[eo]).all() and (gn == mn[eo]).all(), ("merge", md)
        cid, cs, ce, ncl = eng.cluster(build, strict, nc, md)
        assert ncl == len(mc) and (cs == ecs).all() and (ce == ece).all(), ("cluster", md)
        remap = np.empty(len(mc), np.int64)
        remap[eo] = np.arange(len(mc))
        assert (cid == remap[ecid]).all(), ("cluster ids", md)


def _check_sparse_reference(eng, probe, build, nc, strict):
    """overlap (probe order) and count_overlaps == the sparse numpy reference, on every input it is given."""
    rp, rb = sparse_overlap(probe, build, nc, strict)
    p, b = eng.overlap(probe, build, strict, nc, partition_mode=2)
    assert len(p) == len(rp) and (p == rp).all() and (b == rb).all(), "overlap vs sparse numpy reference"
    ec = np.bincount(rp, minlength=len(probe[0])).astype(np.int64)               # (= sparse_count_overlaps, without a second expansion)
    assert (eng.count_overlaps(probe, build, strict, nc) == ec).all(), "count vs sparse reference"


def _names(t):
    return sorted(t)


def _has(t, prefix):
    return any(k.startswith(prefix) for k in t)


# ---- (3) the sparse numpy reference itself (CPU) ---------------------------------------------------------------------------

@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("seed", range(6))
def test_sparse_reference_equals_the_brute_force_oracle(seed, strict):
    """The sparse reference == O.overlap_brute / O.count_overlaps_brute on small random inputs with inverted rows and ids outside
    the dictionary (the brute force matches any equal ids, so it gets the build side without them)."""
    rng = np.random.default_rng(880 + seed)
    nc = int(rng.choice([1, 3, 64, 300]))
    probe = random_side(rng, int(rng.integers(1, 500)), nc + 2, 3000, 200)
    build = random_side(rng, int(rng.integers(1, 600)), nc, 3000, 200)
    inv = rng.random(len(build[0])) < 0.1
    build = (build[0], np.where(inv, build[2], build[1]).astype(np.int32), np.where(inv, build[1], build[2]).astype(np.int32))
    build = _plant_outside(rng, build, nc, per_id=1) if len(build[0]) >= 5 else build
    pinv = rng.random(len(probe[0])) < 0.1                           # inverted rows on both sides: the predicate's both operands
    probe = (np.where(rng.random(len(probe[0])) < 0.05, np.int32(I32.min), probe[0]).astype(np.int32),
             np.where(pinv, probe[2], probe[1]).astype(np.int32), np.where(pinv, probe[1], probe[2]).astype(np.int32))
    keep = np.nonzero((build[0] >= 0) & (build[0] < nc))[0]
    bp, bb = O.overlap_brute(O.Side(*probe), O.Side(*(a[keep] for a in build)), strict)
    bb = keep[bb].astype(np.int32)
    o = np.lexsort((bb, build[1][bb], bp))                           # brute: probe row, then (build start, build row) -- unchanged by keep
    rp, rb = sparse_overlap(probe, build, nc, strict)
    assert len(rp) == len(bp) and (rp == bp[o]).all() and (rb == bb[o]).all()
    sp, sb = sparse_overlap(probe, build, nc, strict, block=97)     # expanded in many small blocks: the same pairs
    assert len(sp) == len(rp) and (sp == rp).all() and (sb == rb).all()
    ec = O.count_overlaps_brute(O.Side(*probe), O.Side(*(a[keep] for a in build)), strict)
    assert (sparse_count_overlaps(probe, build, nc, strict) == ec).all()
    assert len(rp) > 0 or len(build[0]) < 20


# ---- (1a) threshold sweep --------------------------------------------------------------------------------------------------

SWEEP = [1, 63, 64, 65, 255, 256, 257, 1021, 1022, 1023, 1024, 1025, 2047, 2048, 2049, 4096, 4097]


@gpu
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("nc", SWEEP)
def test_threshold_sweep_every_operation(eng, nc, strict, monkeypatch):
    probe, build = _sweep_sides(nc, 7000 + nc)
    _cmp_all(eng, probe, build, nc, strict)
    _check_sortscan(eng, probe, build, nc, strict)
    _check_sparse_reference(eng, probe, build, nc, strict)
    ix = O.Index(O.Side(*build), nc)
    ps = O.Side(*probe)
    if nc <= 256:
        # count_overlaps with the per-contig metadata read from global memory (the kernel above 256 contigs), both modes
        e = _fresh(monkeypatch, IVJ_COUNT_NOLDS="1")
        try:
            ec = O.count_overlaps_fast(ix, ps, strict)
            for tm, pm in ((0, 0), (2, 2), (1, 2), (1, 1)):
                assert (e.count_overlaps(probe, build, strict, nc, table_mode=tm, partition_mode=pm) == ec).all(), ("NOLDS", tm, pm)
        finally:
            e.close()
            monkeypatch.delenv("IVJ_COUNT_NOLDS")
    if nc in (63, 64, 65):
        # the round-2 slice path (contig-aligned slices off): its direct-address bucket table serves up to 64 contigs
        ep, eb = O.overlap_fast(ix, ps, strict)
        e = _fresh(monkeypatch, IVJ_CS="0")
        try:
            e.enable_timing(2)
            for sr in (64, 0):
                e.timings()
                p, b = _canon(*e.overlap(probe, build, strict, nc, partition_mode=6, slice_rows=sr))
                t = e.timings()
                assert len(p) == len(ep) and (p == ep).all() and (b == eb).all(), ("round-2 slices", sr)
                assert _has(t, "slice_join") and not _has(t, "cs_"), _names(t)
                assert ("slice_tab" in t) == (nc <= 64), ("direct-address table at", nc, _names(t))
            hp, hb = _fused_overlap(e, probe, build, strict, nc, 6, len(ep))
            p, b = _canon(hp, hb)
            assert (p == ep).all() and (b == eb).all(), "round-2 slices, fused"
        finally:
            e.close()


# ---- (1b) which implementation runs on each side of a threshold ------------------------------------------------------------

@gpu
@pytest.mark.parametrize("nc", [255, 256])
def test_balanced_index_build_up_to_255_contigs(nc):
    """The balanced build holds nc + 1 <= 256 contig keys: 255 contigs take it, 256 the LSD sort (200 k build rows, inside the
    automatic size window of the balanced build)."""
    rng = np.random.default_rng(61)
    build = random_side(rng, 200_000, nc, 3_000_000, 2000)
    probe = random_side(rng, 60_000, nc + 1, 3_000_000, 2000)
    ps = O.Side(*probe)
    ix = O.Index(O.Side(*build), nc)
    e = _engine.Engine(0)
    try:
        e.enable_timing(2)
        for strict in (True, False):
            ep, eb = O.overlap_fast(ix, ps, strict)
            e.timings()
            p, b = e.overlap(probe, build, strict, nc, partition_mode=2)
            t = e.timings()
            if nc == 255:
                assert "ix3_local" in t and "ix_final" not in t, _names(t)
            else:
                assert "ix_final" in t and "ix3_local" not in t, _names(t)
            assert len(p) == len(ep) and (p == ep).all() and (b == eb).all()
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("nc", [256, 257])
def test_contig_aligned_slices_up_to_256_contigs(nc):
    """600 k x 80 k rows under the automatic choice: the contig-aligned slice kernels at 256 contigs, none at 257 (and no round-2
    slices either: the count -> fill pair never takes them automatically); exact pairs both times."""
    rng = np.random.default_rng(62)
    build = random_side(rng, 80_000, nc, 3_000_000, 2000)
    probe = random_side(rng, 600_000, nc, 3_000_000, 150)
    ps = O.Side(*probe)
    ix = O.Index(O.Side(*build), nc)
    e = _engine.Engine(0)
    try:
        e.enable_timing(2)
        for strict in (True, False):
            ep, eb = O.overlap_fast(ix, ps, strict)
            e.timings()
            p, b = _canon(*e.overlap(probe, build, strict, nc))
            t = e.timings()
            if nc == 256:
                assert _has(t, "cs_join"), _names(t)
            else:
                assert not _has(t, "cs_") and not _has(t, "slice_"), _names(t)
            assert len(p) == len(ep) and (p == ep).all() and (b == eb).all()
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("nc", [256, 257])
def test_nearest_lines_up_to_256_contigs(nc):
    """table_mode 3 asks for the nearest lines; k_nearest_k1_lines keeps its per-contig metadata in LDS, so it serves 256
    contigs and not 257 (the two-gather kernel does); exact either way."""
    rng = np.random.default_rng(63)
    build = random_side(rng, 50_000, nc, 2_000_000, 1000)
    probe = random_side(rng, 40_000, nc + 2, 2_000_000, 300)
    ps = O.Side(*probe)
    ix = O.Index(O.Side(*build), nc)
    e = _engine.Engine(0)
    try:
        e.enable_timing(2)
        for strict in (True, False):
            ei, ed, en = O.nearest_fast(ix, ps, strict, 1, True)
            e.timings()
            i, d, n = e.nearest(probe, build, strict, nc, 1, True, table_mode=3)
            t = e.timings()
            assert ("nearest_k1_lines" in t) == (nc == 256), _names(t)
            assert (n == en).all() and (d == ed).all() and (i == ei).all()
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("nc", [257, 1023, 1025, 4097])
def test_forced_round2_slices_above_256_contigs(nc):
    """partition_mode 6 above 256 contigs: the round-2 slice kernels (no contig-aligned ones), exact pairs."""
    probe, build = _sweep_sides(nc, 64 + nc, n_build=100_000, n_probe=80_000, span=200_000, max_len=300)
    ps = O.Side(*probe)
    ix = O.Index(O.Side(*build), nc)
    e = _engine.Engine(0)
    try:
        e.enable_timing(2)
        for strict in (True, False):
            ep, eb = O.overlap_fast(ix, ps, strict)
            e.timings()
            p, b = _canon(*e.overlap(probe, build, strict, nc, partition_mode=6))
            t = e.timings()
            assert _has(t, "slice_join") and not _has(t, "cs_"), _names(t)
            assert len(p) == len(ep) and (p == ep).all() and (b == eb).all()
            e.timings()
            hp, hb = _fused_overlap(e, probe, build, strict, nc, 6, len(ep))
            t = e.timings()
            assert _has(t, "slice_join") and not _has(t, "cs_"), _names(t)
            p, b = _canon(hp, hb)
            assert (p == ep).all() and (b == eb).all()
    finally:
        e.close()


# ---- (1c) large sparse dictionaries ----------------------------------------------------------------------------------------

SPARSE = [  # (n_contigs, build rows, probe rows, occupied contigs, start offset, span)
    (5000, 30_000, 20_000, 2000, 0, 1_000_000),
    (70_000, 20_000, 20_000, 8000, 0, 1_000_000),                    # more contigs than build rows
    ((1 << 20) + 1, 40_000, 20_000, 10_000, -500_000, 2_000_000),
    ((1 << 24) + 1, 30_000, 20_000, 5000, int(I32.min) + 10, (1 << 32) - 5_000_000),   # starts over nearly all of int32
]


def _lsd_passes(nc):
    bits = max(1, int(nc).bit_length())                               # os_bits_for: contig keys 0 .. nc
    return (32 + bits + 10) // 11


@gpu
@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("nc,n_build,n_probe,occupied,lo,span", SPARSE, ids=["5000", "70000", "2^20+1", "2^24+1"])
def test_large_sparse_dictionaries(eng, nc, n_build, n_probe, occupied, lo, span, strict):
    rng = np.random.default_rng(nc % 100_003)
    build = sparse_side(rng, n_build, nc, occupied, span, 2000, lo)
    counts = np.bincount(build[0], minlength=nc)
    assert counts[0] > 0 and counts[nc - 1] > 0 and (counts == 0).sum() > nc // 2 and (counts == 1).sum() > 100 and counts.max() > 1000
    pc = np.where(rng.random(n_probe) < 0.8, build[0][rng.integers(0, n_build, n_probe)], rng.integers(0, nc, n_probe)).astype(np.int32)
    ps = (lo + rng.integers(0, span, n_probe, dtype=np.int64))
    pe = np.minimum(ps + rng.integers(0, 3000, n_probe), int(I32.max))
    probe = _plant_outside(rng, (pc, ps.astype(np.int32), pe.astype(np.int32)), nc)
    build = _plant_outside(rng, build, nc)
    _cmp_all(eng, probe, build, nc, strict)
    occ = np.nonzero(counts)[0]
    view_ids = np.concatenate([occ, rng.integers(0, nc, 500)])
    _check_sortscan(eng, probe, build, nc, strict, view_ids=view_ids)
    _check_sparse_reference(eng, probe, build, nc, strict)
    # the LSD index build launches one pass per 11 bits the (contig, start) keys of this dictionary can need: 6 for 2^24 + 1
    # contigs.  Only the launch count is visible (a pass beyond the data's key width exits on the device), so the input
    # itself is checked to span nearly all of int32, which makes every one of the 6 passes sort real digits.
    eng.enable_timing(2)
    try:
        eng.timings()
        eng.overlap(probe, build, strict, nc, partition_mode=2)
        t = eng.timings()
    finally:
        eng.enable_timing(0)
    assert t["ix_pass"]["launches"] == _lsd_passes(nc), (_lsd_passes(nc), _names(t))
    if nc == (1 << 24) + 1:
        assert _lsd_passes(nc) == 6 and int(build[1].min()) < -(1 << 30) and int(build[1].max()) > (1 << 30)


# ---- (1d) relabelled contigs give the same answers -------------------------------------------------------------------------

def _all_ops(eng, probe, build, nc, strict):
    p, b = _canon(*eng.overlap(probe, build, strict, nc))
    return {"pairs": (p.copy(), b.copy()), "count": eng.count_overlaps(probe, build, strict, nc),
            "nearest": eng.nearest(probe, build, strict, nc), "coverage": eng.coverage(probe, build, strict, nc),
            "merge": eng.merge(build, strict, nc)}


def _relabel(side, f):
    return (f[side[0]].astype(np.int32), side[1], side[2])


@gpu
@pytest.mark.parametrize("strict", [True, False])
def test_embedding_invariance_10M_x_1M(eng, strict):
    """synth's 10 M x 1 M, 24-contig input relabelled injectively into 256 contigs (random permutation: contig-aligned slices) and
    into 2^20 contigs (c -> 40009 c + 17: the window kernels) gives the 24-contig answers, which are the oracle's."""
    probe = synth.make_side(10_000_000, 42, synth.PROBE_LEN, 24)
    build = synth.make_side(1_000_000, 43, synth.BUILD_LEN, 24)
    base = _all_ops(eng, probe, build, 24, strict)
    ps, bs = O.Side(*probe), O.Side(*build)
    ix = O.Index(bs, 24)
    cores = os.cpu_count() or 1
    ep, eb = O.overlap_fast(ix, ps, strict, threads=cores)
    assert len(base["pairs"][0]) == len(ep) and (base["pairs"][0] == ep).all() and (base["pairs"][1] == eb).all()
    assert (base["count"] == O.count_overlaps_fast(ix, ps, strict, threads=cores)).all()
    ei, ed, en = O.nearest_fast(ix, ps, strict, 1, True)
    assert (base["nearest"][0] == ei).all() and (base["nearest"][1] == ed).all() and (base["nearest"][2] == en).all()
    assert (base["coverage"] == O.np_coverage_fast(ps, bs, strict)).all()
    _, _, _, (mc, ms, me, mn) = O.np_cluster(bs, strict, 0)
    gm = base["merge"]
    assert (gm[0] == mc).all() and (gm[1] == ms).all() and (gm[2] == me).all() and (gm[3] == mn).all()
    rng = np.random.default_rng(65)
    for nc, f in ((256, rng.permutation(256)[:24]), (1 << 20, np.arange(24) * 40009 + 17)):
        got = _all_ops(eng, _relabel(probe, f), _relabel(build, f), nc, strict)
        assert (got["pairs"][0] == base["pairs"][0]).all() and (got["pairs"][1] == base["pairs"][1]).all(), nc
        assert (got["count"] == base["count"]).all(), nc
        for g, w in zip(got["nearest"], base["nearest"]):
            assert (g == w).all(), nc
        assert (got["coverage"] == base["coverage"]).all(), nc
        inv = np.full(nc, -1, np.int64)
        inv[f] = np.arange(24)
        mc2 = inv[got["merge"][0]]
        o = np.lexsort((got["merge"][1], mc2))
        assert len(o) == len(gm[0]) and (mc2[o] == gm[0]).all(), nc
        assert all((got["merge"][k][o] == gm[k]).all() for k in (1, 2, 3)), nc


# ---- (1e) the round-2 slice path under the automatic choice ----------------------------------------------------------------

@gpu
@pytest.mark.parametrize("strict", [True, False])
def test_full_size_round2_slices_by_the_automatic_choice(eng, strict):
    """Above 256 contigs the automatic choice takes the round-2 slices only for the fused pass of >= 24 Mi probes x >= 4 Mi build
    rows: 26 M x 4.5 M rows over 1000 contigs (4.5 M rows fit 1536 slices x 5120 rows).  Pair total and build-row checksum == the
    oracle's baseline; the slice kernels ran."""
    rng = np.random.default_rng(66)
    nc, n_p, n_b, clen = 1000, 26_000_000, 4_500_000, 3_000_000
    def side(n, lens):
        c = rng.integers(0, nc, n).astype(np.int32)
        ln = rng.integers(lens[0], lens[1] + 1, n)
        s = rng.integers(0, clen - lens[1], n)
        return c, s.astype(np.int32), (s + ln).astype(np.int32)
    probe, build = side(n_p, synth.PROBE_LEN), side(n_b, synth.BUILD_LEN)
    assert n_p >= 24 << 20 and n_b >= 4 << 20 and n_b <= 1536 * 5120
    ix = O.Index(O.Side(*build), nc)
    total, checksum = O.overlap_baseline(ix, O.Side(*probe), strict, os.cpu_count() or 1)
    eng.enable_timing(2)
    try:
        eng.timings()
        hp, hb = _fused_overlap(eng, probe, build, strict, nc, 0, total)
        t = eng.timings()
    finally:
        eng.enable_timing(0)
    assert _has(t, "slice_join_fused") and not _has(t, "cs_"), _names(t)
    assert len(hb) == total and int(hb.astype(np.int64).sum()) == checksum
    assert (probe[0][hp] == build[0][hb]).all()


# ---- (1f) refusal --------------------------------------------------------------------------------------------------------

@gpu
def test_dictionary_beyond_the_int32_tables_is_refused(eng):
    """2 * rows + 2 * n_contigs + 64 > 2^31: every host entry that builds an index refuses on the host (IVJ_EINVAL) before it
    allocates an index or launches a kernel."""
    nc = (1 << 30) + 1
    one = (np.zeros(1, np.int32), np.array([5], np.int32), np.array([9], np.int32))
    calls = {
        "overlap": lambda: eng.overlap(one, one, True, nc),
        "overlap_rows": lambda: eng.overlap_rows(one, one, True, nc),
        "count_overlaps": lambda: eng.count_overlaps(one, one, False, nc),
        "nearest k=1": lambda: eng.nearest(one, one, True, nc),
        "nearest k=3": lambda: eng.nearest(one, one, True, nc, 3, False),
        "coverage": lambda: eng.coverage(one, one, True, nc),
        "subtract": lambda: eng.subtract(one, one, True, nc),
        "complement": lambda: eng.complement(one, one, True, nc),
        "merge": lambda: eng.merge(one, True, nc),
        "cluster": lambda: eng.cluster(one, True, nc),
        "probe_stream": lambda: eng.probe_stream(one, True, nc),
    }
    for name, call in calls.items():
        with pytest.raises(_engine.EngineError) as ei:
            call()
        assert ei.value.code == -1 and "2*rows + 2*contigs" in str(ei.value), (name, str(ei.value))
    ptrs = [eng.dev_alloc(16) for _ in range(3)]
    try:
        for p, col in zip(ptrs, one):
            eng.h2d(p, col)
        with pytest.raises(_engine.EngineError) as ei:
            eng.index_build_dev(eng.dev_side(*ptrs, 1), _engine.make_opts(True, nc))
        assert ei.value.code == -1
    finally:
        for p in ptrs:
            eng.dev_free(p)
    p, b = eng.overlap(one, one, True, 1)                            # the context still works
    assert p.tolist() == [0] and b.tolist() == [0]


# ---- (2) the front door with thousands of chrom names --------------------------------------------------------------------

def _scaffold_frame(rng, n, n_names, zero_based, span=3000):
    names = np.array([f"scaffold_{i}" for i in range(9000)], dtype=object)
    start = rng.integers(1, span, n)
    df = pd.DataFrame({"chrom": names[rng.integers(0, n_names, n)], "start": start.astype(np.int64),
                       "end": (start + rng.integers(0, 400, n)).astype(np.int64), "id": np.arange(n, dtype=np.int64)})
    df.attrs["coordinate_system_zero_based"] = zero_based
    return df


def _front_door_results(df1, df2):
    out = {}
    ov = pb.overlap(df1, df2, output_type="pandas.DataFrame")
    out["overlap"] = ov.sort_values(["id_1", "id_2"]).reset_index(drop=True)
    out["count"] = pb.count_overlaps(df1, df2, output_type="pandas.DataFrame")
    for k, o in ((1, True), (3, False)):
        out[f"nearest{k}{o}"] = pb.nearest(df1, df2, k=k, overlap=o, output_type="pandas.DataFrame")
    out["coverage"] = pb.coverage(df1, df2, output_type="pandas.DataFrame")
    out["merge"] = pb.merge(df1, output_type="pandas.DataFrame")
    return out


def _plain(df):
    """Chrom columns as plain objects (a categorical input gives categorical chrom columns), missing values as None."""
    df = df.reset_index(drop=True)
    for col in ("chrom", "chrom_1", "chrom_2"):
        if col in df.columns:
            v = df[col].astype(object)
            df[col] = v.where(v.notna(), None)
    return df


def _frames_equal(got, exp):
    for k in exp:
        pd.testing.assert_frame_equal(got[k].reset_index(drop=True), exp[k].reset_index(drop=True), check_dtype=False, obj=k)


@gpu
@pytest.mark.parametrize("zero_based", [True, False])
def test_front_door_9000_scaffolds_equals_the_oracle_engine(zero_based, monkeypatch):
    """9000 chrom names (more than the front door's own encoder takes: pyarrow's encoder runs), df2 on 8000 of them; pandas,
    pyarrow and a categorical chrom of 70 k categories (most unused): the HIP engine == the oracle-backed engine, and overlap /
    count / coverage == the per-contig oracle on contig ids taken from the raw strings (so a mis-encoding that both engines
    share would still show); every pair joins equal chrom names."""
    rng = np.random.default_rng(67)
    df1 = _scaffold_frame(rng, 40_000, 9000, zero_based)
    df2 = _scaffold_frame(rng, 30_000, 8000, zero_based)
    assert df1["chrom"].nunique() > 4096
    cats = [f"scaffold_{i}" for i in range(70_000)]
    c1, c2 = df1.copy(), df2.copy()
    c1["chrom"] = pd.Categorical(c1["chrom"], categories=cats)
    c2["chrom"] = pd.Categorical(c2["chrom"], categories=cats)
    c1.attrs["coordinate_system_zero_based"] = c2.attrs["coordinate_system_zero_based"] = zero_based
    md = {b"coordinate_system_zero_based": str(zero_based).lower().encode()}
    t1 = pa.Table.from_pandas(df1, preserve_index=False).replace_schema_metadata(md)
    t2 = pa.Table.from_pandas(df2, preserve_index=False).replace_schema_metadata(md)
    got = {"pandas": _front_door_results(df1, df2), "arrow": _front_door_results(t1, t2), "categorical": _front_door_results(c1, c2)}
    with monkeypatch.context() as m:
        m.setattr(range_op, "default_engine", lambda: OracleEngine())
        exp = _front_door_results(df1, df2)
    assert len(exp["overlap"]) > 10_000
    # independent of either encoder: contig ids from the raw strings, per-contig oracle on them
    names = np.unique(np.concatenate([df1["chrom"].to_numpy(str), df2["chrom"].to_numpy(str)]))
    side = lambda df: (np.searchsorted(names, df["chrom"].to_numpy(str)).astype(np.int32),   # noqa: E731
                       df["start"].to_numpy(np.int32), df["end"].to_numpy(np.int32))
    ps, bs = O.Side(*side(df1)), O.Side(*side(df2))
    ix = O.Index(bs, len(names))
    ep, eb = O.overlap_fast(ix, ps, zero_based)
    eo = np.lexsort((eb, ep))
    ec = O.count_overlaps_fast(ix, ps, zero_based)
    ecov = O.np_coverage_fast(ps, bs, zero_based)
    c1s, c2s = df1["chrom"].to_numpy(str), df2["chrom"].to_numpy(str)
    for kind, g in got.items():
        ov = _plain(g["overlap"])
        i1, i2 = ov["id_1"].to_numpy(np.int64), ov["id_2"].to_numpy(np.int64)
        assert len(i1) == len(ep) and (i1 == ep[eo]).all() and (i2 == eb[eo]).all(), (kind, "overlap vs per-contig oracle")
        ch1, ch2 = ov["chrom_1"].to_numpy(str), ov["chrom_2"].to_numpy(str)
        assert (ch1 == ch2).all() and (ch1 == c1s[i1]).all() and (ch2 == c2s[i2]).all(), (kind, "chrom names of the pairs")
        assert (g["count"]["count"].to_numpy() == ec).all(), (kind, "count vs per-contig oracle")
        assert (g["coverage"]["coverage"].to_numpy() == ecov).all(), (kind, "coverage vs per-contig oracle")
        for k in exp:
            pd.testing.assert_frame_equal(_plain(g[k]), _plain(exp[k]), check_dtype=False, obj=f"{kind} {k}")


@gpu
def test_two_device_slots_equal_one_on_9000_scaffolds():
    """Contig sharding over thousands of contigs: two device slots give the one-slot answers."""
    rng = np.random.default_rng(68)
    df1 = _scaffold_frame(rng, 60_000, 9000, True)
    df2 = _scaffold_frame(rng, 30_000, 8000, True)
    ref = _front_door_results(df1, df2)
    pb.set_option("ivj.devices", "0,0")
    try:
        got = _front_door_results(df1, df2)
    finally:
        pb.set_option("ivj.devices", "auto")
    _frames_equal(got, ref)
