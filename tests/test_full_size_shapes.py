"""Parity at full size on nested, clustered and sorted interval sets (tests/_shapes.py).

tests/test_full_size.py runs every operation at its stated size on ONE kind of input (short rows, uniform positions), where the
slice path takes one set of branches: the plain join kernel, the sampled partition, 8-byte records, the nearest lines.  The
cases here give the other branches the same sizes -- probe sides beyond 32 Mi rows (16 384-probe tiles with implied row ids,
the large-n jchunk rule), record offsets beyond 2^28 bytes -- and assert from the engine's timings that the branch ran:

  A  chains            32 Mi uniform probes x 5 M nested rows: the walking join kernel (k_cs_join over the block maxima)
  B  sorted / hot      read pile-ups in sorted runs: the sampled regions overflow, the call is redone histogram-first
  C  long probes       rows between the sampled groups that an 8-byte record cannot hold: the 12-byte redo and its give-up rule
  D  dense nested      >= 16 pairs per probe: the flat kernel, which hands long sparse windows on
  E  tail at the limit far share just above / below CS_FAR_LIMIT: both join kernels, one knob apart
  F  nearest / count_overlaps on nested build sides
  G  the front door once (pandas frames of case E)

Every case: the oracle's counts must equal the two-rank formula #{s2 < e1} - #{e2 <= s1} computed here at full size (no
prefix-max structure: nesting cannot fool it), the device counts must equal them, and the pair lists must have exactly these
multiplicities, satisfy the predicate and be contiguous, strictly ascending runs per probe row with the oracle's checksum
(test_full_size._check_pair_properties); one path per case is also compared with the oracle's exact list.
"""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import _shapes as S
from oracle import oracle as O
from polars_bio_amd import _engine
from test_full_size import _Dev, _check_pair_properties

pytestmark = pytest.mark.gpu

THREADS = max(1, min(16, len(os.sched_getaffinity(0))))
PAIR_LIMIT = 300_000_000            # two int32 pair columns + a sort index next to the inputs, host and HBM


@pytest.fixture(scope="module")
def eng():
    e = _engine.Engine(0)
    e.enable_timing(2)
    yield e
    e.close()


@pytest.fixture(scope="module")
def chain_a():
    """Case A's build side (cases B and C share it) and its statistics."""
    build = S.chain_side(**S.CASE_A_BUILD)
    st = S.shape_stats(build, 24)
    assert st["far_share"] >= 100 * S.CS_FAR_LIMIT and st["mean_depth"] >= 4, st
    return build


def _two_rank(probe, build, strict):
    """O.np_count_overlaps over row ranges of the probe side, one range per thread (numpy releases the GIL in its sorts)."""
    n = len(probe[0])
    bs = O.Side(*build)
    cuts = np.linspace(0, n, 2 * THREADS + 1).astype(np.int64)

    def part(i):
        lo, hi = int(cuts[i]), int(cuts[i + 1])
        return O.np_count_overlaps(O.Side(*(a[lo:hi] for a in probe)), bs, strict)
    with ThreadPoolExecutor(THREADS) as ex:
        return np.concatenate(list(ex.map(part, range(2 * THREADS))))


class _Expect:
    """The oracle's answer for one (probe, build, strict), checked against the two-rank formula before any device work."""

    def __init__(self, probe, build, nc, strict, hit=(0.25, 0.20), two_rank=True):
        self.probe, self.build, self.nc, self.strict = probe, build, nc, strict
        ps = O.Side(*probe)
        ix = O.Index(O.Side(*build), nc)
        self.counts = O.count_overlaps_fast(ix, ps, strict, threads=THREADS)
        self.total = int(self.counts.sum())
        assert self.total <= PAIR_LIMIT, self.total
        if two_rank:
            assert (self.counts == _two_rank(probe, build, strict)).all(), "the oracle's counts differ from the two-rank formula"
        if hit is not None:
            some = float((self.counts > 0).mean())
            assert some >= hit[0] and 1.0 - some >= hit[1], ("vacuous: share of probes with a hit", some)
        self.ep, self.eb = O.overlap_fast(ix, ps, strict, threads=THREADS)
        assert len(self.ep) == self.total
        self.checksum = int(self.eb.astype(np.int64).sum())
        ix.close()

    def check(self, hp, hb, what, exact=False):
        assert (self.probe[0][hp] == self.build[0][hb]).all(), (what, "contig")
        _check_pair_properties(hp, hb, self.probe, self.build, self.counts, self.checksum, what, strict=self.strict)
        if exact:
            o = np.argsort(hp, kind="stable")
            assert (hp[o] == self.ep).all() and (hb[o] == self.eb).all(), (what, "exact list")


class _Run:
    """Both sides in HBM, the index and two pair columns of the expected size on one engine."""

    def __init__(self, eng, x, index_nc=None):
        self.eng, self.x = eng, x
        self.d = _Dev(eng, x.probe, x.build)
        self.op, self.ob = self.d.alloc(4 * x.total), self.d.alloc(4 * x.total)
        self.ix = eng.index_build_dev(self.d.build, _engine.make_opts(x.strict, x.nc))

    def opts(self, pm=0, det=False):
        return _engine.make_opts(self.x.strict, self.x.nc, partition_mode=pm, deterministic=det)

    def _pairs(self):
        hp, hb = np.empty(self.x.total, np.int32), np.empty(self.x.total, np.int32)
        self.eng.d2h(hp, self.op)
        self.eng.d2h(hb, self.ob)
        return hp, hb

    def fused(self, pm=0, probe=None):
        got, fits = self.eng.overlap_fused_dev(self.ix, probe or self.d.probe, self.opts(pm), self.op, self.ob, self.x.total)
        assert fits and got == self.x.total, (pm, got, self.x.total)
        return self._pairs()

    def count_fill(self, pm=0, det=False):
        o = self.opts(pm, det)
        assert self.eng.overlap_count_dev(self.ix, self.d.probe, o) == self.x.total, (pm, det)
        self.eng.overlap_fill_dev(self.ix, self.d.probe, o, self.op, self.ob, self.x.total)
        return self._pairs()

    def counts(self):
        n = len(self.x.probe[0])
        cp = self.d.alloc(8 * n)
        self.eng.count_overlaps_dev(self.ix, self.d.probe, self.opts(), cp)
        got = np.empty(n, np.int64)
        self.eng.d2h(got, cp)
        return got

    def close(self):
        self.ix.close()
        self.d.close()


def _fresh_engine():
    e = _engine.Engine(0)
    e.enable_timing(2)
    return e


# ---- A: chains at headline size ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strict", [True, False], ids=["strict", "weak"])
def test_full_size_chains_take_the_walking_join_kernel(eng, chain_a, strict, monkeypatch):
    """32 Mi + 12 345 uniform probes x 5 M nested rows (far share 0.97, mean depth 10; ~ 1.26e8 pairs): auto mode and mode 6
    -- fused pass, count -> fill pair, the deterministic pair twice with identical bytes -- the 256-bucket path as a cross-check,
    count_overlaps; hier_low and the three cs_join passes must have run (cs_join_fill: the fill that matches again,
    IVJ_CS_NOCACHE=1; the default fill reads COUNT's words, cs_fill_cached).  The plain kernel forced onto the same data
    (IVJ_CS_WALK=0, fresh engine) gives the same answer without the block maxima."""
    probe = S.uniform_side(**S.CASE_A_PROBES)
    assert len(probe[0]) >= S.N_32MI
    x = _Expect(probe, chain_a, 24, strict)
    r = _Run(eng, x)
    try:
        eng.timings()
        x.check(*r.fused(0), "fused auto")
        x.check(*r.count_fill(0), "count -> fill auto", exact=True)
        assert (r.counts() == x.counts).all(), "count_overlaps"
        t = eng.timings()
        assert "hier_low" in t, sorted(t)
        assert "cs_join_fused" in t and "cs_join_count" in t and "cs_fill_cached" in t, sorted(t)
        assert "cs_regions" in t and "cs_hist" not in t, sorted(t)                 # benign probes: sampled, not redone
        x.check(*r.fused(6), "fused slices")
        x.check(*r.count_fill(6), "count -> fill slices")
        hp, hb = r.count_fill(6, det=True)
        x.check(hp, hb, "deterministic pair")
        hp2, hb2 = r.count_fill(6, det=True)
        assert hp2.tobytes() == hp.tobytes() and hb2.tobytes() == hb.tobytes(), "the deterministic pair differs between two runs"
        del hp, hb, hp2, hb2
        t = eng.timings()
        assert "cs_scatter_stable" in t and "cs_join_count" in t, sorted(t)
        x.check(*r.fused(1), "fused 256 buckets")
    finally:
        r.close()
    for env, name in (("IVJ_CS_WALK", "0"), ("IVJ_CS_NOCACHE", "1")):
        monkeypatch.setenv(env, name)
        e = _fresh_engine()
        monkeypatch.delenv(env)
        r = _Run(e, x)
        try:
            if env == "IVJ_CS_WALK":
                x.check(*r.fused(0), "plain kernel on nested data")
                t = e.timings()
                assert "cs_join_fused" in t and "hier_low" not in t, sorted(t)
            else:
                x.check(*r.count_fill(0), "count -> fill that matches again")
                t = e.timings()
                assert "cs_join_fill" in t and "cs_join_count" in t and "hier_low" in t and "cs_fill_cached" not in t, sorted(t)
        finally:
            r.close()
            e.close()


# ---- B: sorted and hot probes --------------------------------------------------------------------------------------------------

def test_full_size_pileups_overflow_the_sampled_regions_and_are_redone(chain_a):
    """Read pile-ups of >= 32 Mi rows over case A's build side (dictionary of 25: 3 % of the reads sit on a contig the build
    side lacks): fully sorted by (contig, start); 30 % of the reads in 1 / 500 of one contig, in sorted runs of 8192 rows; every
    read in ONE slice.  Each variant's largest bucket holds >= 8 x the average bucket.  In sorted runs of 8192 rows a bucket's
    rows sit at the same offsets of every run, the sample reads 8 rows of every 512: most buckets are never sampled, their
    regions (slack 16 384 + n / 16 nb < the 22 k rows they receive) overflow, and the call must be redone histogram-first --
    cs_hist next to cs_regions, two cs_scatter launches -- with the exact answer.  A benign call on the same context
    afterwards is sampled again (cs_force_exact does not stick)."""
    benign = S.uniform_side(2_000_000, 113)
    bx = _Expect(benign, chain_a, 25, True)
    redone = {}
    for name, kw in S.CASE_B_PROBES.items():
        kw = dict(kw)
        if name == "one_bucket":
            kw["window"] = S.one_slice_window(chain_a)
        probe = S.pileup_side(**kw)
        assert len(probe[0]) >= S.N_32MI
        st = S.shape_stats(probe, 25, build=chain_a)
        assert st["bucket_share"] * st["n_buckets"] >= 8, (name, st)
        x = _Expect(probe, chain_a, 25, True)
        e = _fresh_engine()
        r = _Run(e, x)
        try:
            e.timings()
            x.check(*r.fused(0), f"{name}: fused auto", exact=True)
            t = e.timings()
            assert "cs_regions" in t, (name, sorted(t))                         # the first attempt was sampled
            redone[name] = "cs_hist" in t
            if redone[name]:
                assert t["cs_scatter"]["launches"] >= 2, (name, t["cs_scatter"])
            x.check(*r.count_fill(0), f"{name}: count -> fill auto")
            assert (r.counts() == x.counts).all(), name
            # the next call on this context: benign probes, sampled again, exact
            e.timings()
            d2 = _Dev(e, benign, (np.zeros(1, np.int32),) * 3)
            try:
                op, ob = d2.alloc(4 * bx.total), d2.alloc(4 * bx.total)
                got, fits = e.overlap_fused_dev(r.ix, d2.probe, r.opts(0), op, ob, bx.total)
                assert fits and got == bx.total
                hp, hb = np.empty(bx.total, np.int32), np.empty(bx.total, np.int32)
                e.d2h(hp, op)
                e.d2h(hb, ob)
            finally:
                d2.close()
            t = e.timings()
            assert "cs_regions" in t and "cs_hist" not in t, (name, sorted(t))
            bx.check(hp, hb, f"{name}: benign call afterwards", exact=True)
        finally:
            r.close()
            e.close()
    print("redone histogram-first:", redone)
    assert redone["hot"], redone
    assert any(redone.values()), "no variant overflowed its sampled regions at the default slack"


# ---- C: long probes between the sampled rows -----------------------------------------------------------------------------------

def test_full_size_long_probes_between_the_samples_and_the_give_up_rule(chain_a):
    """Case A's probes with every (512 x 37)-th row from row 100 stretched by 8 Mbp (more than a slice is wide): the sample
    picks 8-byte records, the scatter meets rows they cannot hold, the call is redone with 12-byte records (two cs_scatter
    launches, no histogram) and is exact.  Then the first 1 M rows: CS_REC8_GIVE_UP such calls in a row make the context stop
    offering the 8-byte form (one cs_scatter launch, no cs_scatter12), benign calls keep that up, and within 64 calls the
    form is offered again (host_cslice.hip.h::cs_partition); every call is exact."""
    base = S.uniform_side(**S.CASE_A_PROBES)
    probe = S.stretch_between_samples(base)
    x = _Expect(probe, chain_a, 24, True)
    cut = 1_000_000
    xl = _Expect(tuple(a[:cut] for a in probe), chain_a, 24, True, hit=None, two_rank=False)
    xb = _Expect(tuple(a[:cut] for a in base), chain_a, 24, True, hit=None, two_rank=False)
    assert (xl.counts != xb.counts).any()
    e = _fresh_engine()
    r = _Run(e, x)
    try:
        e.timings()
        x.check(*r.fused(0), "fused auto", exact=True)
        t = e.timings()
        assert t["cs_scatter"]["launches"] == 2 and "cs_scatter12" in t and "cs_hist" not in t, t
        assert "hier_low" in t, sorted(t)
        # the 1 M-row cuts: the long one is the head of the columns already in HBM, the benign one is uploaded next to it
        p = r.d.ptrs
        long_cut = e.dev_side(p[0], p[1], p[2], cut)
        bp = [r.d.alloc(4 * cut) for _ in range(3)]
        for ptr, col in zip(bp, xb.probe):
            e.h2d(ptr, np.ascontiguousarray(col, np.int32))
        benign_cut = e.dev_side(bp[0], bp[1], bp[2], cut)

        def call(side, xe):
            e.timings()
            got, fits = e.overlap_fused_dev(r.ix, side, r.opts(0), r.op, r.ob, xe.total)     # (a capacity >= 16 n would read as a dense result)
            assert fits and got == xe.total
            hp, hb = np.empty(xe.total, np.int32), np.empty(xe.total, np.int32)
            e.d2h(hp, r.op)
            e.d2h(hb, r.ob)
            key = np.sort((hp.astype(np.int64) << 32) | hb)
            assert (key == np.sort((xe.ep.astype(np.int64) << 32) | xe.eb)).all(), "a call of the give-up sequence is not exact"
            return e.timings()

        for i in range(3):                                  # CS_REC8_GIVE_UP (cslice.hip.h) calls in a row, behind the full-size one
            t = call(long_cut, xl)
            assert "cs_scatter" in t and "cs_hist" not in t, sorted(t)
            if i == 0:
                assert t["cs_scatter"]["launches"] == 2 and "cs_scatter12" in t, t      # still offered, overflowed, redone
        sticky, offered = 0, None
        for i in range(64):
            t = call(benign_cut, xb)
            assert t["cs_scatter"]["launches"] == 1 and "cs_hist" not in t, (i, t)
            if "cs_scatter12" in t:                          # both forms queued: the 8-byte form is offered again
                offered = i
                break
            sticky += 1
        assert sticky >= 1, "the sticky 12-byte fallback never engaged"
        assert offered is not None, "the 8-byte form was not offered again within 64 calls"
        t = call(benign_cut, xb)                             # ... and stays: the call that fitted reset the streak
        assert "cs_scatter12" in t and t["cs_scatter"]["launches"] == 1, t
    finally:
        r.close()
        e.close()


# ---- D: dense nested ------------------------------------------------------------------------------------------------------------

def test_full_size_dense_nested_result_takes_the_flat_kernel_which_hands_on(eng):
    """4 M probes x 2 M rows of deep chains (children 0.2 .. 0.8 of their parent) + a contig-wide row on four contigs: >= 16
    pairs per probe, so the fill of the count -> fill pair is the flat kernel at the exact capacity; under the contig-wide rows a
    probe's candidate range is its contig (flat.hip.h FLAT_MAX_CAND), the flat kernel flags the call and the window kernels
    redo it.  Exact."""
    build = S.with_wide_rows(S.chain_side(**S.CASE_D_BUILD), S.CASE_D_WIDE, scale=S.CASE_D_BUILD["scale"])
    probe = S.uniform_side(**S.CASE_D_PROBES)
    x = _Expect(probe, build, 24, True, hit=None)
    assert x.total >= 16 * len(probe[0]), x.total / len(probe[0])
    r = _Run(eng, x)
    try:
        eng.timings()
        x.check(*r.count_fill(0), "dense count -> fill", exact=True)
        t = eng.timings()
        assert "overlap_flat" in t, sorted(t)
        assert "overlap_fill" in t or any(k.startswith("cs_") for k in t), sorted(t)
        assert "overlap_fused" in t, sorted(t)                 # the window kernel that took the call over from the flat one
        x.check(*r.fused(0), "dense fused")
        assert (r.counts() == x.counts).all()
    finally:
        r.close()


# ---- E: tail build at the limit -------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tail_e():
    sides = {k: S.tail_side(**kw) for k, kw in S.CASE_E_BUILD.items()}
    far = {k: S.shape_stats(v, 24)["far_share"] for k, v in sides.items()}
    assert S.CS_FAR_LIMIT < far["above"] <= 3 * S.CS_FAR_LIMIT, far
    assert S.CS_FAR_LIMIT / 3 <= far["below"] < S.CS_FAR_LIMIT, far
    return sides, S.uniform_side(**S.CASE_E_PROBES)


@pytest.mark.parametrize("side", ["above", "below"])
def test_full_size_tail_build_on_both_sides_of_the_far_limit(tail_e, side):
    """10 M probes x 1 M exon-like rows with a thin tail of genes: far share 1.7 x CS_FAR_LIMIT / 0.5 x CS_FAR_LIMIT (from
    shape_stats, the rule of k_cs_bins): the walking kernel with its block maxima above the limit, the plain kernel below."""
    sides, probe = tail_e
    x = _Expect(probe, sides[side], 24, True)
    e = _fresh_engine()
    r = _Run(e, x)
    try:
        e.timings()
        x.check(*r.fused(0), "fused auto", exact=True)
        x.check(*r.count_fill(0), "count -> fill auto")
        assert (r.counts() == x.counts).all()
        t = e.timings()
        assert "cs_join_fused" in t and "cs_join_count" in t, sorted(t)
        assert ("hier_low" in t) == (side == "above"), (side, sorted(t))
    finally:
        r.close()
        e.close()


# ---- F: nearest and count_overlaps on nested build sides -----------------------------------------------------------------------

def test_full_size_nearest_on_a_nested_build_side(eng):
    """20 M pile-up probes x 2 M chain rows (dictionary of 25: 3 % of the probes on a contig without rows; reads beyond a
    contig's last build row come with the uniform positions): row, distance and n_found of every probe equal the oracle's.  On
    nested rows the nearest row to the left is NOT the positional neighbour: it is found through the prefix maxima."""
    build = S.chain_side(**S.CASE_F_BUILD)
    probe = S.pileup_side(**S.CASE_F_PROBES)
    n, nc = len(probe[0]), 25
    ix = O.Index(O.Side(*build), nc)
    last = np.zeros(nc + 1, np.int64)
    np.maximum.at(last, build[0], build[2])
    assert int((probe[1] > last[probe[0]])[probe[0] < 24].sum()) > 0, "no probe beyond the last build row of its contig"
    assert int((probe[0] == 24).sum()) > 0
    d = _Dev(eng, probe, build)
    try:
        ixd = eng.index_build_dev(d.build, _engine.make_opts(True, nc))
        for k, incl in ((1, True), (1, False), (3, True)):
            ei, ed, en = O.nearest_fast(ix, O.Side(*probe), True, k, incl, threads=THREADS)
            opts = _engine.make_opts(True, nc, k=k, include_overlaps=incl)
            pi, pd, pn = d.alloc(4 * n * k), d.alloc(8 * n * k), d.alloc(4 * n)
            eng.timings()
            eng.nearest_dev(ixd, d.probe, opts, pi, pd, pn)
            gi, gd, gn = np.empty((n, k), np.int32), np.empty((n, k), np.int64), np.empty(n, np.int32)
            eng.d2h(gi, pi)
            eng.d2h(gd, pd)
            eng.d2h(gn, pn)
            t = eng.timings()
            if k == 1 and incl:
                assert "nearest_k1_lines" in t and "nearest_k1_rest" in t, sorted(t)
                assert int((gd == 0).sum()) > n // 5 and int((gd > 0).sum()) > n // 5
            else:
                assert "nearest_general" in t, sorted(t)
            assert (gn == en).all() and (gd == ed).all() and (gi == ei).all(), (k, incl)
            assert int((gn == 0).sum()) >= int((probe[0] == 24).sum()) > 0
        ixd.close()
    finally:
        d.close()


def test_full_size_count_overlaps_of_pileups_on_a_nested_build_side(eng):
    """100 M pile-up probes x 200 k chain rows: the device counts equal the two-rank formula (and the oracle's) for every row."""
    build = S.chain_side(**S.CASE_F_COUNT_BUILD)
    probe = S.pileup_side(**S.CASE_F_COUNT_PROBES)
    n, nc = len(probe[0]), 25
    expect = _two_rank(probe, build, True)
    ix = O.Index(O.Side(*build), nc)
    assert (O.count_overlaps_fast(ix, O.Side(*probe), True, threads=THREADS) == expect).all()
    assert int((expect > 0).sum()) > 1_000_000 and int((expect == 0).sum()) > 1_000_000
    d = _Dev(eng, probe, build)
    try:
        opts = _engine.make_opts(True, nc)
        ixd = eng.index_build_dev(d.build, opts, with_end_order=True)
        cp = d.alloc(8 * n)
        eng.count_overlaps_dev(ixd, d.probe, opts, cp)
        got = np.empty(n, np.int64)
        eng.d2h(got, cp)
        ixd.close()
    finally:
        d.close()
    assert (got == expect).all()


# ---- G: the front door once -----------------------------------------------------------------------------------------------------

def test_full_size_tail_frames_through_the_front_door(tail_e, monkeypatch):
    """pb.overlap and pb.count_overlaps on case E's sides as pandas frames (range_op's policy sees the shape too): the frames
    the engine returns equal the ones the oracle engine returns."""
    import pandas as pd
    import polars_bio_amd as pb
    from polars_bio_amd import range_op, synth
    from _util import OracleEngine
    sides, probe = tail_e
    names = np.array(synth.CONTIG_NAMES)

    def frame(side):
        df = pd.DataFrame({"chrom": names[side[0]], "start": side[1], "end": side[2]})
        df.attrs["coordinate_system_zero_based"] = True
        return df
    df1, df2 = frame(probe), frame(sides["above"])
    got = pb.overlap(df1, df2, output_type="pandas.DataFrame")
    got_c = pb.count_overlaps(df2, df1, output_type="pandas.DataFrame")
    monkeypatch.setattr(range_op, "default_engine", lambda: OracleEngine())
    exp = pb.overlap(df1, df2, output_type="pandas.DataFrame")
    exp_c = pb.count_overlaps(df2, df1, output_type="pandas.DataFrame")
    assert len(got) == len(exp) > len(df1) // 4 and list(got.columns) == list(exp.columns)
    num = [c for c in got.columns if got[c].dtype.kind in "iu"]
    assert len(num) == 4, list(got.columns)
    og = np.lexsort([got[c].to_numpy() for c in num])
    oe = np.lexsort([exp[c].to_numpy() for c in num])
    for c in got.columns:
        assert (got[c].to_numpy()[og] == exp[c].to_numpy()[oe]).all(), c
    assert list(got_c.columns) == list(exp_c.columns) and len(got_c) == len(df2)
    for c in got_c.columns:
        assert (got_c[c].to_numpy() == exp_c[c].to_numpy()).all(), c
    assert int(got_c["count"].sum()) == len(got)
