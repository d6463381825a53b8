"""depth, the set operations with set_stats, multi_inter, overlap_bases and depth_summary ("all five ops") put through the
project's cross-cutting matrices, which their own modules -- each built around its kernel's tile -- leave out:

  (1) contig-dictionary sizes on both sides of every threshold test_contig_dictionaries.py names, and a sparse dictionary of
      2^24 + 1 ids, with every out-of-dictionary id planted in every frame;
  (2) the index build forms: the LSD sort, the balanced build with its merge and staging knobs, its two hand-overs, and the
      automatic choice at 140 000 rows -- pinned by kernel name;
  (3) the indexes the operations build for themselves (depth_core's sanitised re-index, multi_core's run index) under the
      balanced build and its hand-over;
  (4) many calls on one long-lived index in different orders, and one context under alternating large and small inputs;
  (5) on the CPU: the generators have the properties the GPU tests rely on, and the two independent references of every
      operation agree on them.

Expected values are the int64 numpy forms of the feature modules' util files; every comparison is bit-exact, order included."""
import numpy as np
import pytest

import _depth_util as U
import _setop_util as SO
import _multi_util as M
import _depth_sum_util as DS
import _depth_summary_util as DQ
import _position_ops_util as P
from oracle import oracle as O
from polars_bio_amd import _engine
from test_contig_dictionaries import OUTSIDE, _fresh
from test_gpu_parity import _v3_cases

gpu = pytest.mark.gpu
MODES = [pytest.param(True, id="strict"), pytest.param(False, id="weak")]
V3 = _v3_cases()
V3_IDS = ["ragged", "one_row", "rows_70k_outside", "negative_equal_keys", "bucket_above_lds", "linear_keys_33_bits"]
assert len(V3) == len(V3_IDS)


@pytest.fixture(scope="module")
def eng():
    return _engine.Engine(0)


@pytest.fixture(scope="module")
def dj():
    import torch  # noqa: F401
    from polars_bio_amd.device_api import DeviceJoin
    return DeviceJoin(0)


def _engine_under(monkeypatch, env):
    """(a fresh engine created under `env`, the function that closes it and restores the environment)"""
    e = _fresh(monkeypatch, **env)

    def done():
        e.close()
        for k in env:
            monkeypatch.delenv(k)
    return e, done


# ---- (5) CPU: the generators and the reference pairs -------------------------------------------------------------------------------------

def _references_agree(case, strict, what, brute=False, probes=400):
    """events vs dense, events vs brute, prefix vs pair, block vs dense on a case whose spans the dense forms can hold"""
    nc = case.nc
    exp = P.expected(case, strict, only=("depth", "setop", "set_stats", "bases", "summary") + (("multi",) if brute else ()))
    U.assert_blocks_equal(U.depth_dense(*case.frame, strict, nc), exp["depth"], f"{what}: depth_dense")
    for op in SO.OPS:
        regions, totals = SO.setop_dense(*case.pair, strict, nc, op)
        SO.assert_regions_equal(regions, exp["setop:" + op], f"{what}: setop_dense {op}")
        assert tuple(totals) == tuple(exp["set_stats"][:3]), f"{what}: totals {op}"
    if brute:
        for key, k, con in P.multi_keys(case):
            M.assert_equal(M.multi_brute(case.frames, strict, nc, k, con), exp[key], f"{what}: multi_brute {key}")
    if len(case.probe[0]):
        idx = DS.sample(len(case.probe[0]), len(case.frame[0]), cells=probes * max(len(case.frame[0]), 1))
        assert (DS.pair_form(case.probe, case.frame, strict, nc, idx) == exp["bases"][idx]).all(), f"{what}: pair_form"
        md, bg = DQ.dense_form(case.probe, case.frame, strict, nc, P.THRESHOLDS, idx)
        assert (md == exp["summary"][0][idx]).all() and (bg == exp["summary"][1][:, idx]).all(), f"{what}: dense_form"


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("nc", [1, 65, 257, 1025])
def test_cpu_sweep_inputs_and_reference_pairs(nc, strict):
    case = P.sweep_case(nc)
    for side in [case.probe, case.frame] + case.frames:
        assert 20_000 <= len(side[0]) <= 30_000
        assert set(OUTSIDE(nc)) <= set(side[0].tolist()), "every out-of-dictionary id in every frame"
        assert (side[0] == 0).any() and (side[0] == nc - 1).any()
    if nc > 7:
        empty = np.arange(3, nc - 1, 7)
        empty = empty[empty != 0]
        assert not np.isin(case.frame[0], empty).any() and np.isin(case.probe[0], empty).any(), "contigs on one side only"
    _references_agree(case, strict, case.name)
    # the out-of-dictionary rows change nothing in the references either
    bare, keep = P.without_outside(case)
    exp, exp_bare = P.expected(case, strict), P.expected(bare, strict)
    P.assert_same(exp, exp_bare, case.name, probe_keep=keep)


@pytest.mark.parametrize("strict", MODES)
def test_cpu_sparse_dictionary_inputs_and_reference_pairs(strict):
    case = P.sparse_case()
    nc = case.nc
    assert nc == (1 << 24) + 1
    counts = np.bincount(case.frame[0][P.inside(case.frame, nc)], minlength=nc)
    assert counts[0] > 0 and counts[nc - 1] > 0 and (counts == 0).sum() > nc // 2 and (counts == 1).sum() > 1000 and counts.max() > 1000
    for side in case.frames:
        assert set(OUTSIDE(nc)) <= set(side[0].tolist())
    rng = np.random.default_rng(5)
    occupied = np.flatnonzero(counts)
    contigs = np.unique(np.concatenate([[0, nc - 1], np.argpartition(counts, -4)[-4:], rng.choice(occupied, 40)]))
    _references_agree(P.on_contigs(case, contigs), strict, case.name)


@pytest.mark.parametrize("strict", MODES)
def test_cpu_index_form_inputs(strict):
    """the shapes of _v3_cases() really take the build their GPU test names, as a whole and as the row subsets of the set
    operations; the small-span ones under both references"""
    for entry, vid in zip(V3, V3_IDS):
        case, balanced = P.v3_case(entry), entry[4]
        for side in (case.frame,) + case.pair:
            if len(side[0]):
                assert P.takes_balanced_build(side, case.nc) == balanced, (vid, P.v3_geometry(side, case.nc))
        assert sum(len(f[0]) for f in case.frames) == len(case.frame[0]) == sum(len(f[0]) for f in case.pair)
        if vid in ("ragged", "negative_equal_keys"):
            _references_agree(case, strict, vid)
    span, _ = P.v3_geometry(P.v3_case(V3[5]).frame, 2)
    assert span > 1 << 32, "the linear keys of the last shape span more than 32 bits"
    span, fullest = P.v3_geometry(P.v3_case(V3[4]).frame, 1)
    assert span <= 0xffffffff and fullest > P.V3_CAP
    auto = P.auto_case()
    assert all(P.V3_AUTO_FROM <= len(f[0]) for f in auto.frames) and all(P.takes_balanced_build(f, auto.nc) for f in auto.frames)


@pytest.mark.parametrize("strict", MODES)
def test_cpu_own_index_inputs(strict):
    for case in (P.degenerate_case(30_000, 9000), P.degenerate_case(140_000, 40_000)):
        for f in case.frames:
            assert 0.2 < P.inverted_share(f) < 0.3, "a quarter of the rows inverted"
            assert 0.2 < float((f[1] == f[2]).mean()) < 0.3, "a quarter zero-length"
    # the sanitised re-index keeps every row (dropped ones as contig -1): 140 000 rows fall into the automatic window
    assert len(P.degenerate_case(140_000, 40_000).frame[0]) >= P.V3_AUTO_FROM
    _references_agree(P.degenerate_case(30_000, 9000), strict, "degenerate_30000")
    # a scaled-down copy of the same recipe inside multi_brute's universe
    small = P.degenerate_case(3000, 3500)
    assert max(int(f[2].max()) for f in small.frames) < M.UNIVERSE
    _references_agree(small, strict, "degenerate_3000", brute=True)

    many = P.many_runs_case()
    runs = P.all_runs(many, strict)
    assert len(many.frames) == 64 and len(runs[0]) > 131_072, len(runs[0])
    assert P.takes_balanced_build((runs[0], runs[1], runs[2]), many.nc), "the run index stays in the balanced build"
    tiny = P.many_runs_case(n_frames=64, runs=25)
    assert max(int(f[2].max()) for f in tiny.frames) < M.UNIVERSE
    for key, k, con in P.multi_keys(tiny):
        M.assert_equal(M.multi_brute(tiny.frames, strict, tiny.nc, k, con), M.multi_events(tiny.frames, strict, tiny.nc, k, con), key)

    for narrow, auto in ((P.narrow_window_case(3, 3000), False), (P.narrow_window_case(64, 2200), True)):
        runs = P.all_runs(narrow, strict)
        span, fullest = P.v3_geometry(runs, narrow.nc)
        assert span <= 0xffffffff and fullest > P.V3_CAP and len(runs[0]) > P.V3_CAP, (span, fullest)
        assert (len(runs[0]) >= P.V3_AUTO_FROM) == auto
        assert all(P.takes_balanced_build(f, narrow.nc) for f in narrow.frames), "the frames themselves do not hand over"


# ---- (1) dictionary sizes ------------------------------------------------------------------------------------------------------------

def _dictionary_checks(eng, case, strict, only=None):
    exp = P.expected_once(case, strict)
    got = P.run(eng, case, strict, only=only)
    assert got, only
    P.check(got, {k: exp[k] for k in got}, case.name)
    P.assert_in_dictionary(got, case.nc, case.name)
    bare, keep = P.without_outside(case)
    P.assert_same(got, P.run(eng, bare, strict, only=only), f"{case.name}: with and without the out-of-dictionary rows", probe_keep=keep)
    for pm in (1, 2):
        other = P.run(eng, case, strict, partition_mode=pm, only=[k for k in ("bases", "summary") if k in got])
        P.check(other, {k: exp[k] for k in other}, f"{case.name}: partition_mode {pm}")
        P.assert_same(other, {k: got[k] for k in other}, f"{case.name}: partition_mode {pm} vs 0")


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("nc", P.SWEEP)
def test_dictionary_sizes(eng, nc, strict):
    _dictionary_checks(eng, P.sweep_case(nc), strict)


# (every index of this dictionary is gigabytes of tables, and multi_inter holds four of them at once: its two modes are cases of
# their own so that each case stays within a few seconds)
SPARSE_CALLS = [("depth", "setop", "set_stats", "bases", "summary"), ("multi:segments",), ("multi:consensus",)]


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("only", SPARSE_CALLS, ids=["one_and_two_frames", "multi_segments", "multi_consensus"])
def test_sparse_dictionary_of_2_24_plus_1_ids(eng, only, strict):
    _dictionary_checks(eng, P.sparse_case(), strict, only=only)


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("nc", [24, 257])
@pytest.mark.parametrize("knob", ["IVJ_COUNT_NOLDS", "IVJ_JOINT_BINS"])
def test_joint_grid_knobs(knob, nc, strict, monkeypatch):
    """the per-contig grid metadata read from global memory, and one bin per row instead of two: overlap_bases and depth_summary
    rank on count_overlaps' joint grid"""
    case = P.sweep_case(nc)
    exp = P.expected_once(case, strict)
    e, done = _engine_under(monkeypatch, {knob: "1"})
    try:
        for pm in (0, 1, 2):
            got = P.run(e, case, strict, partition_mode=pm, only=None if pm == 0 else ("bases", "summary"))
            P.check(got, {k: exp[k] for k in got}, f"{case.name}, {knob}=1, partition_mode {pm}")
    finally:
        done()


# ---- (2) index build forms -----------------------------------------------------------------------------------------------------------

ONE_INDEX = ("depth", "set_stats", "bases") + tuple("setop:" + op for op in SO.OPS)      # calls that build frame indexes only


def _assert_build(names, form, balanced, what):
    """which index build ran, by kernel name.  The calls of ONE_INDEX sort their frames only, so the names are exact; multi_inter
    and depth_summary also sort what they derive (union runs, depth blocks), which may take the other build: for them the name of
    the frames' build must be present."""
    v3 = form.get("IVJ_IX_V3") == "1"
    for key, t in names.items():
        local, final = "ix3_local" in t, "ix_final" in t
        if not v3:
            assert final and not local, (what, key, t)
        elif key in ONE_INDEX:
            assert local == balanced and final != balanced, (what, key, t)
        else:
            assert (local if balanced else final), (what, key, t)


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("entry", V3, ids=V3_IDS)
def test_index_build_forms(entry, strict, monkeypatch):
    case, balanced = P.v3_case(entry), entry[4]
    exp = P.expected(case, strict)
    blobs = []
    for form in P.FORMS:
        e, done = _engine_under(monkeypatch, form)
        try:
            e.enable_timing(2)
            names = {}
            got = P.run(e, case, strict, names=names)
            P.check(got, exp, f"{case.name} under {form}")
            _assert_build(names, form, balanced, f"{case.name} under {form}")
            blobs.append(P.blob(got))
        finally:
            done()
    assert all(b == blobs[0] for b in blobs), "byte-identical results under every index build form"


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_automatic_balanced_build_at_140k_rows(strict):
    """no knob: 140 000 rows on 24 contigs take the balanced build by the automatic rule, in every one of the five ops"""
    case = P.auto_case()
    e = _engine.Engine(0)
    try:
        e.enable_timing(2)
        names = {}
        got = P.run(e, case, strict, names=names)
        for key, t in names.items():
            assert "ix3_local" in t, (key, t)
            assert key not in ONE_INDEX or "ix_final" not in t, (key, t)
        P.check(got, P.expected_once(case, strict), case.name)
    finally:
        e.close()


# ---- (3) the operations' own indexes under the balanced build ------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("n,span,env", [(30_000, 9000, {"IVJ_IX_V3": "1"}), (140_000, 40_000, {})], ids=["forced_30k", "automatic_140k"])
def test_sanitised_reindex_under_the_balanced_build(n, span, env, strict, monkeypatch):
    """frames with a quarter of inverted rows: depth_core indexes them again without the rows that cover nothing (sweep only + end
    order, dropped rows as contig -1), and that index takes the balanced build too"""
    case = P.degenerate_case(n, span)
    e, done = _engine_under(monkeypatch, env)
    try:
        e.enable_timing(2)
        names = {}
        got = P.run(e, case, strict, names=names)
        for key, t in names.items():
            # (overlap_bases reads the index's prefix sums, not its depth blocks: it never takes the re-index)
            assert "ix3_local" in t and (key == "bases" or "depth_sanitize" in t), (key, t)
            assert key not in ONE_INDEX or "ix_final" not in t, (key, t)
        P.check(got, P.expected_once(case, strict), case.name)
    finally:
        done()


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_run_index_of_64_frames_takes_the_balanced_build(strict):
    """64 frames x 2200 runs: the frames are small (the LSD sort), their ~ 140 000 union runs together are not -- multi_core's one
    index over all runs takes the balanced build by the automatic rule"""
    case = P.many_runs_case()
    e = _engine.Engine(0)
    try:
        e.enable_timing(2)
        names = {}
        got = P.run(e, case, strict, names=names, only=("multi",))
        for key, t in names.items():
            assert "ix3_local" in t and "ix_final" in t and "multi_count" in t, (key, t)
        P.check(got, P.expected(case, strict, only=("multi",)), case.name)
        P.assert_in_dictionary(got, case.nc, case.name)
    finally:
        e.close()


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("frames,runs,env", [(3, 3000, {"IVJ_IX_V3": "1"}), (64, 2200, {})], ids=["forced_3x3000", "automatic_64x2200"])
def test_run_index_in_one_narrow_window_hands_over(frames, runs, env, strict, monkeypatch):
    """every run inside one bucket of the balanced build: the run index starts as a balanced build (ix3_pass) and is handed to the
    LSD sort (ix_final).  Forced: the frames themselves take the balanced build, so ix_final can only be the run index's.
    Automatic: the frames are small, so ix3_pass can only be the run index's, and no ix3_local follows it."""
    case = P.narrow_window_case(frames, runs)
    e, done = _engine_under(monkeypatch, env)
    try:
        e.enable_timing(2)
        names = {}
        got = P.run(e, case, strict, names=names, only=("multi",))
        first = True
        for key, t in names.items():
            if env:
                assert "ix3_local" in t and "ix3_pass" in t and "ix_final" in t, (key, t)
            elif first:
                # (after two hand-overs in a row a context leaves the balanced build out for a while: only the first calls try it)
                assert "ix3_pass" in t and "ix3_local" not in t and "ix_final" in t, (key, t)
            first = False
        P.check(got, P.expected(case, strict, only=("multi",)), case.name)
    finally:
        done()


# ---- (4) one index, many calls; one context, changing sizes --------------------------------------------------------------------------

CALLS = ("count", "bases", "summary", "depth", "coverage", "nearest")
ORDERS = [("summary", "count", "bases", "depth", "coverage", "nearest"),
          ("summary", "nearest", "coverage", "depth", "bases", "count"),
          ("depth", "bases", "nearest", "count", "coverage", "summary"),
          ("nearest", "coverage", "count", "bases", "depth", "summary"),
          ("bases", "summary", "depth", "summary", "count", "nearest", "coverage", "bases")]

_sequence_expected = {}


def _sequence_reference(strict):
    if strict not in _sequence_expected:
        case = P.sequence_case()
        ps, bs = O.Side(*case.probe), O.Side(*case.frame)
        ox = O.Index(bs, case.nc)
        exp = P.expected(case, strict, only=("depth", "bases", "summary"))
        exp["count"] = O.count_overlaps_fast(ox, ps, strict)
        exp["coverage"] = O.np_coverage_fast(ps, bs, strict)
        exp["nearest"] = O.nearest_fast(ox, ps, strict, 3, True)
        _sequence_expected[strict] = exp
    return _sequence_expected[strict]


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("order", ORDERS, ids=["-".join(o) for o in ORDERS])
def test_calls_on_one_index_in_any_order(dj, order, strict):
    """one DeviceIndex built without the end order; the end order, the position sums of overlap_bases, the start tables and the
    nearest records are completed on it by whichever call needs them first, and depth_summary builds and releases its own
    structures between them: every result equals the reference whatever ran before it"""
    import torch
    from polars_bio_amd.device_api import DeviceSide
    case, exp = P.sequence_case(), _sequence_reference(strict)
    nc, n = case.nc, len(case.probe[0])
    t = lambda a: torch.from_numpy(np.array(a, np.int32)).cuda()                      # noqa: E731
    probe, frame = DeviceSide(*(t(a) for a in case.probe)), DeviceSide(*(t(a) for a in case.frame))
    opts = _engine.make_opts(strict, nc)
    ix = dj.engine.index_build_dev(frame.as_c(), opts, False)
    try:
        for step, call in enumerate(order):
            what = f"step {step} ({call}) of {order}"
            if call == "count":
                got = dj.count_overlaps(probe, frame, strict, nc, index=ix).cpu().numpy()
                assert (got == exp["count"]).all(), what
            elif call == "bases":
                out = torch.full((n,), -7, dtype=torch.int64, device="cuda")
                dj.overlap_bases(probe, frame, strict, nc, index=ix, out=out)
                DS.assert_bases_equal(out.cpu().numpy(), exp["bases"], what)
            elif call == "summary":
                md, bg = dj.depth_summary(probe, frame, strict, nc, P.THRESHOLDS, index=ix)
                DQ.assert_summary_equal((md.cpu().numpy(), bg.cpu().numpy()), exp["summary"], what)
            elif call == "depth":
                nb = len(exp["depth"][0])
                out = tuple(torch.full((nb,), -7, dtype=torch.int32, device="cuda") for _ in range(4))
                total, fits = dj.engine.depth_dev(ix, opts, nb, *(o.data_ptr() for o in out))
                assert (total, fits) == (nb, True), what
                U.assert_blocks_equal([o.cpu().numpy() for o in out], exp["depth"], what)
            elif call == "coverage":
                got = dj.coverage(probe, frame, strict, nc, index=ix).cpu().numpy()
                assert (got == exp["coverage"]).all(), what
            else:
                i, d, f = (x.cpu().numpy() for x in dj.nearest(probe, frame, strict, nc, k=3, index=ix))
                ei, ed, en = exp["nearest"]
                assert (f == en).all() and (d == ed).all() and (i == ei).all(), what
    finally:
        ix.close()


# (the call, large or small input, mode): every one of the five ops at both sizes, large and small inputs in turn
ALTERNATION = [("depth", True, True), ("summary", False, False), ("setop", True, False), ("multi", False, True), ("bases", True, True),
               ("depth", False, False), ("summary", True, True), ("set_stats", False, True), ("multi", True, False), ("bases", False, False),
               ("setop", False, True), ("set_stats", True, False), ("summary", False, True), ("depth", True, False), ("multi", False, False)]


@gpu
def test_one_context_under_alternating_large_and_small_inputs():
    """150 000 and 300 rows in turn on ONE engine: the recycled index slab and the arena are larger than the next call needs, and
    only the slab's small head is zeroed again.  Every result equals the reference and what a fresh engine returns."""
    e = _engine.Engine(0)
    try:
        for step, (op, large, strict) in enumerate(ALTERNATION):
            case = P.sized_case(150_000 if large else 300, 900 + step % 4)
            what = f"step {step}: {op} on {case.name}, strict={strict}"
            got = P.run(e, case, strict, only=(op,))
            P.check(got, P.expected(case, strict, only=(op,)), what)
            fresh = _engine.Engine(0)
            try:
                P.assert_same(got, P.run(fresh, case, strict, only=(op,)), what + " vs a fresh engine")
            finally:
                fresh.close()
    finally:
        e.close()
