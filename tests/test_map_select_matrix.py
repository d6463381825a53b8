"""map_overlaps (k_oagg_gather / k_overlap_agg) and the semi / anti / left outer join kinds (k_select_count / k_select_emit) put through
the project's cross-cutting matrices, which their own modules -- each built around its kernel's tile, wavefront and chunk -- leave out:

  (A) the bucketed probe path (partition_mode 1, 5, 6 against 0 and 2, which path ran pinned by kernel name), a probe side with
      row_id, an index built from a build side with a permuted row_id and ids outside [0, n), columns that are not 16-byte aligned;
  (B) contig-dictionary sizes on both sides of every layout threshold with every out-of-dictionary id planted on both sides, the
      IVJ_COUNT_NOLDS / IVJ_JOINT_BINS table forms, a sparse dictionary of 2^24 + 1 ids;
  (C) the index build forms, pinned by kernel name, results byte-identical between forms; the automatic balanced build at 140 000
      rows and the hand-over at automatic size -- both with 40 tiles of probes;
  (D) call sequences: one long-lived index under seven calls in six orders, a pending count -> fill hand-over across one
      overlap_agg_dev / overlap_select_dev call, one context under alternating large and small inputs;
  (E) rows at INT32_MIN / INT32_MAX;
  (CPU) the fast references of _map_select_util equal the literal ones on scaled-down copies of every generator, the comparisons
      are not blind, and the generators have the properties the GPU tests rely on.

Which path buckets: map_overlaps and every thresholded call bucket the probes under partition_mode 1, 5 and 6.  The PLAIN semi /
anti selection takes its counts from count_overlaps' int32 form, which never buckets (host_join.hip.h, count_overlaps_dev); the
plain outer join's inner part is the plain join's own count -> fill pair, which buckets under 1 and 5 and takes the
contig-aligned slice path, with a scatter of its own, under 6.  All of it is pinned by kernel name as it is.

One condition of the generators is waived for one input: "a candidate run longer than one wavefront" cannot hold for the one-row
shape of _v3_cases(), whose build side is a single row and which C1 has to run like every other shape.  Every other input meets
it; those whose contigs hold a few rows each get one run of 130 build rows under one probe written in (_map_select_util.with_run).

Every comparison is bit-exact and no tolerance appears anywhere."""
import numpy as np
import pytest

import _join_kinds_util as K
import _join_ops_util as J
import _limits
import _map_select_util as S
import _overlap_agg_util as A
import _position_ops_util as P
import _thresholds_util as T
import test_join_ops_matrix as X
from oracle import oracle as O
from polars_bio_amd import _engine
from test_contig_dictionaries import OUTSIDE
from test_coordinate_limits import NC as LIMIT_NC, _small as _limit_small
from test_join_ops_matrix import _engines_under, _names_of, _assert_build

gpu = pytest.mark.gpu
MODES = X.MODES
V3, V3_IDS = X.V3, X.V3_IDS
TILE = J.TILE
WAVE = 64
PRED = [pytest.param(False, id="plain"), pytest.param(True, id="thresh")]
MASKS = [["sum"], ["min", "max", "count"], ["mean", "count"]]          # D3: three columns with different op masks


@pytest.fixture(scope="module")
def eng():
    return _engine.Engine(0)


@pytest.fixture(scope="module")
def dj():
    import torch  # noqa: F401
    from polars_bio_amd.device_api import DeviceJoin
    return DeviceJoin(0)


def _limit_embed():
    """E: 600 + 600 limit rows written over rows of partition_sides() at random positions, on its first two contigs (spread over
    all 24 the rows long enough for min_overlap 2^31 + 1 meet in fewer than 100 pairs)"""
    def build():
        rng = np.random.default_rng(5100)
        probe, frame, _ = J.partition_sides()
        return (_limits.embed(probe, _limits.limit_rows(rng, 600, 2), rng),
                _limits.embed(frame, _limits.limit_rows(rng, 600, 2), rng))
    return J._once(("limit_embed",), build)


LIMIT_THR = dict(min_overlap=2)                              # E: the threshold set the limit inputs are also run under
LIMIT_LONGEST = dict(min_overlap=(1 << 31) + 1)               # ... and the one only rows longer than half of int32 can meet
LIMIT_CASES = ["small", "small_inverted", "embedded"]


def _limit_case(case):
    """E -> (probe, build, n_contigs)"""
    if case == "embedded":
        return (*_limit_embed(), 24)
    return (*_limit_small(0, case == "small_inverted"), LIMIT_NC)


_gpu_inputs_cache = {}


def _gpu_inputs():
    """name -> (probe, build, n_contigs, threshold set): exactly the inputs the GPU tests run, under the names their references
    are shared by (built once)"""
    out = _gpu_inputs_cache
    if out:
        return out
    probe, build, thr = J.partition_sides()
    out["partition"] = (probe, build, 24, J.THR)
    out["partition_never"] = (probe, build, 24, thr)
    for n in (TILE - 1, TILE + 1, 2 * TILE + 3):
        p, b, _ = J.partition_sides(n_probe=n)
        out[f"partition_{n}"] = (p, b, 24, J.THR)
    for nc in P.SWEEP + [24]:
        out[f"sweep_{nc}"] = (*S.sweep_sides(nc), nc, J.THR)
    out["sparse"] = (*S.sparse_sides(), P.SPARSE_NC, J.THR)
    for entry, vid in zip(V3, V3_IDS):
        probe, build, nc = S.v3_sides(entry)
        out["v3_" + vid] = (probe, build, nc, J.THR)
    out["auto"] = (*S.auto_sides(), J.THR)
    out["handover"] = (*S.handover_sides(), J.THR)
    out["sequence"] = (*J.sequence_sides(), J.THR)
    for n, seed, _ in J.D3_ROUNDS:
        out[f"sized_{n}_{seed}"] = (*S.sized_sides(n, seed), J.THR)
    for case in LIMIT_CASES:
        out["limits_" + case] = (*_limit_case(case), LIMIT_THR)
    return out


_a3_cache = {}


def _a3_sets(strict):
    """A3: (name, threshold set as the reference sees it -- build_min by POSITION --, build_min as the caller gives it -- by id --
    or None, the reference), over partition_sides() with J.build_ids (built once)"""
    if strict in _a3_cache:
        return _a3_cache[strict]
    probe, build, never = J.partition_sides()
    nb = len(build[0])
    bid, _ = J.build_ids(nb)
    inside = (bid >= 0) & (bid < nb)
    by_id = J.never_mix(np.random.default_rng(9), nb)                     # entry i belongs to id i
    by_position = np.where(inside, by_id[np.where(inside, bid, 0)], J.NEVER).astype(np.uint32)
    sets = [("plain", None, None),
            ("min_overlap", dict(min_overlap=2, probe_min=never["probe_min"]), None),
            ("build_min", dict(min_overlap=2, probe_min=never["probe_min"], build_min=by_position), by_id)]
    _a3_cache[strict] = [(what, thr, given, S.reference_once("partition_ids_" + what, probe, build, 24, strict, thr)) for what, thr, given in sets]
    return _a3_cache[strict]


def _ref(name, strict, thresholded):
    probe, build, nc, thr = _gpu_inputs()[name]
    return S.reference_once(name, probe, build, nc, strict, thr if thresholded else None)


# ---- (CPU) the fast references equal the literal ones; the comparisons see; the generators' properties -----------------------------------

def _scaled_inputs():
    """name -> (probe, build, n_contigs): scaled-down copies of every generator the GPU tests use"""
    out = {name: v[:3] for name, v in X._scaled_inputs().items()}
    # ... and with the long run written in, as the GPU tests run them: every scaled copy that is large enough for it
    for name, (probe, build, nc) in list(out.items()):
        if name.startswith(("sweep", "sparse", "v3", "auto", "sized")) and len(build[0]) >= 2 * S.RUN:
            out[name + "_run"] = (*S.with_run(("scaled", name), probe, build, nc), nc)
    out["handover_run"] = S.handover_sides(n=3000, n_probe=500)
    probe, build = _limit_small(0, True)
    out["limits"] = (probe, build, LIMIT_NC)
    rng = np.random.default_rng(5101)
    probe, build, _ = J.partition_sides(n_probe=600, n_build=500)
    out["limit_embed"] = (_limits.embed(probe, _limits.limit_rows(rng, 100, 24, outside=True), rng),
                          _limits.embed(build, _limits.limit_rows(rng, 100, 24), rng), 24)
    return out


@pytest.mark.parametrize("strict", MODES)
def test_cpu_fast_references_equal_the_literal_ones(strict):
    seen = dict(outside=0, degenerate_matches=0, never=0, no_valid=0, anti=0, semi=0)
    for name, (probe, build, nc) in _scaled_inputs().items():
        n, m = len(probe[0]), len(build[0])
        rng = np.random.default_rng(len(name))
        never = dict(min_overlap=2, probe_min=J.never_mix(rng, n), build_min=J.never_mix(rng, m))
        columns = J.agg_columns(m, len(name))
        for thr in (None, J.THR, never):
            ref = S.reference(probe, build, nc, strict, thr)
            lit = K.expected(probe, build, nc, strict, **(thr or {}))
            exp = S.select_expected(ref, n)
            for key in ("cnt", "semi", "anti"):
                assert exp[key].dtype == lit[key].dtype and exp[key].shape == lit[key].shape and (exp[key] == lit[key]).all(), (name, thr, key)
            for key in ("inner", "left"):
                for k in range(2):
                    assert len(exp[key][k]) == len(lit[key][k]) and (exp[key][k] == lit[key][k]).all(), (name, thr, key, k)
            p, b = A.pairs(probe, build, nc, strict, **(thr or {}))
            fast = S.map_expected(ref, n, columns)
            for j, (v, valid, _) in enumerate(columns):
                J.assert_lists_equal(J.as_lists(fast[j]), A.group_by(p, b, n, v, valid), v.dtype, (name, thr, j))
                seen["no_valid"] += int((~fast[j]["has"]).sum())
            seen["semi"] += len(exp["semi"])
            seen["anti"] += len(exp["anti"])
            if thr is None:                                 # rows that cover no position match under the plain predicate
                none = (probe[2] < probe[1]) | ((probe[2] == probe[1]) & strict)
                seen["degenerate_matches"] += int(exp["cnt"][none].sum())
        for side in (probe, build):
            seen["outside"] += int((~P.inside(side, nc)).sum())
        seen["never"] += int((never["probe_min"] == J.NEVER).sum())
    assert all(v > 50 for v in seen.values()), seen


def _hand_made():
    probe = (np.zeros(5, np.int32), np.array([0, 10, 100, 20, 300], np.int32), np.array([5, 30, 110, 25, 310], np.int32))
    build = (np.zeros(4, np.int32), np.array([1, 12, 22, 24], np.int32), np.array([4, 26, 40, 28], np.int32))
    ref = S.reference(probe, build, 1, True)
    assert ref[2].tolist() == [1, 3, 0, 3, 0]
    return probe, build, ref


def test_cpu_the_comparisons_are_not_blind():
    probe, build, ref = _hand_made()
    v = np.array([1.0, 2.0, 4.0, 8.0])
    columns = [(v, np.array([1, 1, 1, 0], bool), J.ALL)]
    exp = S.map_expected(ref, 5, columns)
    assert exp[0]["count"].tolist() == [1, 2, 0, 2, 0] and exp[0]["sum"].tolist() == [1.0, 6.0, 0.0, 6.0, 0.0] and exp[0]["max"][1] == 4.0
    good = {op: exp[0][op].copy() for op in J.ALL}
    good["min"][2] = 99.0                                    # unspecified: skipped
    S.map_check({"host": [good]}, exp, columns, "")
    for op, k, x in (("sum", 2, 1.0), ("min", 0, 2.0), ("mean", 1, 2.0), ("count", 4, 1), ("sum", 3, 14.0)):
        bad = {o: good[o].copy() for o in J.ALL}
        bad[op][k] = x
        with pytest.raises(AssertionError):
            S.map_check({"host": [bad]}, exp, columns, "")
    # build row ids: the value of a row is values[id]; ids outside [0, n_values) carry nothing
    ids = np.array([3, 0, -1, 7], np.int32)
    by_id = S.map_expected(ref, 5, [(v, None, J.ALL)], build_row_id=ids)[0]
    assert by_id["count"].tolist() == [1, 1, 0, 1, 0] and by_id["sum"].tolist() == [8.0, 1.0, 0.0, 1.0, 0.0]

    sel = S.select_expected(ref, 5)
    assert sel["semi"].tolist() == [0, 1, 3] and sel["anti"].tolist() == [2, 4]
    outer = (np.concatenate([ref[0], sel["anti"]]).astype(np.int32), np.concatenate([ref[1], [-1, -1]]).astype(np.int32))
    ok = {"host_semi": sel["semi"], "host_anti": sel["anti"], "dev_semi": sel["semi"], "dev_anti": sel["anti"], "host_outer": outer}
    S.select_check(ok, sel, build, "")
    rid = np.array([50, 40, 30, 20, 10], np.int32)
    S.select_check({"dev_semi": rid[sel["semi"]], "dev_anti": rid[sel["anti"]]}, sel, build, "", probe_row_id=rid)
    with pytest.raises(AssertionError):                      # positions where ids belong
        S.select_check({"dev_semi": sel["semi"]}, sel, build, "", probe_row_id=rid)
    with pytest.raises(AssertionError):                      # one semi row missing
        S.select_check(dict(ok, host_semi=sel["semi"][:-1]), sel, build, "")
    with pytest.raises(AssertionError):                      # an anti row among the semi rows
        S.select_check(dict(ok, dev_semi=np.array([0, 1, 2, 3], np.int32)), sel, build, "")
    moved = (outer[0].copy(), outer[1].copy())               # one -1 of the tail misplaced: it swaps places with an inner pair
    k = len(ref[0]) - 1
    for a in moved:
        a[k], a[k + 1] = a[k + 1], a[k]
    with pytest.raises(AssertionError):
        S.select_check(dict(ok, host_outer=moved), sel, build, "")
    swapped = (outer[0].copy(), outer[1].copy())             # the tail out of ascending order
    swapped[0][-2:] = swapped[0][-2:][::-1]
    with pytest.raises(AssertionError):
        S.select_check(dict(ok, host_outer=swapped), sel, build, "")
    assert S.select_blob(ok) != S.select_blob(dict(ok, host_outer=swapped)) and S.map_blob({"host": [good]}) == S.map_blob({"host": [{op: exp[0][op] for op in J.ALL}]})


@pytest.mark.parametrize("strict", MODES)
def test_cpu_generator_properties(strict):
    """what the GPU tests rely on, asserted on the very inputs they run: both semi and anti rows, more than 100 matched pairs, a
    probe whose candidate run is longer than one wavefront (it MATCHES more than 64 rows: its run is at least that long), a pair
    that the threshold set removes -- under both predicates where they apply; outside ids, row ids and tile counts where the
    tests say so"""
    for name, (probe, build, nc, thr) in _gpu_inputs().items():
        n = len(probe[0])
        plain, kept = _ref(name, strict, False), _ref(name, strict, True)
        for what, ref in (("plain", plain), ("thresholded", kept)):
            assert 0 < (ref[2] > 0).sum() < n, f"{name} {what}: semi and anti rows"
            assert len(ref[0]) > 100, f"{name} {what}: {len(ref[0])} pairs"
        assert len(kept[0]) < len(plain[0]), f"{name}: the threshold set removes no pair"
        if len(build[0]) == 1:                               # the one-row shape: one candidate at most; the only exception
            assert name == "v3_one_row"
        else:
            # (the candidates of a probe are the same rows under either predicate: the thresholds only reject more of them)
            assert plain[2].max() > WAVE, f"{name}: no candidate run longer than a wavefront ({plain[2].max()})"

    probe, build, thr = J.partition_sides()
    assert len(probe[0]) == 3 * TILE + 17
    rid = J.probe_ids(len(probe[0]))
    assert len(np.unique(rid)) == len(rid) and rid.min() > len(rid)
    bid, moved = J.build_ids(len(build[0]))
    nb = len(build[0])
    assert len(np.unique(bid)) == nb and ((bid < 0) | (bid >= nb)).sum() == 6 == len(moved) and (bid != np.arange(nb)).mean() > 0.99
    for thresholded in (False, True):                        # the rows with outside ids overlap probes, and so do rows with moved ids
        ref = _ref("partition", strict, thresholded)
        assert np.isin(ref[1], moved).sum() > 0 and (~np.isin(ref[1], moved)).sum() > 100
    n = len(probe[0])
    for what, thr, given, ref in _a3_sets(strict):           # A3's own references: the same conditions, and what each set is there for
        assert 0 < (ref[2] > 0).sum() < n and len(ref[0]) > 100 and (~np.isin(ref[1], moved)).sum() > 100, what
        assert _ref("partition", strict, False)[2].max() > WAVE           # (the same sides: the same candidate runs)
        if given is None:                                    # nothing is looked up by id: rows with outside ids match, and must carry no value
            assert np.isin(ref[1], moved).any(), what
        else:                                                # build_min by id: rows with outside ids never match
            assert not np.isin(ref[1], moved).any() and len(ref[0]) < len(_a3_sets(strict)[1][3][0]), what
    for nc in P.SWEEP:
        probe, build = S.sweep_sides(nc)
        for side in (probe, build):
            assert set(OUTSIDE(nc)) <= set(side[0].tolist()), "every out-of-dictionary id on both sides"
            assert (side[0] == 0).any() and (side[0] == nc - 1).any()
    probe, build = S.sparse_sides()
    assert all(set(OUTSIDE(P.SPARSE_NC)) <= set(s[0].tolist()) for s in (probe, build))
    counts = np.bincount(build[0][P.inside(build, P.SPARSE_NC)], minlength=P.SPARSE_NC)
    assert counts[0] > 0 and counts[P.SPARSE_NC - 1] > 0 and (counts == 1).sum() > 1000
    for entry, vid in zip(V3, V3_IDS):
        probe, build, nc = S.v3_sides(entry)
        assert P.takes_balanced_build(build, nc) == entry[4], vid
    probe, build, nc = S.auto_sides()
    assert len(build[0]) == 140_000 >= P.V3_AUTO_FROM and P.takes_balanced_build(build, nc) and len(probe[0]) > 8 * TILE
    probe, build, nc = S.handover_sides()
    span, fullest = P.v3_geometry(build, nc)
    assert len(build[0]) >= P.V3_AUTO_FROM and span <= 0xffffffff and fullest > P.V3_CAP and len(probe[0]) > 8 * TILE
    assert (len(probe[0]) + TILE - 1) // TILE == 40
    assert [n for n, _, _ in J.D3_ROUNDS] == [150_000, 300, 150_000, 300, 150_000]
    # E (the loop above holds the three inputs under the plain predicate and LIMIT_THR): limit rows among the matches of every
    # input, and the third threshold set keeps some pairs and removes others
    for case in LIMIT_CASES:
        probe, build, nc = _limit_case(case)
        p, b, _ = _ref("limits_" + case, strict, False)
        _limits.assert_touches(p, b, probe, build, strict)
        longest = S.reference_once("limits_" + case, probe, build, nc, strict, LIMIT_LONGEST)
        assert 100 < len(longest[0]) < len(_ref("limits_" + case, strict, True)[0]) and 0 < (longest[2] > 0).sum() < len(probe[0]), case


# ---- (A) partitioning, row ids, alignment --------------------------------------------------------------------------------------------

def _kw(probe, build, strict, thr):
    return S.engine_kw(probe, build, strict, thr)


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("thresholded", PRED)
def test_bucketed_probe_path_against_the_unbucketed_one(thresholded, strict):
    """A1.  partition_mode 1, 5, 6 bucket the probes: k_overlap_agg then reads probe_min[pos] and writes at pos = pt_row of the
    partition; the thresholded selection counts at pos.  The outputs are in input order either way, so which path ran is read from
    the kernel names (part_scatter: the partition of host_join.hip.h)."""
    from polars_bio_amd.device_api import DeviceJoin
    probe, build, _ = J.partition_sides()
    thr = J.THR if thresholded else None
    ref = _ref("partition", strict, thresholded)
    n = len(probe[0])
    columns = J.agg_columns(len(build[0]), 71)
    mexp, sexp = S.map_expected(ref, n, columns), S.select_expected(ref, n)
    kw = _kw(probe, build, strict, thr)
    e, d = _engine.Engine(0), DeviceJoin(0)
    try:
        e.enable_timing(2)
        d.engine.enable_timing(2)
        base = None
        for pm in (0, 1, 2, 5, 6):
            what = f"partition_mode {pm}"
            bucketing = pm in (1, 5, 6)
            got, t = _names_of(e, lambda: S.map_run(e, None, probe, build, 24, strict, columns, kw, partition_mode=pm))
            assert ("part_scatter" in t) == bucketing and "overlap_agg" in t and "overlap_agg_gather" in t, (what, t)
            dev, t = _names_of(d.engine, lambda: S.map_run(None, d, probe, build, 24, strict, columns, kw, partition_mode=pm))
            assert ("part_scatter" in t) == bucketing and "overlap_agg" in t, (what, t)
            got.update(dev)
            S.map_check(got, mexp, columns, what)
            sel = {}
            for mode in ("semi", "anti"):
                sel["host_" + mode], t = _names_of(e, lambda: e.overlap_select(probe, build, strict, 24, mode, partition_mode=pm, **kw))
                # (the plain selection counts with count_overlaps' int32 form, which never buckets)
                assert ("part_scatter" in t) == (bucketing and thresholded) and "select_count" in t and "select_emit" in t, (what, mode, t)
            outer, t = _names_of(e, lambda: e.overlap_outer(probe, build, strict, 24, partition_mode=pm, **kw))
            if thresholded or pm != 6:
                assert ("part_scatter" in t) == bucketing, (what, "outer", t)
            else:                                            # the plain join's count -> fill pair under 6: the contig-aligned slice path and its own scatter
                assert "part_scatter" not in t and any(k.startswith("cs_scatter") for k in t) and "overlap_count" not in t, (what, "outer", t)
            sel["host_outer"] = (np.array(outer[0]), np.array(outer[1]))
            dsel, t = _names_of(d.engine, lambda: S.select_run(None, d, probe, build, 24, strict, kw, partition_mode=pm))
            assert ("part_scatter" in t) == (bucketing and thresholded), (what, "device select", t)
            sel.update(dsel)
            S.select_check(sel, sexp, build, what)
            blobs = (S.map_blob(got), S.select_blob(sel, len(ref[0])))
            base = base or blobs
            assert blobs == base, f"{what}: not byte-identical to partition_mode 0"
    finally:
        e.close()
        d.engine.close()


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("pm", [0, 1, 2])
def test_probe_side_with_row_ids(dj, pm, strict):
    """A2.  the selection reports row_id[position] (all above n_probe: neither can stand in for the other); map_overlaps ignores
    the ids, writes by position and reads probe_min by position"""
    probe, build, never = J.partition_sides()
    n = len(probe[0])
    rid = J.probe_ids(n)
    columns = J.agg_columns(len(build[0]), 72)
    for name, thr in (("partition", None), ("partition", J.THR), ("partition_never", never)):
        ref = S.reference_once(name, probe, build, 24, strict, thr)
        kw = _kw(probe, build, strict, thr)
        what = f"probe row_id, partition_mode {pm}, {'plain' if thr is None else sorted(thr)}"
        sel = S.select_run(None, dj, probe, build, 24, strict, kw, partition_mode=pm, probe_row_id=rid)
        assert all(g.min() > n for g in sel.values()), "the selection reports ids"
        S.select_check(sel, S.select_expected(ref, n), build, what, probe_row_id=rid)
        got = S.map_run(None, dj, probe, build, 24, strict, columns, kw, partition_mode=pm, probe_row_id=rid)
        S.map_check(got, S.map_expected(ref, n, columns), columns, what)


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_index_built_from_a_build_side_with_row_ids(dj, strict):
    """A3.  k_oagg_gather reads values[b_row[p]] and valid[b_row[p]] with b_row = the build side's ids: a permutation far from the
    identity, six ids outside [0, n).  Rows with outside ids contribute to no operation, count included -- with build_min (which
    k_thresh_gather maps to "never" for them) and without.  The selection looks nothing up by id without build_min."""
    probe, build, _ = J.partition_sides()
    n, nb = len(probe[0]), len(build[0])
    bid, moved = J.build_ids(nb)
    columns = J.agg_columns(nb, 73)
    for pm in (0, 1):
        for what, thr, given, ref in _a3_sets(strict):
            kw = _kw(probe, build, strict, thr)
            if given is not None:
                kw = dict(kw, build_min=given)
            exp = S.map_expected(ref, n, columns, build_row_id=bid)
            unaware = S.map_expected(ref, n, columns)
            assert (exp[0]["count"] != unaware[0]["count"]).any() and (exp[1]["sum"] != unaware[1]["sum"]).any()
            got = S.map_run(None, dj, probe, build, 24, strict, columns, kw, partition_mode=pm, build_row_id=bid)
            S.map_check(got, exp, columns, f"build row_id, {what}, partition_mode {pm}")
            sel = S.select_run(None, dj, probe, build, 24, strict, kw, partition_mode=pm, build_row_id=bid)
            S.select_check(sel, S.select_expected(ref, n), build, f"build row_id, {what}, partition_mode {pm}")


@gpu
@pytest.mark.parametrize("n", [TILE - 1, TILE + 1, 2 * TILE + 3])
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_columns_that_are_not_16_byte_aligned(dj, shift, n):
    """A4.  probe columns (and row_id for the selection) as views `shift` elements into larger tensors: vec_ok is false and every
    probe is read by the scalar path, whose tail guard meets the last tile at these sizes; separately the value columns, the
    validity bytes and all five result columns one element into sentinel-filled tensors (8-byte aligned only).  Unbucketed
    (partition_mode 2: the kernels read the caller's columns) and bucketed (the partition reads them)."""
    strict = (shift + n) % 2 == 0
    probe, build, _ = J.partition_sides(n_probe=n)
    rid = J.probe_ids(n)
    columns = J.agg_columns(len(build[0]), 74)
    for thresholded in (False, True):
        thr = J.THR if thresholded else None
        ref = _ref(f"partition_{n}", strict, thresholded)
        mexp, sexp = S.map_expected(ref, n, columns), S.select_expected(ref, n)
        kw = _kw(probe, build, strict, thr)
        for pm in (2, 1):
            what = f"shift {shift}, n {n}, partition_mode {pm}, thresholded {thresholded}"
            aligned = S.map_run(None, dj, probe, build, 24, strict, columns, kw, partition_mode=pm)
            got = S.map_run(None, dj, probe, build, 24, strict, columns, kw, partition_mode=pm, shift=shift)
            S.map_check(got, mexp, columns, what)
            assert S.map_blob(got) == S.map_blob(aligned), what + ": differs from the aligned run"
            off = {"device": S.map_dev_offset(dj, probe, build, 24, strict, columns, kw, partition_mode=pm, shift=shift)}
            S.map_check(off, mexp, columns, what + ", value and result columns 8-byte aligned")
            assert S.map_blob(off) == S.map_blob(aligned), what + ": the offset columns differ from the aligned run"
            for ids in (None, rid):
                aligned = S.select_run(None, dj, probe, build, 24, strict, kw, partition_mode=pm, probe_row_id=ids)
                sel = S.select_run(None, dj, probe, build, 24, strict, kw, partition_mode=pm, probe_row_id=ids, shift=shift)
                S.select_check(sel, sexp, build, what, probe_row_id=ids)
                assert S.select_blob(sel) == S.select_blob(aligned), what + ": the selection differs from the aligned run"


# ---- (B) dictionary sizes --------------------------------------------------------------------------------------------------------------

def _dictionary_checks(eng, dj, probe, build, nc, strict, name):
    n, nb = len(probe[0]), len(build[0])
    in_p, in_b = P.inside(probe, nc), P.inside(build, nc)
    assert (~in_p).sum() >= 10 and (~in_b).sum() >= 10
    columns = J.agg_columns(nb, 75)
    bare_p, bare_b = P.rows(probe, in_p), P.rows(build, in_b)
    bare_columns = [(v[in_b], None if m is None else m[in_b], ops) for v, m, ops in columns]
    for thresholded in (False, True):
        thr = J.THR if thresholded else None
        ref = S.reference_once(name, probe, build, nc, strict, thr)
        assert in_p[ref[0]].all() and in_b[ref[1]].all(), "the reference matches no out-of-dictionary row"
        mexp, sexp = S.map_expected(ref, n, columns), S.select_expected(ref, n)
        kw = _kw(probe, build, strict, thr)
        what = f"{name}, {'thresholded' if thresholded else 'plain'}"
        got = S.map_run(eng, dj, probe, build, nc, strict, columns, kw)
        S.map_check(got, mexp, columns, what)
        sel = S.select_run(eng, dj, probe, build, nc, strict, kw)
        S.select_check(sel, sexp, build, what)
        if not thresholded:
            cnt = eng.count_overlaps(probe, build, strict, nc)
            assert (ref[2] == cnt).all(), f"{what}: the plain reference is count_overlaps"
        outside = np.flatnonzero(~in_p)
        for key, res in got.items():
            for r in res:
                assert not r["count"][~in_p].any() and not r["sum"][~in_p].view(np.uint64).any(), f"{what} {key}: an out-of-dictionary probe with a count or a sum"
        for key in ("host_anti", "dev_anti"):
            assert np.isin(outside, sel[key]).all(), f"{what} {key}: an out-of-dictionary probe is no anti row"
        assert in_b[sel["host_outer"][1][sel["host_outer"][1] >= 0]].all(), f"{what}: an out-of-dictionary build row in the outer join"
        # ... the same call without the out-of-dictionary rows, re-indexed
        bkw = _kw(bare_p, bare_b, strict, thr)
        bare = S.map_run(eng, dj, bare_p, bare_b, nc, strict, bare_columns, bkw)
        cut = {key: [{op: a[in_p] for op, a in r.items()} for r in res] for key, res in got.items()}
        assert S.map_blob(cut) == S.map_blob(bare), f"{what}: map_overlaps differs without the out-of-dictionary rows"
        bsel = S.select_run(eng, dj, bare_p, bare_b, nc, strict, bkw)
        new_p = (np.cumsum(in_p) - 1).astype(np.int32)
        new_b = np.concatenate([np.cumsum(in_b) - 1, [-1]]).astype(np.int32)        # (-1 stays -1)
        for key, g in sel.items():
            if key.endswith("outer"):
                keep = in_p[g[0]]
                want = {key: (new_p[g[0][keep]], new_b[g[1][keep]])}
            else:
                want = {key: new_p[g[in_p[g]]]}
            k = int(in_p[ref[0]].sum())
            assert S.select_blob(want, k) == S.select_blob({key: bsel[key]}, k), f"{what} {key}: differs without the out-of-dictionary rows"
        for pm in (1, 2):
            other = S.map_run(eng, dj, probe, build, nc, strict, columns, kw, partition_mode=pm)
            assert S.map_blob(other) == S.map_blob(got), f"{what}: map_overlaps under partition_mode {pm} differs from 0"
            osel = S.select_run(eng, dj, probe, build, nc, strict, kw, partition_mode=pm)
            S.select_check(osel, sexp, build, f"{what}, partition_mode {pm}")
            assert S.select_blob(osel, len(ref[0])) == S.select_blob(sel, len(ref[0])), f"{what}: the selection under partition_mode {pm} differs from 0"


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("nc", P.SWEEP)
def test_across_dictionary_sizes(eng, dj, nc, strict):
    """B1.  k_overlap_agg sits on flat_range and build_flat: exactly the tables the dictionary size lays out differently"""
    probe, build = S.sweep_sides(nc)
    _dictionary_checks(eng, dj, probe, build, nc, strict, f"sweep_{nc}")


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("nc", [24, 257])
@pytest.mark.parametrize("knob", ["IVJ_COUNT_NOLDS", "IVJ_JOINT_BINS"])
def test_under_the_table_knobs(knob, nc, strict, monkeypatch):
    """B2.  the per-contig grid metadata read from global memory, and one bin per row instead of two"""
    probe, build = S.sweep_sides(nc)
    e, d, done = _engines_under(monkeypatch, {knob: "1"})
    try:
        _dictionary_checks(e, d, probe, build, nc, strict, f"sweep_{nc}")
    finally:
        done()


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_on_a_sparse_dictionary_of_2_24_plus_1_ids(eng, dj, strict):
    """B3"""
    probe, build = S.sparse_sides()
    nc = P.SPARSE_NC
    n = len(probe[0])
    columns = J.agg_columns(len(build[0]), 76)
    for thresholded in (False, True):
        thr = J.THR if thresholded else None
        ref = _ref("sparse", strict, thresholded)
        mexp, sexp = S.map_expected(ref, n, columns), S.select_expected(ref, n)
        kw = _kw(probe, build, strict, thr)
        base = None
        for pm in (0, 1):
            what = f"sparse, thresholded {thresholded}, partition_mode {pm}"
            got = S.map_run(eng, dj, probe, build, nc, strict, columns, kw, partition_mode=pm)
            S.map_check(got, mexp, columns, what)
            sel = S.select_run(eng, dj, probe, build, nc, strict, kw, partition_mode=pm)
            S.select_check(sel, sexp, build, what)
            blobs = (S.map_blob(got), S.select_blob(sel, len(ref[0])))
            base = base or blobs
            assert blobs == base, what + ": differs from partition_mode 0"


# ---- (C) index build forms -------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("entry", V3, ids=V3_IDS)
def test_index_build_forms(entry, strict, monkeypatch):
    """C1.  k_oagg_gather reads b_row, k_overlap_agg rec4 and the flat tables (and, build_min being given, the minima gathered
    along b_row) as the build form left them.  Equal starts keep their input order under every form and every fold has one fixed
    shape given the sorted order, so the results are byte-identical between forms."""
    probe, build, nc = S.v3_sides(entry)
    vid = V3_IDS[[e[0] for e in V3].index(entry[0])]
    n = len(probe[0])
    kw = _kw(probe, build, strict, J.THR)
    assert kw["build_min"] is not None
    columns = J.agg_columns(len(build[0]), 77)
    ref = _ref("v3_" + vid, strict, True)
    mexp, sexp = S.map_expected(ref, n, columns), S.select_expected(ref, n)
    pref = _ref("v3_" + vid, strict, False)
    pexp = S.select_expected(pref, n)
    blobs = []
    for form in P.FORMS:
        e, d, done = _engines_under(monkeypatch, form)
        try:
            e.enable_timing(2)
            what = f"v3 {vid} under {form}"
            got, t = _names_of(e, lambda: S.map_run(e, None, probe, build, nc, strict, columns, kw))
            assert "overlap_agg" in t and "overlap_agg_gather" in t and "thresh_gather" in t, (what, t)
            _assert_build(t, form, entry[4], what)
            semi, t = _names_of(e, lambda: e.overlap_select(probe, build, strict, nc, "semi", **kw))
            assert "select_count" in t and "select_emit" in t, (what, t)
            _assert_build(t, form, entry[4], what)
            got.update(S.map_run(None, d, probe, build, nc, strict, columns, kw))
            S.map_check(got, mexp, columns, what)
            sel = S.select_run(e, d, probe, build, nc, strict, kw)
            assert sel["host_semi"].tobytes() == semi.tobytes()
            S.select_check(sel, sexp, build, what)
            plain = S.select_run(e, d, probe, build, nc, strict, dict(S.PLAIN))
            S.select_check(plain, pexp, build, what + ", plain")
            blobs.append((S.map_blob(got), S.select_blob(sel, len(ref[0])), S.select_blob(plain, len(pref[0]))))
        finally:
            done()
    assert all(b == blobs[0] for b in blobs), "byte-identical results under every index build form"


def _large_build_checks(e, d, probe, build, nc, strict, name):
    n = len(probe[0])
    assert (n + TILE - 1) // TILE > 8, "more than eight tiles of probes"
    columns = J.agg_columns(len(build[0]), 78)
    for thresholded in (False, True):
        thr = J.THR if thresholded else None
        ref = _ref(name, strict, thresholded)
        kw = _kw(probe, build, strict, thr)
        what = f"{name}, thresholded {thresholded}"
        got = S.map_run(e, d, probe, build, nc, strict, columns, kw)
        S.map_check(got, S.map_expected(ref, n, columns), columns, what)
        sel = S.select_run(e, d, probe, build, nc, strict, kw)
        S.select_check(sel, S.select_expected(ref, n), build, what)


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_automatic_balanced_build_at_140k_rows(strict):
    """C2.  no knob: 140 000 build rows on 24 contigs take the balanced build by the automatic rule; 20 000 probes are 40 tiles
    (the grid is 8 * ceil(tiles / 8) with xcd_tile64)"""
    from polars_bio_amd.device_api import DeviceJoin
    probe, build, nc = S.auto_sides()
    e, d = _engine.Engine(0), DeviceJoin(0)
    try:
        e.enable_timing(2)
        columns = J.agg_columns(len(build[0]), 78)
        _, t = _names_of(e, lambda: S.map_run(e, None, probe, build, nc, strict, columns, dict(S.PLAIN)))
        assert "ix3_local" in t and "ix_final" not in t and "overlap_agg" in t, t
        _large_build_checks(e, d, probe, build, nc, strict, "auto")
    finally:
        e.close()
        d.engine.close()


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_hand_over_to_the_lsd_sort_at_automatic_size(strict):
    """C3.  140 000 rows in one narrow window: the balanced build starts by the automatic rule, finds one bucket above its
    capacity and hands the index to the LSD sort.  Nearly all build rows lie in one window of 140 000 positions, so the candidate
    runs of a tile of probes span many chunks.  (The names are asserted on the first call of a fresh engine only.)"""
    from polars_bio_amd.device_api import DeviceJoin
    probe, build, nc = S.handover_sides()
    e, d = _engine.Engine(0), DeviceJoin(0)
    try:
        e.enable_timing(2)
        columns = J.agg_columns(len(build[0]), 78)
        _, t = _names_of(e, lambda: S.map_run(e, None, probe, build, nc, strict, columns, dict(S.PLAIN)))
        assert "ix3_pass" in t and "ix3_local" not in t and "ix_final" in t and "overlap_agg" in t, t
        _large_build_checks(e, d, probe, build, nc, strict, "handover")
    finally:
        e.close()
        d.engine.close()


# ---- (D) call sequences ----------------------------------------------------------------------------------------------------------------

CALLS = ("map_plain", "map_thresh_bucketed", "semi_plain_bucketed", "anti_thresh", "thresh_pairs_bucketed", "count_bucketed", "bases_bucketed")
ORDERS = [CALLS,
          CALLS[::-1],
          ("thresh_pairs_bucketed", "map_plain", "bases_bucketed", "anti_thresh", "count_bucketed", "map_thresh_bucketed", "semi_plain_bucketed"),
          ("semi_plain_bucketed", "count_bucketed", "map_thresh_bucketed", "thresh_pairs_bucketed", "map_plain", "bases_bucketed", "anti_thresh"),
          ("anti_thresh", "map_thresh_bucketed", "bases_bucketed", "map_plain", "semi_plain_bucketed", "thresh_pairs_bucketed", "count_bucketed"),
          ("bases_bucketed", "semi_plain_bucketed", "anti_thresh", "count_bucketed", "map_plain", "thresh_pairs_bucketed", "map_thresh_bucketed")]


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_calls_on_one_index_in_any_order(dj, strict):
    """D1.  one long-lived DeviceIndex of 50 000 rows.  map_overlaps buckets the probes into the context's pt_* columns and takes
    arena scratch that it reuses column after column; the bucketed count, overlap_bases and the thresholded join rewrite pt_* and
    the arena between the calls; the flat tables are built on the index by whichever call needs them first."""
    import torch
    import _depth_sum_util as DS
    probe, build, nc = J.sequence_sides()
    n = len(probe[0])
    columns = J.agg_columns(len(build[0]), 79)
    kw = _kw(probe, build, strict, J.THR)
    dkw = S.dev_kw(kw)
    plain, kept = _ref("sequence", strict, False), _ref("sequence", strict, True)
    mplain, mkept = S.map_expected(plain, n, columns), S.map_expected(kept, n, columns)
    splain, skept = S.select_expected(plain, n), S.select_expected(kept, n)
    bases = DS.prefix_form(probe, build, strict, nc)
    dp, db = J.dev_side(probe), J.dev_side(build)
    agg = S.dev_agg(columns)
    first = None
    for order in ORDERS:
        assert sorted(order) == sorted(CALLS)
        ix = dj.build_index(db, strict, nc)
        results = {}
        try:
            for step, call in enumerate(order):
                what = f"step {step} ({call}) of {order}"
                if call.startswith("map"):
                    thresholded = call != "map_plain"
                    res = dj.overlap_agg(dp, db, strict, nc, agg, index=ix, partition_mode=int(thresholded), **(dkw if thresholded else {}))
                    got = {"device": [{op: t.cpu().numpy() for op, t in r.items()} for r in res]}
                    S.map_check(got, mkept if thresholded else mplain, columns, what)
                    results[call] = S.map_blob(got)
                    continue
                if call == "semi_plain_bucketed":
                    got = (dj.overlap_select(dp, db, strict, nc, "semi", index=ix, partition_mode=1).cpu().numpy(),)
                    assert len(got[0]) == len(splain["semi"]) and (got[0] == splain["semi"]).all(), what
                elif call == "anti_thresh":
                    got = (dj.overlap_select(dp, db, strict, nc, "anti", index=ix, **dkw).cpu().numpy(),)
                    assert len(got[0]) == len(skept["anti"]) and (got[0] == skept["anti"]).all(), what
                elif call == "thresh_pairs_bucketed":
                    got = tuple(x.cpu().numpy() for x in dj.overlap_thresh(dp, db, strict, nc, index=ix, partition_mode=1, **dkw))
                    T.assert_order(*got, build)
                    T.assert_pairs(got, kept[:2], what)
                elif call == "count_bucketed":
                    got = (dj.count_overlaps(dp, db, strict, nc, index=ix, partition_mode=1).cpu().numpy(),)
                    assert (got[0] == plain[2]).all(), what
                else:
                    out = torch.full((n,), -7, dtype=torch.int64, device="cuda")
                    dj.overlap_bases(dp, db, strict, nc, index=ix, out=out, partition_mode=1)
                    got = (out.cpu().numpy(),)
                    DS.assert_bases_equal(got[0], bases, what)
                results[call] = b"|".join(np.ascontiguousarray(a).tobytes() for a in got)
        finally:
            ix.close()
        first = first or results
        assert results == first, f"{order}: a result differs from the first order's"


@gpu
@pytest.mark.parametrize("between", ["map_plain", "map_thresh", "select_thresh", "select_plain"])
def test_a_call_between_count_and_fill(dj, between):
    """D2.  overlap_agg_dev and the thresholded overlap_select_dev set ov_n = -1 and reuse the buffers the pending count -> fill
    hand-over lives in: the fill after them fails with IVJ_ESTATE and writes nothing.  The PLAIN selection keeps its counts in
    sel_buf and counts with count_overlaps' int32 form, which never buckets and touches neither ov_n nor the ov_* / pt_* buffers
    of the hand-over: the fill after it succeeds, and its pairs are right.  A fresh count -> fill pair afterwards returns the
    right pairs in every case."""
    import torch
    probe, build, nc = J.sequence_sides()
    strict = True
    plain = _ref("sequence", strict, False)
    total = len(plain[0])
    columns = J.agg_columns(len(build[0]), 79)[:1]
    kw = _kw(probe, build, strict, J.THR)
    dkw = S.dev_kw(kw)
    dp, db = J.dev_side(probe), J.dev_side(build)
    opts = _engine.make_opts(strict, nc, partition_mode=1)
    eng = dj.engine
    ix = dj.build_index(db, strict, nc)
    try:
        assert eng.overlap_count_dev(ix, dp.as_c(), opts) == total
        if between.startswith("map"):
            res = dj.overlap_agg(dp, db, strict, nc, S.dev_agg(columns), index=ix, partition_mode=1, **(dkw if between == "map_thresh" else {}))
            ref = _ref("sequence", strict, between == "map_thresh")
            S.map_check({"device": [{op: t.cpu().numpy() for op, t in r.items()} for r in res]}, S.map_expected(ref, len(probe[0]), columns), columns, between)
        else:
            thresholded = between == "select_thresh"
            rows = dj.overlap_select(dp, db, strict, nc, "semi", index=ix, partition_mode=1, **(dkw if thresholded else {})).cpu().numpy()
            assert (rows == S.select_expected(_ref("sequence", strict, thresholded), len(probe[0]))["semi"]).all()
        bufs = [torch.full((total + 16,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
        failed = False
        try:
            eng.overlap_fill_dev(ix, dp.as_c(), opts, bufs[0].data_ptr(), bufs[1].data_ptr(), total)
        except _engine.EngineError as err:
            failed = True
            assert err.code == _engine.IVJ_ESTATE, err
        torch.cuda.synchronize()
        assert failed == (between != "select_plain"), "the fill ran on a hand-over that the call in between ended" if not failed else \
            "the fill failed after a plain selection, which touches nothing of the hand-over"
        if failed:
            assert all(bool((t == -7).all()) for t in bufs), "a failed fill wrote into the pair buffers"
        else:
            T.assert_pairs(tuple(t[:total].cpu().numpy() for t in bufs), plain[:2], "the fill after a plain selection")
            assert all(bool((t[total:] == -7).all()) for t in bufs)
        assert eng.overlap_count_dev(ix, dp.as_c(), opts) == total
        out = [torch.full((total + 16,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
        eng.overlap_fill_dev(ix, dp.as_c(), opts, out[0].data_ptr(), out[1].data_ptr(), total)
        torch.cuda.synchronize()
        T.assert_pairs(tuple(t[:total].cpu().numpy() for t in out), plain[:2], "a fresh count -> fill pair")
        assert all(bool((t[total:] == -7).all()) for t in out)
    finally:
        ix.close()


@gpu
def test_one_context_under_alternating_large_and_small_inputs():
    """D3.  150 000 and 300 rows in turn on ONE engine and ONE DeviceJoin, five rounds: the small calls follow the large ones on
    the regrown arena and sel_buf"""
    from polars_bio_amd.device_api import DeviceJoin
    e, d = _engine.Engine(0), DeviceJoin(0)
    try:
        for step, (nrows, seed, strict) in enumerate(J.D3_ROUNDS):
            probe, build, nc = S.sized_sides(nrows, seed)
            n, name = len(probe[0]), f"sized_{nrows}_{seed}"
            columns = [(v, m, ops) for (v, m, _), ops in zip(J.agg_columns(len(build[0]), 80 + seed) + [(J.wide_ints(len(build[0]), seed), None, None)], MASKS)]
            for thresholded in (False, True):
                ref = _ref(name, strict, thresholded)
                kw = _kw(probe, build, strict, J.THR if thresholded else None)
                mexp, sexp = S.map_expected(ref, n, columns), S.select_expected(ref, n)
                for pm in (0, 1):
                    what = f"round {step}: {nrows} rows, strict={strict}, thresholded={thresholded}, partition_mode {pm}"
                    S.map_check(S.map_run(e, d, probe, build, nc, strict, columns, kw, partition_mode=pm), mexp, columns, what)
                    S.select_check(S.select_run(e, d, probe, build, nc, strict, kw, partition_mode=pm), sexp, build, what)
    finally:
        e.close()
        d.engine.close()


# ---- (E) coordinate limits -----------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("case", LIMIT_CASES)
def test_rows_at_the_int32_limits(eng, dj, case, strict):
    """E.  rows that start or end at INT32_MIN / INT32_MAX, the whole-range row, rows whose length needs 32 bits: without
    thresholds k_overlap_agg evaluates the plain predicate as written on loose, never-tightened ranges; min_overlap 2^31 + 1 can
    be met by the longest rows only"""
    probe, build, nc = _limit_case(case)
    n = len(probe[0])
    columns = J.agg_columns(len(build[0]), 81)
    sets = [None, LIMIT_THR, LIMIT_LONGEST]
    for thr in sets:
        ref = S.reference_once("limits_" + case, probe, build, nc, strict, thr)
        what = f"limits {case}, {thr}"
        if thr is None:
            _limits.assert_touches(ref[0], ref[1], probe, build, strict)
            assert (eng.count_overlaps(probe, build, strict, nc) == ref[2]).all(), "the plain count is count_overlaps"
        elif thr["min_overlap"] > 2:
            assert 0 < len(ref[0]) < len(S.reference_once("limits_" + case, probe, build, nc, strict, sets[1])[0])
        kw = _kw(probe, build, strict, thr)
        mexp, sexp = S.map_expected(ref, n, columns), S.select_expected(ref, n)
        base = None
        for pm in (0, 1):
            got = S.map_run(eng, dj, probe, build, nc, strict, columns, kw, partition_mode=pm)
            S.map_check(got, mexp, columns, f"{what}, partition_mode {pm}")
            assert (got["host"][0]["count"] <= ref[2]).all()
            sel = S.select_run(eng, dj, probe, build, nc, strict, kw, partition_mode=pm)
            S.select_check(sel, sexp, build, f"{what}, partition_mode {pm}")
            blobs = (S.map_blob(got), S.select_blob(sel, len(ref[0])))
            base = base or blobs
            assert blobs == base, f"{what}: partition_mode 1 differs from 0"
