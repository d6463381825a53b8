"""The thresholded join / count (k_overlap_thresh) and the merge aggregates (k_magg_tiles / k_magg_span) put through the project's
cross-cutting matrices, which their own modules -- each built around its kernel's tile -- leave out:

  (A) thresholds: the bucketed probe path (partition_mode 1, 5, 6 against 0 and 2), a probe side with row_id, an index built from
      a build side with row_id, device columns that are not 16-byte aligned (the scalar load path);
  (B) contig-dictionary sizes on both sides of every layout threshold with every out-of-dictionary id planted on both sides, the
      IVJ_COUNT_NOLDS / IVJ_JOINT_BINS table forms, and a sparse dictionary of 2^24 + 1 ids -- thresholds and merge_agg;
  (C) the index build forms: the LSD sort, the balanced build with its merge and staging knobs, its two hand-overs, the automatic
      choice at 140 000 rows and a hand-over at automatic size -- pinned by kernel name, results byte-identical between forms;
  (D) call sequences: one long-lived index under six calls in five orders (bucketing calls of other operations rewrite the pt_*
      columns between thresholded calls), merge_agg_dev at changing min_dist on one index, one context under alternating large
      and small inputs;
  (CPU) the fast references of _join_ops_util equal the literal ones (_thresholds_util.brute, _merge_agg_util.group_by) on
      scaled-down copies of every generator, and the generators have the properties the GPU tests rely on.

Thresholded calls go through all four entries (host pairs, host counts, device pairs, device counts); every comparison is
bit-exact and no tolerance appears anywhere."""
import numpy as np
import pytest

import _depth_sum_util as DS
import _join_ops_util as J
import _merge_agg_util as M
import _position_ops_util as P
import _thresholds_util as T
from oracle import oracle as O
from polars_bio_amd import _engine
from test_contig_dictionaries import OUTSIDE, _fresh
from test_gpu_parity import _v3_cases

gpu = pytest.mark.gpu
MODES = [pytest.param(True, id="strict"), pytest.param(False, id="weak")]
V3 = _v3_cases()
# (test id, words of the shape's own name in _v3_cases() that the id stands for: a shape that is added, dropped or moved fails here)
V3_NAMES = [("ragged", "ragged"), ("one_row", "one row"), ("rows_70k_outside", "70 k rows"), ("negative_equal_keys", "3000 equal keys"),
            ("bucket_above_lds", "one bucket above the LDS capacity"), ("linear_keys_33_bits", "linear keys beyond 32 bits")]
assert len(V3) == len(V3_NAMES) and all(words in entry[0] for entry, (_, words) in zip(V3, V3_NAMES)), [entry[0] for entry in V3]
V3_IDS = [vid for vid, _ in V3_NAMES]
TILE, MAGG_TILE = J.TILE, J.MAGG_TILE
I32 = np.iinfo(np.int32)


@pytest.fixture(scope="module")
def eng():
    return _engine.Engine(0)


@pytest.fixture(scope="module")
def dj():
    import torch  # noqa: F401
    from polars_bio_amd.device_api import DeviceJoin
    return DeviceJoin(0)


def _engines_under(monkeypatch, env):
    """(a fresh host engine and a fresh DeviceJoin created under `env`, the function that closes them and restores the environment)"""
    from polars_bio_amd.device_api import DeviceJoin
    e = _fresh(monkeypatch, **env)
    d = DeviceJoin(0)

    def done():
        e.close()
        d.engine.close()
        for k in env:
            monkeypatch.delenv(k)
    return e, d, done


_thresh_expected = {}


def _thresh_reference(name, probe, build, nc, strict, thr):
    """sorted_candidates of a named input, computed once and shared by the tests that run it"""
    key = (name, strict)
    if key not in _thresh_expected:
        _thresh_expected[key] = J.sorted_candidates(probe, build, nc, strict, **thr)
    return _thresh_expected[key]


# ---- (CPU) the fast references equal the literal ones; the generators' properties ---------------------------------------------------------

def _degenerate_sides():
    rng = np.random.default_rng(77)
    return P.degenerate_frame(rng, 500, 3, 900), P.degenerate_frame(rng, 600, 3, 900), 3


def _scaled_inputs():
    """name -> (probe, build, n_contigs, threshold set): scaled-down copies of every generator the GPU tests use"""
    out = {}
    probe, build, thr = J.partition_sides(n_probe=600, n_build=500)
    out["partition"] = (probe, build, 24, thr)
    for nc in (1, 65, 257):
        out[f"sweep_{nc}"] = (*J.sweep_sides(nc, n_build=800, n_probe=600), nc, J.THR)
    out["sparse"] = (*J.sparse_sides(n_build=1200, n_probe=800, occupied=300), P.SPARSE_NC, J.THR)
    for entry, vid in zip(V3, V3_IDS):
        probe, build, nc = J.v3_sides(entry)
        out["v3_" + vid] = (J.scaled(probe, 500, 1), J.scaled(build, 700, 2), nc, J.THR)
    probe, build, nc = J.auto_sides()
    out["auto"] = (J.scaled(probe, 600, 3), J.scaled(build, 2000, 4), nc, J.THR)
    out["handover"] = (*J.handover_sides(n=3000, n_probe=500)[:2], 1, J.THR)
    probe, build, nc = J.sequence_sides()
    out["sequence"] = (J.scaled(probe, 600, 5), J.scaled(build, 1500, 6), nc, J.THR)
    probe, build, nc = J.sized_sides(J.SMALL_ROWS, 901)
    out["sized"] = (probe, build, nc, J.THR)
    out["degenerate"] = (*_degenerate_sides(), J.THR)
    return out


@pytest.mark.parametrize("strict", MODES)
def test_cpu_sorted_candidates_equal_the_brute_force(strict):
    seen = dict(outside=0, zero=0, inverted=0, never=0)
    for name, (probe, build, nc, thr) in _scaled_inputs().items():
        rng = np.random.default_rng(len(name))
        sets = [thr, dict(min_overlap=1), dict(min_overlap=2, probe_min=J.never_mix(rng, len(probe[0])), build_min=J.never_mix(rng, len(build[0]))),
                dict(min_frac1=1.0), dict(min_frac2=0.5, min_overlap=7)]
        for t in sets:
            fast, lit = J.sorted_candidates(probe, build, nc, strict, **t), T.brute(probe, build, nc, strict, **t)
            for k in range(3):
                assert fast[k].dtype == lit[k].dtype and fast[k].shape == lit[k].shape and (fast[k] == lit[k]).all(), (name, t.keys(), k)
            # ... and in chunks of a few candidates (a probe's range then spans chunks)
            small = J.sorted_candidates(probe, build, nc, strict, cells=97, **t)
            assert all((small[k] == lit[k]).all() for k in range(3)), (name, "chunked")
        for side in (probe, build):
            seen["outside"] += int((~P.inside(side, nc)).sum())
            seen["zero"] += int((side[1] == side[2]).sum())
            seen["inverted"] += int((side[1] > side[2]).sum())
        seen["never"] += int((sets[2]["probe_min"] == J.NEVER).sum())
    assert all(v > 50 for v in seen.values()), seen


def _scaled_frames():
    """name -> (frame, n_contigs): the merge_agg inputs of the GPU tests, scaled down"""
    out = {}
    for nc in (1, 65, 257):
        out[f"sweep_{nc}"] = (J.chained_frame(J.sweep_sides(nc, n_build=800, n_probe=600)[1], 200), nc)
    out["sparse"] = (J.sparse_sides(n_build=1200, n_probe=800, occupied=300)[1], P.SPARSE_NC)
    for entry, vid in zip(V3, V3_IDS):
        _, build, nc = J.v3_sides(entry)
        out["v3_" + vid] = (J.scaled(build, 700, 2), nc)
    out["auto"] = (J.scaled(J.auto_sides()[1], 1500, 4), 24)
    out["handover"] = (J.handover_sides(n=3000, n_probe=500)[1], 1)
    out["sequence"] = (J.scaled(J.sequence_sides()[1], 1500, 6), 24)
    out["sized"] = (J.sized_sides(J.SMALL_ROWS, 901)[1], 24)
    out["degenerate"] = (_degenerate_sides()[1], 3)
    return out


@pytest.mark.parametrize("strict", MODES)
def test_cpu_vectorised_group_by_equals_the_literal_one(strict):
    seen = dict(no_valid=0, nan=0, wrapped=0, outside=0)
    for name, (frame, nc) in _scaled_frames().items():
        n = len(frame[0])
        for min_dist in (0, 50):
            cid, table = M.clusters(frame, nc, strict, min_dist)
            for values, valid, _ in J.agg_columns(n, len(name)) + [(J.wide_ints(n, 3), np.zeros(n, bool), J.ALL)]:
                fast, lit = J.group_by_fast(cid, len(table[0]), values, valid), M.group_by(cid, len(table[0]), values, valid)
                J.assert_lists_equal(J.as_lists(fast), lit, values.dtype, (name, min_dist))
                J.assert_agg_equal({op: np.asarray([0 if x is None else x for x in lit[op]]).astype(fast[op].dtype) for op in J.ALL}, fast,
                                   values.dtype, f"{name}: the vectorised comparison accepts the literal result")
                seen["no_valid"] += int((~fast["has"]).sum())
                if values.dtype == np.float64:
                    seen["nan"] += int(np.isnan(fast["sum"]).sum())
                elif valid is not None and valid.any():
                    exact = [0] * len(table[0])
                    for k, x in zip(cid[valid].tolist(), values[valid].tolist()):
                        exact[k] += x
                    seen["wrapped"] += sum(not -(1 << 63) <= x < (1 << 63) for x in exact)
        seen["outside"] += int((~P.inside(frame, nc)).sum())
    assert all(v > 20 for v in seen.values()), seen


def test_cpu_the_vectorised_comparison_is_not_blind():
    cid = np.array([0, 0, 1, 2, 2, 2])
    v = np.array([1.0, 2.0, np.nan, 5.0, 6.0, 7.0])
    exp = J.group_by_fast(cid, 4, v, np.array([1, 1, 1, 1, 1, 0], bool))
    assert exp["count"].tolist() == [2, 1, 2, 0] and exp["sum"][0] == 3.0 and np.isnan(exp["sum"][1]) and exp["max"][2] == 6.0 and exp["sum"][3] == 0
    good = {op: exp[op].copy() for op in J.ALL}
    good["min"][3] = 99.0                                    # unspecified: skipped
    J.assert_agg_equal(good, exp, np.float64, "")
    for op, k, x in (("sum", 3, 1.0), ("min", 0, 2.0), ("mean", 2, 5.0), ("count", 3, 1), ("max", 1, 0.0)):
        bad = {o: good[o].copy() for o in J.ALL}
        bad[op][k] = x
        with pytest.raises(AssertionError):
            J.assert_agg_equal(bad, exp, np.float64, "")


@pytest.mark.parametrize("strict", MODES)
def test_cpu_generator_properties(strict):
    """what the GPU tests rely on: outside ids on both sides, non-identity row ids, probes out of position order, every thresholded
    case keeps > 100 pairs and removes a pair of the plain predicate, the v3 shapes take the build the GPU test names, the
    aggregate frames have clusters that cross tile boundaries"""
    probe, build, thr = J.partition_sides()
    assert len(probe[0]) == 3 * TILE + 17 and len(build[0]) == 5000
    key = probe[0].astype(np.int64) << 32 | probe[1].astype(np.int64)
    assert (np.argsort(key, kind="stable") != np.arange(len(key))).mean() > 0.99, "the bucket permutation is far from the identity"
    assert (thr["probe_min"] == J.NEVER).sum() > 100 and (thr["build_min"] == J.NEVER).sum() > 100
    kept, plain = J.kept_and_removed(probe, build, 24, strict, thr)
    assert 100 < kept < plain
    for n in (TILE - 1, TILE + 1, 2 * TILE + 3):
        p, b, t = J.partition_sides(n_probe=n)
        kept, plain = J.kept_and_removed(p, b, 24, strict, t)
        assert 100 < kept < plain, n
    n = len(probe[0])
    rid = J.probe_ids(n)
    assert len(np.unique(rid)) == n and rid.min() > n and (rid != np.arange(n)).all()
    bid, moved = J.build_ids(5000)
    assert len(np.unique(bid)) == 5000 and ((bid < 0) | (bid >= 5000)).sum() == 6 == len(moved) and (bid != np.arange(5000)).mean() > 0.99
    # the rows that carry outside ids overlap probes: leaving out the range check of the gather, or of a build_min lookup, shows
    sub = P.rows(build, moved)
    assert len(J.sorted_candidates(probe, sub, 24, strict, min_overlap=1)[0]) > 0

    for nc in P.SWEEP:
        probe, build = J.sweep_sides(nc)
        for side in (probe, build):
            assert set(OUTSIDE(nc)) <= set(side[0].tolist()), "every out-of-dictionary id on both sides"
            assert (side[0] == 0).any() and (side[0] == nc - 1).any()
        if nc > 7:
            empty = np.arange(3, nc - 1, 7)
            assert not np.isin(build[0], empty).any() and np.isin(probe[0], empty).any(), "every 7th contig empty on the build side"
        kept, plain = J.kept_and_removed(probe, build, nc, strict, J.THR)
        assert 100 < kept < plain, nc
        frame = J.sweep_frame(nc)
        assert set(OUTSIDE(nc)) <= set(frame[0].tolist()) and len(frame[0]) == len(build[0]) + MAGG_TILE + 50
        for min_dist in (0, 50):
            sizes = np.bincount(M.clusters(frame, nc, strict, min_dist)[0])
            assert sizes[0] > MAGG_TILE and J.tiles_crossed(sizes, MAGG_TILE) > 0, (nc, min_dist)

    probe, build = J.sparse_sides()
    nc = P.SPARSE_NC
    counts = np.bincount(build[0][P.inside(build, nc)], minlength=nc)
    assert counts[0] > 0 and counts[nc - 1] > 0 and (counts == 0).sum() > nc // 2 and (counts == 1).sum() > 1000 and counts.max() > 1000
    assert all(set(OUTSIDE(nc)) <= set(s[0].tolist()) for s in (probe, build))
    kept, plain = J.kept_and_removed(probe, build, nc, strict, J.THR)
    assert 100 < kept < plain
    cid, table = M.clusters(build, nc, strict, 0)
    sizes = np.bincount(cid)
    assert len(build[0]) > 4 * MAGG_TILE and (sizes == 1).sum() > 1000, "one-row clusters ..."
    holder = np.repeat(np.arange(len(sizes)), sizes)                       # sorted position -> its cluster (the engine numbers them in order)
    edges = np.arange(MAGG_TILE, len(build[0]), MAGG_TILE)
    assert ((sizes[holder[edges - 1]] == 1) & (sizes[holder[edges]] == 1)).any(), "... on both sides of a tile boundary"
    assert (table[0] == -1).sum() >= 1, "the pseudo-contig has clusters"

    for entry, vid in zip(V3, V3_IDS):
        probe, build, nc = J.v3_sides(entry)
        assert P.takes_balanced_build(build, nc) == entry[4], vid
        kept, plain = J.kept_and_removed(probe, build, nc, strict, J.THR)
        assert 100 < kept < plain, (vid, kept, plain)
        sizes = np.bincount(M.clusters(build, nc, strict, 0)[0])
        if len(build[0]) == 1:                               # one row: one tile, nothing to cross
            assert vid.startswith("one_row")
        elif sizes.max() <= 2:                               # starts over all of int32, rows under 100 long: every tile boundary falls BETWEEN clusters
            assert vid.startswith("linear_keys") and len(build[0]) > 4 * MAGG_TILE and J.tiles_crossed(sizes, MAGG_TILE) == 0
        else:
            assert J.tiles_crossed(sizes, MAGG_TILE) > 0, vid
    probe, build, nc = J.auto_sides()
    assert len(build[0]) == 140_000 >= P.V3_AUTO_FROM and len(probe[0]) == 20_000 and P.takes_balanced_build(build, nc)
    kept, plain = J.kept_and_removed(probe, build, nc, strict, J.THR)
    assert 100 < kept < plain
    probe, build, nc = J.handover_sides()
    span, fullest = P.v3_geometry(build, nc)
    assert len(build[0]) >= P.V3_AUTO_FROM and span <= 0xffffffff and fullest > P.V3_CAP, "the automatic rule, then the hand-over"
    kept, plain = J.kept_and_removed(probe, build, nc, strict, J.THR)
    assert 100 < kept < plain
    cid, table = M.clusters(build, nc, strict, 0)
    sizes = np.bincount(cid)
    assert sizes.max() >= len(build[0]) - 2 and J.tiles_crossed(sizes, MAGG_TILE) == (len(build[0]) - 1) // MAGG_TILE, "one chain over every tile"

    probe, build, nc = J.sequence_sides()
    kept, plain = J.kept_and_removed(probe, build, nc, strict, J.THR)
    assert 100 < kept < plain and len(build[0]) == 50_000
    for min_dist in (0, 1000):
        sizes = np.bincount(M.clusters(build, nc, strict, min_dist)[0])
        assert J.tiles_crossed(sizes, MAGG_TILE) > 0
    assert [n for n, _, _ in J.D3_ROUNDS] == [150_000, 300, 150_000, 300, 150_000]
    for n, seed, mode in J.D3_ROUNDS:                        # exactly the inputs and modes the rounds of D3 run
        probe, build, nc = J.sized_sides(n, seed)
        kept, plain = J.kept_and_removed(probe, build, nc, mode, J.THR)
        assert len(build[0]) == n and 100 < kept < plain, (n, seed, mode, kept, plain)


# ---- (A) partitioning, row ids, alignment --------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("strict", MODES)
def test_bucketed_probe_path_against_the_unbucketed_one(eng, dj, strict):
    """A1.  partition_mode 1, 5, 6 bucket the probes (0 and 2 do not at this size): the kernel then reads probe_min[pos], writes
    counts[pos] and reports pos, pos = pt_row of the partition; the emit pass reuses the pt_* columns the count pass left."""
    probe, build, thr = J.partition_sides()
    exp = _thresh_reference("partition", probe, build, 24, strict, thr)
    kw = J.engine_kw(probe, build, strict, **thr)
    base = J.thresh_run(eng, dj, probe, build, 24, strict, kw, partition_mode=0)
    J.thresh_check(base, exp, build, "partition_mode 0")
    for pm in (0, 1, 2, 5, 6):
        got = base if pm == 0 else J.thresh_run(eng, dj, probe, build, 24, strict, kw, partition_mode=pm)
        J.thresh_check(got, exp, build, f"partition_mode {pm}")
        J.assert_thresh_same(got, base, f"partition_mode {pm} vs 0", keys=("host_counts", "dev_counts"))
        for key in ("host_pairs", "dev_pairs"):              # which path ran shows in the order of the probe rows
            backwards = bool((np.diff(got[key][0]) < 0).any())
            assert backwards == (pm in (1, 5, 6)), f"partition_mode {pm} {key}: probe rows {'bucket by bucket' if backwards else 'in input order'}"


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("pm", [0, 1, 2])
def test_probe_side_with_row_ids(dj, pm, strict):
    """A2.  include/ivjoin.h: probe_min and the counts go by the row's position in the probe columns, the pairs carry row_id.  The
    ids lie above n_probe, so neither can stand in for the other.  (Device entries: the host binding carries no row_id.)"""
    probe, build, thr = J.partition_sides()
    rid = J.probe_ids(len(probe[0]))
    exp = _thresh_reference("partition", probe, build, 24, strict, thr)
    kw = J.engine_kw(probe, build, strict, **thr)
    got = J.thresh_run(None, dj, probe, build, 24, strict, kw, partition_mode=pm, probe_row_id=rid)
    assert got["dev_pairs"][0].min() > len(probe[0]), "the pairs report ids"
    J.thresh_check(got, exp, build, f"probe row_id, partition_mode {pm}", probe_row_id=rid)


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_index_built_from_a_build_side_with_row_ids(dj, strict):
    """A3.  build_min is indexed by the id the index reports; ids outside [0, build rows) never match when build_min is given
    (include/ivjoin.h; k_thresh_gather maps them to "never").  Without build_min nothing is looked up by id: the header attaches
    "never match" to build_min's indexing only, and the kernel reports b_row as it is -- so rows with outside ids match like any
    other row and the pairs carry those ids.  Both are pinned here.  Among equal starts the pairs follow the build row's POSITION
    (the index sort is stable in input order), not its id."""
    probe, build, thr = J.partition_sides()
    n = len(build[0])
    bid, moved = J.build_ids(n)
    inside = (bid >= 0) & (bid < n)
    by_id = J.never_mix(np.random.default_rng(9), n)                      # build_min as the caller gives it: entry i belongs to id i
    by_position = np.where(inside, by_id[np.where(inside, bid, 0)], J.NEVER).astype(np.uint32)
    for pm in (0, 1):
        t = dict(min_overlap=2, probe_min=thr["probe_min"], build_min=by_position)
        exp = J.sorted_candidates(probe, build, 24, strict, **t)
        assert len(exp[0]) > 100 and not np.isin(exp[1], moved).any()
        got = J.thresh_run(None, dj, probe, build, 24, strict, dict(t, build_min=by_id), partition_mode=pm, build_row_id=bid)
        assert not np.isin(got["dev_pairs"][1], bid[moved]).any(), "an id outside [0, build rows) matched although build_min is given"
        J.thresh_check(got, exp, build, f"build row_id with build_min, partition_mode {pm}", build_row_id=bid)
        t = dict(min_overlap=2, probe_min=thr["probe_min"])
        exp = J.sorted_candidates(probe, build, 24, strict, **t)
        assert np.isin(exp[1], moved).any()
        got = J.thresh_run(None, dj, probe, build, 24, strict, dict(t, build_min=None), partition_mode=pm, build_row_id=bid)
        J.thresh_check(got, exp, build, f"build row_id without build_min, partition_mode {pm}", build_row_id=bid)


@gpu
@pytest.mark.parametrize("n", [TILE - 1, TILE + 1, 2 * TILE + 3])
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_columns_that_are_not_16_byte_aligned(dj, shift, n):
    """A4.  contig / start / end (and row_id) as views that start 1, 2, 3 elements into a larger tensor: the vector loads are off
    and every probe is read by the scalar path, whose tail guard i0 + k < n meets the last tile at these sizes.  Unbucketed
    (partition_mode 2: the kernel reads the caller's columns) and bucketed (the partition reads them)."""
    strict = (shift + n) % 2 == 0
    probe, build, thr = J.partition_sides(n_probe=n)
    exp = J.sorted_candidates(probe, build, 24, strict, **thr)
    kw = J.engine_kw(probe, build, strict, **thr)
    rid = J.probe_ids(n)
    for pm in (2, 1):
        for ids in (None, rid):
            what = f"shift {shift}, n {n}, partition_mode {pm}, row_id {ids is not None}"
            aligned = J.thresh_run(None, dj, probe, build, 24, strict, kw, partition_mode=pm, probe_row_id=ids)
            got = J.thresh_run(None, dj, probe, build, 24, strict, kw, partition_mode=pm, probe_row_id=ids, shift=shift)
            J.thresh_check(got, exp, build, what, probe_row_id=ids)
            J.assert_thresh_same(got, aligned, what + " vs aligned copies")


# ---- (B) dictionary sizes --------------------------------------------------------------------------------------------------------------

def _thresh_dictionary_checks(eng, dj, probe, build, nc, strict, name):
    exp = _thresh_reference(name, probe, build, nc, strict, J.THR)
    kw = J.engine_kw(probe, build, strict, **J.THR)
    got = J.thresh_run(eng, dj, probe, build, nc, strict, kw)
    J.thresh_check(got, exp, build, name)
    in_p, in_b = P.inside(probe, nc), P.inside(build, nc)
    assert (~in_p).sum() >= 10 and (~in_b).sum() >= 10
    for key, g in got.items():
        if key.endswith("pairs"):
            assert in_p[g[0]].all() and in_b[g[1]].all(), f"{name} {key}: an out-of-dictionary row in a pair"
        else:
            assert not g[~in_p].any(), f"{name} {key}: an out-of-dictionary probe with a non-zero count"
    bare_p, bare_b = P.rows(probe, in_p), P.rows(build, in_b)
    bare = J.thresh_run(eng, dj, bare_p, bare_b, nc, strict, J.engine_kw(bare_p, bare_b, strict, **J.THR))
    for key, g in got.items():
        want = J.reindexed(g, in_p, in_b) if key.endswith("pairs") else (g[in_p],)
        have = bare[key] if key.endswith("pairs") else (bare[key],)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(want, have)), f"{name} {key}: differs without the out-of-dictionary rows"
    for pm in (1, 2):
        other = J.thresh_run(eng, dj, probe, build, nc, strict, kw, partition_mode=pm)
        J.thresh_check(other, exp, build, f"{name}, partition_mode {pm}")
        J.assert_thresh_same(other, got, f"{name}: partition_mode {pm} vs 0", keys=("host_counts", "dev_counts"))


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("nc", P.SWEEP)
def test_thresholds_across_dictionary_sizes(eng, dj, nc, strict):
    """B1"""
    probe, build = J.sweep_sides(nc)
    _thresh_dictionary_checks(eng, dj, probe, build, nc, strict, f"sweep_{nc}")


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("nc", [24, 257])
@pytest.mark.parametrize("knob", ["IVJ_COUNT_NOLDS", "IVJ_JOINT_BINS"])
def test_thresholds_under_the_table_knobs(knob, nc, strict, monkeypatch):
    """B2.  the per-contig grid metadata read from global memory, and one bin per row instead of two: build_flat sits on these
    tables"""
    probe, build = J.sweep_sides(nc)
    e, d, done = _engines_under(monkeypatch, {knob: "1"})
    try:
        _thresh_dictionary_checks(e, d, probe, build, nc, strict, f"sweep_{nc}")
    finally:
        done()


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_thresholds_on_a_sparse_dictionary_of_2_24_plus_1_ids(eng, dj, strict):
    """B3"""
    probe, build = J.sparse_sides()
    nc = P.SPARSE_NC
    exp = _thresh_reference("sparse", probe, build, nc, strict, J.THR)
    kw = J.engine_kw(probe, build, strict, **J.THR)
    got = J.thresh_run(eng, dj, probe, build, nc, strict, kw)
    J.thresh_check(got, exp, build, "sparse")
    ix = dj.build_index(J.dev_side(build), strict, nc)
    try:
        other = J.thresh_run(None, dj, probe, build, nc, strict, kw, partition_mode=1, index=ix)
    finally:
        ix.close()
    J.thresh_check(other, exp, build, "sparse, partition_mode 1")
    J.assert_thresh_same(other, got, "sparse: partition_mode 1 vs 0", keys=("dev_counts",))


def _agg_dictionary_checks(eng, dj, frame, nc, strict, name):
    columns = J.agg_columns(len(frame[0]), 31)
    for min_dist in (0, 50):
        exp = J.agg_expected(name, frame, nc, strict, min_dist, columns)
        assert (exp[0][0] == -1).any() and exp[1][0]["has"][exp[0][0] == -1].any(), "the pseudo-contig's clusters carry aggregates"
        got = J.agg_run(eng, dj, frame, nc, strict, min_dist, columns)
        J.agg_check(got, exp, columns, f"{name}, min_dist {min_dist}")


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("nc", P.SWEEP)
def test_merge_agg_across_dictionary_sizes(eng, dj, nc, strict):
    """B4.  the out-of-dictionary rows form a pseudo-contig after every real contig; its clusters are compared like any other"""
    _agg_dictionary_checks(eng, dj, J.sweep_frame(nc), nc, strict, f"sweep_{nc}")


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_merge_agg_on_a_sparse_dictionary_of_2_24_plus_1_ids(eng, dj, strict):
    """B3.  thousands of single-row contigs: one-row clusters across the tile boundaries"""
    _agg_dictionary_checks(eng, dj, J.sparse_sides()[1], P.SPARSE_NC, strict, "sparse")


# ---- (C) index build forms -------------------------------------------------------------------------------------------------------------

def _names_of(e, fn):
    e.timings()
    out = fn()
    return out, sorted(e.timings())


def _assert_build(t, form, balanced, what):
    """which index build ran, by kernel name (one frame is indexed per call: the names are exact)"""
    local, final = "ix3_local" in t, "ix_final" in t
    if form.get("IVJ_IX_V3") != "1":
        assert final and not local, (what, t)
    else:
        assert local == balanced and final != balanced, (what, t)


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("entry", V3, ids=V3_IDS)
def test_index_build_forms(entry, strict, monkeypatch):
    """C1.  k_overlap_thresh reads rec4, the flat tables and (through k_thresh_gather, build_min is given) b_row as the build form
    left them; the aggregate kernels gather values[b_row[p]] along cid1.  Equal starts keep their input order under every form,
    so results are byte-identical between forms, the emitted pair order included."""
    probe, build, nc = J.v3_sides(entry)
    balanced = entry[4]
    name = "v3: " + entry[0]
    exp = _thresh_reference(name, probe, build, nc, strict, J.THR)
    kw = J.engine_kw(probe, build, strict, **J.THR)
    assert kw["build_min"] is not None
    columns = J.agg_columns(len(build[0]), 41)
    aexp = J.agg_expected(name, build, nc, strict, 0, columns)
    blobs = []
    for form in P.FORMS:
        e, d, done = _engines_under(monkeypatch, form)
        try:
            e.enable_timing(2)
            what = f"{name} under {form}"
            (p, b), t = _names_of(e, lambda: e.overlap_thresh(probe, build, strict, nc, **kw))
            assert "thresh_gather" in t and ("overlap_thresh_emit" in t or len(exp[0]) == 0), (what, t)
            _assert_build(t, form, balanced, what)
            agg_host, t = _names_of(e, lambda: J.agg_run(e, None, build, nc, strict, 0, columns))
            assert "merge_agg_tiles" in t, (what, t)
            _assert_build(t, form, balanced, what)
            got = J.thresh_run(e, d, probe, build, nc, strict, kw)
            assert got["host_pairs"][0].tobytes() == np.array(p).tobytes() and got["host_pairs"][1].tobytes() == np.array(b).tobytes(), what
            J.thresh_check(got, exp, build, what)
            agg = dict(agg_host, **J.agg_run(None, d, build, nc, strict, 0, columns))
            J.agg_check(agg, aexp, columns, what)
            blobs.append((J.thresh_blob(got), J.agg_blob(agg)))
        finally:
            done()
    assert all(b == blobs[0] for b in blobs), "byte-identical results under every index build form"


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_automatic_balanced_build_at_140k_rows(strict):
    """C2.  no knob: 140 000 build rows on 24 contigs take the balanced build by the automatic rule"""
    from polars_bio_amd.device_api import DeviceJoin
    probe, build, nc = J.auto_sides()
    e, d = _engine.Engine(0), DeviceJoin(0)
    try:
        e.enable_timing(2)
        kw = J.engine_kw(probe, build, strict, **J.THR)
        _, t = _names_of(e, lambda: e.count_overlaps_thresh(probe, build, strict, nc, **kw))
        assert "ix3_local" in t and "ix_final" not in t and "overlap_thresh_count" in t, t
        got = J.thresh_run(e, d, probe, build, nc, strict, kw)
        J.thresh_check(got, _thresh_reference("auto", probe, build, nc, strict, J.THR), build, "auto_140k")
        columns = J.agg_columns(len(build[0]), 43)
        agg, t = _names_of(e, lambda: J.agg_run(e, None, build, nc, strict, 0, columns))
        assert "ix3_local" in t and "ix_final" not in t and "merge_agg_span" in t, t
        agg.update(J.agg_run(None, d, build, nc, strict, 0, columns))
        J.agg_check(agg, J.agg_expected("auto", build, nc, strict, 0, columns), columns, "auto_140k")
    finally:
        e.close()
        d.engine.close()


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_hand_over_to_the_lsd_sort_at_automatic_size(strict):
    """C3.  140 000 rows in one narrow window: the balanced build starts by the automatic rule (ix3_pass), finds one bucket above
    its capacity and hands the index to the LSD sort (ix_final, no ix3_local).  Nearly all rows are ONE cluster chain that crosses
    every tile of the aggregate kernel.  (After two hand-overs in a row a context leaves the balanced build out for a while: the
    names are asserted on the first call of a fresh engine only.)"""
    from polars_bio_amd.device_api import DeviceJoin
    probe, build, nc = J.handover_sides()
    e, d = _engine.Engine(0), DeviceJoin(0)
    try:
        e.enable_timing(2)
        columns = J.agg_columns(len(build[0]), 45)
        agg, t = _names_of(e, lambda: J.agg_run(e, None, build, nc, strict, 0, columns))
        assert "ix3_pass" in t and "ix3_local" not in t and "ix_final" in t and "merge_agg_span" in t, t
        agg.update(J.agg_run(None, d, build, nc, strict, 0, columns))
        exp = J.agg_expected("handover", build, nc, strict, 0, columns)
        assert exp[0][3].max() >= len(build[0]) - 2
        J.agg_check(agg, exp, columns, "hand-over")
        kw = J.engine_kw(probe, build, strict, **J.THR)
        got = J.thresh_run(e, d, probe, build, nc, strict, kw)
        J.thresh_check(got, _thresh_reference("handover", probe, build, nc, strict, J.THR), build, "hand-over")
    finally:
        e.close()
        d.engine.close()


# ---- (D) call sequences ----------------------------------------------------------------------------------------------------------------

CALLS = ("overlap", "count_bucketed", "thresh_pairs_bucketed", "thresh_counts", "bases_bucketed", "thresh_pairs")
ORDERS = [CALLS,
          ("thresh_pairs", "bases_bucketed", "thresh_counts", "thresh_pairs_bucketed", "count_bucketed", "overlap"),
          ("thresh_pairs_bucketed", "bases_bucketed", "thresh_pairs", "count_bucketed", "thresh_counts", "overlap"),
          ("bases_bucketed", "thresh_pairs_bucketed", "overlap", "thresh_pairs", "count_bucketed", "thresh_counts"),
          ("count_bucketed", "thresh_counts", "bases_bucketed", "thresh_pairs", "overlap", "thresh_pairs_bucketed")]


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_calls_on_one_index_in_any_order(dj, strict):
    """D1.  one long-lived DeviceIndex of 50 000 rows.  plain count with partition_mode 1 and overlap_bases with partition_mode 1
    rewrite the context's pt_* columns, which a bucketed thresholded call also uses between its count and emit passes; the flat
    tables are built on the index by whichever thresholded call comes first.  Every result equals the first order's byte for
    byte (the plain join's pairs after sorting: their order across tiles is not part of its contract) and the reference."""
    import torch
    probe, build, nc = J.sequence_sides()
    n = len(probe[0])
    kw = J.engine_kw(probe, build, strict, **J.THR)
    dkw = dict(min_overlap=kw["min_overlap"], probe_min=J.dev_min(kw["probe_min"]), build_min=J.dev_min(kw["build_min"]))
    ox = O.Index(O.Side(*build), nc)
    ep, eb, ecnt = _thresh_reference("sequence", probe, build, nc, strict, J.THR)
    plain_p, plain_b = T.sort_pairs(*O.overlap_fast(ox, O.Side(*probe), strict))
    plain_cnt = O.count_overlaps_fast(ox, O.Side(*probe), strict)
    bases = DS.prefix_form(probe, build, strict, nc)
    assert 100 < len(ep) < len(plain_p)
    dp, db = J.dev_side(probe), J.dev_side(build)
    first = None
    for order in ORDERS:
        assert sorted(order) == sorted(CALLS)
        ix = dj.build_index(db, strict, nc)
        results = {}
        try:
            for step, call in enumerate(order):
                what = f"step {step} ({call}) of {order}"
                if call == "overlap":
                    p, b = T.sort_pairs(*(x.cpu().numpy() for x in dj.overlap(dp, db, strict, nc, index=ix)))
                    assert len(p) == len(plain_p) and (p == plain_p).all() and (b == plain_b).all(), what
                    got = (p, b)
                elif call == "count_bucketed":
                    got = (dj.count_overlaps(dp, db, strict, nc, index=ix, partition_mode=1).cpu().numpy(),)
                    assert (got[0] == plain_cnt).all(), what
                elif call.startswith("thresh_pairs"):
                    pm = 1 if call.endswith("bucketed") else 0
                    got = tuple(x.cpu().numpy() for x in dj.overlap_thresh(dp, db, strict, nc, index=ix, partition_mode=pm, **dkw))
                    T.assert_order(*got, build)
                    T.assert_pairs(got, (ep, eb), what)
                elif call == "thresh_counts":
                    got = (dj.count_overlaps_thresh(dp, db, strict, nc, index=ix, **dkw).cpu().numpy(),)
                    assert (got[0] == ecnt).all(), what
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
@pytest.mark.parametrize("strict", MODES)
def test_merge_agg_on_one_index_with_changing_min_dist(dj, strict):
    """D2.  one sweep-only DeviceIndex; every merge_agg_dev call derives cid1 anew for its min_dist, and merge_dev / cluster_dev
    between them leave their own cluster tables in the context"""
    import torch
    probe, build, nc = J.sequence_sides()
    n = len(build[0])
    columns = J.agg_columns(n, 47)
    opts = _engine.make_opts(strict, nc)
    ix = dj.engine.index_build_dev(J.dev_side(build).as_c(), opts, False, sweep_only=True)
    try:
        def agg(min_dist):
            got = {"device": J.agg_dev_call(dj.engine, ix, nc, strict, min_dist, columns, n)}
            J.agg_check(got, J.agg_expected("sequence", build, nc, strict, min_dist, columns), columns, f"min_dist {min_dist}")
            return J.agg_blob(got)
        a0 = agg(0)
        cid, table = M.clusters(build, nc, strict, 37)
        out = [torch.empty(n, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.int32, torch.int64)]
        total, fits = dj.engine.merge_dev(ix, opts, 37, n, *(t.data_ptr() for t in out))
        assert fits and total == len(table[0]) and all((t[:total].cpu().numpy() == x).all() for t, x in zip(out, table))
        a1000 = agg(1000)
        cl = [torch.empty(n, dtype=dt, device="cuda") for dt in (torch.int64, torch.int32, torch.int32)]
        assert dj.engine.cluster_dev(ix, opts, 37, *(t.data_ptr() for t in cl)) == len(table[0])
        assert (cl[0].cpu().numpy() == cid).all() and (cl[1].cpu().numpy() == table[1][cid]).all() and (cl[2].cpu().numpy() == table[2][cid]).all()
        assert agg(0) == a0 != a1000
    finally:
        ix.close()


@gpu
def test_one_context_under_alternating_large_and_small_inputs():
    """D3.  150 000 and 300 rows in turn on ONE engine and ONE DeviceJoin, five rounds: the small calls follow the large ones on a
    regrown arena and ov_buf, and on a recycled index slab that is larger than they need"""
    from polars_bio_amd.device_api import DeviceJoin
    e, d = _engine.Engine(0), DeviceJoin(0)
    try:
        for step, (n, seed, strict) in enumerate(J.D3_ROUNDS):
            probe, build, nc = J.sized_sides(n, seed)
            what = f"round {step}: {len(build[0])} rows, strict={strict}"
            name = f"sized_{n}_{seed}"
            for pm in (0, 1):
                got = J.thresh_run(e, d, probe, build, nc, strict, J.engine_kw(probe, build, strict, **J.THR), partition_mode=pm)
                J.thresh_check(got, _thresh_reference(name, probe, build, nc, strict, J.THR), build, f"{what}, partition_mode {pm}")
            columns = J.agg_columns(len(build[0]), 49 + seed)
            agg = J.agg_run(e, d, build, nc, strict, 0, columns)
            J.agg_check(agg, J.agg_expected(name, build, nc, strict, 0, columns), columns, what)
    finally:
        e.close()
        d.engine.close()
