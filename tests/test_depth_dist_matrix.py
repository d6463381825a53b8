"""depth_histogram (k_depth_hist, k_depth_hist_contigs) and depth_quantiles (k_depth_quant) with their shared host step
(depth_blocks_build of host_depth_hist.hip.h) put through the project's cross-cutting matrices, which tests/test_depth_hist_gpu.py
and tests/test_depth_quant_gpu.py -- built around the kernels' own tiles, chunks and passes -- leave out:

  (B) contig-dictionary sizes on both sides of every layout threshold, the sparse dictionary of 2^24 + 1 ids, every id outside the
      dictionary, contigs the build lacks, the IVJ_COUNT_NOLDS / IVJ_JOINT_BINS forms of the grid, every partition_mode (ignored),
      the tile of k_depth_hist under IVJ_HIST_LDS_KB;
  (C) the index build forms, for the caller's index AND for the index of the depth blocks that every call builds with the caller's
      options: the LSD sort, the balanced build and its knobs, the hand-overs, the automatic rule for 258 000 blocks of 140 000
      rows, and for 150 000 blocks of 100 000 rows (the caller's index below the rule, the blocks' above it, in one call);
  (T) probe edges that ARE block boundaries, one position off either way, contigs of one block and of two abutting blocks, ranks
      on the cumulative boundaries a clip moves;
  (D) call sequences on one long-lived index built without the end order; one context under alternating large and small inputs;
  (A) probe columns, ranks and outputs that are 4- / 8-byte but not 16-byte aligned, the outputs between sentinels, row ids on
      either side;
  (CPU) the block forms equal the per-base forms and a third, block-free form on a scaled-down copy of every generator, the
      generators have the properties the GPU tests rely on, and the comparisons are not blind.

Entries: Engine.depth_hist / depth_hist_contigs / depth_quantiles and DeviceJoin.depth_histogram / depth_histogram_contigs /
depth_quantiles into a caller's prefilled buffer.  max_depth 6 and K in {1, 3, 16} by the case's name where a group names no other.
Every comparison is exact (int64 / int32 equality, or byte equality between two engine results); no tolerance appears anywhere."""
import numpy as np
import pytest

import _depth_dist_matrix_util as Y
import _depth_hist_util as H
import _depth_profile_matrix_util as X
import _depth_profile_util as DP
import _depth_quant_util as Q
import _depth_sum_util as DS
import _depth_summary_util as DQ
import _join_ops_util as J
import _position_ops_util as P
from polars_bio_amd import _engine
from test_contig_dictionaries import OUTSIDE, _fresh
from test_depth_profile_matrix import V3_IDS
from test_join_ops_matrix import _engines_under, _names_of, _assert_build
from test_position_ops_matrix import _sequence_reference

gpu = pytest.mark.gpu
MODES = [pytest.param(True, id="strict"), pytest.param(False, id="weak")]
MD = Y.MAX_DEPTH
A_PARAMS = [(1, 1), (6, 3), (100, 16)]          # (max_depth, K) of group A
LDS_DEPTHS = [6, 682]


@pytest.fixture(scope="module")
def eng():
    return _engine.Engine(0)


@pytest.fixture(scope="module")
def dj():
    import torch  # noqa: F401
    from polars_bio_amd.device_api import DeviceJoin
    return DeviceJoin(0)


def _full_size_cases(strict):
    """every case the GPU tests run, by name"""
    out = {f"sweep_{nc}": Y.sweep_case(nc, strict) for nc in P.SWEEP}
    out.update({"sparse": Y.sparse_case(strict), "t": Y.t_case(strict), "auto": Y.auto_case(strict), "inner_auto": Y.inner_auto_case(strict),
                "sequence": Y.sequence_case(), "sized_large": Y.sized_case(150_000, 900, strict),
                "sized_small": Y.sized_case(J.SMALL_ROWS, 901, strict), "a": Y.a_case(strict)})
    out.update({f"v3_{vid}": Y.v3_case(entry, strict) for entry, vid in zip(X.v3_entries(), V3_IDS)})
    return out


# ---- (CPU) ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strict", MODES)
def test_cpu_block_forms_equal_the_per_base_and_the_rank_form_on_every_generator(strict):
    dense = 0
    for name, make in Y.SCALED.items():
        case = make(strict)
        assert case.n <= 2000 and len(case.build[0]) <= 2000, name
        md, ranks = Y.md_of(case), Y.ranks_of(case, strict)
        hist, val = Y.hist_ref(case, strict), Y.quant_ref(case, strict)
        h3, v3 = Y.rank_form(case, strict, md, ranks)
        H.assert_hist_equal(h3, hist, f"{name}: rank form")
        Q.assert_quant_equal(v3.astype(np.int32), val, f"{name}: rank form")
        if Y.dense_fits(case, strict):                           # (the 33-bit keys and the rows at the int32 limits do not)
            dense += 1
            H.assert_hist_equal(H.dense_form(case.windows, case.build, strict, case.nc, md), hist, f"{name}: per-base form")
            Q.assert_quant_equal(Q.dense_form(case.windows, case.build, strict, case.nc, ranks).astype(np.int32), val, f"{name}: per-base form")
        # a row sums to its positions; the contig form is the sum of the block lengths, and its sparse form the same rows
        assert (hist.sum(axis=1) == H.positions(case.windows, strict, case.nc)).all(), name
        ids, rows = Y.contig_rows(case.build, strict, case.nc, md)
        if case.nc <= 10_000:
            full = Y.contig_ref(case, strict)
            assert np.array_equal(np.flatnonzero(full.any(axis=1)), ids) and np.array_equal(full[ids], rows), name
    assert dense >= len(Y.SCALED) - 2, dense


@pytest.mark.parametrize("strict", MODES)
def test_cpu_the_comparisons_are_not_blind(strict):
    """among the probes inside the dictionary at least half have a non-zero bin above bin 0, the clamp bin is non-zero somewhere, at
    least a quarter of the valid ranks answer above 0 and at least three distinct answers occur -- for every case the GPU tests
    run.  (The one-row shape of group C is one block of depth 1: it runs at max_depth 1, where that depth is the clamp bin, and
    its valid ranks have two answers, 0 and 1; the bar there is every answer the build allows.)  The assert helpers raise on a
    +-1 change of the first, a middle and the last cell, on two swapped rows and on a wrong dtype."""
    ks = set()
    for name, case in _full_size_cases(strict).items():
        above, clamp, positive, distinct = Y.bars(case, strict)
        deepest = int(Y.contig_rows(case.build, strict, case.nc, 64)[1].any(axis=0).nonzero()[0].max())
        assert above >= 0.5 and clamp > 0 and positive >= 0.25 and distinct >= min(3, deepest + 1), (name, above, clamp, positive, distinct)
        assert deepest >= Y.md_of(case), (name, deepest)
        ks.add(Y.k_of(case))
        if name.startswith("sweep") and case.nc not in (64, 1025):
            continue                                             # (the perturbations below: on a few of the fifteen sweep cases)
        hist, val = Y.hist_ref(case, strict), Y.quant_ref(case, strict)
        for exp, check, other in ((hist, H.assert_hist_equal, np.int32), (val.astype(np.int32), lambda g, e, w: Q.assert_quant_equal(g, e.astype(np.int64), w), np.int64)):
            check(exp.copy(), exp, name)
            n, m = exp.shape
            for d in (1, -1):
                for r, b in ((0, 0), (n // 2, m // 2), (n - 1, m - 1)):
                    bad = exp.copy()
                    bad[r, b] += d
                    with pytest.raises(AssertionError):
                        check(bad, exp, name)
            differ = np.flatnonzero((exp != exp[0]).any(axis=1))
            assert len(differ), name
            bad = exp.copy()
            bad[[0, differ[0]]] = bad[[differ[0], 0]]
            with pytest.raises(AssertionError):
                check(bad, exp, name)
            with pytest.raises(AssertionError):
                check(exp.astype(other), exp, name)
    assert ks == set(Q.KS), ks


@pytest.mark.parametrize("strict", MODES)
def test_cpu_properties_of_the_dictionary_and_alignment_generators(strict):
    ks = set()
    for nc in P.SWEEP:
        case = Y.sweep_case(nc, strict)
        base = X.sweep_case(nc)
        assert case.n == base.n + 2 * Y.PILE_PROBES == 40_008 and len(case.build[0]) == 30_000 + 2 * Y.PILE_DEPTH
        assert all(np.array_equal(a[:base.n], b) for a, b in zip(case.windows, base.windows))
        inside = P.inside(case.windows, nc)
        assert set(OUTSIDE(nc)) <= set(case.windows[0][~inside].tolist()), "every out-of-dictionary id among the probes"
        have = np.unique(case.build[0][P.inside(case.build, nc)])
        lacking = inside & ~np.isin(case.windows[0], have)
        assert nc <= 7 or lacking.sum() > 100, "probes on contigs the build lacks"
        L = H.positions(case.windows, strict, nc)
        hist, val = Y.hist_ref(case, strict), Y.quant_ref(case, strict)
        valid = (Y.ranks_of(case, strict) < L[:, None])
        assert not hist[~inside].any() and (val[~inside] == -1).all()
        assert (hist[lacking][:, 0] == L[lacking]).all() and not hist[lacking][:, 1:].any() and (val[lacking][valid[lacking]] == 0).all()
        bare, keep = Y.bare_case(case)
        assert keep.sum() == inside.sum() == bare.n
        ks.add(Y.k_of(case))
    assert ks == set(Q.KS), "K cycles over 1, 3 and 16 within the sweep"
    case = Y.sparse_case(strict)
    inside = P.inside(case.windows, case.nc)
    assert case.nc == P.SPARSE_NC == (1 << 24) + 1 and set(OUTSIDE(case.nc)) <= set(case.windows[0][~inside].tolist())
    have = np.unique(case.build[0][P.inside(case.build, case.nc)])
    assert (inside & ~np.isin(case.windows[0], have)).sum() > 100
    ids, rows = Y.contig_rows(case.build, strict, case.nc, 1)
    # (a contig whose only rows hold no position has a row but no block)
    assert 3000 < len(ids) <= len(have) and np.isin(ids, have).all() and rows[:, 1].all() and not rows[:, 0].any() and ids[0] == 0 and ids[-1] == case.nc - 1
    # the tiles: IVJ_HIST_LDS_KB = 128 moves k_depth_hist's tile at 683 bins and leaves it at the cap at 7
    assert H.HIST_LDS_BYTES == 64 << 10 and all(Y.lds_tile(md, H.HIST_LDS_BYTES) == H.tile(md) for md in (1, MD, 100, 682, H.MAX_HIST_DEPTH))
    tiles = {md: (H.tile(md), Y.lds_tile(md, 128 << 10)) for md in LDS_DEPTHS}
    assert tiles[6] == (H.HIST_MAX_TILE, H.HIST_MAX_TILE) and tiles[682] == (11, 23), tiles
    for md, k in A_PARAMS:
        a = Y.a_case(strict)
        assert a.n == 3 * DP.TILE + 17 + 4 + 16 * Y.PILE_PROBES and (~P.inside(a.windows, a.nc)).any()
        assert a.n > H.tile(md) and a.n > Q.tile(k) and a.n % H.tile(md) and a.n % Q.tile(k), "more than one tile, the last one partial"
        assert (a.n * (md + 1)) % 2 == (md + 1) % 2 and a.n % 2 == 1
    rid = J.probe_ids(a.n)
    assert len(np.unique(rid)) == a.n and rid.min() > a.n


@pytest.mark.parametrize("strict", MODES)
def test_cpu_block_counts_of_the_index_form_cases(strict):
    """C.  the blocks of the automatic case and of the 100 000-row case reach the automatic rule and take the balanced build as a
    side of their own; the forms' shapes keep the build they are named for"""
    auto = Y.auto_case(strict)
    nb = Y.n_blocks(auto.build, strict, auto.nc)
    assert len(auto.build[0]) == 140_000 + 2 * Y.PILE_DEPTH and auto.n == 20_000 + 2 * Y.PILE_PROBES and P.takes_balanced_build(auto.build, auto.nc)
    assert nb >= 250_000 > P.V3_AUTO_FROM and P.takes_balanced_build(Y.blocks_side(auto.build, strict, auto.nc), auto.nc), nb
    inner = Y.inner_auto_case(strict)
    nb = Y.n_blocks(inner.build, strict, inner.nc)
    assert len(inner.build[0]) == 100_000 + 2 * Y.PILE_DEPTH < P.V3_AUTO_FROM and 150_000 <= nb <= 150_040, nb
    assert nb >= P.V3_AUTO_FROM and P.takes_balanced_build(Y.blocks_side(inner.build, strict, inner.nc), inner.nc)
    for entry, vid in zip(X.v3_entries(), V3_IDS):
        case = Y.v3_case(entry, strict)
        assert P.takes_balanced_build(case.build, case.nc) == entry[4], vid
        own = case.note["own"]
        assert all(np.array_equal(a[:own], b) for a, b in zip(case.windows, entry[1])), vid
        assert (len(case.build[0]) == 1) == (vid == "one_row") and Y.md_of(case) == (1 if vid == "one_row" else MD)
    large, small = Y.sized_case(150_000, 900, strict), Y.sized_case(J.SMALL_ROWS, 901, strict)
    assert len(large.build[0]) == 150_000 + 2 * Y.PILE_DEPTH and len(small.build[0]) == 300 + 2 * Y.PILE_DEPTH
    seq = Y.sequence_case()
    assert all(np.array_equal(a, b) for a, b in zip(seq.windows + seq.build, P.sequence_case().probe + P.sequence_case().frame))


@pytest.mark.parametrize("strict", MODES)
def test_cpu_probe_edges_of_the_lattice_are_block_boundaries(strict):
    """T.  100 % of the starts and half-open ends of the aligned probes equal a block start and a block end in position space, 0 %
    of those moved by one; the probes of the one- and two-block contigs end and start just below, on and just above every
    boundary; every rank asked lies on a cumulative boundary of its row, one below or one above"""
    case = Y.t_case(strict)
    w = 0 if strict else 1
    kind = case.note["kind"]
    kc, ks, ke, kd = H.U.depth_events(*case.build, strict, case.nc)
    ke = ke + w
    assert 3000 <= len(case.build[0]) <= 8000 and 100 <= case.n <= 600 and len(kc) > 1700
    x = np.stack([case.windows[1].astype(np.int64), case.windows[2].astype(np.int64) + w], axis=1)
    hits = {0: [0, 0, 0], 1: [0, 0, 0], -1: [0, 0, 0]}
    for c in (0, 1):
        starts, ends = ks[kc == c], ke[kc == c]
        assert kd[kc == c].min() == 3 and kd[kc == c].max() == 7 and len(starts) == case.note["cells"], "a block per lattice cell"
        for d in hits:
            e = x[(case.windows[0] == c) & (kind == d)].reshape(-1)
            assert len(e) >= 40
            hits[d][0] += len(e)
            hits[d][1] += int(np.isin(e, starts).sum())
            hits[d][2] += int(np.isin(e, ends).sum())
        whole = x[(case.windows[0] == c) & (kind == 2)]
        assert whole.shape == (1, 2) and whole[0, 0] == starts.min() and whole[0, 1] == ends.max()
    assert hits[0][1] == hits[0][2] == hits[0][0] and hits[1][1:] == [0, 0] and hits[-1][1:] == [0, 0], hits
    for c, blocks in Y.T_BLOCKS.items():
        assert [(int(s), int(e), int(d)) for s, e, d in zip(ks[kc == c], ke[kc == c], kd[kc == c])] == blocks, "exactly these blocks"
        on = case.windows[0] == c
        for b in {v for s, e, _ in blocks for v in (s, e)}:
            for d in (-1, 0, 1):
                assert (x[on][:, 1] == b + d).any() and (x[on][:, 0] == b + d).any(), (c, b, d)
    # the ranks: cumulative boundaries of the unclamped histogram, one below and one above
    hist = H.block_form(case.windows, case.build, strict, case.nc, 64)
    L = H.positions(case.windows, strict, case.nc)
    ranks = Y.ranks_of(case, strict)
    assert ranks.shape == (case.n, 16) and Y.k_of(case) == 16 and not hist[:, 64].any()
    on_boundary = 0
    for r in np.flatnonzero(L > 0):
        cum = np.cumsum(hist[r])[hist[r] > 0][:5]               # (five boundaries x 3 = 15 of the 16 ranks)
        want = np.clip(np.concatenate([cum - 1, cum, cum + 1]), 0, L[r] - 1)
        assert np.isin(want, ranks[r]).all() and ((ranks[r] >= 0) & (ranks[r] < L[r])).all(), r
        on_boundary += int(np.isin(ranks[r], cum[cum < L[r]]).any())
    assert on_boundary >= case.n // 2, on_boundary             # (a probe that is one lattice cell, or lies in one block, holds one depth)
    above, clamp, positive, distinct = Y.bars(case, strict)
    assert above > 0.5 and clamp > 0 and positive > 0.25 and distinct >= 6


# ---- (B) --------------------------------------------------------------------------------------------------------------------------------

def _dictionary_checks(eng, dj, case, strict, contigs=True):
    got = Y.check_all(eng, dj, case, strict, contigs=contigs)
    ranks = Y.ranks_of(case, strict)
    inside = P.inside(case.windows, case.nc)
    have = np.unique(case.build[0][P.inside(case.build, case.nc)])
    lacking = inside & ~np.isin(case.windows[0], have)
    L = H.positions(case.windows, strict, case.nc)
    valid = (ranks >= 0) & (ranks < L[:, None])
    assert set(OUTSIDE(case.nc)) <= set(case.windows[0][~inside].tolist()) and (lacking.any() or case.nc <= 7)
    for entry in ("host_hist", "dev_hist"):
        g = got[entry]
        assert not g[~inside].any(), f"{case.name}: {entry}: a probe outside the dictionary has a non-zero bin"
        assert (g[lacking][:, 0] == L[lacking]).all() and not g[lacking][:, 1:].any(), f"{case.name}: {entry}: a contig without blocks is |Q| in bin 0"
    for entry in ("host_quant", "dev_quant"):
        g = got[entry]
        assert (g[~inside] == -1).all(), f"{case.name}: {entry}: a probe outside the dictionary answers"
        assert (g[lacking][valid[lacking]] == 0).all() and (g[lacking][~valid[lacking]] == -1).all(), f"{case.name}: {entry}: a contig without blocks"
    bare, keep = Y.bare_case(case)
    kept = np.ascontiguousarray(ranks[keep])
    assert Y.blob(Y.host_hist(eng, bare, strict)) == Y.blob(got["host_hist"][keep]), "with and without the outside rows: host hist"
    assert Y.blob(Y.dev_hist(dj, bare, strict)) == Y.blob(got["dev_hist"][keep]), "with and without the outside rows: device hist"
    assert Y.blob(Y.host_quant(eng, bare, strict, kept)) == Y.blob(got["host_quant"][keep]), "with and without the outside rows: host quantiles"
    assert Y.blob(Y.dev_quant(dj, bare, strict, kept)) == Y.blob(got["dev_quant"][keep]), "with and without the outside rows: device quantiles"
    if contigs:
        assert Y.blob(Y.host_contigs(eng, bare, strict)) == Y.blob(got["host_contigs"]) == Y.blob(got["dev_contigs"])
    for pm in (0, 1, 2):
        what = f"{case.name}: partition_mode {pm}"
        assert Y.blob(Y.host_hist(eng, case, strict, partition_mode=pm)) == Y.blob(got["host_hist"]), what
        assert Y.blob(Y.host_quant(eng, case, strict, partition_mode=pm)) == Y.blob(got["host_quant"]), what
        assert Y.blob(Y.dev_hist(dj, case, strict, partition_mode=pm)) == Y.blob(got["dev_hist"]), what
        assert Y.blob(Y.dev_quant(dj, case, strict, partition_mode=pm)) == Y.blob(got["dev_quant"]), what
    assert Y.blob(got["host_hist"]) == Y.blob(got["dev_hist"]) and Y.blob(got["host_quant"]) == Y.blob(got["dev_quant"])


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("nc", P.SWEEP)
def test_across_dictionary_sizes(eng, dj, nc, strict):
    """B.  cmeta_j[2 c] per probe from LDS (LM) or from memory; k_depth_hist_contigs' LDS histogram for the tile's first contig and
    global atomics for the others (from a few hundred contigs on most tiles hold several); every id outside the dictionary;
    contigs the build lacks"""
    _dictionary_checks(eng, dj, Y.sweep_case(nc, strict), strict)


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_on_a_sparse_dictionary_of_2_24_plus_1_ids(eng, dj, strict):
    """B.  the region form and the quantiles as in the sweep; the contig form at max_depth 1 only (2^24 + 1 rows x 2 bins x 8 bytes
    = 256 MiB), compared through its non-zero rows, every other row zero"""
    case = Y.sparse_case(strict)
    _dictionary_checks(eng, dj, case, strict, contigs=False)
    ids, rows = Y.contig_rows(case.build, strict, case.nc, 1)
    for entry, got in (("host", Y.host_contigs(eng, case, strict, md=1)), ("device", Y.dev_contigs(dj, case, strict, md=1))):
        assert got.dtype == np.int64 and got.shape == (case.nc, 2), entry
        H.assert_hist_equal(got[ids], rows, f"{entry} entry: the rows of the contigs that hold a block")
        assert np.count_nonzero(got.any(axis=1)) == len(ids), f"{entry} entry: a contig without a block has a non-zero bin"
        del got


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("nc", [24, 257])
@pytest.mark.parametrize("knob", ["IVJ_COUNT_NOLDS", "IVJ_JOINT_BINS"])
def test_under_the_joint_grid_knobs(knob, nc, strict, monkeypatch):
    """B.  the per-contig grid metadata read from memory, and one bin per row instead of two: the grid of the blocks' index that
    dh_range reads"""
    case = Y.deepened(X.sweep_case(nc), strict)
    e, d, done = _engines_under(monkeypatch, {knob: "1"})
    try:
        Y.check_all(e, d, case, strict, what=f"{case.name} under {knob}=1")
    finally:
        done()


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("md", LDS_DEPTHS)
def test_the_lds_budget_knob_changes_the_tile_and_nothing_else(eng, dj, md, strict, monkeypatch):
    """B.  IVJ_HIST_LDS_KB=128: P of k_depth_hist goes from 11 to 23 rows at 683 bins (other rows share a workgroup, other tiles
    start on an odd 8-byte word) and stays 512 at 7: byte-identical to the default"""
    case = Y.a_case(strict)
    exp = Y.hist_ref(case, strict, md)
    base_host, base_dev = Y.host_hist(eng, case, strict, md), Y.dev_hist(dj, case, strict, md)
    H.assert_hist_equal(base_host, exp, "default budget: host entry")
    H.assert_hist_equal(base_dev, exp, "default budget: device entry")
    assert (Y.lds_tile(md, 128 << 10) != H.tile(md)) == (md == 682)
    e, d, done = _engines_under(monkeypatch, {"IVJ_HIST_LDS_KB": "128"})
    try:
        assert Y.blob(Y.host_hist(e, case, strict, md)) == Y.blob(base_host), "128 KiB: host entry"
        assert Y.blob(Y.dev_hist(d, case, strict, md)) == Y.blob(base_dev) == Y.blob(base_host), "128 KiB: device entry"
    finally:
        done()


# ---- (C) --------------------------------------------------------------------------------------------------------------------------------

def _on_a_built_index(d, case, strict):
    """(results of the three device entries on one index built without the end order, names of the build, names per entry)"""
    ix, built = _names_of(d.engine, lambda: d.build_index(J.dev_side(case.build), strict, case.nc))
    try:
        hist, th = _names_of(d.engine, lambda: Y.dev_hist(d, case, strict, index=ix))
        quant, tq = _names_of(d.engine, lambda: Y.dev_quant(d, case, strict, index=ix))
        contigs, tc = _names_of(d.engine, lambda: Y.dev_contigs(d, case, strict, index=ix))
    finally:
        ix.close()
    return {"dev_hist": hist, "dev_quant": quant, "dev_contigs": contigs}, built, {"dev_hist": th, "dev_quant": tq, "dev_contigs": tc}


def _on_the_host(e, case, strict):
    hist, th = _names_of(e, lambda: Y.host_hist(e, case, strict))
    quant, tq = _names_of(e, lambda: Y.host_quant(e, case, strict))
    contigs, tc = _names_of(e, lambda: Y.host_contigs(e, case, strict))
    return {"host_hist": hist, "host_quant": quant, "host_contigs": contigs}, {"host_hist": th, "host_quant": tq, "host_contigs": tc}


def _assert_results(got, case, strict, what):
    for key, g in got.items():
        if key.endswith("_hist"):
            H.assert_hist_equal(g, Y.hist_ref(case, strict), f"{what}: {key}")
        elif key.endswith("_quant"):
            Q.assert_quant_equal(g, Y.quant_ref(case, strict), f"{what}: {key}")
        else:
            H.assert_hist_equal(g, Y.contig_ref(case, strict), f"{what}: {key}")


def _assert_kernels(names):
    for key, t in names.items():
        want = {"hist": "depth_hist", "quant": "depth_quant", "contigs": "depth_hist_contigs"}[key.split("_", 1)[1]]
        assert want in t, (key, t)


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shape", range(X.V3_SHAPES), ids=V3_IDS)
def test_index_build_forms(shape, strict, monkeypatch):
    """C.  dh_range reads the joint grid, b_start and e_end of the BLOCKS' index, which index_build makes under the same knobs as
    the caller's; depth_core reads the caller's index as its build form left it.  The caller's index is built in a call of its
    own on the device side, so that its kernel names are exact (_assert_build); the blocks' index may take either build."""
    entry = X.v3_entries()[shape]
    case, balanced = Y.v3_case(entry, strict), entry[4]
    blobs = []
    for form in P.FORMS:
        e, d, done = _engines_under(monkeypatch, form)
        try:
            e.enable_timing(2)
            d.engine.enable_timing(2)
            what = f"{case.name} under {form}"
            host, th = _on_the_host(e, case, strict)
            dev, built, td = _on_a_built_index(d, case, strict)
            _assert_results({**host, **dev}, case, strict, what)
            _assert_kernels({**th, **td})
            _assert_build(built, form, balanced, what)
            blobs.append(tuple(Y.blob(g) for _, g in sorted({**host, **dev}.items())))
        finally:
            done()
    assert all(b == blobs[0] for b in blobs), "byte-identical results under every index build form"
    assert blobs[0][0] == blobs[0][3] and blobs[0][1] == blobs[0][4] and blobs[0][2] == blobs[0][5], "host and device entries differ"


def _fresh_pair():
    from polars_bio_amd.device_api import DeviceJoin
    e, d = _engine.Engine(0), DeviceJoin(0)
    e.enable_timing(2)
    d.engine.enable_timing(2)
    return e, d


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_automatic_balanced_build_of_the_blocks_at_140k_rows(strict):
    """C.  no knob: 140 000 build rows make 258 000 blocks; on an index built beforehand the only index a call builds is the
    blocks', and it takes the balanced build by the automatic rule (ix3_local among the names of the hist and of the quant call)"""
    case = Y.auto_case(strict)
    e, d = _fresh_pair()
    try:
        host, th = _on_the_host(e, case, strict)
        dev, built, td = _on_a_built_index(d, case, strict)
        _assert_results({**host, **dev}, case, strict, case.name)
        _assert_kernels({**th, **td})
        assert "ix3_local" in built and "ix_final" not in built, built
        for key in ("dev_hist", "dev_quant"):
            assert "ix3_local" in td[key] and "ix_final" not in td[key], (key, td[key])
        assert "ix3_local" not in td["dev_contigs"] and "ix_final" not in td["dev_contigs"], "the contig form builds no index"
        for key in ("host_hist", "host_quant"):
            assert "ix3_local" in th[key], (key, th[key])
    finally:
        e.close()
        d.engine.close()


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_blocks_above_the_automatic_rule_under_a_build_side_below_it(strict):
    """C.  100 018 build rows (the LSD sort: ix_final) whose 150 016 blocks take the balanced build (ix3_local) within the one call:
    the host entries and the device entries that build their own index show both names; on an index built beforehand the names
    tell the two builds apart -- ix_final and no ix3_local for the caller's index, ix3_local and no ix_final in the calls"""
    case = Y.inner_auto_case(strict)
    e, d = _fresh_pair()
    try:
        host, th = _on_the_host(e, case, strict)
        dev, built, td = _on_a_built_index(d, case, strict)
        own = {}
        own["dev_hist"], t_own_h = _names_of(d.engine, lambda: Y.dev_hist(d, case, strict))
        own["dev_quant"], t_own_q = _names_of(d.engine, lambda: Y.dev_quant(d, case, strict))
        _assert_results({**host, **dev}, case, strict, case.name)
        _assert_results(own, case, strict, case.name + ": own index")
        _assert_kernels({**th, **td})
        assert "ix_final" in built and "ix3_local" not in built, built
        for key in ("dev_hist", "dev_quant"):
            assert "ix3_local" in td[key] and "ix_final" not in td[key], (key, td[key])
        for t in (th["host_hist"], th["host_quant"], t_own_h, t_own_q):
            assert "ix_final" in t and "ix3_local" in t, t
    finally:
        e.close()
        d.engine.close()


# ---- (T) --------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("strict", MODES)
def test_probe_edges_on_block_boundaries(eng, dj, strict):
    """T.  every start and end a block start and a block end (he / hs of dh_range on a key of the grid, the two edge clips of
    length 0 avoided by the exact range), one position below and above, one probe over a whole contig; contigs of one and of two
    blocks; 16 ranks per row on, one below and one above the row's cumulative boundaries"""
    case = Y.t_case(strict)
    got = Y.check_all(eng, dj, case, strict)
    assert Y.blob(got["host_hist"]) == Y.blob(got["dev_hist"]) and Y.blob(got["host_quant"]) == Y.blob(got["dev_quant"])


# ---- (D) --------------------------------------------------------------------------------------------------------------------------------

ORDERS = [("hist", "count", "quant", "bases", "hist_contigs", "summary", "profile"),
          ("quant", "profile", "hist", "summary", "count", "hist_contigs", "bases"),
          ("count", "bases", "hist_contigs", "quant", "summary", "profile", "hist"),
          ("summary", "hist", "profile", "hist", "bases", "count", "hist_contigs", "quant"),
          ("profile", "quant", "hist_contigs", "quant", "count", "summary", "bases", "hist")]


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("order", ORDERS, ids=["-".join(o) for o in ORDERS])
def test_calls_on_one_index_in_any_order(dj, order, strict):
    """D.  one DeviceIndex built without the end order: depth_core completes it for whichever call comes first, every hist / quant
    call builds the blocks' index, re-reserves the arena behind it and releases everything -- hist and quant in first, middle and
    last position, and twice: every result equals its reference whatever ran before it"""
    import torch
    base, exp = P.sequence_case(), _sequence_reference(strict)
    case = Y.sequence_case()
    nc, n = case.nc, case.n
    probe, frame = J.dev_side(base.probe), J.dev_side(base.frame)
    ix = dj.engine.index_build_dev(frame.as_c(), _engine.make_opts(strict, nc), False)
    try:
        for step, call in enumerate(order):
            what = f"step {step} ({call}) of {order}"
            if call == "hist":
                H.assert_hist_equal(Y.dev_hist(dj, case, strict, index=ix), Y.hist_ref(case, strict), what)
            elif call == "quant":
                Q.assert_quant_equal(Y.dev_quant(dj, case, strict, index=ix), Y.quant_ref(case, strict), what)
            elif call == "hist_contigs":
                H.assert_hist_equal(Y.dev_contigs(dj, case, strict, index=ix), Y.contig_ref(case, strict), what)
            elif call == "profile":
                DP.assert_profile_equal(X.run_dev(dj, case, strict, X.BINS, None, index=ix), X.reference_once(case, strict, X.BINS, None), what)
            elif call == "count":
                assert (dj.count_overlaps(probe, frame, strict, nc, index=ix).cpu().numpy() == exp["count"]).all(), what
            elif call == "bases":
                out = torch.full((n,), -7, dtype=torch.int64, device="cuda")
                dj.overlap_bases(probe, frame, strict, nc, index=ix, out=out)
                DS.assert_bases_equal(out.cpu().numpy(), exp["bases"], what)
            else:
                md, bg = dj.depth_summary(probe, frame, strict, nc, P.THRESHOLDS, index=ix)
                DQ.assert_summary_equal((md.cpu().numpy(), bg.cpu().numpy()), exp["summary"], what)
    finally:
        ix.close()


# (the call, large or small input, Strict)
ALTERNATION = [("bases", True, True), ("hist", True, True), ("quant", False, False), ("summary", False, False), ("quant", True, False),
               ("hist", False, True), ("bases", False, False), ("hist", True, False), ("quant", False, True), ("summary", True, True)]


@gpu
def test_one_context_under_alternating_large_and_small_inputs(monkeypatch):
    """D.  150 000 and 300 build rows in turn on ONE engine and ONE DeviceJoin, hist and quant between overlap_bases and
    depth_summary: the recycled index slab (the caller's index and the blocks' index trade it) and the arena are larger than the
    next call needs.  Every result equals the reference, and every hist / quant result what a fresh engine returns."""
    from polars_bio_amd.device_api import DeviceJoin
    e, d = _engine.Engine(0), DeviceJoin(0)
    try:
        for step, (op, large, strict) in enumerate(ALTERNATION):
            size, seed = (150_000, 900) if large else (J.SMALL_ROWS, 901)
            what = f"step {step}: {op} on {size} rows, strict={strict}"
            if op in ("bases", "summary"):
                base = P.sized_case(size, seed)
                P.check(P.run(e, base, strict, only=(op,)), P.expected(base, strict, only=(op,)), what)
                continue
            case = Y.sized_case(size, seed, strict)
            fresh = _fresh(monkeypatch)
            try:
                if op == "hist":
                    host, dev, ref = Y.host_hist(e, case, strict), Y.dev_hist(d, case, strict), Y.host_hist(fresh, case, strict)
                    H.assert_hist_equal(host, Y.hist_ref(case, strict), what + ": host entry")
                    H.assert_hist_equal(dev, Y.hist_ref(case, strict), what + ": device entry")
                    hc, dc = Y.host_contigs(e, case, strict), Y.dev_contigs(d, case, strict)
                    H.assert_hist_equal(hc, Y.contig_ref(case, strict), what + ": contig form, host entry")
                    assert Y.blob(hc) == Y.blob(dc) == Y.blob(Y.host_contigs(fresh, case, strict)), what + ": contig form vs a fresh engine"
                else:
                    host, dev, ref = Y.host_quant(e, case, strict), Y.dev_quant(d, case, strict), Y.host_quant(fresh, case, strict)
                    Q.assert_quant_equal(host, Y.quant_ref(case, strict), what + ": host entry")
                    Q.assert_quant_equal(dev, Y.quant_ref(case, strict), what + ": device entry")
                assert Y.blob(host) == Y.blob(dev) == Y.blob(ref), what + " vs a fresh engine"
            finally:
                fresh.close()
    finally:
        e.close()
        d.engine.close()


# ---- (A) --------------------------------------------------------------------------------------------------------------------------------

def _assert_between_sentinels(whole, at, count, pad, what):
    fill = Y.sentinel_of(whole.dtype)
    assert (whole[:at] == fill).all() and (whole[at + count:] == fill).all(), what + ": a sentinel was overwritten"
    assert len(whole) - at - count == pad


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("md,k", A_PARAMS, ids=[f"d{md}_k{k}" for md, k in A_PARAMS])
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_unaligned_columns_ranks_and_outputs_between_sentinels(dj, shift, md, k, strict):
    """A.  the probe columns `shift` int32 elements into larger tensors (4-byte aligned, not 16), the ranks from an odd int64 element,
    the quantiles an (n, K) view from int32 element `shift`, the histograms (n, D + 1) and (n_contigs, D + 1) views from an odd
    int64 element of sentinel-filled tensors (the head / pairs / tail stores of k_depth_hist with cnt - head odd and even); the
    probes carry a row_id and the index is built from a side with row ids -- neither is read.  Byte-identical to the aligned
    run; every sentinel around the outputs is intact."""
    case = Y.a_case(strict)
    ranks = Y.ranks_of(case, strict, k)
    assert ranks.shape == (case.n, k)
    base_h, base_q, base_c = Y.dev_hist(dj, case, strict, md), Y.dev_quant(dj, case, strict, ranks), Y.dev_contigs(dj, case, strict, md)
    H.assert_hist_equal(base_h, Y.hist_ref(case, strict, md), "aligned, no row ids: hist")
    Q.assert_quant_equal(base_q, Y.quant_ref(case, strict, k), "aligned, no row ids: quantiles")
    H.assert_hist_equal(base_c, Y.contig_ref(case, strict, md), "aligned, no row ids: contig form")
    bid, _ = J.build_ids(len(case.build[0]))
    pid = J.probe_ids(case.n)
    ix = dj.build_index(J.dev_side(case.build, bid, shift), strict, case.nc)
    try:
        off = 2 * shift + 1
        kw = dict(index=ix, shift=shift, build_row_id=bid, whole=True)
        got_h, whole_h, at_h = Y.dev_hist(dj, case, strict, md, probe_row_id=pid, out_offset=off, **kw)
        got_q, whole_q, at_q = Y.dev_quant(dj, case, strict, ranks, probe_row_id=pid, rank_offset=2 * shift - 1, out_offset=shift, **kw)
        got_c, whole_c, at_c = Y.dev_contigs(dj, case, strict, md, out_offset=off, **kw)
    finally:
        ix.close()
    assert at_h == at_c == off and off % 2 == 1 and at_q == shift
    assert Y.blob(got_h) == Y.blob(base_h) and Y.blob(got_q) == Y.blob(base_q) and Y.blob(got_c) == Y.blob(base_c), f"shift {shift}"
    _assert_between_sentinels(whole_h, at_h, case.n * (md + 1), 5, "hist")
    _assert_between_sentinels(whole_q, at_q, case.n * k, 5, "quantiles")
    _assert_between_sentinels(whole_c, at_c, case.nc * (md + 1), 5, "contig form")
    assert not (got_h == Y.SENTINEL).any() and not (got_q == Y.SENTINEL32).any() and not (got_c == Y.SENTINEL).any()
