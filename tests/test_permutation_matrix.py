"""permutation_test (k_perm_zmark / k_permute / k_permute_fold, host_permute.hip.h and the two C entries) put through the project's
cross-cutting matrices, which tests/test_permutation_gpu.py -- built around the kernel's tile, block and chunk -- leaves out:

  (Z) the prefix arrays of the df2 rows without a position: 30 - 50 % such rows, placed so that zs and ze differ by more than 100 at
      many positions, df2 sizes around device_scan's tile, and a single such row at either end of the start order;
  (O) df2 rows across either end of the contig, across both, entirely outside it and at the int32 limits;
  (R) deep and wide rank searches: thousands of rows in one bin at the end of a contig's segment, a grid wider than 2^16 per bin,
      contigs of one row and of two identical rows;
  (A) df1 with a row_id, an index built from a side with row ids, columns and tables that are not 16-byte aligned, outputs between
      sentinels, every partition_mode;
  (B) contig-dictionary sizes on both sides of every layout threshold, the IVJ_COUNT_NOLDS / IVJ_JOINT_BINS table forms, the sparse
      dictionary of 2^24 + 1 ids (three offset pieces on the host entry), and an uneven two-piece case (63 + 7 permutations);
  (C) the df1 sort through the index build forms: the automatic balanced build and the hand-over at 140 000 rows;
  (D) call sequences on one long-lived index, a pending count -> fill hand-over across one permute call, one context under
      alternating large and small inputs;
  (P) 4097 tiles: the partials of one launch reach PERM_PARTIAL_BYTES and a launch takes 960 permutations, not PERM_CHUNK;
  (CPU) the rank identity equals the literal brute force on a scaled-down copy of every generator, the generators have the
      properties the GPU tests rely on, and the comparisons are not blind.

Every comparison is exact (int64 equality per permutation, both statistics); no tolerance appears anywhere."""
import numpy as np
import pytest

import _join_ops_util as J
import _limits
import _map_select_util as S
import _permutation_matrix_util as M
import _permutation_util as U
import _position_ops_util as P
import _thresholds_util as T
from polars_bio_amd import _engine
from test_contig_dictionaries import OUTSIDE
from test_join_ops_matrix import _engines_under, _names_of, _assert_build

gpu = pytest.mark.gpu
I32 = np.int32
MODES = [pytest.param(True, id="strict"), pytest.param(False, id="weak")]
TILE, BLOCK, CHUNK = M.TILE, M.BLOCK, M.CHUNK
SCAN = M.scan_tile()
MAXI = M.MAXI
Z_SIZES = [SCAN - 2, SCAN - 1, SCAN, 2 * SCAN, 50_000]            # df2 rows n: the scans run over n + 1 entries
O_CASES = {"small": dict(L=77, n=TILE + 9, m=120, width=300, bwidth=200),
           "medium": dict(L=300_000, n=2 * TILE + 5, m=3000, width=40_000, bwidth=20_000),
           "large": dict(L=MAXI, n=TILE + 9, m=1500, width=2 ** 30, bwidth=2 ** 28)}
KERNELS = ("permute_overlaps", "permute_fold", "permute_zmark", "permute_zscan")
FLAT_TABLES = {"bins_records", "lot_mark", "lot_scan", "rec4", "tab2"}     # launches of build_flat: the df2 index build under partition_mode 5 only


@pytest.fixture(scope="module")
def eng():
    return _engine.Engine(0)


@pytest.fixture(scope="module")
def dj():
    import torch  # noqa: F401
    from polars_bio_amd.device_api import DeviceJoin
    return DeviceJoin(0)


# ---- (CPU) ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strict", MODES)
def test_cpu_rank_identity_equals_the_brute_force_on_every_generator(strict):
    seen = dict(pairs=0, wraps=0, no_position=0, below_zero=0, beyond_l=0, ineligible=0)
    for name, make in M.SCALED.items():
        case = make(strict)
        n = len(case.probe[0])
        assert n * len(case.off) <= M.BRUTE_MAX and n <= 1000 and len(case.off) <= 8, name
        lit = U.expected(*case.args[:3], strict, case.lengths, case.off)
        fast = U.ranks(*case.args[:3], strict, case.lengths, case.off)
        M.assert_stats(fast, lit, name)
        assert lit[0].sum() > 0, name
        one = 0 if strict else 1
        ok = M.eligible(case.probe, case.nc, strict, case.lengths)
        for i in range(0, n, 7):                             # the vectorised eligibility is pieces_of's
            assert bool(ok[i]) == bool(U.pieces_of(case.probe[0][i], case.probe[1][i], case.probe[2][i], case.nc, strict, case.lengths, case.off[-1])), (name, i)
        inside = P.inside(case.build, case.nc)
        bl = case.lengths.astype(np.int64)[np.clip(case.build[0], 0, case.nc - 1)]
        seen["pairs"] += int(lit[0].sum())
        seen["no_position"] += int(M.no_position(case.build, strict).sum())
        seen["below_zero"] += int((inside & (case.build[1].astype(np.int64) - one < 0)).sum())
        seen["beyond_l"] += int((inside & (case.build[2] > bl)).sum())
        seen["ineligible"] += int((~ok).sum())
        seen["wraps"] += sum(len(U.pieces_of(case.probe[0][i], case.probe[1][i], case.probe[2][i], case.nc, strict, case.lengths, o)) == 2
                             for i in range(0, n, 5) for o in case.off)
    assert all(v > 50 for v in seen.values()), seen


@pytest.mark.parametrize("strict", MODES)
def test_cpu_rows_on_a_contig_df2_lacks_contribute_nothing(strict):
    """P's reference takes the hot rows only: on the scaled-down copy (TILE -> 40 rows) the brute force over ALL rows equals it"""
    case = M.SCALED["p"](strict)
    hot = M.hot_rows(case)
    assert len(hot[0]) == 30 and len(case.probe[0]) == 8 * 40 + 6 and not (case.build[0] == 1).any()
    lit = U.expected(*case.args[:3], strict, case.lengths, case.off)
    M.assert_stats(U.ranks(hot, case.build, case.nc, strict, case.lengths, case.off), lit, "hot rows only")
    assert lit[0].sum() > 0


@pytest.mark.parametrize("strict", MODES)
def test_cpu_the_comparisons_are_not_blind(strict):
    for name, make in M.SCALED.items():
        case = make(strict)
        exp = M.reference_once(case, strict)
        M.assert_stats((exp[0].copy(), exp[1].copy()), exp, name)
        for k in range(2):
            for p in (0, len(case.off) - 1):
                bad = [exp[0].copy(), exp[1].copy()]
                bad[k][p] += 1
                with pytest.raises(AssertionError):
                    M.assert_stats(bad, exp, name)
        with pytest.raises(AssertionError):
            M.assert_stats((exp[0].astype(np.int32), exp[1]), exp, name)
        assert M.blob(exp) != M.blob((exp[1], exp[0])) or (exp[0] == exp[1]).all()


def _z_gap(case, strict):
    zs, ze, nop_by_start = M.z_prefixes(case.build, strict)
    return np.abs(zs - ze), zs, ze, nop_by_start


@pytest.mark.parametrize("strict", MODES)
def test_cpu_properties_of_the_z_o_and_r_generators(strict):
    one = 0 if strict else 1
    for m in Z_SIZES:
        case = M.z_case(strict, m)
        bc, bs, be = (a.astype(np.int64) for a in case.build)
        nop = M.no_position(case.build, strict)
        assert len(bc) == m and 0.3 <= nop.mean() <= 0.5 and len(case.probe[0]) == 2 * TILE + 3 and len(case.off) == 9 and case.nc == 4
        d = bs[nop] - one - be[nop]                          # half-open start - end: 0 (start == end; closed: end == start - 1) or more
        assert 0.4 < (d == 0).mean() < 0.6 and (d >= 0).all()
        assert not nop[bc == 1].any() and nop[(bc == 0) & (bs < 20_100)].sum() > m // 8 and nop[(bc == 3) & (bs > 85_000)].sum() > m // 8
        assert not nop[(bc == 0) & (bs > 20_100)].any() and not nop[(bc == 3) & (bs < 85_000)].any() and not nop[bc == 2].any()
        gap = _z_gap(case, strict)[0]
        assert (gap > 100).sum() > (m + 1) // 20, (m, int((gap > 100).sum()))
    for which in ("last", "first"):
        case = M.z_edge_case(strict, which)
        _, zs, ze, by_start = _z_gap(case, strict)
        n = len(case.build[0])
        assert by_start.sum() == 1 and by_start[n - 1 if which == "last" else 0] and zs[n] == 1 and ze[n] == 1
        assert zs[n - 1] == (0 if which == "last" else 1) and zs[0] == 0 and zs[1] == (0 if which == "last" else 1)
    for key, kw in O_CASES.items():
        case = M.o_case(strict, **kw)
        L = kw["L"]
        on0 = case.build[0] == 0
        hs, he = case.build[1].astype(np.int64)[on0] - one, case.build[2].astype(np.int64)[on0]
        assert ((hs < 0) & (he > 0) & (he < L)).any() and ((hs < 0) & (he >= L)).any() and ((he <= 0) & (hs < he)).any(), key
        if L < MAXI:
            assert ((hs > 0) & (hs < L) & (he > L)).any() and ((hs < 0) & (he > L)).any() and ((hs >= L) & (hs < he)).any(), key
        assert (case.build[1] == _limits.MIN).any() and (case.build[2] == _limits.MAX).any() and (case.build[1] == _limits.MAX).any(), key
        assert case.off[0].tolist() == [0, 0] and case.off[1, 0] == 1 % L and case.off[2].tolist() == [L - 1, 999]
        i, p = case.note["ends_at_L"]
        assert U.pieces_of(0, case.probe[1][i], case.probe[2][i], 2, strict, case.lengths, case.off[p])[-1][1] == L
        assert len(U.pieces_of(0, case.probe[1][i], case.probe[2][i], 2, strict, case.lengths, case.off[p])) == 1
        j, p = case.note["second_piece_0_1"]
        two = U.pieces_of(0, case.probe[1][j], case.probe[2][j], 2, strict, case.lengths, case.off[p])
        assert len(two) == 2 and two[0][1] == L and two[1] == (0, 1), (key, two)
        ok = M.eligible(case.probe, 2, strict, case.lengths)
        assert 3 <= (~ok).sum() <= 8, "only the ineligible kinds _frames plants"
        exp = M.reference_once(case, strict)
        assert exp[0].min() > 0 and len(set(exp[0].tolist())) > 3, key
    # R1: the clusters end their orders on contig 0, contig 1 follows with smaller coordinates, targets fall just above the clusters
    case = M.r1_case(strict)
    bc, bs, be = (a.astype(np.int64) for a in case.build)
    on0 = bc == 0
    assert (bs[on0] - one == M.R1_X).sum() == 3000 and bs[on0].max() - one == M.R1_X and (be[on0] == M.R1_Y).sum() == 3000
    # (the end order of contig 0 closes with the 3000 rows at Y and ONE row at L, which lifts the grid's upper edge above the targets)
    assert (be[on0] > M.R1_Y).sum() == 1 and be[on0].max() == M.R1_L > M.R1_Y + 17 + 16
    assert bs[bc == 1].max() < M.R1_X and be[bc == 1].max() < M.R1_Y and (bc == 1).sum() == 200 and case.lengths[0] == 200_000
    pc, ps, pe = (a.astype(np.int64) for a in case.probe)
    assert 700 <= len(pc) <= 1100 and len(case.off) == 8 and not case.off[0].any()
    assert ((pc == 0) & (pe > M.R1_X) & (pe <= M.R1_X + 16)).sum() > 50 and ((pc == 0) & (ps - one >= M.R1_Y) & (ps - one <= M.R1_Y + 16)).sum() > 50
    shift = M.contig_shift(case.build, 0)
    assert shift <= 16
    # ... in the clusters' own bins and above their keys (zero offsets, permutation 0): te = end (+ 1 closed) against the starts,
    # ts = half-open start + 1 against the ends, bins counted from the grid's lower edge
    ulo = min(bs[on0].min(), be[on0].min())
    same_bin = lambda t, key: ((t - ulo) >> shift == (key - ulo) >> shift) & (t > key)       # noqa: E731
    assert (same_bin(pe[pc == 0] + one, M.R1_X + one)).sum() >= 5 and (same_bin(ps[pc == 0] - one + 1, M.R1_Y)).sum() >= 5
    # R2: the grid of contig 1 is wider than 2^16 per bin; targets below, inside and above the window and in the empty bins
    case = M.r2_case(strict)
    shift = M.contig_shift(case.build, 1)
    assert shift > 16 and case.lengths[1] == MAXI and 700 <= len(case.probe[0]) <= 1100 and len(case.off) == 8
    bc, bs, be = (a.astype(np.int64) for a in case.build)
    on1 = bc == 1
    inwin = on1 & (bs - one >= M.R2_MID - 500) & (be <= M.R2_MID + 500)
    assert inwin.sum() == 5000 and on1.sum() == 5002 and (on1 & (be < 100)).sum() == 1 and (on1 & (bs > MAXI - 100)).sum() == 1
    assert (bc == 0).sum() > 100 and (bc == 2).sum() > 100
    pc, ps, pe = (a.astype(np.int64) for a in case.probe)
    lo, hi, width = M.R2_MID - 500, M.R2_MID + 500, 1 << shift
    s1 = (ps[pc == 1][None, :] - one + case.off[:, 1].astype(np.int64)[:, None]) % MAXI
    for what, sel in (("below", (s1 < lo) & (s1 > lo - 3000)), ("inside", (s1 >= lo) & (s1 < hi)), ("above", (s1 >= hi) & (s1 < hi + 3000)),
                      ("empty bins below", (s1 < lo - width) & (s1 > lo - 3 * width)), ("empty bins above", (s1 > hi + width) & (s1 < hi + 3 * width)),
                      ("at the last row", s1 > MAXI - 60), ("at the first row", s1 < 30)):
        assert sel.sum() >= 20, (what, int(sel.sum()))
    case = M.r3_case(strict)
    counts = np.bincount(case.build[0], minlength=3)
    assert counts[0] == 1 and counts[1] == 2 and counts[2] > 100 and 700 <= len(case.probe[0]) <= 1100 and len(case.off) == 8
    two = np.flatnonzero(case.build[0] == 1)
    assert all(case.build[k][two[0]] == case.build[k][two[1]] for k in range(3))
    for case in (M.r1_case(strict), M.r2_case(strict), M.r3_case(strict)):
        exp = M.reference_once(case, strict)
        assert exp[0].min() > 0 and len(set(exp[0].tolist())) > 4, case.name


@pytest.mark.parametrize("strict", MODES)
def test_cpu_properties_of_the_matrix_generators(strict):
    n = 3 * TILE + 17
    rid = J.probe_ids(n)
    assert len(np.unique(rid)) == n and rid.min() > n
    case = M.a_case(strict)
    assert len(case.probe[0]) == n and (~M.eligible(case.probe, case.nc, strict, case.lengths)).sum() >= 6
    for nc in P.SWEEP + [24]:
        case = M.sweep_case(strict, nc)
        for side in (case.probe, case.build):
            assert set(OUTSIDE(nc)) <= set(side[0].tolist()), "every out-of-dictionary id on both sides"
        share = 1.0 - M.eligible(case.probe, nc, strict, case.lengths).mean()
        assert 0.02 <= share <= 0.30, (nc, share)
        assert M.reference_once(case, strict)[0].min() > 0
    case = M.sparse_case(strict)
    assert case.nc == P.SPARSE_NC == (1 << 24) + 1 and len(case.off) == 3 and M.piece_rows(case.nc, 3) == 1
    exp = M.reference_once(case, strict)
    assert len(set(exp[0].tolist())) == 3 and len(set(exp[1].tolist())) == 3 and exp[0].min() > 0, exp
    case = M.pieces_case(strict)
    assert case.nc == 262_145 and len(case.off) == 70 and M.piece_rows(case.nc, 70) == 63
    assert 2000 <= len(case.probe[0]) <= 5000 and 100 < len(np.unique(case.build[0])) < 500
    exp = M.reference_once(case, strict)
    assert len(set(exp[0].tolist())) > 35
    case = M.auto_case(strict)
    assert len(case.probe[0]) == 140_000 >= P.V3_AUTO_FROM and P.takes_balanced_build(case.probe, case.nc) and len(case.build[0]) == 20_000 and len(case.off) == 4
    case = M.handover_case(strict)
    span, fullest = P.v3_geometry(case.probe, case.nc)
    assert len(case.probe[0]) == 140_000 and span <= 0xffffffff and fullest > P.V3_CAP and len(case.off) == 4
    assert [r[0] for r in J.D3_ROUNDS] == [150_000, 300, 150_000, 300, 150_000]
    # P: 4097 tiles, 960 permutations per launch, the hot rows in the first and the last tiles of the (contig, start) order
    n, n_perm = 4096 * TILE + 1 + 500, 961
    per = M.partial_bytes() // (((n + TILE - 1) // TILE) * 16) // BLOCK * BLOCK
    assert (n + TILE - 1) // TILE == 4097 and per == 960 == M.per_launch(n, n_perm) < CHUNK and M.per_launch(4096 * TILE, n_perm) == min(CHUNK, n_perm)
    case = M.p_case(strict)
    pc = case.probe[0]
    assert len(pc) == n and len(case.off) == n_perm and not (case.build[0] == 1).any()
    k0, k2 = int((pc == 0).sum()), int((pc == 2).sum())      # (contig, start) order: contig 0 first, contig 2 last, every row is in the dictionary
    assert k0 + k2 == 3000 and ((pc >= 0) & (pc < 3)).all() and (k0 - 1) // TILE <= 1 and (n - k2) // TILE >= 4097 - 2
    order = np.argsort(pc, kind="stable")
    assert (pc[order[:k0]] == 0).all() and (pc[order[n - k2:]] == 2).all()


# ---- (Z) --------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("m", Z_SIZES)
def test_prefix_arrays_of_the_rows_without_a_position(eng, dj, m, strict):
    """Z.  count = (hi - zs[hi]) - (r - ze[r]) with 40 % of the df2 rows in the two prefix arrays and the scans over n + 1 entries
    around device_scan's tile"""
    case = M.z_case(strict, m)
    exp, _ = M.check_both(eng, dj, case, strict)
    assert exp[0].min() > 0


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("which", ["last", "first"])
def test_one_row_without_a_position_at_either_end_of_the_start_order(eng, dj, which, strict):
    """Z.  entry n of zs is the only non-zero one / every entry from 1 on is"""
    exp, _ = M.check_both(eng, dj, M.z_edge_case(strict, which), strict)
    assert exp[0].min() > 0


# ---- (O) --------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("key", list(O_CASES))
def test_df2_rows_outside_the_contig_and_at_the_int32_limits(eng, dj, key, strict):
    """O.  the grid of contig 0 extends past [0, L) on both sides: te / ts against ulo / uhi with pieces that end at L or start at 0"""
    case = M.o_case(strict, **O_CASES[key])
    assert key != "small" or len(case.probe[0]) * len(case.off) <= M.BRUTE_MAX
    M.check_both(eng, dj, case, strict)


# ---- (R) --------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("which", ["r1", "r2", "r3"])
def test_deep_and_wide_rank_searches(eng, dj, which, strict):
    """R.  joint_rank's gallop over thousands of equal keys up to the segment's end (R1), from a bin of a grid wider than 2^16 (R2),
    and on segments of one and two rows (R3)"""
    case = {"r1": M.r1_case, "r2": M.r2_case, "r3": M.r3_case}[which](strict)
    M.check_both(eng, dj, case, strict)


# ---- (A) --------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("strict", MODES)
def test_row_ids_on_either_side_change_nothing(dj, strict):
    """A.  df1 with a permuted row_id outside [0, n); the df2 index built from a side with row ids (six of them outside [0, n))"""
    case = M.a_case(strict)
    exp = M.reference_once(case, strict)
    base = M.run_dev(dj, case, strict)
    M.assert_stats(base, exp, "no row ids")
    got = M.run_dev(dj, case, strict, probe_row_id=J.probe_ids(len(case.probe[0])))
    assert M.blob(got) == M.blob(base), "df1 with a row_id"
    bid, _ = J.build_ids(len(case.build[0]))
    got = M.run_dev(dj, case, strict, build_row_id=bid)
    assert M.blob(got) == M.blob(base), "df2 with a row_id"
    db = J.dev_side(case.build, bid)
    ix = dj.build_index(db, strict, case.nc)
    try:
        got = M.run_dev(dj, case, strict, probe_row_id=J.probe_ids(len(case.probe[0])), build_row_id=bid, index=ix)
    finally:
        ix.close()
    assert M.blob(got) == M.blob(base), "an index built from a side with row ids"


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("shift", [1, 2, 3])
def test_columns_and_tables_that_are_not_16_byte_aligned(dj, shift, strict):
    """A.  the six columns, contig_len and offsets as views `shift` elements into larger tensors"""
    for n in (TILE - 1, TILE + 1, 2 * TILE + 3):
        case = M.a_case(strict, n=n)
        exp = M.reference_once(case, strict)
        got = M.run_dev(dj, case, strict, shift=shift)
        M.assert_stats(got, exp, f"shift {shift}, {n} rows")
        assert M.blob(got) == M.blob(M.run_dev(dj, case, strict))


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("n_perm", [1, 63, 65, 1025])
def test_outputs_between_sentinels_on_the_raw_device_entry(dj, n_perm, strict):
    """A.  n_pairs / n_rows in the middle of one int64 tensor (8-byte aligned only), sentinels before, between and after"""
    import torch
    case = M.a_case(strict, n=600, m=2000, n_perm=n_perm)
    exp = M.reference_once(case, strict)
    pad = 5
    out = torch.full((2 * n_perm + 3 * pad,), S.SENTINEL, dtype=torch.int64, device="cuda")
    a, b = pad, 2 * pad + n_perm
    dp, db = J.dev_side(case.probe), J.dev_side(case.build)
    lengths, off = M.dev_tables(case)
    ix = dj.build_index(db, strict, case.nc)
    try:
        dj.engine.permute_overlaps_dev(ix, dp.as_c(), _engine.make_opts(strict, case.nc), lengths.data_ptr(), off.data_ptr(), n_perm,
                                       out[a:].data_ptr(), out[b:].data_ptr())
        torch.cuda.synchronize()
    finally:
        ix.close()
    host = out.cpu().numpy()
    M.assert_stats((host[a:a + n_perm], host[b:b + n_perm]), exp, f"{n_perm} permutations")
    keep = np.ones(len(host), bool)
    keep[a:a + n_perm] = keep[b:b + n_perm] = False
    assert keep.sum() == 3 * pad and (host[keep] == S.SENTINEL).all(), "a sentinel was overwritten"


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_every_partition_mode_runs_the_same_kernels(strict):
    """A.  permute_plan routes every partition_mode to the one form: the same bytes and the same launches (no partition).  On a
    caller-owned index the launches of a call are the same set in every mode.  The host entry builds the df2 index itself, with
    the caller's partition_mode: under 5 that build also lays out the flat tables of the fused join (index_build calls build_flat
    for partition_mode 5 only: exactly the launches of FLAT_TABLES), which the permutation kernels never read -- pinned as it is;
    every other launch, and every launch under the other modes, is the same."""
    from polars_bio_amd.device_api import DeviceJoin
    case = M.a_case(strict)
    exp = M.reference_once(case, strict)
    e, d = _engine.Engine(0), DeviceJoin(0)
    ix = d.build_index(J.dev_side(case.build), strict, case.nc, True)
    try:
        e.enable_timing(2)
        d.engine.enable_timing(2)
        M.check_both(e, d, case, strict)                     # (the first call of a context also grows its buffers)
        M.run_dev(d, case, strict, index=ix)                 # (... and the first call on an index builds what it lacks)
        names = {}
        for pm in (0, 1, 2, 5, 6):
            got, t = _names_of(e, lambda: M.run_host(e, case, strict, partition_mode=pm))
            dev, td = _names_of(d.engine, lambda: M.run_dev(d, case, strict, partition_mode=pm, index=ix))
            M.assert_stats(got, exp, f"host, partition_mode {pm}")
            assert M.blob(got) == M.blob(exp) == M.blob(dev), pm
            assert M.blob(M.run_dev(d, case, strict, partition_mode=pm)) == M.blob(exp), pm
            names[pm] = (t, td)
            assert all(k in t and k in td for k in KERNELS) and "part_scatter" not in t and "part_scatter" not in td, (pm, t, td)
            assert td == names[0][1], (pm, td, names[0][1])
            if pm == 5:
                assert set(names[0][0]) <= set(t) and set(t) - set(names[0][0]) == FLAT_TABLES, (pm, t, names[0][0])
            else:
                assert t == names[0][0], (pm, t, names[0][0])
    finally:
        ix.close()
        e.close()
        d.engine.close()


# ---- (B) --------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("nc", P.SWEEP + [24])
def test_across_dictionary_sizes(eng, dj, nc, strict):
    """B.  k_permute reads cmeta_j[2 c] and offsets[p * n_contigs + c] per row: every dictionary size around the layout thresholds,
    every out-of-dictionary id on both sides, a share of df1 rows that end beyond their contig"""
    M.check_both(eng, dj, M.sweep_case(strict, nc), strict)


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("nc", [64, 1025])
def test_under_the_table_knobs(nc, strict, monkeypatch):
    """B.  the forms of the joint grid that IVJ_COUNT_NOLDS and IVJ_JOINT_BINS select"""
    case = M.sweep_case(strict, nc)
    exp = M.reference_once(case, strict)
    blobs = []
    for env in ({"IVJ_COUNT_NOLDS": "1"}, {"IVJ_JOINT_BINS": "1"}, {"IVJ_JOINT_BINS": "2"}):
        e, d, done = _engines_under(monkeypatch, env)
        try:
            _, got = M.check_both(e, d, case, strict, exp, f"{case.name} under {env}")
            blobs.append((M.blob(got["host"]), M.blob(got["device"])))
        finally:
            done()
    assert all(b == blobs[0] for b in blobs) and blobs[0][0] == blobs[0][1] == M.blob(exp)


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_on_a_sparse_dictionary_of_2_24_plus_1_ids(eng, dj, strict):
    """B.  one row of offsets is 64 MiB: the host entry ships three pieces of one permutation each through one device buffer"""
    case = M.sparse_case(strict)
    exp, _ = M.check_both(eng, dj, case, strict)
    assert len(set(exp[0].tolist())) == 3 and len(set(exp[1].tolist())) == 3


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_two_uneven_offset_pieces(eng, dj, strict):
    """B.  70 permutations x 262 145 contigs: pieces of 63 and 7 permutations (offsets + p0 * nc, d_pairs + p0)"""
    case = M.pieces_case(strict)
    exp, _ = M.check_both(eng, dj, case, strict)
    assert len(set(exp[0].tolist())) > 35


# ---- (C) --------------------------------------------------------------------------------------------------------------------------------

def _sort_names(d, case, strict):
    """the launches of ONE device-entry call on a df2 index built beforehand: the only index build among them is the df1 sort"""
    db = J.dev_side(case.build)
    ix = d.build_index(db, strict, case.nc, True)
    try:
        return _names_of(d.engine, lambda: M.run_dev(d, case, strict, index=ix))
    finally:
        ix.close()


@gpu
@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("which", ["auto", "handover"])
def test_df1_sort_through_the_index_build_forms(which, strict, monkeypatch):
    """C.  df1 is sorted by index_build: 140 000 rows take the balanced build by the automatic rule (no knob), or start it and hand
    over to the LSD sort (one narrow window); then every build form, byte-identical"""
    from polars_bio_amd.device_api import DeviceJoin
    case = (M.auto_case if which == "auto" else M.handover_case)(strict)
    balanced = which == "auto"
    exp = M.reference_once(case, strict)
    e, d = _engine.Engine(0), DeviceJoin(0)
    try:
        d.engine.enable_timing(2)
        got, t = _sort_names(d, case, strict)
        M.assert_stats(got, exp, f"{which}, no knob")
        if balanced:
            assert "ix3_local" in t and "ix_final" not in t and "permute_overlaps" in t, t
        else:
            assert "ix3_pass" in t and "ix3_local" not in t and "ix_final" in t and "permute_overlaps" in t, t
        M.check_both(e, None, case, strict, exp, f"{which}, no knob")
    finally:
        e.close()
        d.engine.close()
    blobs = []
    for form in P.FORMS:
        e, d, done = _engines_under(monkeypatch, form)
        try:
            d.engine.enable_timing(2)
            got, t = _sort_names(d, case, strict)
            M.assert_stats(got, exp, f"{which} under {form}")
            _assert_build(t, form, balanced, f"{which} under {form}")
            host = M.run_host(e, case, strict)
            M.assert_stats(host, exp, f"{which} under {form}: host entry")
            blobs.append((M.blob(got), M.blob(host)))
        finally:
            done()
    assert all(b == blobs[0] for b in blobs), "byte-identical results under every index build form"


# ---- (D) --------------------------------------------------------------------------------------------------------------------------------

CALLS = ("permute", "count", "map", "thresh_count", "nearest", "permute_again")
ORDERS = [CALLS,
          CALLS[::-1],
          ("map", "permute", "nearest", "permute_again", "count", "thresh_count"),
          ("thresh_count", "nearest", "permute_again", "map", "permute", "count"),
          ("nearest", "count", "permute", "thresh_count", "permute_again", "map"),
          ("count", "permute_again", "thresh_count", "permute", "map", "nearest")]


def _sequence_call(dj, call, case, strict, dp, db, tables, agg, ix):
    if call.startswith("permute"):
        return tuple(t.cpu().numpy() for t in dj.permute_overlaps(dp, db, strict, case.nc, *tables, index=ix))
    if call == "count":
        return (dj.count_overlaps(dp, db, strict, case.nc, index=ix, partition_mode=1).cpu().numpy(),)
    if call == "map":
        res = dj.overlap_agg(dp, db, strict, case.nc, agg, index=ix, partition_mode=1)
        return tuple(res[0][op].cpu().numpy() for op in ("sum", "count"))
    if call == "thresh_count":
        return (dj.count_overlaps_thresh(dp, db, strict, case.nc, min_overlap=3, index=ix, partition_mode=1).cpu().numpy(),)
    idx, dist, nf = (t.cpu().numpy() for t in dj.nearest(dp, db, strict, case.nc, index=ix))
    found = nf > 0                                           # idx / dist of a row without a neighbour are unspecified
    return nf, np.where(found, idx[:, 0], -1), np.where(found, dist[:, 0], -1)


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_calls_on_one_index_in_any_order(dj, strict):
    """D.  one long-lived DeviceIndex: the permute call builds the end order and the joint grid on it where they are missing, takes
    the arena and ends a pending hand-over; the other calls rewrite the arena and the partition's columns in between"""
    case = M.sequence_case(strict)
    exp = M.reference_once(case, strict)
    dp, db = J.dev_side(case.probe), J.dev_side(case.build)
    tables = M.dev_tables(case)
    columns = [(v, m, ["sum", "count"]) for v, m, _ in J.agg_columns(len(case.build[0]), 91)[:1]]
    agg = S.dev_agg(columns)
    fresh = {}
    for call in CALLS:
        ix = dj.build_index(db, strict, case.nc)
        try:
            fresh[call] = M.blob(_sequence_call(dj, call, case, strict, dp, db, tables, agg, ix))
        finally:
            ix.close()
    counts = S.reference_once("sequence", case.probe, case.build, case.nc, strict, None)[2]
    assert fresh["permute"] == fresh["permute_again"] == M.blob(exp)
    assert fresh["count"] == M.blob((counts.astype(np.int64),))
    for order in ORDERS:
        assert sorted(order) == sorted(CALLS)
        ix = dj.build_index(db, strict, case.nc)
        try:
            for step, call in enumerate(order):
                got = M.blob(_sequence_call(dj, call, case, strict, dp, db, tables, agg, ix))
                assert got == fresh[call], f"step {step} ({call}) of {order} differs from the call on a fresh index"
        finally:
            ix.close()


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_a_permute_call_between_count_and_fill(dj, strict):
    """D.  permute_plan sets ov_n = -1 and retakes the arena: the fill of a count -> fill hand-over that was pending across a
    permute_overlaps_dev call fails with IVJ_ESTATE and writes nothing; a fresh count -> fill pair afterwards is right"""
    import torch
    case = M.sequence_case(strict)
    exp = M.reference_once(case, strict)
    plain = S.reference_once("sequence", case.probe, case.build, case.nc, strict, None)
    total = len(plain[0])
    dp, db = J.dev_side(case.probe), J.dev_side(case.build)
    lengths, off = M.dev_tables(case)
    n_perm = len(case.off)
    eng = dj.engine
    for pm in (0, 1):
        opts = _engine.make_opts(strict, case.nc, partition_mode=pm)
        ix = dj.build_index(db, strict, case.nc)
        try:
            assert eng.overlap_count_dev(ix, dp.as_c(), opts) == total
            out = torch.full((2, n_perm), -7, dtype=torch.int64, device="cuda")
            eng.permute_overlaps_dev(ix, dp.as_c(), opts, lengths.data_ptr(), off.data_ptr(), n_perm, out[0].data_ptr(), out[1].data_ptr())
            torch.cuda.synchronize()
            M.assert_stats(tuple(out.cpu().numpy()), exp, "the permute call in between")
            bufs = [torch.full((total + 16,), -7, dtype=torch.int32, device="cuda") for _ in range(2)]
            with pytest.raises(_engine.EngineError) as err:
                eng.overlap_fill_dev(ix, dp.as_c(), opts, bufs[0].data_ptr(), bufs[1].data_ptr(), total)
            assert err.value.code == _engine.IVJ_ESTATE, err.value
            torch.cuda.synchronize()
            assert all(bool((t == -7).all()) for t in bufs), "a failed fill wrote into the pair buffers"
            assert eng.overlap_count_dev(ix, dp.as_c(), opts) == total
            eng.overlap_fill_dev(ix, dp.as_c(), opts, bufs[0].data_ptr(), bufs[1].data_ptr(), total)
            torch.cuda.synchronize()
            T.assert_pairs(tuple(t[:total].cpu().numpy() for t in bufs), plain[:2], "a fresh count -> fill pair")
            assert all(bool((t[total:] == -7).all()) for t in bufs)
        finally:
            ix.close()


@gpu
@pytest.mark.parametrize("strict", MODES)
def test_one_context_under_alternating_large_and_small_inputs(strict):
    """D.  150 000 and 300 rows in turn on ONE engine and ONE DeviceJoin, five rounds: the small calls follow the large ones on the
    regrown arena; the large rounds are byte-identical"""
    from polars_bio_amd.device_api import DeviceJoin
    e, d = _engine.Engine(0), DeviceJoin(0)
    large = []
    try:
        for step, (nrows, seed, _) in enumerate(J.D3_ROUNDS):
            case = M.sized_case(strict, nrows, seed)
            _, got = M.check_both(e, d, case, strict, what=f"round {step}: {nrows} rows")
            if nrows > J.SMALL_ROWS:
                large.append((M.blob(got["host"]), M.blob(got["device"])))
    finally:
        e.close()
        d.engine.close()
    assert len(large) == 3 and large[1] == large[0] and large[2] == large[0]


# ---- (P) --------------------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("strict", MODES)
def test_4097_tiles_take_960_permutations_per_launch(dj, strict):
    """P.  4096 * TILE + 501 rows x 961 permutations on the device entry: a launch of 960 permutations and a tail launch of one.
    All but 3000 rows lie on a contig df2 lacks (they contribute nothing: the CPU group shows it by brute force), the 3000 in the
    first and the last tiles, so that the partials of both ends of the tile range carry the result."""
    case = M.p_case(strict)
    n, n_perm = len(case.probe[0]), len(case.off)
    assert M.per_launch(n, n_perm) == 960 < CHUNK and n_perm % 960 == 1
    exp = M.reference(case, strict, probe=M.hot_rows(case))
    assert exp[0].min() > 0 and len(set(exp[0].tolist())) > 400
    M.assert_stats(M.run_dev(dj, case, strict), exp, case.name)
