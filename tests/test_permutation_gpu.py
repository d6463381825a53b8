"""pb.permutation_test on the GPU: the host entry (Engine.permute_overlaps) and the device entry (DeviceJoin.permute_overlaps) are
both compared EXACTLY with the yardstick of tests/_permutation_util.py -- the literal brute force where the case is small, the
two-rank identity (checked against the brute force in test_permutation_cpu.py) where it is not.  Shapes come from the kernel's
header: rows around the workgroup tile, permutations around the permutation block and the per-launch chunk."""
import numpy as np
import pytest

import _permutation_util as U
import _position_ops_util as P
from polars_bio_amd import _engine
from test_contig_dictionaries import _fresh
from test_permutation_cpu import HAND_LEN, HAND_OFF, HAND_PAIRS, HAND_ROWS, hand_case

pytestmark = pytest.mark.gpu
I32 = np.int32
MODES = [pytest.param(True, id="strict"), pytest.param(False, id="weak")]
TILE, WAVE_ROWS, BLOCK, CHUNK = U.kernel_geometry()
BRUTE_MAX = 400_000                    # (df1 rows x permutations) up to which the literal brute force is the reference


@pytest.fixture(scope="module")
def eng():
    return _engine.Engine(0)


@pytest.fixture(scope="module")
def dj():
    import torch  # noqa: F401
    from polars_bio_amd.device_api import DeviceJoin
    return DeviceJoin(0)


def _dev(dj, probe, build, strict, nc, lengths, off, **kw):
    import torch
    from polars_bio_amd.device_api import DeviceSide
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=I32)).cuda()
    pairs, rows = dj.permute_overlaps(DeviceSide(*map(t, probe)), DeviceSide(*map(t, build)), strict, nc, t(lengths),
                                      t(np.asarray(off).reshape(len(off), nc)), **kw)
    return pairs.cpu().numpy(), rows.cpu().numpy()


def _check(eng, dj, probe, build, strict, nc, lengths, off, what, brute=None):
    """Both entries against the reference -> the reference."""
    off = np.ascontiguousarray(off, dtype=I32).reshape(len(off), nc)
    lengths = np.ascontiguousarray(lengths, dtype=I32)
    use_brute = len(probe[0]) * len(off) <= BRUTE_MAX if brute is None else brute
    exp = (U.expected if use_brute else U.ranks)(probe, build, nc, strict, lengths, off)
    for name, got in (("host", eng.permute_overlaps(probe, build, strict, nc, lengths, off)), ("device", _dev(dj, probe, build, strict, nc, lengths, off))):
        for k, stat in enumerate(("n_pairs", "n_rows")):
            assert got[k].dtype == np.int64 and got[k].shape == (len(off),), (what, name, stat)
            bad = np.flatnonzero(got[k] != exp[k])
            assert len(bad) == 0, f"{what}: {name} entry, {stat}: {len(bad)} permutations differ, first {bad[0]}: {got[k][bad[0]]} != {exp[k][bad[0]]}"
    return exp


def _frames(rng, n, m, nc, lengths, strict, width=300, bwidth=200, bad=True):
    """n df1 rows inside their contigs and m df2 rows; with ``bad`` also rows of every ineligible kind / without a position."""
    one = 0 if strict else 1
    lengths = np.asarray(lengths, np.int64)

    def inside(k, w):
        c = rng.integers(0, nc, k)
        ln = np.minimum(rng.integers(1, w + 1, k), lengths[c])
        hs = (rng.random(k) * (lengths[c] - ln + 1)).astype(np.int64)
        return c.astype(I32), (hs + one).astype(I32), (hs + ln).astype(I32)
    pc, ps, pe = inside(n, width)
    bc, bs, be = inside(m, bwidth)
    if bad and n >= 16:
        k = rng.choice(n, 8, replace=False)
        pe[k[0]] = ps[k[0]] - one                              # covers no position
        pe[k[1]] = ps[k[1]] - one - 3                          # inverted
        pe[k[2]] = min(int(lengths[pc[k[2]]]) + 1, 2 ** 31 - 1)                  # beyond the contig's end (where L + 1 is representable)
        ps[k[3]] = one - 1                                     # position -1 (closed: start 0)
        pc[k[4]] = nc                                          # outside the dictionary
        pc[k[5]] = -1                                          # no contig
        pc[k[6]] = 2 ** 31 - 1
        ps[k[7]], pe[k[7]] = -5, -2
    if bad and m >= 8:
        k = rng.choice(m, 4, replace=False)
        be[k[0]] = bs[k[0]] - one                              # df2 rows without a position: never match
        be[k[1]] = bs[k[1]] - one - 7
        bc[k[2]] = nc
        bc[k[3]] = -1
    return (pc, ps, pe), (bc, bs, be)


def _offsets(rng, n_perm, lengths):
    return rng.integers(0, np.asarray(lengths, np.int64)[None, :], size=(n_perm, len(lengths))).astype(I32)


@pytest.mark.parametrize("strict", MODES)
def test_hand_worked_wraps(eng, dj, strict):
    probe, build = hand_case(strict)
    exp = _check(eng, dj, probe, build, strict, 2, HAND_LEN, HAND_OFF, "hand-worked wraps")
    assert exp[0].tolist() == HAND_PAIRS and exp[1].tolist() == HAND_ROWS


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("n", [0, 1, WAVE_ROWS - 1, WAVE_ROWS + 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 1])
def test_rows_around_the_tile(eng, dj, n, strict):
    rng = np.random.default_rng(100 + n)
    lengths = [5000, 1, 77, 300_000]
    probe, build = _frames(rng, n, 500, 4, lengths, strict)
    exp = _check(eng, dj, probe, build, strict, 4, lengths, _offsets(rng, 5, lengths), f"{n} rows")
    assert n < 16 or exp[0].sum() > 0


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("n_perm", [1, 2, BLOCK - 1, BLOCK, BLOCK + 1, CHUNK - 1, CHUNK, CHUNK + 1])
def test_permutations_around_the_block_and_the_chunk(eng, dj, n_perm, strict):
    rng = np.random.default_rng(200 + n_perm)
    lengths = [4000, 1, 900]
    probe, build = _frames(rng, 300, 120, 3, lengths, strict, width=120, bwidth=60)
    exp = _check(eng, dj, probe, build, strict, 3, lengths, _offsets(rng, n_perm, lengths), f"{n_perm} permutations", brute=True)
    assert exp[0].sum() > 0 and (n_perm < 8 or len(set(exp[0].tolist())) > 1)


@pytest.mark.parametrize("strict", MODES)
def test_every_row_of_a_tile_wraps_none_wraps_and_offsets_l_minus_1(eng, dj, strict):
    rng = np.random.default_rng(7)
    one = 0 if strict else 1
    L, n = 100_000, TILE + 5
    ln = rng.integers(20, 41, n)
    hs = L - 50 - rng.integers(0, 11, n)                       # [L - 60, L - 50] + [20, 40]: every row ends in [L - 40, L - 10]
    probe = (np.zeros(n, I32), (hs + one).astype(I32), (hs + ln).astype(I32))
    _, build = _frames(rng, 0, 3000, 1, [L], strict, bwidth=40)
    build[1][:200] = one + rng.integers(0, 30, 200)            # df2 rows at the contig's start, where the second pieces land
    build[2][:200] = build[1][:200] + rng.integers(0, 30, 200)
    build[1][200:500] = L - 100 + one + rng.integers(0, 90, 300)   # ... and at its end, where the rows and the first pieces lie
    build[2][200:500] = np.minimum(build[1][200:500] + rng.integers(0, 30, 300), L)
    off = np.array([[0], [30], [L - 1], [45], [5]], I32)
    assert all(len(U.pieces_of(0, probe[1][i], probe[2][i], 1, strict, [L], off[3])) == 2 for i in range(n))      # every row wraps
    assert all(len(U.pieces_of(0, probe[1][i], probe[2][i], 1, strict, [L], o)) == 1 for i in range(n) for o in (off[0], off[4]))
    exp = _check(eng, dj, probe, build, strict, 1, [L], off, "wraps")
    assert exp[0].min() > 0


@pytest.mark.parametrize("strict", MODES)
def test_empty_sides_and_a_contig_df2_lacks(eng, dj, strict):
    rng = np.random.default_rng(9)
    lengths = [1000, 2000, 50]
    probe, build = _frames(rng, 200, 100, 3, lengths, strict, bad=False)
    off = _offsets(rng, 3, lengths)
    empty = (np.empty(0, I32),) * 3
    for p, b, what in ((empty, build, "empty df1"), (probe, empty, "empty df2"), (empty, empty, "both empty")):
        exp = _check(eng, dj, p, b, strict, 3, lengths, off, what)
        assert exp[0].sum() == 0 and exp[1].sum() == 0
    keep = build[0] != 1                                       # df2 has no row on contig 1
    exp = _check(eng, dj, probe, tuple(a[keep] for a in build), strict, 3, lengths, off, "a contig df2 lacks")
    assert exp[0].sum() > 0
    # [6,6) [10,2) [8,6) [8,8) half-open; [6,5] [10,2] [8,6] [8,7] closed
    only_bad = (np.zeros(4, I32), np.array([6, 10, 8, 8], I32), np.array([6, 2, 6, 8] if strict else [5, 2, 6, 7], I32))
    exp = _check(eng, dj, probe, only_bad, strict, 3, lengths, off, "df2 rows without a position only")
    assert exp[0].sum() == 0


@pytest.mark.parametrize("strict", MODES)
@pytest.mark.parametrize("nc", [1, 24, 257, 1025])
def test_dictionary_sizes(eng, dj, nc, strict):
    rng = np.random.default_rng(300 + nc)
    lengths = rng.integers(1, 20_000, nc)
    lengths[rng.integers(0, nc)] = 1
    probe, build = _frames(rng, 1500, 1200, nc, lengths, strict, width=400, bwidth=300)
    exp = _check(eng, dj, probe, build, strict, nc, lengths, _offsets(rng, 9, lengths), f"{nc} contigs")
    assert exp[0].sum() > 0


@pytest.mark.parametrize("strict", MODES)
def test_contig_of_length_int32_max(eng, dj, strict):
    one = 0 if strict else 1
    L = 2 ** 31 - 1
    hs = np.array([0, 0, 1, 5, L - 1, L - 5, L - 100, 2 ** 30, 0], np.int64)
    he = np.array([1, L, L, 50, L, L, L - 3, 2 ** 30 + 7, L - 1], np.int64)
    probe = (np.zeros(len(hs), I32), (hs + one).astype(I32), he.astype(I32))
    bs = np.array([0, 0, L - 1, L - 10, 17, 2 ** 30 - 3, 2 ** 30 + 6, L - 2, 3], np.int64)
    be = np.array([1, L, L, L - 4, 40, 2 ** 30 + 1, 2 ** 31 - 1, L - 1, 3], np.int64)
    build = (np.zeros(len(bs), I32), (bs + one).astype(I32), be.astype(I32))
    off = np.array([[0], [1], [L - 1], [L - 2], [2 ** 30], [2 ** 30 - 1], [L - 50], [5]], I32)
    exp = _check(eng, dj, probe, build, strict, 1, [L], off, "L = 2^31 - 1")
    assert exp[0].min() > 0 and exp[1].max() == len(hs)


@pytest.mark.parametrize("strict", MODES)
def test_index_build_forms(strict, monkeypatch):
    rng = np.random.default_rng(17)
    lengths = [60_000, 9000, 1]
    probe, build = _frames(rng, 4000, 30_000, 3, lengths, strict)
    off = _offsets(rng, 6, lengths)
    exp = U.ranks(probe, build, 3, strict, lengths, off)
    for form in P.FORMS:
        e = _fresh(monkeypatch, **form)
        try:
            got = e.permute_overlaps(probe, build, strict, 3, np.array(lengths, I32), off)
        finally:
            e.close()
            for k in form:
                monkeypatch.delenv(k)
        assert (got[0] == exp[0]).all() and (got[1] == exp[1]).all(), form


@pytest.mark.parametrize("strict", MODES)
def test_twenty_seeds(eng, dj, strict):
    for seed in range(20):
        rng = np.random.default_rng(1000 + seed)
        nc = int(rng.integers(1, 6))
        lengths = rng.integers(1, 3000, nc)
        probe, build = _frames(rng, int(rng.integers(16, 700)), int(rng.integers(8, 400)), nc, lengths, strict, width=int(rng.integers(1, 500)),
                               bwidth=int(rng.integers(1, 500)))
        _check(eng, dj, probe, build, strict, nc, lengths, _offsets(rng, int(rng.integers(1, 12)), lengths), f"seed {seed}", brute=True)


@pytest.mark.parametrize("strict", MODES)
def test_larger_case_repeats_and_ignores_partition_mode(eng, dj, strict):
    """A few thousand rows x 64 permutations against the rank identity; a second run and every partition_mode give the same bits;
    the new launches show up in the context's timings."""
    rng = np.random.default_rng(23)
    nc = 24
    lengths = rng.integers(50_000, 400_000, nc)
    probe, build = _frames(rng, 5 * TILE + 77, 20_000, nc, lengths, strict, width=2000, bwidth=1500)
    off = _offsets(rng, 64, lengths)
    exp = _check(eng, dj, probe, build, strict, nc, lengths, off, "larger case", brute=False)
    assert len(set(exp[0].tolist())) > 32
    L32 = np.array(lengths, I32)
    eng.enable_timing(2)
    try:
        again = eng.permute_overlaps(probe, build, strict, nc, L32, off)
        names = eng.timings()
    finally:
        eng.enable_timing(0)
    assert names["permute_overlaps"]["launches"] >= 1 and names["permute_fold"]["launches"] >= 1, names
    assert again[0].tobytes() == exp[0].tobytes() and again[1].tobytes() == exp[1].tobytes()
    for mode in (1, 2, 6):
        got = eng.permute_overlaps(probe, build, strict, nc, L32, off, partition_mode=mode)
        assert got[0].tobytes() == exp[0].tobytes() and got[1].tobytes() == exp[1].tobytes(), mode
        got = _dev(dj, probe, build, strict, nc, L32, off, partition_mode=mode)
        assert got[0].tobytes() == exp[0].tobytes() and got[1].tobytes() == exp[1].tobytes(), mode


@pytest.mark.parametrize("strict", MODES)
def test_zero_offsets_are_the_thresholded_count(eng, dj, strict):
    rng = np.random.default_rng(31)
    lengths = [80_000, 500, 20_000]
    probe, build = _frames(rng, 2 * TILE + 9, 5000, 3, lengths, strict, bad=False)
    counts = eng.count_overlaps_thresh(probe, build, strict, 3, min_overlap=1)
    pairs, rows = eng.permute_overlaps(probe, build, strict, 3, np.array(lengths, I32), np.zeros((2, 3), I32))
    assert pairs.tolist() == [int(counts.sum())] * 2 and rows.tolist() == [int((counts > 0).sum())] * 2 and counts.sum() > 0
    pairs, rows = _dev(dj, probe, build, strict, 3, lengths, np.zeros((1, 3), I32))
    assert pairs[0] == counts.sum() and rows[0] == (counts > 0).sum()


def test_device_entry_on_a_caller_owned_index(dj):
    import torch
    from polars_bio_amd.device_api import DeviceSide
    rng = np.random.default_rng(41)
    lengths = [30_000, 7000]
    probe, build = _frames(rng, 900, 2500, 2, lengths, True)
    off = _offsets(rng, 70, lengths)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=I32)).cuda()
    dp, db = DeviceSide(*map(t, probe)), DeviceSide(*map(t, build))
    ix = dj.build_index(db, True, 2)                           # without the end order: the call builds what it needs
    try:
        exp = U.ranks(probe, build, 2, True, lengths, off)
        for _ in range(2):                                     # the second call finds the index's tables built
            pairs, rows = dj.permute_overlaps(dp, db, True, 2, t(lengths), t(off), index=ix)
            assert (pairs.cpu().numpy() == exp[0]).all() and (rows.cpu().numpy() == exp[1]).all()
        counts = dj.count_overlaps(dp, db, True, 2, index=ix)  # the index still serves the other calls
        assert counts.shape[0] == 900
    finally:
        ix.close()
