"""pb.permutation_test without a GPU: the yardstick of tests/_permutation_util.py against independent facts (the oracle's brute
count for the unshifted rows, wraps worked by hand on a contig of length 10, the 1-based closed form of the same cases, its two
routes against each other), the header <-> binding consistency of the two new entries, and every refusal that needs no device."""
import ctypes as C
import re

import numpy as np
import pandas as pd
import pytest

import polars_bio_amd as pb
from polars_bio_amd import _engine, namespace, range_op
from oracle import oracle as O
import _permutation_util as U

I32 = np.int32
IVJ_EINVAL = int(re.search(r"IVJ_EINVAL\s*=?\s*(-?\d+)", open(f"{U.ROOT}/include/ivjoin.h").read()).group(1))


def _side(rows):
    c, s, e = zip(*rows) if rows else ((), (), ())
    return np.array(c, I32), np.array(s, I32), np.array(e, I32)


# ---- hand-worked wraps: contig 0 of length 10, contig 1 of length 1 (half-open, 0-based) ------------------------------------------
# build: b0 = [0,2)  b1 = [8,10)  b2 = [4,5)  b3 = contig 1 [0,1)  b4 = [5,5) covers no position
# probe: r0 = [7,10) ends exactly at L     r1 = [0,10) has length L     r2 = contig 1 [0,1), L = 1     r3 = [5,7)
# off 0: r0 [7,10): b1 | r1 [0,10): b0 b1 b2 | r2: b3 | r3 [5,7): none                                   -> 5 pairs, 3 rows
# off 3: r0 s' = 0: [0,3): b0 | r1 [3,10): b1 b2 + [0,3): b0 | r2: b3 | r3 [8,10): b1                    -> 6 pairs, 4 rows
# off 4: r0 [1,4): b0 | r1 [4,10): b1 b2 + [0,4): b0 | r2: b3 | r3 [9,10): b1 + [0,1): b0                -> 7 pairs, 4 rows
# off 5: r0 [2,5): b2 | r1 [5,10): b1 + [0,5): b0 b2 | r2: b3 | r3 s' = 0: [0,2): b0                     -> 6 pairs, 4 rows
# off 9: r0 [6,9): b1 | r1 [9,10): b1 + [0,9): b0 b2 b1 -- b1 TWICE | r2: b3 | r3 [4,6): b2              -> 7 pairs, 4 rows
HAND_BUILD = [(0, 0, 2), (0, 8, 10), (0, 4, 5), (1, 0, 1), (0, 5, 5)]
HAND_PROBE = [(0, 7, 10), (0, 0, 10), (1, 0, 1), (0, 5, 7)]
HAND_LEN = np.array([10, 1], I32)
HAND_OFF = np.array([[0, 0], [3, 0], [4, 0], [5, 0], [9, 0]], I32)
HAND_PAIRS, HAND_ROWS = [5, 6, 7, 6, 7], [3, 4, 4, 4, 4]


def hand_case(strict):
    """The hand-worked case in 0-based half-open (strict) or 1-based closed coordinates: start + 1, [5,5) becomes the inverted [6,5]."""
    one = 0 if strict else 1
    shift = lambda rows: _side([(c, s + one, e) for c, s, e in rows])
    return shift(HAND_PROBE), shift(HAND_BUILD)


@pytest.mark.parametrize("strict", [True, False], ids=["half_open", "closed_1_based"])
def test_yardstick_wraps_by_hand(strict):
    probe, build = hand_case(strict)
    for route in (U.expected, U.ranks):
        pairs, rows = route(probe, build, 2, strict, HAND_LEN, HAND_OFF)
        assert pairs.tolist() == HAND_PAIRS and rows.tolist() == HAND_ROWS, route.__name__


def test_yardstick_pieces_by_hand():
    assert U.pieces_of(0, 7, 10, 1, True, [10], [0]) == [(7, 10)]                 # ends exactly at L: one piece
    assert U.pieces_of(0, 7, 10, 1, True, [10], [3]) == [(0, 3)]                  # lands on s' = 0: one piece
    assert U.pieces_of(0, 0, 10, 1, True, [10], [4]) == [(4, 10), (0, 4)]         # length L, shifted: two pieces
    assert U.pieces_of(0, 0, 10, 1, True, [10], [0]) == [(0, 10)]
    assert U.pieces_of(0, 0, 1, 1, True, [1], [0]) == [(0, 1)]                    # L = 1
    assert U.pieces_of(0, 8, 10, 1, False, [10], [0]) == [(7, 10)]                # closed [8,10] = half-open [7,10)
    L = 2 ** 31 - 1
    assert U.pieces_of(0, L - 5, L, 1, True, [L], [L - 1]) == [(L - 6, L - 1)]
    assert U.pieces_of(0, L - 5, L, 1, True, [L], [L - 3]) == [(L - 8, L - 3)]
    assert U.pieces_of(0, 1, L, 1, True, [L], [L - 1]) == [(0, L - 1)]
    assert U.pieces_of(0, 0, L, 1, True, [L], [L - 1]) == [(L - 1, L), (0, L - 1)]   # e' = 2 L - 1 > 2^31
    for bad in [(0, 5, 5), (0, 6, 5), (0, -1, 4), (0, 5, 11), (1, 0, 5), (-1, 0, 5)]:   # no position, inverted, < 0, > L, outside x 2
        assert U.pieces_of(*bad, 1, True, [10], [0]) == []
    assert U.pieces_of(0, 0, 4, 1, False, [10], [0]) == []                        # closed start 0 is position -1


@pytest.mark.parametrize("strict", [True, False])
def test_yardstick_zero_offsets_are_the_oracle_counts(strict):
    rng = np.random.default_rng(5)
    nc, L = 3, 5000
    one = 0 if strict else 1

    def mk(k, width):
        s = rng.integers(one, L - 200, k)
        return rng.integers(0, nc + 1, k).astype(I32), s.astype(I32), (s + rng.integers(0, width, k)).astype(I32)   # id nc = outside
    probe, build = mk(400, 200), mk(300, 150)
    probe[1][:5] = L + 10                                                         # beyond the contig's end: ineligible
    lengths = np.full(nc, L, I32)
    pairs, rows = U.expected(probe, build, nc, strict, lengths, np.zeros((1, nc), I32))
    hs, he = probe[1].astype(np.int64) - one, probe[2].astype(np.int64)
    ok = (probe[0] < nc) & (0 <= hs) & (hs < he) & (he <= L)
    assert 5 < ok.sum() < len(ok) - 5
    bok = (build[0] < nc) & (build[1].astype(np.int64) - one < build[2])         # the oracle counts rows without a position: drop them
    want = O.count_overlaps_brute(O.Side(*(a[ok] for a in probe)), O.Side(*(a[bok] for a in build)), strict)
    assert pairs[0] == want.sum() and rows[0] == (want > 0).sum() and want.sum() > 500
    assert [a.tolist() for a in U.ranks(probe, build, nc, strict, lengths, np.zeros((1, nc), I32))] == [pairs.tolist(), rows.tolist()]


@pytest.mark.parametrize("strict", [True, False])
def test_yardstick_routes_agree_on_random_shifts(strict):
    rng = np.random.default_rng(11)
    nc, one = 4, 0 if strict else 1
    lengths = np.array([1, 37, 1000, 2 ** 31 - 1], I32)
    c = rng.integers(0, nc, 120).astype(I32)
    s = (rng.integers(0, lengths[c].astype(np.int64)) * (rng.random(120) < 0.8)).astype(np.int64)
    e = np.minimum(s + rng.integers(0, 40, 120), lengths[c])
    probe = (c, (s + one).astype(I32), e.astype(I32))
    bc = rng.integers(0, nc, 90).astype(I32)
    bs = rng.integers(0, np.minimum(lengths[bc].astype(np.int64), 1200))
    build = (bc, (bs + one).astype(I32), np.minimum(bs + rng.integers(0, 60, 90), lengths[bc]).astype(I32))
    off = rng.integers(0, lengths[None, :].astype(np.int64), size=(40, nc))
    a, b = U.expected(probe, build, nc, strict, lengths, off), U.ranks(probe, build, nc, strict, lengths, off)
    assert a[0].tolist() == b[0].tolist() and a[1].tolist() == b[1].tolist() and a[0].sum() > 0


def test_geometry_reads_the_header():
    tile, wave_rows, block, chunk = U.kernel_geometry()
    assert tile % wave_rows == 0 and chunk % block == 0 and block == 64


# ---- the ABI -----------------------------------------------------------------------------------------------------------------

NAMES = ("ivj_permute_overlaps", "ivj_permute_overlaps_dev")


def test_abi_symbols_and_header():
    L = _engine.load_library()
    hdr = open(f"{U.ROOT}/include/ivjoin.h").read()
    for s in NAMES:
        assert s in _engine.ABI_SYMBOLS and hasattr(L, s)
        assert re.search(rf"\bint {s}\(ivj_ctx\* ctx,", hdr), s
        decl = hdr[hdr.index(f"int {s}("):]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        assert len(decl.split(",")) == len(getattr(L, s).argtypes), s
    assert "#define IVJ_ABI_VERSION 6" in hdr and _engine.ABI_VERSION == 6 and L.ivj_abi_version() == 6
    assert callable(_engine.Engine.permute_overlaps) and callable(_engine.Engine.permute_overlaps_dev)
    from polars_bio_amd import device_api
    assert callable(device_api.DeviceJoin.permute_overlaps)
    dev = hdr[hdr.index("Device form on an index of ivj_index_build_dev (opts->n_contigs must be the index's)"):]
    dev = dev[:dev.index("int ivj_permute_overlaps_dev")]
    assert "NOT validated" in dev and "never reads outside the tables" in dev


def _einval(L, fn, *args):
    rc = fn(*args)
    assert rc == IVJ_EINVAL, rc
    return L.ivj_last_error().decode()


def test_einval_without_a_device():
    """The argument checks of both entries come before the context's, so they answer without a device (ctx = NULL)."""
    L = _engine.load_library()
    probe, build = _side([(0, 1, 5)]), _side([(0, 2, 6)])
    ps, keep_p = _engine._host_side(*probe)
    bs, keep_b = _engine._host_side(*build)
    o = _engine.make_opts(True, 1)
    lens, off = np.array([10], I32), np.zeros((2, 1), I32)
    out_p, out_r = np.zeros(2, np.int64), np.zeros(2, np.int64)
    good = dict(lens=lens.ctypes.data, off=off.ctypes.data, n=2, p=out_p.ctypes.data, r=out_r.ctypes.data)

    def call(fn, dev, **kw):
        a = {**good, **kw}
        head = (None, None) if dev else (None,)
        sides = (C.byref(ps),) if dev else (C.byref(ps), C.byref(bs))
        return _einval(L, fn, *head, *sides, C.byref(o), a["lens"], a["off"], a["n"], a["p"], a["r"])

    for fn, dev in ((L.ivj_permute_overlaps, False), (L.ivj_permute_overlaps_dev, True)):
        assert "n_perm" in call(fn, dev, n=0)
        assert "n_perm" in call(fn, dev, n=-3)
        assert "n_perm" in call(fn, dev, n=2 ** 20 + 1)
        assert "NULL" in call(fn, dev, lens=None)
        assert "NULL" in call(fn, dev, off=None)
        assert "NULL" in call(fn, dev, p=None)
        assert "NULL" in call(fn, dev, r=None)
        assert "ctx" in call(fn, dev)                                   # everything else in order: only the context is missing
    bad_len = np.array([0], I32)
    assert "contig_len[0]" in call(L.ivj_permute_overlaps, False, lens=bad_len.ctypes.data)
    for v in (-1, 10):
        bad_off = np.array([[0], [v]], I32)
        assert "offsets[1][0]" in call(L.ivj_permute_overlaps, False, off=bad_off.ctypes.data)
    del keep_p, keep_b


# ---- the front door against a stand-in engine --------------------------------------------------------------------------------

class YardstickEngine:
    calls = []

    def permute_overlaps(self, probe, build, strict, n_contigs, contig_len, offsets):
        assert offsets.dtype == I32 and contig_len.dtype == I32 and offsets.shape[1] == n_contigs == len(contig_len)
        YardstickEngine.calls.append((probe, build, strict, n_contigs, contig_len.copy(), offsets.copy()))
        return U.expected(probe, build, n_contigs, strict, contig_len, offsets)


@pytest.fixture
def stand_in(monkeypatch):
    YardstickEngine.calls = []
    monkeypatch.setattr(range_op, "default_engine", lambda: YardstickEngine())


def _frames(zero_based=True):
    df1 = pd.DataFrame({"chrom": ["chr1", "chr1", "chr2", None, "chr1"], "start": [1, 100, 1, 0, 900], "end": [50, 200, 10, 50, 1000],
                        "strand": ["+", "-", "+", "+", None]})
    df2 = pd.DataFrame({"chrom": ["chr1", "chr1", "chr3", "chr2"], "start": [10, 150, 5, 5], "end": [20, 160, 6, 6], "strand": ["+", "+", "-", "+"]})
    df1.attrs["coordinate_system_zero_based"] = zero_based
    df2.attrs["coordinate_system_zero_based"] = zero_based
    return df1, df2


GENOME = {"chr2": 10, "chr1": 1000, "chrX": 77}


def test_front_door_errors(stand_in):
    df1, df2 = _frames()
    kw = dict(output_type="pandas.DataFrame")
    with pytest.raises(ValueError, match="'chr2' is not in genome"):
        pb.permutation_test(df1, df2, {"chr1": 1000}, **kw)
    with pytest.raises(ValueError, match="df1 row 4"):
        pb.permutation_test(df1, df2, {"chr1": 999, "chr2": 10}, **kw)            # row 4 ends beyond chr1
    bad = df1.copy()
    bad.attrs = dict(df1.attrs)
    bad.loc[1, "end"] = 100                                                       # covers no position
    with pytest.raises(ValueError, match="df1 row 1"):
        pb.permutation_test(bad, df2, GENOME, **kw)
    closed1, closed2 = _frames(False)
    closed1.loc[0, "start"] = 0                                                   # 1-based: position 0 does not exist
    with pytest.raises(ValueError, match="df1 row 0"):
        pb.permutation_test(closed1, closed2, GENOME, **kw)
    for genome in ({}, {"chr1": 0, "chr2": 10}, {"chr1": 2 ** 31, "chr2": 10}, {"chr1": 10.5, "chr2": 10}, pd.DataFrame({"a": ["chr1"]}),
                   pd.DataFrame({"a": ["chr1", "chr1"], "b": [5, 6]})):
        with pytest.raises(ValueError, match="genome"):
            pb.permutation_test(df1, df2, genome, **kw)
    for n_perm in (0, -1, 2 ** 20, 1.5):
        with pytest.raises(ValueError, match="n_perm"):
            pb.permutation_test(df1, df2, GENOME, n_perm=n_perm, **kw)
    for offsets in (np.zeros((3, 2), np.int64), np.zeros(3, np.int64), np.zeros((0, 3), np.int64), np.zeros((2, 3)), np.full((2, 3), -1),
                    np.array([[0, 10, 0]])):
        with pytest.raises(ValueError, match="offsets"):
            pb.permutation_test(df1, df2, GENOME, offsets=offsets, **kw)
    with pytest.raises(ValueError, match="output"):
        pb.permutation_test(df1, df2, GENOME, output="pairs", **kw)
    assert YardstickEngine.calls == []


def test_front_door_refuses_a_multi_device_engine(monkeypatch):
    class Several:
        pass
    monkeypatch.setattr(range_op, "default_engine", lambda: Several())
    with pytest.raises(NotImplementedError, match="single-device"):
        pb.permutation_test(*_frames(), GENOME, n_perm=2, output_type="pandas.DataFrame")


def test_front_door_maps_the_genome_to_the_dictionary(stand_in):
    df1, df2 = _frames()
    names, off = range_op.permutation_offsets(GENOME, 6, seed=4)
    assert names == ["chr1", "chr2", "chrX"]
    null = pb.permutation_test(df1, df2, GENOME, n_perm=6, seed=4, output="null", output_type="pandas.DataFrame")
    probe, build, strict, nc, lens, table = YardstickEngine.calls[0]
    assert strict and table.shape == (7, nc) and (table[0] == 0).all()
    # the engine's dictionary: chr1, chr2 of df1 then chr3 of df2, which the genome does not name (length 1, offset 0)
    assert nc == 3 and lens.tolist() == [1000, 10, 1] and (table[1:, 0] == off[:, 0]).all() and (table[1:, 1] == off[:, 1]).all()
    assert (table[:, 2] == 0).all()
    assert null["permutation"].tolist() == list(range(6)) and str(null["n_pairs"].dtype) == "int64"
    assert "permutation_test" in namespace._ALIASES and "permutation_test" in pb.__all__
