"""Directional nearest at the engine level (ivj_opts.nearest_ignore): every kernel path, every mask, against the oracle's ordered
candidate list with the ignored classes removed (tests/_nearest_direction_util.py).  idx, dist and n_found are compared exactly."""
import ctypes as C
import functools

import numpy as np
import pytest

from _nearest_direction_util import directed, full_lists, left_right_ties
from oracle import oracle as O
from polars_bio_amd import _engine

N_CONTIGS = 4                 # dictionary size; contig 3 has no build rows
MASKS = (1, 2, 3)


def _base():
    """3000 probes x 400 build rows, coordinates in [0, 20000), lengths 1 .. 300: left / right ties and overlaps are common."""
    rng = np.random.default_rng(20261017)
    nb = 400
    bc = rng.integers(0, 3, nb).astype(np.int32)
    bs = rng.integers(0, 20000 - 300, nb).astype(np.int32)
    be = (bs + rng.integers(1, 301, nb)).astype(np.int32)
    bc[:20], bs[:20], be[:20] = 1, 7000, 7100                                  # identical rows: the (start, row) tie-break
    bc[20], bs[20], be[20] = 2, 0, 20000                                      # a contig-wide row
    bc[21:71], bs[21:71] = 0, 12000                                            # one start, 50 rows: more than three rows of a lines
    be[21:71] = (12001 + rng.integers(0, 300, 50)).astype(np.int32)           # bin below a probe's end (k_nearest_k1_rest)
    n = 3000
    pc = rng.integers(0, N_CONTIGS, n).astype(np.int32)
    pc[:40] = -1
    pc[40:80] = N_CONTIGS + rng.integers(0, 3, 40).astype(np.int32)           # ids the dictionary lacks
    ps = rng.integers(0, 20000 - 300, n).astype(np.int32)
    pe = (ps + rng.integers(1, 301, n)).astype(np.int32)
    ps[80:200] = rng.integers(11900, 12400, 120).astype(np.int32)             # around the cluster
    pe[80:200] = (ps[80:200] + rng.integers(1, 301, 120)).astype(np.int32)
    return (pc, ps, pe), (bc, bs, be)


def _few():
    """A build side of 5 rows on one contig: k = 7 runs out of candidates."""
    c = np.full(5, 1, np.int32)
    s = np.array([3000, 3000, 9000, 9100, 15000], np.int32)
    e = np.array([3100, 3050, 9200, 9150, 15010], np.int32)
    return c, s, e


PROBE, BUILD = _base()
BUILDS = {"base": BUILD, "few": _few()}


@functools.lru_cache(maxsize=None)
def _lists(build, strict, include_overlaps):
    return full_lists(PROBE, BUILDS[build], strict, include_overlaps)


def _expect(build, strict, include_overlaps, mask, k):
    return directed(_lists(build, strict, include_overlaps), mask, k)


def _same(got, exp):
    (i, d, n), (ei, ed, en) = got, exp
    assert (n == en).all(), np.flatnonzero(n != en)[:5]
    assert (d == ed).all(), np.argwhere(d != ed)[:5]
    assert (i == ei).all(), np.argwhere(i != ei)[:5]


def test_the_filter_with_mask_0_is_the_oracle_itself():
    """CPU: dropping nothing from the full list and cutting it to k reproduces nearest_brute(k)."""
    for strict in (True, False):
        for inc in (True, False):
            for k in (1, 3, 7):
                exp = O.nearest_brute(O.Side(*PROBE), O.Side(*BUILD), strict, k, inc)
                _same(_expect("base", strict, inc, 0, k), exp)
    _same(_expect("few", True, True, 0, 7), O.nearest_brute(O.Side(*PROBE), O.Side(*BUILDS["few"]), True, 7, True))


def test_the_shape_has_overlaps_ties_and_both_sides():
    for strict in (True, False):
        lists = _lists("base", strict, True)
        assert (lists[2] == 0).any() and left_right_ties(lists).sum() >= 3
        assert (_expect("base", strict, True, 1, 1)[2] == 0).any()            # some probe has nothing but left rows
        assert ((lists[2] == 1).any(1) & (lists[2] == 2).any(1)).any()


def test_make_opts_carries_and_checks_the_mask():
    assert [_engine.make_opts(True, 4, nearest_ignore=m).nearest_ignore for m in (0, 1, 2, 3)] == [0, 1, 2, 3]
    for bad in (4, -1):
        with pytest.raises(ValueError):
            _engine.make_opts(True, 4, nearest_ignore=bad)


@pytest.fixture(scope="module")
def eng():
    e = _engine.Engine(0)
    e.enable_timing(2)
    yield e
    e.close()


K1_PATHS = {"record": ({}, "nearest_k1"), "bucketed": ({"partition_mode": 1}, "nearest_k1"), "lines": ({"table_mode": 3}, "nearest_k1_lines")}
SUFFIX = {1: "_noleft", 2: "_noright", 3: "_ovonly"}


@pytest.mark.gpu
@pytest.mark.parametrize("path", list(K1_PATHS))
@pytest.mark.parametrize("strict", [True, False])
def test_k1_paths(eng, strict, path):
    kw, kernel = K1_PATHS[path]
    for mask in MASKS:
        got = eng.nearest(PROBE, BUILD, strict, N_CONTIGS, 1, True, nearest_ignore=mask, **kw)
        t = eng.timings()
        assert kernel + SUFFIX[mask] in t, sorted(t)                           # the path that was asked for, in its directional form
        if path == "lines":
            assert "nearest_k1_rest" + SUFFIX[mask] in t, sorted(t)
        if path == "bucketed":
            assert "unpermute" in t, sorted(t)
        _same(got, _expect("base", strict, True, mask, 1))


@pytest.mark.gpu
@pytest.mark.parametrize("partition_mode", [0, 1])
@pytest.mark.parametrize("strict", [True, False])
def test_general_kernel(eng, strict, partition_mode):
    for k, inc in ((1, False), (3, True), (3, False), (7, True), (7, False)):
        for mask in MASKS:
            for build in ("base", "few"):
                got = eng.nearest(PROBE, BUILDS[build], strict, N_CONTIGS, k, inc, nearest_ignore=mask, partition_mode=partition_mode)
                assert "nearest_general" + SUFFIX[mask] in eng.timings()
                _same(got, _expect(build, strict, inc, mask, k))
    few = _expect("few", strict, True, 1, 7)
    assert 0 < few[2].max() < 7                                                # k = 7 did run out of candidates


@pytest.mark.gpu
def test_mask_0_is_todays_call(eng):
    for kw in ({}, {"partition_mode": 1}, {"table_mode": 3}):
        _same(eng.nearest(PROBE, BUILD, True, N_CONTIGS, nearest_ignore=0, **kw), eng.nearest(PROBE, BUILD, True, N_CONTIGS, **kw))
        _same(eng.nearest(PROBE, BUILD, True, N_CONTIGS, nearest_ignore=0, **kw), O.nearest_brute(O.Side(*PROBE), O.Side(*BUILD), True, 1, True))
    _same(eng.nearest(PROBE, BUILD, False, N_CONTIGS, 3, False, nearest_ignore=0), O.nearest_brute(O.Side(*PROBE), O.Side(*BUILD), False, 3, False))


@pytest.mark.gpu
def test_the_library_refuses_other_masks(eng):
    o = _engine.make_opts(True, N_CONTIGS)
    o.nearest_ignore = 4
    ps, keep_p = _engine._host_side(*PROBE)
    bs, keep_b = _engine._host_side(*BUILD)
    idx, dist, nf = np.empty((ps.n, 1), np.int32), np.empty((ps.n, 1), np.int64), np.empty(ps.n, np.int32)
    rc = eng.L.ivj_nearest(eng.h, C.byref(ps), C.byref(bs), C.byref(o), idx.ctypes.data, dist.ctypes.data, nf.ctypes.data)
    assert rc == -1 and b"nearest_ignore" in eng.L.ivj_last_error()
    with eng.probe_stream(BUILD, True, N_CONTIGS, _engine.STREAM_NEAREST, 1000) as st:
        with pytest.raises(ValueError):
            st.set_nearest_ignore(4)
        assert eng.L.ivj_stream_set_nearest_ignore(st.h, 4) == -1
    with eng.probe_stream(BUILD, True, N_CONTIGS, _engine.STREAM_COUNT, 1000) as st:
        assert eng.L.ivj_stream_set_nearest_ignore(st.h, 1) == -1


@pytest.mark.gpu
@pytest.mark.parametrize("k,inc", [(1, True), (3, False)])
def test_stream_latches_the_mask_per_batch(eng, k, inc):
    """Three batches of 1000 probes, the mask changed between them: a batch is joined one submit later, under ITS mask."""
    masks = (1, 2, 3)
    out = {}
    with eng.probe_stream(BUILD, True, N_CONTIGS, _engine.STREAM_NEAREST, 1000, k=k, include_overlaps=inc, nearest_ignore=masks[0]) as st:
        for b, mask in enumerate(masks):
            if b:
                st.set_nearest_ignore(mask)
            r = st.submit(tuple(a[1000 * b:1000 * (b + 1)] for a in PROBE))
            if r is not None:
                out[r["batch"]] = r
        while True:
            r = st.flush()
            if r is None:
                break
            out[r["batch"]] = r
    assert sorted(out) == [0, 1, 2]
    for b, mask in enumerate(masks):
        ei, ed, en = _expect("base", True, inc, mask, k)
        sl = slice(1000 * b, 1000 * (b + 1))
        _same((out[b]["build_idx"], out[b]["dist"], out[b]["n_found"]), (ei[sl], ed[sl], en[sl]))


@pytest.mark.gpu
def test_torch_device_api_takes_the_mask():
    import torch
    from polars_bio_amd.device_api import DeviceJoin, DeviceSide
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    join = DeviceJoin(0)
    i, d, n = join.nearest(DeviceSide(*map(up, PROBE)), DeviceSide(*map(up, BUILD)), True, N_CONTIGS, nearest_ignore=1)
    _same((i.cpu().numpy(), d.cpu().numpy(), n.cpu().numpy()), _expect("base", True, True, 1, 1))
    i, d, n = join.nearest(DeviceSide(*map(up, PROBE)), DeviceSide(*map(up, BUILD)), False, N_CONTIGS, k=3, include_overlaps=False, nearest_ignore=1)
    _same((i.cpu().numpy(), d.cpu().numpy(), n.cpu().numpy()), _expect("base", False, False, 1, 3))
