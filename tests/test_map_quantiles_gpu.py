"""pb.map_quantiles on the GPU (overlap_quant.hip.h) through both entries -- host (Engine.overlap_quantiles =
ivj_overlap_quantiles) and device (DeviceJoin.overlap_quantiles = ivj_overlap_quantiles_dev) -- compared exactly with the literal
sort-and-index of tests/_map_quantiles_util.py: int64 bit for bit, doubles bit for bit but for the sign of a zero and the payload
of a NaN.  Every shape is read from the kernel's geometry."""
import numpy as np
import pytest

from polars_bio_amd import _engine, range_op
import _map_quantiles_util as U
from _util import random_side

pytestmark = pytest.mark.gpu

TILE, CHUNK, THREADS, WAVE = U.kernel_geometry()
PER = U.per_wave(CHUNK)
NEVER = U.A.T.NEVER
I64, F64 = np.int64, np.float64
OUTSIDE = 1 << 20                                    # a contig id outside every dictionary used here
QS8 = [0.0, 0.1, 0.25, 1 / 3, 0.5, 0.7, 0.9, 1.0]
Q16, UP16 = QS8 + QS8, [0] * 8 + [1] * 8             # every quantile with both roundings: IVJ_MAX_OVQ_RANKS requests
Q3, UP3 = [0.5, 0.5, 0.9], [0, 1, 0]


@pytest.fixture(scope="module")
def eng():
    return _engine.Engine(0)


@pytest.fixture(scope="module")
def dj():
    import torch  # noqa: F401
    from polars_bio_amd.device_api import DeviceJoin
    return DeviceJoin(0)


def _side(cols):
    import torch
    from polars_bio_amd.device_api import DeviceSide
    return DeviceSide(*[torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in cols])


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _min_dev(m):
    return None if m is None else _dev(np.ascontiguousarray(m, np.uint32).view(np.int32).copy())


def _engine_kw(min_overlap=None, probe_min=None, build_min=None):
    return dict(min_overlap=int(min_overlap or 0), probe_min=None if probe_min is None else np.asarray(probe_min, np.uint32),
                build_min=None if build_min is None else np.asarray(build_min, np.uint32))


def _host(eng, probe, build, nc, strict, values, valid, q, upper, kw, partition_mode=0):
    return eng.overlap_quantiles(probe, build, strict, nc, values, valid, q, upper, partition_mode=partition_mode, **kw)


def _device(dj, probe, build, nc, strict, values, valid, q, upper, kw, partition_mode=0, n_values=None):
    n_values = len(build[0]) if n_values is None else n_values
    dkw = dict(min_overlap=kw["min_overlap"], probe_min=_min_dev(kw["probe_min"]), build_min=_min_dev(kw["build_min"]))
    out, count = dj.overlap_quantiles(_side(probe), _side(build), strict, nc, _dev(values[:n_values]),
                                      None if valid is None else _dev(np.asarray(valid)[:n_values].astype(np.uint8)), q, upper,
                                      partition_mode=partition_mode, **dkw)
    return out.cpu().numpy(), count.cpu().numpy()


def check(eng, dj, probe, build, nc, strict, values, valid, q, upper, what="", partition_mode=0, **thr):
    """Both entries against the yardstick -> (expected out, expected count)."""
    kw = _engine_kw(**thr)
    exp, exp_n = U.expected(probe, build, nc, strict, values, valid, q, upper, **thr)
    for name, (got, got_n) in (("host", _host(eng, probe, build, nc, strict, values, valid, q, upper, kw, partition_mode)),
                               ("device", _device(dj, probe, build, nc, strict, values, valid, q, upper, kw, partition_mode))):
        assert got_n.dtype == I64 and (got_n == exp_n).all(), f"{what} {name}: counts differ at {np.nonzero(got_n != exp_n)[0][:5]}"
        U.assert_same(got, exp, f"{what} {name}")
    return exp, exp_n


def _stacks(counts, slots=None, n_probe=None, stride=1000):
    """Probe k matches exactly counts[k] build rows: in one contig, probe k = [stride k + 2, stride k + 8) over counts[k] rows
    [stride k + (0, 1 or 2), stride k + 10).  slots: the probe rows that carry them, every other of n_probe rows lies outside the
    dictionary.  Build rows come in shuffled order."""
    counts = np.asarray(counts)
    k = np.arange(len(counts))
    slots = k if slots is None else np.asarray(slots)
    n_probe = len(counts) if n_probe is None else n_probe
    pc, ps, pe = np.full(n_probe, OUTSIDE, np.int32), np.zeros(n_probe, np.int32), np.ones(n_probe, np.int32)
    pc[slots], ps[slots], pe[slots] = 0, stride * k + 2, stride * k + 8
    owner = np.repeat(k, counts)
    j = np.arange(len(owner)) - np.repeat(np.cumsum(counts) - counts, counts)      # 0 .. counts[k] - 1 within probe k
    rng = np.random.default_rng(len(owner))
    order = rng.permutation(len(owner))
    owner, j = owner[order], j[order]
    build = (np.zeros(len(owner), np.int32), (stride * owner + j % 3).astype(np.int32), (stride * owner + 10).astype(np.int32))
    return (pc, ps, pe), build, owner, j


def _mixed_values(rng, n, dtype):
    if dtype == I64:
        return rng.integers(-1000, 1000, n).astype(I64)
    return np.round(rng.standard_normal(n) * 100, 2)


# ---- a few matches under one probe ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [I64, F64], ids=["i64", "f64"])
def test_one_probe_with_few_matches(eng, dj, dtype):
    counts = [1, 2, 3, WAVE - 1, WAVE, WAVE + 1]
    probe, build, _, _ = _stacks(counts)
    v = _mixed_values(np.random.default_rng(1), len(build[0]), dtype)
    for strict in (True, False):
        _, n = check(eng, dj, probe, build, 1, strict, v, None, Q16, UP16, f"few matches strict={strict}")
        assert n.tolist() == counts


# ---- the rank the device chooses ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [I64, F64], ids=["i64", "f64"])
def test_rank_arithmetic(eng, dj, dtype):
    """Probe k matches exactly k rows whose values are 0 .. k - 1 in shuffled row order: the answer IS the rank, so it shows which
    rank the device formed from q (k - 1) -- a contracted or float32 product lands on another rank for some (k, q)."""
    counts = np.arange(1, 301)
    probe, build, owner, j = _stacks(counts)
    got, n = check(eng, dj, probe, build, 1, True, j.astype(dtype), None, Q16, UP16, "ranks")
    lo, hi, _ = range_op.quantile_ranks(counts[:, None], np.array(QS8)[None, :])
    assert (n == counts).all() and (got[:, :8] == lo).all() and (got[:, 8:] == hi).all()
    assert (lo != hi).sum() > 1000


# ---- the walk: wavefront sub-ranges, chunks, tiles ----------------------------------------------------------------------------------

@pytest.mark.parametrize("thresholded", [pytest.param(False, id="plain"), pytest.param(True, id="thresh")])
def test_runs_across_sub_range_and_chunk_boundaries(eng, dj, thresholded):
    # one tile per case: `before` candidates of a first probe, then a probe of `run` candidates that begins there
    cases = [(before, run) for before in (0, 3, PER - 1, PER, PER + 1, CHUNK - 1, CHUNK, CHUNK + 1) for run in (PER + 1, CHUNK - 1, CHUNK + 1)]
    cases += [(5, 2 * CHUNK + CHUNK // 2), (CHUNK - 2, 2 * CHUNK + CHUNK // 2 + 1)]
    rows = U.rows_per_workgroup(len(Q3))
    counts, slots = [], []
    for t, (before, run) in enumerate(cases):
        counts += [before, run, 3]
        slots += [t * rows + 5, t * rows + 6, t * rows + rows - 7]
    probe, build, _, _ = _stacks(counts, slots, len(cases) * rows)
    rng = np.random.default_rng(9)
    thr = dict(min_overlap=2) if thresholded else {}
    for dtype in (I64, F64):
        v = _mixed_values(rng, len(build[0]), dtype)
        _, n = check(eng, dj, probe, build, 1, True, v, np.arange(len(v)) % 5 != 0, Q3, UP3, "runs", **thr)
        assert n.sum() > 0.7 * sum(counts)


def test_tile_edges_of_the_probe_side(eng, dj):
    rng = np.random.default_rng(3)
    build = random_side(rng, 3000, 2, 6000, 400)
    v = _mixed_values(rng, 3000, F64)
    p16 = U.rows_per_workgroup(16)
    for n_probe, q, up in ((TILE + 1, [0.5], [0]), (2 * TILE, Q3, UP3), (p16 + 1, Q16, UP16), (3 * p16 - 1, Q16, UP16),
                           (U.rows_per_workgroup(3) + 1, Q3, UP3)):
        probe = random_side(rng, n_probe, 2, 6000, 300)
        _, n = check(eng, dj, probe, build, 2, n_probe % 2 == 0, v, None, q, up, f"{n_probe} probes, {len(q)} requests")
        assert n.sum() > 10 * n_probe


def test_empty_tile_between_two_full_ones(eng, dj):
    rng = np.random.default_rng(4)
    build = random_side(rng, 2000, 1, 5000, 300)
    a, b = random_side(rng, TILE, 1, 5000, 200), random_side(rng, TILE, 1, 5000, 200)
    hole = (np.full(TILE, OUTSIDE, np.int32), np.zeros(TILE, np.int32), np.ones(TILE, np.int32))
    probe = tuple(np.concatenate([x, h, y]) for x, h, y in zip(a, hole, b))
    _, n = check(eng, dj, probe, build, 1, True, _mixed_values(rng, 2000, I64), None, [0.5], [1], "hole")
    assert not n[TILE:2 * TILE].any() and n[:TILE].sum() > 1000 and n[2 * TILE:].sum() > 1000


# ---- the order of the keys ----------------------------------------------------------------------------------------------------------

def _cycled(pool, counts, dtype):
    """Values for _stacks(counts): probe k sees pool[(k + 0 .. counts[k] - 1) mod len(pool)] -- repeats once counts[k] > len(pool)."""
    def f(owner, j):
        return np.asarray(pool, dtype)[(owner + j) % len(pool)]
    return f


def test_key_order_int64(eng, dj):
    pool = [np.iinfo(I64).min, -1, 0, 1, np.iinfo(I64).max]
    counts = [1, 2, 3, 4, 5, 7, 11, 40]
    probe, build, owner, j = _stacks(counts)
    v = _cycled(pool, counts, I64)(owner, j)
    exp, _ = check(eng, dj, probe, build, 1, True, v, None, Q16, UP16, "int64 limits")
    assert exp.min() == np.iinfo(I64).min and exp.max() == np.iinfo(I64).max


def test_key_order_double(eng, dj):
    pool = np.array([-np.inf, -1.5, -0.0, 0.0, 5e-324, 1.0, np.inf, np.nan, -np.nan], F64)
    assert np.signbit(pool[-1]) and np.signbit(pool[2])
    counts = [1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 50]
    probe, build, owner, j = _stacks(counts)
    v = _cycled(pool, counts, F64)(owner, j)
    exp, _ = check(eng, dj, probe, build, 1, True, v, None, Q16, UP16, "double specials")
    assert np.isnan(exp).any() and np.isinf(exp).any() and (exp == 5e-324).any()
    # a NaN with a payload and a sign comes back as a NaN; it sorts above +inf
    got, _ = _host(eng, probe, build, 1, True, v, None, [1.0], [0], _engine_kw())
    has_nan = np.array([np.isnan(v[owner == k]).any() for k in range(len(counts))])
    assert (np.isnan(got[:, 0]) == has_nan).all()


@pytest.mark.parametrize("dtype", [I64, F64], ids=["i64", "f64"])
def test_keys_that_differ_in_one_bit_or_not_at_all(eng, dj, dtype):
    counts = [6, 9, 64, 3]
    probe, build, owner, j = _stacks(counts)
    base = np.uint64(0x4010000000000000)                         # 4.0 as a double
    pools = {"bit 0": np.array([base, base | np.uint64(1)]), "bit 63": np.array([base, base | np.uint64(1 << 63)]), "all equal": np.array([base])}
    for name, pool in pools.items():
        v = pool[(owner * 2 + j) % len(pool)].view(dtype)
        exp, _ = check(eng, dj, probe, build, 1, True, v, None, Q16, UP16, name)
        assert len(np.unique(exp)) == len(pool)


# ---- the predicate ---------------------------------------------------------------------------------------------------------------------

def test_candidates_that_do_not_match(eng, dj):
    # bookended rows: [0, 10) [10, 20) ... and probes [10 k + 10, 10 k + 20): half-open frames match one row, closed frames three
    nb = 600
    s = (10 * np.arange(nb)).astype(np.int32)
    build = (np.zeros(nb, np.int32), s, (s + 10).astype(np.int32))
    ps = (10 * np.arange(0, nb - 2, 3) + 10).astype(np.int32)
    probe = (np.zeros(len(ps), np.int32), ps, (ps + 10).astype(np.int32))
    v = np.random.default_rng(5).permutation(nb).astype(I64)
    _, n = check(eng, dj, probe, build, 1, True, v, None, Q3, UP3, "bookended, half-open")
    assert (n == 1).all()
    _, n = check(eng, dj, probe, build, 1, False, v, None, Q3, UP3, "bookended, closed")
    assert (n == 3).all()
    # nested rows of alternating length under one start: every other candidate of a probe fails
    s = (np.arange(3000) // 2 * 4).astype(np.int32)
    build = (np.zeros(3000, np.int32), s, np.where(np.arange(3000) % 2 == 0, s + 3, s + 4000).astype(np.int32))
    ps = (3000 + 7 * np.arange(TILE + 5)).astype(np.int32)
    probe = (np.zeros(len(ps), np.int32), ps, (ps + 2).astype(np.int32))
    _, n = check(eng, dj, probe, build, 1, True, _mixed_values(np.random.default_rng(6), 3000, F64), None, Q3, UP3, "interleaved")
    assert n.min() > 300


@pytest.mark.parametrize("strict", [pytest.param(True, id="strict"), pytest.param(False, id="weak")])
def test_thresholds(eng, dj, strict):
    rng = np.random.default_rng(11)
    probe, build = random_side(rng, TILE + 1, 24, 20_000, 300), random_side(rng, 5000, 24, 20_000, 400)
    v = _mixed_values(rng, 5000, F64)
    plain = check(eng, dj, probe, build, 24, strict, v, None, Q3, UP3, "plain")[1].sum()
    for name, thr in (("min_overlap", dict(min_overlap=7)),
                      ("probe_min", dict(probe_min=range_op.min_bases(probe[2].astype(I64) - probe[1] + (0 if strict else 1), 0.5))),
                      ("build_min", dict(build_min=range_op.min_bases(build[2].astype(I64) - build[1] + (0 if strict else 1), 0.7))),
                      ("never", dict(min_overlap=2, probe_min=rng.choice(np.array([0, 3, 40, NEVER], np.uint32), TILE + 1),
                                     build_min=rng.choice(np.array([0, 3, 40, NEVER], np.uint32), 5000)))):
        _, n = check(eng, dj, probe, build, 24, strict, v, None, Q3, UP3, name, **thr)
        assert 50 < n.sum() < plain, f"{name}: the threshold removed nothing, or everything"


def test_validity_n_values_outside_probes_and_empty_sides(eng, dj):
    rng = np.random.default_rng(21)
    probe, build = random_side(rng, TILE + 9, 2, 5000, 300), random_side(rng, 4000, 2, 5000, 400)
    probe[0][::5] = OUTSIDE
    v = _mixed_values(rng, 4000, I64)
    for name, valid in (("alternating", np.arange(4000) % 2 == 1), ("all invalid", np.zeros(4000, bool)), ("all valid", np.ones(4000, bool))):
        _, n = check(eng, dj, probe, build, 2, True, v, valid, Q3, UP3, name)
        assert not n[::5].any() and (n.sum() > 5000) == (name != "all invalid")
    for n_values in (1000, 1):
        exp, exp_n = U.expected(probe, build, 2, False, v, None, Q3, UP3, n_values=n_values)
        got, got_n = _device(dj, probe, build, 2, False, v, None, Q3, UP3, _engine_kw(), n_values=n_values)
        assert (got_n == exp_n).all()
        U.assert_same(got, exp, f"n_values {n_values}")
    none = tuple(np.empty(0, np.int32) for _ in range(3))
    for thr in ({}, dict(min_overlap=2)):
        _, n = check(eng, dj, probe, none, 2, True, np.empty(0, F64), None, Q3, UP3, "empty build", **thr)
        assert not n.any()
        out, n = check(eng, dj, none, build, 2, True, v, None, Q3, UP3, "empty probe", **thr)
        assert out.shape == (0, 3) and n.shape == (0,)


# ---- configurations ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nc", [1, 24, 300])
def test_partition_modes_and_repeats_return_identical_arrays(eng, dj, nc):
    rng = np.random.default_rng(30 + nc)
    probe, build = random_side(rng, 2 * TILE + 77, nc, 10_000, 300), random_side(rng, 6000, nc, 10_000, 2000)
    v = rng.standard_normal(6000) * np.exp(rng.uniform(-20, 20, 6000))
    valid = rng.random(6000) < 0.8
    exp, n = check(eng, dj, probe, build, nc, True, v, valid, Q3, UP3, f"{nc} contigs", min_overlap=3)
    assert n.sum() > 1000
    kw = _engine_kw(min_overlap=3)
    for pm in (0, 1, 2, 0):
        for got, got_n in (_host(eng, probe, build, nc, True, v, valid, Q3, UP3, kw, pm), _device(dj, probe, build, nc, True, v, valid, Q3, UP3, kw, pm)):
            assert (got.view(np.uint64) == exp.view(np.uint64)).all() and (got_n == n).all(), f"partition_mode {pm}"


def test_q0_q1_and_count_are_map_overlaps_min_max_count(eng, dj):
    rng = np.random.default_rng(40)
    probe, build = random_side(rng, TILE + 50, 3, 8000, 300), random_side(rng, 5000, 3, 8000, 500)
    for v in (_mixed_values(rng, 5000, I64), _mixed_values(rng, 5000, F64)):
        valid = rng.random(5000) < 0.7
        for thr in ({}, dict(min_overlap=4)):
            agg = eng.overlap_agg(probe, build, True, 3, agg=[(v, valid, ["min", "max", "count"])], **_engine_kw(**thr))[0]
            out, n = _host(eng, probe, build, 3, True, v, valid, [0.0, 1.0], [0, 0], _engine_kw(**thr))
            some = n > 0
            assert (n == agg["count"]).all() and some.sum() > TILE // 2
            assert (out[some, 0] == agg["min"][some]).all() and (out[some, 1] == agg["max"][some]).all() and not out[~some].any()


@pytest.mark.parametrize("seed", range(6))
def test_random_sweep(eng, dj, seed):
    rng = np.random.default_rng(2000 + seed)
    n, m, nc = int(rng.integers(1, 3000)), int(rng.integers(1, 2000)), int(rng.integers(1, 6))
    probe, build = random_side(rng, n, nc, int(rng.integers(500, 30_000)), 300), random_side(rng, m, nc, 20_000, int(rng.integers(1, 3000)))
    v = [rng.integers(-3, 4, m).astype(I64), rng.standard_normal(m).astype(np.float32).astype(F64), rng.standard_normal(m) * 1e300][seed % 3]
    n_q = int(rng.integers(1, 17))
    q, up = rng.random(n_q).tolist(), rng.integers(0, 2, n_q).tolist()
    thr = [{}, dict(min_overlap=int(rng.integers(1, 50)))][seed % 2]
    check(eng, dj, probe, build, nc, bool(seed % 2), v, [None, rng.random(m) < 0.5][seed // 3], q, up, f"seed {seed}", partition_mode=int(seed % 3 == 0), **thr)


# ---- argument errors -----------------------------------------------------------------------------------------------------------------

def test_einval_and_estate(eng, dj):
    import torch
    rng = np.random.default_rng(41)
    probe, build = random_side(rng, 10, 1, 1000, 100), random_side(rng, 20, 1, 1000, 100)
    v = np.arange(20, dtype=I64)
    for q, up in (([], []), ([0.5] * 17, [0] * 17), ([1.5], [0]), ([-0.1], [0]), ([float("nan")], [1])):
        with pytest.raises(_engine.EngineError) as e:
            eng.overlap_quantiles(probe, build, True, 1, v, None, q, up)
        assert e.value.code == -1, q
    opts = _engine.make_opts(True, 1)
    dp, db = _side(probe), _side(build)
    out = torch.zeros((10, 1), dtype=torch.int64, device="cuda")
    cnt = torch.zeros(10, dtype=torch.int64, device="cuda")
    dv = _dev(v)
    call = lambda ix, thr, col, out_ptr: eng.overlap_quantiles_dev(ix, dp.as_c(), opts, thr, 20, col, [0.5], [0], out_ptr, cnt.data_ptr())
    ix = eng.index_build_dev(db.as_c(), opts, True)
    try:
        call(ix, None, (dv.data_ptr(), 0, _engine.AGG_I64), out.data_ptr())                       # the valid call
        eng.overlap_quantiles_dev(ix, dp.as_c(), opts, None, 20, (dv.data_ptr(), 0, _engine.AGG_I64), [0.5], [0], out.data_ptr(), 0)   # no counts
        for col, out_ptr, thr in (((dv.data_ptr(), 0, 7), out.data_ptr(), None),                 # unknown dtype
                                  ((0, 0, _engine.AGG_I64), out.data_ptr(), None),               # NULL values
                                  ((dv.data_ptr(), 0, _engine.AGG_I64), 0, None),                # NULL out
                                  ((dv.data_ptr(), 0, _engine.AGG_I64), out.data_ptr(), _engine.make_thresholds(0, 0, 0))):
            with pytest.raises(_engine.EngineError) as e:
                call(ix, thr, col, out_ptr)
            assert e.value.code == -1
    finally:
        ix.close()
    sweep = eng.index_build_dev(db.as_c(), opts, False, sweep_only=True)
    try:
        with pytest.raises(_engine.EngineError) as e:
            call(sweep, None, (dv.data_ptr(), 0, _engine.AGG_I64), out.data_ptr())
        assert e.value.code == _engine.IVJ_ESTATE
    finally:
        sweep.close()
    eng.sync()
