"""ivj_merge_agg / ivj_merge_agg_dev and pb.merge(agg=...) on the GPU against the literal group-by of tests/_merge_agg_util.py.

Integer results are compared bit for bit.  Double columns hold integer values with |sum| < 2^53, so every summation order is
exact and they are compared bit for bit too; one case sums random doubles and checks the derivable bound
|got - fsum| <= (count - 1) * 2^-53 * sum|x| per cluster.  The merged table is always compared with ivj_merge's.  Shapes are
built around T = the kernel's tile (read from its header): each frame is a few thousand rows."""
import ctypes as C
import math

import numpy as np
import pandas as pd
import pyarrow as pa
import pytest

import polars_bio_amd as pb
from polars_bio_amd import _engine
import _merge_agg_util as M

pytestmark = pytest.mark.gpu

I64, F64 = np.int64, np.float64
T = M.kernel_tile()
ALL = ["sum", "min", "max", "mean", "count"]
EINVAL, ECAPACITY = -1, _engine.IVJ_ECAPACITY


@pytest.fixture(scope="module")
def eng():
    return _engine.Engine(0)


@pytest.fixture(scope="module")
def join():
    from polars_bio_amd.device_api import DeviceJoin
    return DeviceJoin(0)


def frame_of_sizes(sizes, seed=0, shuffle=True):
    """One contig whose sorted order holds clusters of the given sizes, in that order: the rows of a cluster start one apart and
    are 2 long (each overlaps the next under both coordinate systems), clusters lie 10 apart.  Rows shuffled, so b_row gathers."""
    sizes = np.asarray(sizes, np.int64)
    n = int(sizes.sum())
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    k = np.repeat(np.arange(len(sizes)), sizes)
    within = np.arange(n) - first[k]
    base = np.concatenate([[0], np.cumsum(sizes + 10)[:-1]])
    s = (base[k] + within).astype(np.int32)
    side = (np.zeros(n, np.int32), s, s + 2)
    if shuffle:
        p = np.random.default_rng(seed).permutation(n)
        side = tuple(a[p] for a in side)
    return side


def random_frame(n, nc, seed, span=40_000, maxlen=60, outside=0.0):
    rng = np.random.default_rng(seed)
    c = rng.integers(0, nc, n).astype(np.int32)
    if outside:
        c = np.where(rng.random(n) < outside, rng.choice([-1, -7, nc, nc + 5], n), c).astype(np.int32)
    s = rng.integers(0, span, n).astype(np.int32)
    return c, s, (s + rng.integers(0, maxlen, n)).astype(np.int32)


def int_values(n, seed, lo=-1000, hi=1000):
    return np.random.default_rng(seed).integers(lo, hi, n).astype(I64)


def whole_doubles(n, seed):
    """integer-valued doubles: |sum| over 10^4 rows stays far below 2^53, every order of summation is exact"""
    return np.random.default_rng(seed).integers(-(1 << 30), 1 << 30, n).astype(F64)


def dev_form(join, side, nc, strict, min_dist, columns, row_id=None, n_values=None):
    import torch
    from polars_bio_amd.device_api import DeviceSide
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ds = DeviceSide(*map(up, side), row_id=None if row_id is None else up(row_id))
    agg = [(up(v), None if m is None else up(np.asarray(m).astype(np.uint8)), ops) for v, m, ops in columns]
    *table, results = join.merge(ds, strict, nc, min_dist, agg=agg)
    return [t.cpu().numpy() for t in table], [{k: t.cpu().numpy() for k, t in r.items()} for r in results]


def check(eng, join, side, nc, strict=True, min_dist=0, columns=(), what=""):
    """host form and device form of one input against ivj_merge and the yardstick; -> number of clusters"""
    columns = list(columns)
    cid, etable = M.clusters(side, nc, strict, min_dist)
    plain = eng.merge(side, strict, nc, min_dist)
    *htable, hres = eng.merge_agg(side, strict, nc, columns, min_dist)
    dtable, dres = dev_form(join, side, nc, strict, min_dist, columns)
    for name, table in (("host", htable), ("device", dtable)):
        for k in range(4):
            assert table[k].dtype == plain[k].dtype and (table[k] == plain[k]).all(), f"{what} {name}: merged table column {k} differs from ivj_merge"
            assert (table[k] == etable[k]).all(), f"{what} {name}: merged table column {k} differs from the oracle"
    for j, (values, valid, ops) in enumerate(columns):
        exp = M.group_by(cid, len(etable[0]), values, valid)
        for name, res in (("host", hres), ("device", dres)):
            assert set(res[j]) == set(ops), (what, name, j)
            M.assert_column(res[j], exp, values.dtype, f"{what} {name} column {j}")
    return len(etable[0])


# ---- sizes around the wavefront and the tile ---------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5])
def test_sizes_around_wavefront_and_tile(eng, join, n):
    side = random_frame(n, 3, 100 + n, span=max(8 * n, 10))
    vi, vd = int_values(n, n), whole_doubles(n, n + 1)
    mask = np.random.default_rng(n).random(n) < 0.8
    ncl = check(eng, join, side, 3, True, 0, [(vi, None, ALL), (vd, mask, ALL)], f"n={n}")
    assert ncl <= n and (n < 64 or 1 < ncl < n)


def test_all_singletons(eng, join):
    n = 3 * T + 5
    side = frame_of_sizes([1] * n)
    assert check(eng, join, side, 1, True, 0, [(int_values(n, 1), None, ALL), (whole_doubles(n, 2), None, ALL)], "singletons") == n


def test_one_cluster_over_every_tile(eng, join):
    n = 3 * T + 5                                            # the middle tiles lie wholly inside the cluster
    side = frame_of_sizes([n])
    assert check(eng, join, side, 1, True, 0, [(int_values(n, 3), None, ALL), (whole_doubles(n, 4), None, ALL)], "one cluster") == 1


@pytest.mark.parametrize("edge", [T - 1, T, T + 1])
def test_cluster_boundary_on_the_tile_boundary(eng, join, edge):
    """the first cluster ends one position before / exactly at / one position after the first tile boundary; a second boundary
    does the same at the second tile boundary"""
    sizes = [edge, 2 * T - edge + (edge - T), 7, 1, 40]       # cumulative: edge, T + edge, ...
    assert sum(sizes[:2]) == T + edge
    side = frame_of_sizes(sizes, seed=edge)
    n = len(side[0])
    assert check(eng, join, side, 1, True, 0, [(int_values(n, edge), None, ALL), (whole_doubles(n, edge), None, ["sum", "mean"])], f"edge={edge}") == len(sizes)


def test_cluster_spanning_three_tiles_between_singletons(eng, join):
    sizes = [1] * (T // 2) + [2 * T] + [1] * (T // 2 + 9)      # the cluster covers positions T/2 .. 5T/2: tiles 0, 1 and 2
    side = frame_of_sizes(sizes, seed=5)
    n = len(side[0])
    check(eng, join, side, 1, True, 0, [(int_values(n, 5), None, ALL), (whole_doubles(n, 6), None, ALL)], "three tiles")


def test_two_spanning_clusters_meet_inside_a_tile(eng, join):
    sizes = [3, T + T // 2, T + T // 2 + 11, 2]                # they meet at position 3 + 3T/2, inside tile 1; the second ends in tile 3
    side = frame_of_sizes(sizes, seed=7)
    n = len(side[0])
    assert n > 3 * T
    check(eng, join, side, 1, True, 0, [(int_values(n, 7), None, ALL), (whole_doubles(n, 8), None, ALL)], "two spanning")


def test_many_contigs_and_rows_outside_the_dictionary(eng, join):
    n = 1500
    side = random_frame(n, 300, 11, span=300, maxlen=40, outside=0.1)
    assert ((side[0] < 0) | (side[0] >= 300)).sum() > 50
    ncl = check(eng, join, side, 300, True, 0, [(int_values(n, 11), None, ALL), (whole_doubles(n, 12), None, ALL)], "300 contigs")
    assert ncl > 300


@pytest.mark.parametrize("strict", [True, False])
@pytest.mark.parametrize("min_dist", [0, 1, 1000])
def test_coordinate_systems_and_min_dist(eng, join, strict, min_dist):
    n = T + 300
    side = random_frame(n, 4, 13, span=400_000, maxlen=300)
    side[1][:50] = side[2][50:100]                           # bookended pairs: merge under Weak or min_dist >= 1 only
    side[2][:50] = side[1][:50] + 5
    side[0][:50] = side[0][50:100]
    check(eng, join, side, 4, strict, min_dist, [(int_values(n, 13), None, ALL), (whole_doubles(n, 14), None, ["sum", "min", "max"])],
          f"strict={strict} min_dist={min_dist}")


# ---- values and masks --------------------------------------------------------------------------------------------------------

def test_valid_masks(eng, join):
    sizes = [5, 40, 3, T + 50, 9, 2 * T + 20, 6]               # positions: tile 2 (2T .. 3T) lies wholly inside the last big cluster
    side = frame_of_sizes(sizes, seed=0, shuffle=False)
    n = len(side[0])
    first = np.concatenate([[0], np.cumsum(sizes)])
    mask = np.random.default_rng(15).random(n) < 0.7
    mask[first[1]:first[2]] = False                          # an all-invalid cluster
    mask[first[4]:first[5]] = False                          # another, between the big ones
    assert first[5] < 2 * T and first[6] > 3 * T
    mask[2 * T:3 * T] = False                                # an all-invalid whole tile inside a cluster that has valid rows elsewhere
    p = np.random.default_rng(16).permutation(n)
    side, mask = tuple(a[p] for a in side), mask[p]
    vi, vd = int_values(n, 15), whole_doubles(n, 16)
    check(eng, join, side, 1, True, 0, [(vi, mask, ALL), (vd, mask, ALL), (vi, None, ALL), (vi, np.zeros(n, bool), ALL)], "masks")
    *_, res = eng.merge_agg(side, True, 1, [(vi, mask, ALL), (vd, mask, ALL)])
    for r in res:
        assert r["count"][1] == 0 and r["sum"][1] == 0 and r["count"][4] == 0 and r["count"][5] > 0


def test_int64_sums_wrap_as_numpy_does(eng, join):
    n = T + 77
    side = frame_of_sizes([3, 70, T - 10, 14], seed=17)
    rng = np.random.default_rng(17)
    v = ((1 << 62) - rng.integers(0, 1000, n)).astype(I64) * rng.choice([-1, 1], n).astype(I64)
    v[:5] = [np.iinfo(I64).max, np.iinfo(I64).min, np.iinfo(I64).max, -1, np.iinfo(I64).min]
    check(eng, join, side, 1, True, 0, [(v, None, ALL), (-np.abs(v), None, ALL)], "wrap")
    *_, res = eng.merge_agg(side, True, 1, [(np.full(n, 1 << 62, I64), None, ["sum"])])
    assert res[0]["sum"][1] == np.add.reduce(np.full(70, 1 << 62, I64)) == -(1 << 63)          # 70 * 2^62 = 17 * 2^64 + 2^63


def test_negative_values_nan_and_an_all_nan_cluster(eng, join):
    sizes = [4, 30, 5, T + 3, 8]
    side = frame_of_sizes(sizes, seed=0, shuffle=False)
    n = len(side[0])
    first = np.concatenate([[0], np.cumsum(sizes)])
    vd = -np.abs(whole_doubles(n, 19)) - 1.0
    vd[first[1] + 3] = np.nan                                # a NaN among numbers: sum and mean NaN, min and max numbers
    vd[first[2]:first[3]] = np.nan                           # an all-NaN cluster: everything NaN, count 5
    vd[first[3] + T // 2] = np.nan                           # a NaN inside the cluster that spans tiles
    p = np.random.default_rng(19).permutation(n)
    side, vd = tuple(a[p] for a in side), vd[p]
    check(eng, join, side, 1, True, 0, [(vd, None, ALL), (-np.abs(int_values(n, 20)) - 1, None, ALL)], "nan")
    *_, res = eng.merge_agg(side, True, 1, [(vd, None, ALL)])
    r = res[0]
    assert math.isnan(r["sum"][1]) and math.isnan(r["mean"][1]) and r["min"][1] < 0 and r["max"][1] < 0
    assert all(math.isnan(r[op][2]) for op in ("sum", "min", "max", "mean")) and r["count"][2] == 5
    assert math.isnan(r["sum"][3]) and r["max"][3] < 0 and r["count"][3] == T + 3
    assert not math.isnan(r["sum"][0]) and not math.isnan(r["sum"][4])


@pytest.mark.parametrize("ops", [["sum"], ["min"], ["max"], ["mean"], ["count"], ALL])
def test_every_shape_of_ops(eng, join, ops):
    n = T + 9
    side = random_frame(n, 2, 21, span=6000)
    check(eng, join, side, 2, True, 0, [(int_values(n, 21), None, ops), (whole_doubles(n, 22), None, ops)], f"ops={ops}")


@pytest.mark.parametrize("n_cols", [2, _engine.MAX_AGG_COLS])
def test_several_columns_in_one_call(eng, join, n_cols):
    n = T + 100
    side = random_frame(n, 3, 23, span=9000)
    rng = np.random.default_rng(23)
    columns = []
    for k in range(n_cols):
        values = int_values(n, 30 + k) if k % 2 == 0 else whole_doubles(n, 30 + k)
        mask = None if k % 3 == 0 else rng.random(n) < 0.6
        columns.append((values, mask, [ALL[k % 5], ALL[(k + 2) % 5]]))
    check(eng, join, side, 3, False, 2, columns, f"{n_cols} columns")


def test_random_doubles_within_the_summation_bound(eng, join):
    """any order of n - 1 additions of doubles stays within (n - 1) * u * sum|x| of the exact sum (u = 2^-53, first order; the
    second-order term is below 1e-9 of it at these sizes and the bound is not tight by a factor of the tree depth)"""
    sizes = [1, 2, 63, 64, 65, 500, T + 700, 9]
    side = frame_of_sizes(sizes, seed=25)
    n = len(side[0])
    v = np.random.default_rng(25).standard_normal(n) * np.exp(np.random.default_rng(26).uniform(-20, 20, n))
    cid, etable = M.clusters(side, 1, True, 0)
    for name, res in (("host", eng.merge_agg(side, True, 1, [(v, None, ["sum", "count", "min", "max"])])[4]),
                      ("device", dev_form(join, side, 1, True, 0, [(v, None, ["sum", "count", "min", "max"])])[1])):
        r = res[0]
        for k in range(len(sizes)):
            x = v[cid == k]
            exact, bound = math.fsum(x), (len(x) - 1) * 2.0 ** -53 * math.fsum(np.abs(x))
            print(f"{name} cluster {k}: n={len(x)} |got - fsum|={abs(r['sum'][k] - exact):.3e} bound={bound:.3e}")
            assert r["count"][k] == len(x) and abs(r["sum"][k] - exact) <= bound, (name, k)
            assert r["min"][k] == x.min() and r["max"][k] == x.max()


def test_results_repeat_bit_for_bit(eng):
    n = 3 * T + 5
    side = random_frame(n, 2, 27, span=3 * n)
    v = np.random.default_rng(27).standard_normal(n)
    runs = [eng.merge_agg(side, True, 2, [(v, None, ALL)])[4][0] for _ in range(3)]
    for r in runs[1:]:
        for op in ALL:
            assert (r[op].view(np.uint64) == runs[0][op].view(np.uint64)).all(), op


# ---- the device form's protocol ----------------------------------------------------------------------------------------------

def _dev_call(join, side, nc, capacity, cols, outs, n_values, strict=True, min_dist=0, row_id=None):
    """ivj_merge_agg_dev on torch buffers of `capacity` entries -> (n_merged, fits, table tensors)"""
    import torch
    from polars_bio_amd.device_api import DeviceSide
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    ds = DeviceSide(*map(up, side), row_id=None if row_id is None else up(row_id))
    opts = _engine.make_opts(strict, nc)
    ix = join.engine.index_build_dev(ds.as_c(), opts, False, sweep_only=True)
    try:
        table = [torch.full((max(capacity, 1),), -77, dtype=dt, device=dev) for dt in (torch.int32, torch.int32, torch.int32, torch.int64)]
        n, fits = join.engine.merge_agg_dev(ix, opts, min_dist, capacity, *(t.data_ptr() for t in table), n_values, cols, outs)
        torch.cuda.synchronize()
    finally:
        ix.close()
    return n, fits, table


def test_device_form_capacity_protocol(join):
    import torch
    dev = torch.device("cuda", 0)
    n = T + 40
    side = random_frame(n, 2, 29, span=5 * n)
    v = torch.from_numpy(int_values(n, 29)).to(dev)
    _, etable = M.clusters(side, 2, True, 0)
    total = len(etable[0])
    assert total > 100
    outs = {name: torch.full((total,), -77, dtype=torch.float64 if name == "mean" else torch.int64, device=dev) for name in ALL}
    ptrs = [{name: t.data_ptr() for name, t in outs.items()}]
    cols = [(v.data_ptr(), 0, _engine.AGG_I64, 31)]
    got, fits, table = _dev_call(join, side, 2, total - 1, cols, ptrs, n)
    assert not fits and got == total                           # too small: the total is reported, nothing is written
    assert all((t.cpu().numpy() == -77).all() for t in table) and all((t.cpu().numpy() == -77).all() for t in outs.values())
    got, fits, _ = _dev_call(join, side, 2, 0, cols, [{}], n)
    assert not fits and got == total                           # capacity 0 with no buffers at all: a count query
    got, fits, table = _dev_call(join, side, 2, total, cols, ptrs, n)
    assert fits and got == total and (table[1].cpu().numpy()[:total] == etable[1]).all()
    assert (outs["count"].cpu().numpy() == etable[3]).all()


def test_device_form_reads_values_by_reported_row(join):
    """an index built from a side with row_id: the values are read at the ids, and ids outside [0, n_values) contribute nothing"""
    n = 900
    side = random_frame(n, 2, 31, span=4000)
    rng = np.random.default_rng(31)
    row_id = rng.permutation(n).astype(np.int32) + 5           # ids 5 .. n + 4 into a value column of n entries: the last 5 fall outside
    row_id[:7] = [-1, -2, n, n + 1000, 2 ** 31 - 1, -2 ** 31, 0]
    values = int_values(n, 32)
    inside = (row_id >= 0) & (row_id < n)
    assert 5 <= (~inside).sum() < 20
    cid, etable = M.clusters(side, 2, True, 0)
    exp = M.group_by(cid, len(etable[0]), values[np.where(inside, row_id, 0)], inside)
    _, res = dev_form(join, side, 2, True, 0, [(values, None, ALL)], row_id=row_id)
    M.assert_column(res[0], exp, I64, "row_id")


def _rc(fn):
    with pytest.raises(_engine.EngineError) as e:
        fn()
    return e.value.code


def test_invalid_arguments(eng, join):
    import torch
    dev = torch.device("cuda", 0)
    n = 200
    side = random_frame(n, 2, 33)
    v = int_values(n, 33)
    host = lambda agg: eng.merge_agg(side, True, 2, agg)
    assert _rc(lambda: host([])) == EINVAL                                                     # n_cols = 0
    assert _rc(lambda: host([(v, None, 1)] * (_engine.MAX_AGG_COLS + 1))) == EINVAL            # n_cols = 17
    assert _rc(lambda: host([(v, None, 0)])) == EINVAL                                         # ops == 0
    assert _rc(lambda: host([(v, None, 32)])) == EINVAL and _rc(lambda: host([(v, None, 1 | 64)])) == EINVAL      # unknown bits
    assert len(host([(v, None, 1)] * _engine.MAX_AGG_COLS)[4]) == _engine.MAX_AGG_COLS

    def raw_host(values_ptr, dtype, ops=1):
        fs, keep = _engine._host_side(*side)
        cols = (_engine._AggIn * 1)(_engine._AggIn(values_ptr, None, dtype, ops))
        outs = (_engine._AggOut * 1)()
        out = _engine._Merged()
        rc = eng.L.ivj_merge_agg(eng.h, C.byref(fs), C.byref(_engine.make_opts(True, 2)), 0, 1, cols, C.byref(out), outs)
        if rc == 0:
            eng.L.ivj_merge_agg_free(C.byref(out), outs, 1)
        return rc
    assert raw_host(v.ctypes.data, 2) == EINVAL and raw_host(v.ctypes.data, -1) == EINVAL       # unknown dtype
    assert raw_host(None, _engine.AGG_I64) == EINVAL                                            # NULL values with rows present
    assert raw_host(v.ctypes.data, _engine.AGG_I64) == 0

    tv = torch.from_numpy(v).to(dev)
    cap = n
    outs = {name: torch.empty(cap, dtype=torch.float64 if name == "mean" else torch.int64, device=dev) for name in ALL}
    full = {name: t.data_ptr() for name, t in outs.items()}
    ok = (tv.data_ptr(), 0, _engine.AGG_I64, 31)
    call = lambda cols, ptrs, n_values=n: _dev_call(join, side, 2, cap, cols, ptrs, n_values)
    assert call([ok], [full])[1]
    assert _rc(lambda: call([], [])) == EINVAL
    assert _rc(lambda: call([ok] * 17, [full] * 17)) == EINVAL
    assert _rc(lambda: call([(tv.data_ptr(), 0, _engine.AGG_I64, 0)], [full])) == EINVAL
    assert _rc(lambda: call([(tv.data_ptr(), 0, _engine.AGG_I64, 128)], [full])) == EINVAL
    assert _rc(lambda: call([(tv.data_ptr(), 0, 7, 31)], [full])) == EINVAL
    assert _rc(lambda: call([(0, 0, _engine.AGG_I64, 31)], [full])) == EINVAL
    for name in ALL:                                                                            # a NULL output of a requested operation
        assert _rc(lambda: call([ok], [{k: p for k, p in full.items() if k != name}])) == EINVAL, name
        bit = _engine.AGG_OPS[name]                                                              # ... which is fine when not asked for
        assert call([(tv.data_ptr(), 0, _engine.AGG_I64, 31 & ~bit)], [{k: p for k, p in full.items() if k != name}])[1]


# ---- the front door on the GPU -----------------------------------------------------------------------------------------------

def _front_frame(n=3000, seed=35, zero_based=True):
    rng = np.random.default_rng(seed)
    s = rng.integers(0, 60_000, n)
    score = rng.integers(-300, 300, n).astype(np.int16)
    qual = rng.integers(0, 4000, n).astype(np.float32) / 8          # multiples of 1/8: float32 and float64 sums are exact
    qual[rng.random(n) < 0.15] = np.nan                              # nulls in the value column (pandas: NaN = missing)
    chrom = rng.choice(["chr1", "chr2", "chr10", "chrX"], n).astype(object)
    chrom[rng.random(n) < 0.03] = None                               # rows with a null chrom
    df = pd.DataFrame({"chrom": chrom, "start": s, "end": s + rng.integers(1, 50, n), "strand": rng.choice(["+", "-"], n),
                       "score": score, "qual": qual, "depth": rng.integers(0, 1 << 40, n)})
    df.attrs["coordinate_system_zero_based"] = zero_based
    return df


def _group_by_clusters(df, keys=("chrom",)):
    """pb.cluster + pandas group-by on the same frame -> the table pb.merge(agg=...) must give, in its order"""
    parts = []
    live = df[df["chrom"].notna()]
    live = live.assign(qual=live["qual"].astype(np.float64))         # pandas reduces a float32 column in float32; the values are exact in both
    for _, sub in live.groupby(list(keys[1:]), sort=True) if len(keys) > 1 else [(None, live)]:
        sub = sub.copy()
        sub.attrs["coordinate_system_zero_based"] = df.attrs["coordinate_system_zero_based"]
        cl = pb.cluster(sub, output_type="pandas.DataFrame")
        g = cl.groupby("cluster", sort=True)
        out = g.agg(chrom=("chrom", "first"), start=("cluster_start", "first"), end=("cluster_end", "first"), **{k: (k, "first") for k in keys[1:]},
                    n_intervals=("start", "size"), score_sum=("score", "sum"), score_min=("score", "min"), score_max=("score", "max"),
                    score_mean=("score", "mean"), qual_count=("qual", "count"), qual_sum=("qual", "sum"), qual_max=("qual", "max"),
                    qual_mean=("qual", "mean"), depth_sum=("depth", "sum"))
        parts.append(out)
    return pd.concat(parts).sort_values(list(keys) + ["start"]).reset_index(drop=True)


AGG = {"score": ["sum", "min", "max", "mean"], "qual": ["count", "sum", "max", "mean"], "depth": "sum"}


@pytest.mark.parametrize("kind", ["pandas", "pyarrow"])
@pytest.mark.parametrize("zero_based", [True, False])
def test_front_door_against_cluster_and_groupby(kind, zero_based):
    df = _front_frame(zero_based=zero_based)
    exp = _group_by_clusters(df)
    frame = df
    if kind == "pyarrow":
        frame = pa.Table.from_pandas(df, preserve_index=False).replace_schema_metadata(
            {b"coordinate_system_zero_based": b"true" if zero_based else b"false"})
    res = pb.merge(frame, output_type="pandas.DataFrame", agg=AGG)
    assert list(res.columns) == list(exp.columns)
    assert res["score_min"].dtype == np.int16 and res["score_max"].dtype == np.int16 and res["qual_max"].dtype == np.float32
    assert res["score_sum"].dtype == np.int64 and res["qual_sum"].dtype == np.float64 and res["qual_count"].dtype == np.int64
    assert exp["qual_count"].min() == 0 and exp["n_intervals"].max() > 5         # some cluster has nulls only
    assert res["qual_max"].isna().sum() == (exp["qual_count"] == 0).sum() == res["qual_mean"].isna().sum()
    assert (res.loc[exp["qual_count"] == 0, "qual_sum"] == 0).all()
    pd.testing.assert_frame_equal(res, exp, check_dtype=False, check_exact=True)
    plain = pb.merge(frame, output_type="pandas.DataFrame")
    pd.testing.assert_frame_equal(res[list(plain.columns)], plain)


def test_front_door_on_cols_strand():
    df = _front_frame(seed=37)
    exp = _group_by_clusters(df, keys=("chrom", "strand"))
    res = pb.merge(df, on_cols=["strand"], output_type="pandas.DataFrame", agg=AGG)
    assert list(res.columns) == list(exp.columns)
    pd.testing.assert_frame_equal(res, exp, check_dtype=False, check_exact=True)
    arrow = pb.merge(df, on_cols=["strand"], min_dist=25, output_type="pyarrow.Table", agg={"qual": ["min", "mean"]})
    assert arrow.schema.field("qual_min").type == pa.float32() and arrow.schema.field("qual_mean").type == pa.float64()
    assert arrow.num_rows < len(res)
