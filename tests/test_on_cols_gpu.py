"""on_cols on the GPU: the front door with the HIP engine equals the per-group decomposition of every operation; the device
group-id entry (ivj_group_ids_dev) equals its host twin; DeviceJoin.group feeds the device ops; more than 256 groups, several
device slots and a full-size stranded 100M x 5M join stay exact."""
import os

import numpy as np
import pandas as pd
import pytest

import polars_bio_amd as pb
from oracle import oracle as O
from polars_bio_amd import _engine, _host as H, synth
import _on_cols_util as U
from test_on_cols import DOMAINS, numpy_group_ids, random_keys

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("on_cols", [["strand"], ["strand", "sample"]])
def test_front_door_equals_the_per_group_decomposition(on_cols):
    df1, df2 = U.pair_frames(21)
    U.check_ops(df1, df2, on_cols, batch_rows=(61, 4096))


def test_front_door_device_materialisation():
    df1, df2 = U.pair_frames(22)
    ep, eb = U.expected_pairs(df1, df2, ["strand"])
    for mat in ("device", "pairs", "host"):
        pb.set_option("ivj.materialize", mat)
        try:
            res = pb.overlap(df1, df2, on_cols=["strand"], output_type="pandas.DataFrame")
        finally:
            pb.set_option("ivj.materialize", "host")
        gp, gb = U.got_pairs(res)
        assert (gp == ep).all() and (gb == eb).all(), mat
        # the chrom columns come back from the group table, not as group ids
        assert (res["chrom_1"].to_numpy() == df1["chrom"].to_numpy()[res["id_1"].to_numpy()]).all(), mat
        assert (res["chrom_2"].to_numpy() == df2["chrom"].to_numpy()[res["id_2"].to_numpy()]).all(), mat


@pytest.fixture(scope="module")
def dj():
    import torch  # noqa: F401
    from polars_bio_amd.device_api import DeviceJoin
    return DeviceJoin(0)


def _t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()


# the DOMAINS of the CPU test (LDS-privatized mark pass, D <= 2^18) plus global-bitmap domains past 2^18
DEV_DOMAINS = DOMAINS + [(24, [11000]), (7, [300, 1000]), (2000, [1000, 1000])]


@pytest.mark.parametrize("n_contigs,cards", DEV_DOMAINS)
@pytest.mark.parametrize("n_probe,n_build", [(1, 1), (5000, 700), (1_000_000, 300_000)])
def test_device_group_ids_equal_the_host_twin(dj, n_contigs, cards, n_probe, n_build):
    from polars_bio_amd.device_api import DeviceSide
    rng = np.random.default_rng(n_contigs + 7 * len(cards) + n_build)
    pc, pcodes, bc, bcodes = random_keys(rng, n_probe, n_build, cards, n_contigs)
    hp, hb, hg, htab = H.group_ids(pc, pcodes, bc, bcodes, cards, n_contigs)
    z = lambda n: _t(np.zeros(n, np.int32))
    probe, build = DeviceSide(_t(pc), z(n_probe), z(n_probe)), DeviceSide(_t(bc), z(n_build), z(n_build))
    p2, b2, g, keys = dj.group(probe, build, [_t(c) for c in pcodes], [_t(c) for c in bcodes], cards, n_contigs)
    assert g == hg
    assert (p2.contig.cpu().numpy() == hp).all() and (b2.contig.cpu().numpy() == hb).all()
    assert (keys.cpu().numpy() == htab).all()
    epg, ebg, eg, etab = numpy_group_ids(pc, pcodes, bc, bcodes, cards, n_contigs)
    assert eg == g and (epg == hp).all()


def test_device_api_group_then_overlap_and_count(dj):
    from polars_bio_amd.device_api import DeviceSide
    probe = synth.make_side(400_000, 5, synth.PROBE_LEN, 24)
    build = synth.make_side(60_000, 6, synth.BUILD_LEN, 24)
    rng = np.random.default_rng(9)
    ps, bs = rng.integers(0, 2, len(probe[0])).astype(np.int32), rng.integers(0, 2, len(build[0])).astype(np.int32)
    p2, b2, g, keys = dj.group(DeviceSide(*(_t(a) for a in probe)), DeviceSide(*(_t(a) for a in build)), [_t(ps)], [_t(bs)], [2], 24)
    pg, bg, eg, _ = numpy_group_ids(probe[0], [ps], build[0], [bs], [2], 24)
    assert g == eg == 48
    oc = O.Side(pg, probe[1], probe[2])
    ix = O.Index(O.Side(bg, build[1], build[2]), g)
    p, b = dj.overlap(p2, b2, True, g)
    p, b = p.cpu().numpy(), b.cpu().numpy()
    ep, eb = O.overlap_fast(ix, oc, True)
    o, eo = np.lexsort((b, p)), np.lexsort((eb, ep))
    assert (p[o] == ep[eo]).all() and (b[o] == eb[eo]).all()
    assert (dj.count_overlaps(p2, b2, True, g).cpu().numpy() == O.count_overlaps_fast(ix, oc, True)).all()


def _frame(side, extra):
    df = pd.DataFrame({"chrom": np.array(synth.CONTIG_NAMES, dtype=object)[side[0]], "start": side[1].astype(np.int64),
                       "end": side[2].astype(np.int64), **extra, "id": np.arange(len(side[0]), dtype=np.int64)})
    df.attrs["coordinate_system_zero_based"] = True
    return df


def test_more_than_256_groups_stay_exact():
    """40 samples x 24 contigs = 960 groups: the automatic choice leaves the contig-aligned slice path, the result stays exact."""
    probe = synth.make_side(700_000, 31, synth.PROBE_LEN, 24)
    build = synth.make_side(80_000, 32, synth.BUILD_LEN, 24)
    rng = np.random.default_rng(33)
    names = np.array([f"s{i:02d}" for i in range(40)], dtype=object)
    s1, s2 = rng.integers(0, 40, len(probe[0])), rng.integers(0, 40, len(build[0]))
    df1, df2 = _frame(probe, {"sample": names[s1]}), _frame(build, {"sample": names[s2]})
    pg, bg, g, _ = numpy_group_ids(probe[0], [s1.astype(np.int32)], build[0], [s2.astype(np.int32)], [40], 24)
    assert g == 960
    ix = O.Index(O.Side(bg, build[1], build[2]), g)
    oc = O.Side(pg, probe[1], probe[2])
    ep, eb = O.overlap_fast(ix, oc, True)
    res = pb.overlap(df1, df2, on_cols=["sample"], output_type="pyarrow.Table")
    gp, gb = U.got_pairs(res.select(["id_1", "id_2"]).to_pandas())
    eo = np.lexsort((eb, ep))
    assert (gp == ep[eo]).all() and (gb == eb[eo]).all()
    cnt = pb.count_overlaps(df1, df2, on_cols=["sample"], output_type="pyarrow.Table")
    assert (cnt.column("count").to_numpy() == O.count_overlaps_fast(ix, oc, True)).all()


def test_two_device_slots_equal_one():
    from polars_bio_amd import multi
    probe = synth.make_side(200_000, 42, synth.PROBE_LEN, 24)
    build = synth.make_side(60_000, 43, synth.BUILD_LEN, 24)
    rng = np.random.default_rng(3)
    strands = np.array(["+", "-"], dtype=object)
    df1 = _frame(probe, {"strand": strands[rng.integers(0, 2, len(probe[0]))]})
    df2 = _frame(build, {"strand": strands[rng.integers(0, 2, len(build[0]))]})
    key = ["id_1", "id_2"]
    ref = pb.overlap(df1, df2, on_cols=["strand"], output_type="pandas.DataFrame").sort_values(key).reset_index(drop=True)
    c0 = pb.count_overlaps(df1, df2, on_cols=["strand"], output_type="pandas.DataFrame")
    n0 = pb.nearest(df1, df2, on_cols=["strand"], output_type="pandas.DataFrame")
    pb.set_option("ivj.devices", "0,0")                 # two device slots on whatever GPUs there are (as test_multi_device.py)
    try:
        got = pb.overlap(df1, df2, on_cols=["strand"], output_type="pandas.DataFrame")
        eng = _engine.default_engine()
        assert isinstance(eng, multi.MultiEngine)
        c1 = pb.count_overlaps(df1, df2, on_cols=["strand"], output_type="pandas.DataFrame")
        n1 = pb.nearest(df1, df2, on_cols=["strand"], output_type="pandas.DataFrame")
    finally:
        pb.set_option("ivj.devices", "auto")
    pd.testing.assert_frame_equal(got.sort_values(key).reset_index(drop=True), ref)
    pd.testing.assert_frame_equal(c0, c1)
    pd.testing.assert_frame_equal(n0, n1)


def test_full_size_stranded_overlap_100M_x_5M():
    """synth's 100M x 5M workload with a seeded strand column: pair total and build-row checksum of the engine == the oracle's on
    the test's own numpy-composed group ids."""
    probe, build, nc = synth.workload("overlap_100M_5M_24contig")
    rng = np.random.default_rng(2024)
    ps, bs = rng.integers(0, 2, len(probe[0])).astype(np.int32), rng.integers(0, 2, len(build[0])).astype(np.int32)
    pg = (probe[0].astype(np.int64) * 2 + ps).astype(np.int32)        # every (contig, strand) key occurs in df2: dense ids
    bg = (build[0].astype(np.int64) * 2 + bs).astype(np.int32)
    assert len(np.unique(bg)) == 2 * nc
    hp, hb, g, _ = H.group_ids(probe[0], [ps], build[0], [bs], [2], nc)
    assert g == 2 * nc and (hp == pg).all() and (hb == bg).all()
    cores = os.cpu_count() or 1
    ix = O.Index(O.Side(bg, build[1], build[2]), g)
    total, checksum = O.overlap_baseline(ix, O.Side(pg, probe[1], probe[2]), True, cores)
    eng = _engine.Engine(0)
    try:
        p, b = eng.overlap((hp, probe[1], probe[2]), (hb, build[1], build[2]), True, g)
    finally:
        eng.close()
    assert len(p) == total
    assert int(b.astype(np.int64).sum()) == checksum
    assert (ps[p] == bs[b]).all() and (probe[0][p] == build[0][b]).all()


@pytest.mark.parametrize("zero_based", [True, False])
@pytest.mark.parametrize("n_samples", [3000, 20_000])
def test_more_than_10k_groups_every_operation(n_samples, zero_based):
    """on_cols=["sample"] over 24 chroms x 3000 samples (group domain 72 k, below 2^18) and 24 x 20 000 (480 k, above it), more
    than 10 k groups on each side; 0-based (Strict) and 1-based (Weak) frames.  The front door composes the group ids on the
    host (ivj_host_group_ids); the device mark kernels on both sides of 2^18 are covered by
    test_device_group_ids_equal_the_host_twin.  Here the joins over the group ids run on the GPU."""
    rng = np.random.default_rng(90 + n_samples)
    chroms = [f"chr{i}" for i in range(1, 25)]
    samples = [f"s{i}" for i in range(n_samples)]
    df1 = U.frame(rng, 40_000, span=120, max_len=40, chroms=chroms, samples=samples)
    df2 = U.frame(rng, 30_000, span=120, max_len=40, chroms=chroms, samples=samples)
    for df in (df1, df2):
        df["strand"] = "+"                                           # (check_ops compares the strands of every pair)
        df.attrs["coordinate_system_zero_based"] = zero_based
    assert len(U.groups(df1, df2, ["sample"])) > 10_000 and len(U.groups(df2, df1, ["sample"])) > 10_000
    U.check_ops(df1, df2, ["sample"], outputs=("pandas.DataFrame", "pyarrow.Table"), batch_rows=(4096,), strict=zero_based)
