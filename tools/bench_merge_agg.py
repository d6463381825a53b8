#!/usr/bin/env python3
"""Time merge with aggregates (ivj_merge_agg_dev) on the benchmark's 5 M-row build side against plain merge and against the route
a user had before it, for three cluster shapes.

    python tools/bench_merge_agg.py [--rows 5000000] [--steps 10] [--warmup 3]

One process, one GPU; the index of each shape is built once (sweep-only) and every timed call runs on it.  Per shape:
  merge_ms        (a) ivj_merge_dev alone
  agg_i64_ms      (b) ivj_merge_agg_dev, one int64 column, all five operations
  agg_f64_ms          ... one float64 column, all five
  agg_4cols_ms        ... two int64 and two float64 columns, all five each
  route_ms        (c) ivj_cluster_dev + the cluster ids copied to the host + a numpy group-by there (stable argsort of the ids,
                      np.add.reduceat / np.minimum.reduceat / np.maximum.reduceat, counts from the boundaries), one int64 column;
                      its three parts are reported too
Device times are HIP events around the call (median of --steps after --warmup); the host part of (c) is a wall clock (median of 3).
The three shapes -- the side as synth.make_side draws it, the same rows respaced into singletons, and one cluster per contig --
stand side by side: (b) must not depend on the distribution of the cluster sizes.  (b)'s int64 sums are checked against (c)'s.
Result: one JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "polars-bio_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

N_CONTIGS = 24


def shapes(n):
    import numpy as np
    from polars_bio_amd import synth
    drawn = synth.make_side(n, 43, synth.BUILD_LEN, N_CONTIGS)
    p = np.random.default_rng(7).permutation(n)
    contig = (np.arange(n) % N_CONTIGS).astype(np.int32)[p]
    start = ((np.arange(n) // N_CONTIGS) * 4).astype(np.int32)[p]
    return {"as_generated": drawn,
            "all_singletons": (contig, start, start + 2),          # 2 long, 4 apart: nothing overlaps
            "one_cluster_per_contig": (contig, start, start + 8)}    # 8 long, 4 apart: every row reaches the next


def event_ms(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return {"median": round(times[len(times) // 2], 4), "min": round(times[0], 4), "max": round(times[-1], 4)}


def host_group_by(np, cid, values):
    order = np.argsort(cid, kind="stable")
    c, v = cid[order], values[order]
    first = np.flatnonzero(np.concatenate([[True], c[1:] != c[:-1]]))
    return (np.add.reduceat(v, first), np.minimum.reduceat(v, first), np.maximum.reduceat(v, first),
            np.diff(np.concatenate([first, [len(c)]])))


def run_shape(torch, np, dj, side, steps, warmup):
    from polars_bio_amd._engine import AGG_F64, AGG_I64, make_opts
    from polars_bio_amd.device_api import DeviceSide
    eng = dj.engine
    n = len(side[0])
    ds = DeviceSide(*(torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in side))
    opts = make_opts(True, N_CONTIGS)
    rng = np.random.default_rng(11)
    vi_host = rng.integers(-1000, 1000, n).astype(np.int64)
    vi = [torch.from_numpy(vi_host).cuda(), torch.from_numpy(rng.integers(0, 1 << 40, n).astype(np.int64)).cuda()]
    vf = [torch.from_numpy(rng.standard_normal(n)).cuda(), torch.from_numpy(rng.random(n)).cuda()]
    table = [torch.empty(n, dtype=dt, device="cuda") for dt in (torch.int32, torch.int32, torch.int32, torch.int64)]
    tptr = [t.data_ptr() for t in table]
    names = ("sum", "min", "max", "mean", "count")

    def outs(v):
        return {k: torch.empty(n, dtype=torch.float64 if k == "mean" else torch.int64 if k == "count" else v.dtype, device="cuda") for k in names}
    o = [outs(v) for v in (vi[0], vf[0], vi[1], vf[1])]
    ptrs = [{k: t.data_ptr() for k, t in d.items()} for d in o]
    col = lambda v: (v.data_ptr(), 0, AGG_I64 if v.dtype == torch.int64 else AGG_F64, 31)
    ix = eng.index_build_dev(ds.as_c(), opts, False, sweep_only=True)
    rec = {"rows": n}
    try:
        n_merged, fits = eng.merge_dev(ix, opts, 0, n, *tptr)
        assert fits
        rec["clusters"] = n_merged
        rec["merge_ms"] = event_ms(torch, lambda: eng.merge_dev(ix, opts, 0, n, *tptr), steps, warmup)
        rec["agg_i64_ms"] = event_ms(torch, lambda: eng.merge_agg_dev(ix, opts, 0, n, *tptr, n, [col(vi[0])], ptrs[:1]), steps, warmup)
        rec["agg_f64_ms"] = event_ms(torch, lambda: eng.merge_agg_dev(ix, opts, 0, n, *tptr, n, [col(vf[0])], ptrs[1:2]), steps, warmup)
        four = [col(v) for v in (vi[0], vf[0], vi[1], vf[1])]
        rec["agg_4cols_ms"] = event_ms(torch, lambda: eng.merge_agg_dev(ix, opts, 0, n, *tptr, n, four, ptrs), steps, warmup)
        cid = torch.empty(n, dtype=torch.int64, device="cuda")
        cs, ce = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
        rec["route_cluster_ms"] = event_ms(torch, lambda: eng.cluster_dev(ix, opts, 0, cid.data_ptr(), cs.data_ptr(), ce.data_ptr()), steps, warmup)
        pinned = torch.empty(n, dtype=torch.int64).pin_memory()

        def d2h():
            pinned.copy_(cid, non_blocking=True)
        rec["route_d2h_ms"] = event_ms(torch, d2h, steps, warmup)
        torch.cuda.synchronize()
        cid_host = pinned.numpy()
        walls = []
        for _ in range(3):
            t0 = time.perf_counter()
            got = host_group_by(np, cid_host, vi_host)
            walls.append((time.perf_counter() - t0) * 1e3)
        rec["route_host_ms"] = round(sorted(walls)[1], 3)
        rec["route_ms"] = round(rec["route_cluster_ms"]["median"] + rec["route_d2h_ms"]["median"] + rec["route_host_ms"], 3)
        eng.merge_agg_dev(ix, opts, 0, n, *tptr, n, [col(vi[0])], ptrs[:1])
        torch.cuda.synchronize()
        for k, name in enumerate(("sum", "min", "max", "count")):
            assert (o[0][name][:n_merged].cpu().numpy() == got[k]).all(), f"the two routes disagree on {name}"
    finally:
        ix.close()
    m = rec["merge_ms"]["median"]
    rec["agg_i64_minus_merge_ms"] = round(rec["agg_i64_ms"]["median"] - m, 4)
    rec["agg_f64_minus_merge_ms"] = round(rec["agg_f64_ms"]["median"] - m, 4)
    rec["agg_4cols_minus_merge_ms"] = round(rec["agg_4cols_ms"]["median"] - m, 4)
    rec["route_over_agg_i64"] = round(rec["route_ms"] / rec["agg_i64_ms"]["median"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=5_000_000)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    from polars_bio_amd.device_api import DeviceJoin
    dj = DeviceJoin(0)
    doc = {name: run_shape(torch, np, dj, side, args.steps, args.warmup) for name, side in shapes(args.rows).items()}
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
