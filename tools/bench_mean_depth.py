#!/usr/bin/env python3
"""Time overlap_bases (the per-row sums behind pb.mean_depth) next to count_overlaps and coverage on the same index, and against
the route a user had before it: device overlap pairs summed on the host.

    python tools/bench_mean_depth.py [--steps 10] [--warmup 3] [--scale 1.0] [--baseline]

The driver (no --step) starts one child process per GPU step -- config 3 (100 M x 5 M, 24 contigs), config 5 (200 M x 200 k),
then the host route at config 2 size (10 M x 1 M) -- each under its own `timeout -k 10`, and stops at the first step that fails:
nothing more is started on a device that has just faulted or hung.  Every child builds the uniform tables in-process from
polars_bio_amd.synth (nothing is read from outside the tree) and uploads them once.

A shape step builds ONE index (end order included), then times with HIP events on the engine's stream, after warm-up:
  position_sums_ms   the on-demand prefix sums, once: the engine's own events of the first overlap_bases call on the index
  bases_plain_ms / bases_bucketed_ms   overlap_bases_dev, partition_mode 0 and 1 (median of --steps calls)
  count_ms / coverage_ms               count_overlaps_dev and coverage_dev on the same index in the same process
The host-route step times, per call and end to end (index build included on both sides): DeviceJoin.overlap -> pairs to the host
-> clipped lengths summed per probe with numpy, against DeviceJoin.overlap_bases -> the int64 column to the host.

Result: one JSON line (also profiles/mean_depth/bench_mean_depth.json) and, with --baseline, a row in BASELINE.md."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "polars-bio_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

STEP_TIMEOUT_S = 540
MARK = "<!-- bench_mean_depth -->"
SHAPES = {"config3": "overlap_100M_5M_24contig", "config5": "count_200M_200k_24contig"}
HOST_ROUTE = "overlap_10M_1M_1contig"


def _sides(name, scale):
    import numpy as np
    import torch
    from polars_bio_amd import synth
    from polars_bio_amd.device_api import DeviceSide
    probe, build, nc = synth.workload(name, scale)
    dev = [DeviceSide(*(torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in side)) for side in (probe, build)]
    return probe, build, dev[0], dev[1], nc


def _event_ms(torch, fn, steps, warmup):
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


def run_shape(args):
    import torch
    from polars_bio_amd._engine import make_opts
    from polars_bio_amd.device_api import DeviceJoin
    _, _, p, b, nc = _sides(SHAPES[args.step], args.scale)
    dj = DeviceJoin(0)
    eng = dj.engine
    opts = {m: make_opts(True, nc, partition_mode=m) for m in (0, 1)}
    ix = eng.index_build_dev(b.as_c(), opts[0], True)
    out = torch.empty(p.n, dtype=torch.int64, device="cuda")
    rec = {"step": args.step, "probe_rows": p.n, "build_rows": b.n, "contigs": nc, "calls": args.steps}
    try:
        side = p.as_c()
        eng.count_overlaps_dev(ix, side, opts[0], out.data_ptr())          # the tables and the joint grid exist from here on
        torch.cuda.synchronize()
        eng.enable_timing(2)
        eng.overlap_bases_dev(ix, side, opts[0], out.data_ptr())           # the first call on the index builds the position sums
        first = {k: round(v["ms"], 4) for k, v in eng.timings().items()}
        eng.enable_timing(0)
        rec["first_call_kernel_ms"] = first
        rec["position_sums_ms"] = round(sum(v for k, v in first.items() if k.startswith("position_")), 4)
        rec["bases_checksum"] = int(out.sum().item())
        rec["bases_plain_ms"] = _event_ms(torch, lambda: eng.overlap_bases_dev(ix, side, opts[0], out.data_ptr()), args.steps, args.warmup)
        rec["bases_bucketed_ms"] = _event_ms(torch, lambda: eng.overlap_bases_dev(ix, side, opts[1], out.data_ptr()), args.steps, args.warmup)
        assert int(out.sum().item()) == rec["bases_checksum"]
        rec["count_ms"] = _event_ms(torch, lambda: eng.count_overlaps_dev(ix, side, opts[0], out.data_ptr()), args.steps, args.warmup)
        rec["coverage_ms"] = _event_ms(torch, lambda: eng.coverage_dev(ix, side, opts[0], out.data_ptr()), args.steps, args.warmup)
    finally:
        ix.close()
    for k in ("plain", "bucketed"):
        rec[f"{k}_over_count"] = round(rec[f"bases_{k}_ms"]["median"] / rec["count_ms"]["median"], 3)
        rec[f"{k}_over_coverage"] = round(rec[f"bases_{k}_ms"]["median"] / rec["coverage_ms"]["median"], 3)
    print(json.dumps(rec))


def run_host_route(args):
    import numpy as np
    import torch
    from polars_bio_amd.device_api import DeviceJoin
    probe, build, p, b, nc = _sides(HOST_ROUTE, args.scale)
    dj = DeviceJoin(0)
    ps, pe, bs, be = (np.asarray(a, np.int64) for a in (probe[1], probe[2], build[1], build[2]))

    def pairs_route():
        ip, ib = dj.overlap(p, b, True, nc)
        ip, ib = ip.cpu().numpy(), ib.cpu().numpy()
        shared = np.minimum(pe[ip], be[ib]) - np.maximum(ps[ip], bs[ib])
        return np.bincount(ip, weights=shared, minlength=p.n).astype(np.int64), len(ip)      # exact: every sum is far below 2^53

    def device_route():
        return dj.overlap_bases(p, b, True, nc).cpu().numpy()

    def wall(fn):
        for _ in range(max(1, args.warmup // 2)):
            res = fn()
        times = []
        for _ in range(max(3, args.steps // 2)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            times.append((time.perf_counter() - t0) * 1e3)
        times.sort()
        return res, round(times[len(times) // 2], 3)

    (host_bases, n_pairs), pairs_ms = wall(pairs_route)
    dev_bases, device_ms = wall(device_route)
    assert (host_bases == dev_bases).all(), "the two routes disagree"
    print(json.dumps({"step": "host_route", "probe_rows": p.n, "build_rows": b.n, "pairs": n_pairs, "pairs_plus_host_sum_ms": pairs_ms,
                      "device_ms": device_ms, "speedup": round(pairs_ms / device_ms, 2)}))


def baseline_row(doc):
    def shape(k):
        d = doc[k]
        return (f"{d['probe_rows'] // 1_000_000}M x {d['build_rows'] // 1000}k: plain {d['bases_plain_ms']['median']:.2f} ms, bucketed "
                f"{d['bases_bucketed_ms']['median']:.2f} ms, position sums once {d['position_sums_ms']:.2f} ms; count_overlaps "
                f"{d['count_ms']['median']:.2f} ms (x{d['plain_over_count']:.2f}), coverage {d['coverage_ms']['median']:.2f} ms (x{d['plain_over_coverage']:.2f})")
    h = doc["host_route"]
    c3 = doc["config3"]
    return (f"| overlap_bases (mean_depth), probe kernel on a built index (device API, HIP events) {MARK} | {c3['bases_plain_ms']['median']:.2f} | "
            f"{c3['probe_rows'] / c3['bases_plain_ms']['median'] * 1e3:.2e} probes/s | {shape('config3')}; {shape('config5')} | "
            f"10M x 1M end to end: {h['device_ms']:.1f} ms against {h['pairs_plus_host_sum_ms']:.1f} ms for device pairs ({h['pairs']:,}) summed on the host "
            f"(x{h['speedup']:.1f}) | - |")


def write_baseline(doc):
    path = os.path.join(ROOT, "BASELINE.md")
    lines = open(path).read().split("\n")
    row = baseline_row(doc)
    hit = [i for i, l in enumerate(lines) if MARK in l]
    if hit:
        lines[hit[0]] = row
    else:
        at = min(i for i, l in enumerate(lines) if l.startswith("| depth 100M rows"))        # next to depth, in the newest results table
        lines.insert(at + 1, row)
    open(path, "w").write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="scale every table's rows (a quick check at a small size)")
    ap.add_argument("--step", choices=(*SHAPES, "host_route"))
    ap.add_argument("--baseline", action="store_true", help="also write the row into BASELINE.md")
    args = ap.parse_args()
    if args.step:
        return run_host_route(args) if args.step == "host_route" else run_shape(args)
    doc = {}
    for step in (*SHAPES, "host_route"):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", step, "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--scale", str(args.scale)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.exit(f"step {step} ended with status {p.returncode}: nothing more is started")
        doc[step] = json.loads(p.stdout.strip().split("\n")[-1])
    out_dir = os.path.join(ROOT, "profiles", "mean_depth")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bench_mean_depth.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if args.baseline:
        write_baseline(doc)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
