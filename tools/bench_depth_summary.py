#!/usr/bin/env python3
"""Time depth_summary (per probe row the maximum depth and the bases at depth thresholds) on a built index: its per-call build
share against its probe kernel, next to overlap_bases on the same index, and against the composition it replaces.

    python tools/bench_depth_summary.py [--steps 10] [--warmup 3] [--scale 1.0] [--baseline]

The driver (no --step) starts one child process per GPU step -- config 3 (100 M x 5 M, 24 contigs), then config 5 (200 M x 200 k)
-- each under its own `timeout -k 10`, and stops at the first step that fails: nothing more is started on a device that has just
faulted or hung.  Every child builds the uniform tables in-process from polars_bio_amd.synth and uploads them once.

A step builds ONE index of the build side (end order included), thresholds (1, 10, 20, 30), and reports, after warm-up:
  kernel_ms            the engine's own HIP events of one depth_summary_dev call, per launch name
  build_share_ms       of those, everything but the probe kernel: the blocks (depth_*), the block index (its sort, end order and
                       joint grid), the threshold table and the tree (depth_query_records / _tree / _lengths / _scan / _table)
  probe_kernel_ms      the depth_query launch alone
  summary_ms           the whole depth_summary_dev call (HIP events around it, median of --steps calls)
  bases_ms             overlap_bases_dev on the same index (position sums already built), and summary_over_bases
  composition_ms       the route a user had before, on the device API in the same process: DeviceJoin.depth of the build side, then
                       per threshold a filter `depth >= T` of the block tensors, an index of the filtered blocks and coverage_dev
                       (K + 1 engine calls); summary_speedup = composition / summary.  The two routes' columns are compared.

Result: one JSON line (also profiles/depth_summary/bench_depth_summary.json) and, with --baseline, a row in BASELINE.md."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "polars-bio_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

STEP_TIMEOUT_S = 540
MARK = "<!-- bench_depth_summary -->"
SHAPES = {"config3": "overlap_100M_5M_24contig", "config5": "count_200M_200k_24contig"}
THRESHOLDS = (1, 10, 20, 30)


def _sides(name, scale):
    import numpy as np
    import torch
    from polars_bio_amd import synth
    from polars_bio_amd.device_api import DeviceSide
    probe, build, nc = synth.workload(name, scale)
    dev = [DeviceSide(*(torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in side)) for side in (probe, build)]
    return dev[0], dev[1], nc


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
    from polars_bio_amd.device_api import DeviceJoin, DeviceSide
    p, b, nc = _sides(SHAPES[args.step], args.scale)
    dj = DeviceJoin(0)
    eng = dj.engine
    opts = make_opts(True, nc)
    K = len(THRESHOLDS)
    ix = eng.index_build_dev(b.as_c(), opts, True)
    md = torch.empty(p.n, dtype=torch.int32, device="cuda")
    bg = torch.empty((K, p.n), dtype=torch.int64, device="cuda")
    out = torch.empty(p.n, dtype=torch.int64, device="cuda")
    rec = {"step": args.step, "probe_rows": p.n, "build_rows": b.n, "contigs": nc, "thresholds": list(THRESHOLDS), "calls": args.steps}
    try:
        side = p.as_c()
        summary = lambda: eng.depth_summary_dev(ix, side, opts, THRESHOLDS, md.data_ptr(), bg.data_ptr())
        for _ in range(args.warmup):
            summary()
        torch.cuda.synchronize()
        eng.enable_timing(2)
        summary()
        kern = {k: round(v["ms"], 4) for k, v in eng.timings().items()}
        eng.enable_timing(0)
        rec["kernel_ms"] = kern
        rec["probe_kernel_ms"] = kern.get("depth_query", 0.0)
        rec["build_share_ms"] = round(sum(v for k, v in kern.items() if k != "depth_query"), 4)
        rec["summary_ms"] = _event_ms(torch, summary, args.steps, args.warmup)
        rec["checksum"] = [int(md.sum().item()), *(int(x) for x in bg.sum(dim=1).tolist())]
        eng.overlap_bases_dev(ix, side, opts, out.data_ptr())                # builds the position sums
        rec["bases_ms"] = _event_ms(torch, lambda: eng.overlap_bases_dev(ix, side, opts, out.data_ptr()), args.steps, args.warmup)

        cols = []

        def composition():
            cols.clear()
            bc, bs, be, bd = dj.depth(b, True, nc)
            for t in THRESHOLDS:
                keep = bd >= t
                deep = DeviceSide(bc[keep].contiguous(), bs[keep].contiguous(), be[keep].contiguous())
                cols.append(dj.coverage(p, deep, True, nc))
        rec["composition_ms"] = _event_ms(torch, composition, max(3, args.steps // 2), max(1, args.warmup // 2))
        for k in range(K):
            assert torch.equal(cols[k], bg[k]), f"the two routes disagree at threshold {THRESHOLDS[k]}"
    finally:
        ix.close()
    rec["summary_over_bases"] = round(rec["summary_ms"]["median"] / rec["bases_ms"]["median"], 3)
    rec["probe_over_bases"] = round(rec["probe_kernel_ms"] / rec["bases_ms"]["median"], 3)
    rec["summary_speedup"] = round(rec["composition_ms"]["median"] / rec["summary_ms"]["median"], 3)
    print(json.dumps(rec))


def baseline_row(doc):
    def shape(k):
        d = doc[k]
        return (f"{d['probe_rows'] // 1_000_000}M x {d['build_rows'] // 1000}k: call {d['summary_ms']['median']:.2f} ms = build share "
                f"{d['build_share_ms']:.2f} ms + probe kernel {d['probe_kernel_ms']:.2f} ms; overlap_bases {d['bases_ms']['median']:.2f} ms "
                f"(probe kernel x{d['probe_over_bases']:.2f}, call x{d['summary_over_bases']:.2f}); depth -> filter -> coverage x{len(d['thresholds'])} "
                f"{d['composition_ms']['median']:.2f} ms (x{d['summary_speedup']:.2f})")
    c3 = doc["config3"]
    return (f"| depth_summary, thresholds (1, 10, 20, 30), whole call on a built index (device API, HIP events) {MARK} | {c3['summary_ms']['median']:.2f} | "
            f"{c3['probe_rows'] / c3['summary_ms']['median'] * 1e3:.2e} probes/s | {shape('config3')}; {shape('config5')} | "
            f"one call against the K + 1-call composition in the same process: x{c3['summary_speedup']:.2f} / x{doc['config5']['summary_speedup']:.2f} | - |")


def write_baseline(doc):
    path = os.path.join(ROOT, "BASELINE.md")
    lines = open(path).read().split("\n")
    row = baseline_row(doc)
    hit = [i for i, l in enumerate(lines) if MARK in l]
    if hit:
        lines[hit[0]] = row
    else:
        at = min(i for i, l in enumerate(lines) if "<!-- bench_mean_depth -->" in l)          # next to overlap_bases
        lines.insert(at + 1, row)
    open(path, "w").write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="scale every table's rows (a quick check at a small size)")
    ap.add_argument("--step", choices=tuple(SHAPES))
    ap.add_argument("--baseline", action="store_true", help="also write the row into BASELINE.md")
    args = ap.parse_args()
    if args.step:
        return run_shape(args)
    doc = {}
    for step in SHAPES:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", step, "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--scale", str(args.scale)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.exit(f"step {step} ended with status {p.returncode}: nothing more is started")
        doc[step] = json.loads(p.stdout.strip().split("\n")[-1])
    out_dir = os.path.join(ROOT, "profiles", "depth_summary")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bench_depth_summary.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if args.baseline:
        write_baseline(doc)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
