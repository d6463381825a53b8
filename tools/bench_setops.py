#!/usr/bin/env python3
"""Time the set operations on two uniform frames against depth on each frame alone, device API, index builds included.

    python tools/bench_setops.py [--rows 50000000] [--contigs 24] [--steps 10] [--warmup 3] [--baseline]

The driver (no --step) starts one child process per GPU step -- `set_intersect`, `set_stats`, `depth_a`, `depth_b` -- each
under its own `timeout -k 10`, and stops at the first step that fails: nothing more is started on a device that has just
faulted or hung.  Every child builds both uniform tables in-process from polars_bio_amd.synth (nothing is read from outside
the tree), uploads them once and times `DeviceJoin.setop(.., "intersection")` / `DeviceJoin.set_stats` / `DeviceJoin.depth`
(each call sorts its frames into indexes first).  depth on each frame alone is the floor: the union step of a set operation
is that walk, keeping only the transitions between depth 0 and depth >= 1.

Result: profiles/setops/bench_setops.json -- ms per call, regions produced, the per-kernel times of one extra call (the
engine's own HIP events) with the set walk (`setop_*` kernels) and the two union steps (`depth_*` kernels) summed -- and,
with --baseline, a row in BASELINE.md with the set walk's share of the whole call."""
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

STEP_TIMEOUT_S = 420
STEPS = ("set_intersect", "set_stats", "depth_a", "depth_b")
MARK = "<!-- bench_setops -->"


def human(n):
    return f"{n // 1_000_000}M" if n % 1_000_000 == 0 else str(n)


def run_step(args):
    import numpy as np
    import torch
    from polars_bio_amd import synth
    from polars_bio_amd.device_api import DeviceJoin, DeviceSide

    dj = DeviceJoin(0)
    up = lambda side: DeviceSide(*(torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in side))
    a = up(synth.make_side(args.rows, 42, synth.BUILD_LEN, args.contigs))
    b = up(synth.make_side(args.rows, 43, synth.BUILD_LEN, args.contigs))
    if args.step == "set_intersect":
        out = tuple(torch.empty(2 * args.rows, dtype=torch.int32, device="cuda") for _ in range(3))
        call = lambda: dj.setop(a, b, "intersection", True, args.contigs, out=out)
    elif args.step == "set_stats":
        call = lambda: dj.set_stats(a, b, True, args.contigs)
    else:
        frame = a if args.step == "depth_a" else b
        out = tuple(torch.empty(2 * args.rows, dtype=torch.int32, device="cuda") for _ in range(4))
        call = lambda: dj.depth(frame, True, args.contigs, out=out)
    for _ in range(args.warmup):
        res = call()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        res = call()                                  # returns after the engine's own wait for the region total / the sums
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    rec = {"step": args.step, "rows_per_frame": args.rows, "contigs": args.contigs, "ms_per_call_median": times[len(times) // 2],
           "ms_per_call_min": times[0], "ms_per_call_max": times[-1], "calls": args.steps}
    if args.step == "set_stats":
        rec.update(zip(("only_a", "only_b", "both", "n_intersections"), res))
    else:
        rec["results"] = int(res[0].numel())
    # one more call with the engine's per-kernel events on (kept out of the timed calls)
    dj.engine.enable_timing(2)
    call()
    rec["kernel_ms"] = {k: round(v["ms"], 4) for k, v in sorted(dj.engine.timings().items(), key=lambda kv: -kv[1]["ms"])}
    dj.engine.enable_timing(0)
    rec["set_walk_ms"] = round(sum(v for k, v in rec["kernel_ms"].items() if k.startswith("setop_")), 4)
    rec["depth_walk_ms"] = round(sum(v for k, v in rec["kernel_ms"].items() if k.startswith("depth_")), 4)
    print(json.dumps(rec))


def baseline_row(doc):
    i, s, da, db = (doc[k] for k in STEPS)
    floor = da["ms_per_call_median"] + db["ms_per_call_median"]
    return (f"| set_intersect 2 x {human(i['rows_per_frame'])} rows, {i['contigs']} contigs (device API, index builds included) {MARK} | "
            f"{i['ms_per_call_median']:.2f} | {i['results'] / i['ms_per_call_median'] * 1e3:.2e} regions/s ({i['results']:,} regions) | "
            f"set walk {i['set_walk_ms']:.2f} ms = {i['set_walk_ms'] / i['ms_per_call_median'] * 100:.1f} % of the call, union steps "
            f"{i['depth_walk_ms']:.2f} ms; set_stats {s['ms_per_call_median']:.2f} ms (walk {s['set_walk_ms']:.2f} ms); depth on each frame alone "
            f"{da['ms_per_call_median']:.2f} + {db['ms_per_call_median']:.2f} = {floor:.2f} ms | 32 B per row read by the two union steps + "
            f"12 B per run read twice and 12 B per region written by the walk | — |")


def write_baseline(doc):
    path = os.path.join(ROOT, "BASELINE.md")
    lines = open(path).read().split("\n")
    row = baseline_row(doc)
    hit = [i for i, l in enumerate(lines) if MARK in l]
    if hit:
        lines[hit[0]] = row
    else:
        at = min(i for i, l in enumerate(lines) if "<!-- bench_depth -->" in l)
        lines.insert(at + 1, row)
    open(path, "w").write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000_000, help="rows of each of the two frames")
    ap.add_argument("--contigs", type=int, default=24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--baseline", action="store_true", help="also write the row into BASELINE.md")
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    doc = {}
    for step in STEPS:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", step, "--rows", str(args.rows),
               "--contigs", str(args.contigs), "--steps", str(args.steps), "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.exit(f"step {step} ended with status {p.returncode}: nothing more is started")
        doc[step] = json.loads(p.stdout.strip().split("\n")[-1])
        print(step, doc[step], flush=True)
    out_dir = os.path.join(ROOT, "profiles", "setops")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "bench_setops.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", path)
    print(baseline_row(doc))
    if args.baseline:
        write_baseline(doc)


if __name__ == "__main__":
    main()
