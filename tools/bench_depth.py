#!/usr/bin/env python3
"""Time depth (run-length coverage blocks) against merge on the same frame, device API, index build included.

    python tools/bench_depth.py [--rows 100000000] [--contigs 24] [--steps 10] [--warmup 3] [--baseline]

The driver (no --step) starts one child process per GPU step -- `depth`, then `merge` -- each under its own
`timeout -k 10`, and stops at the first step that fails: nothing more is started on a device that has just faulted or
hung.  Every child builds the uniform table in-process from polars_bio_amd.synth (nothing is read from outside the tree),
uploads it once and times `DeviceJoin.depth` / `DeviceJoin.merge` (each call sorts the frame into an index first -- the
same index walk for both, which is what makes merge the yardstick).

Result: profiles/depth/bench_depth_<rows>.json -- ms per call, blocks produced, algorithmic bytes (16 n read: the sorted
starts, ends and the contig column twice; 16 per block written) --, the per-kernel times of one extra call (the engine's own HIP events) with the operation's own pass summed (`depth_*` /
`cluster_*` kernels: the total minus the index build) -- and, with --baseline, a row in BASELINE.md."""
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
MARK = "<!-- bench_depth -->"


def human(n):
    return f"{n // 1_000_000}M" if n % 1_000_000 == 0 else str(n)


def run_step(args):
    import numpy as np
    import torch
    from polars_bio_amd import synth
    from polars_bio_amd.device_api import DeviceJoin, DeviceSide

    c, s, e = synth.make_side(args.rows, 43, synth.BUILD_LEN, args.contigs)
    dj = DeviceJoin(0)
    frame = DeviceSide(*(torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in (c, s, e)))
    n_out = 2 * args.rows if args.step == "depth" else args.rows
    widths = (torch.int32,) * 4 if args.step == "depth" else (torch.int32, torch.int32, torch.int32, torch.int64)
    out = tuple(torch.empty(n_out, dtype=dt, device="cuda") for dt in widths)
    call = (lambda: dj.depth(frame, True, args.contigs, out=out)) if args.step == "depth" else \
           (lambda: dj.merge(frame, True, args.contigs, out=out))
    for _ in range(args.warmup):
        res = call()
    torch.cuda.synchronize()
    times = []
    for _ in range(args.steps):
        t0 = time.perf_counter()
        res = call()                                  # returns after the engine's own wait for the block / interval total
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    n_res = int(res[0].numel())
    rec = {"step": args.step, "rows": args.rows, "contigs": args.contigs, "ms_per_call_median": times[len(times) // 2],
           "ms_per_call_min": times[0], "ms_per_call_max": times[-1], "calls": args.steps, "results": n_res}
    if args.step == "depth":
        rec["max_depth"] = int(res[3].max().item()) if n_res else 0
        rec["algorithmic_bytes"] = 16 * args.rows + 16 * n_res
    # one more call with the engine's per-kernel events on (kept out of the timed calls): the split between the index build and
    # the operation's own pass
    dj.engine.enable_timing(2)
    call()
    rec["kernel_ms"] = {k: round(v["ms"], 4) for k, v in sorted(dj.engine.timings().items(), key=lambda kv: -kv[1]["ms"])}
    dj.engine.enable_timing(0)
    own = ("depth_",) if args.step == "depth" else ("cluster_",)
    rec["own_pass_ms"] = round(sum(v for k, v in rec["kernel_ms"].items() if k.startswith(own)), 4)
    print(json.dumps(rec))


def baseline_row(doc):
    d, m = doc["depth"], doc["merge"]
    gb = d["algorithmic_bytes"] / 1e9
    return (f"| depth {human(d['rows'])} rows, {d['contigs']} contigs (device API, index build included) {MARK} | {d['ms_per_call_median']:.2f} | "
            f"{d['results'] / d['ms_per_call_median'] * 1e3:.2e} blocks/s ({d['results']:,} blocks) | own pass {d['own_pass_ms']:.2f} ms; merge on the same frame: "
            f"{m['ms_per_call_median']:.2f} ms, own pass {m['own_pass_ms']:.2f} ms ({m['results']:,} intervals) | {gb:.2f} GB algorithmic | "
            f"{gb / d['ms_per_call_median'] * 1e3 / 8000 * 100:.1f} % |")


def write_baseline(doc):
    path = os.path.join(ROOT, "BASELINE.md")
    lines = open(path).read().split("\n")
    row = baseline_row(doc)
    hit = [i for i, l in enumerate(lines) if MARK in l]
    if hit:
        lines[hit[0]] = row
    else:
        at = min(i for i, l in enumerate(lines) if l.startswith("| merge 100M rows"))       # the newest results table comes first
        lines.insert(at + 1, row)
    open(path, "w").write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--contigs", type=int, default=24)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--step", choices=("depth", "merge"))
    ap.add_argument("--baseline", action="store_true", help="also write the row into BASELINE.md")
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    doc = {}
    for step in ("depth", "merge"):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", step, "--rows", str(args.rows),
               "--contigs", str(args.contigs), "--steps", str(args.steps), "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.exit(f"step {step} ended with status {p.returncode}: nothing more is started")
        doc[step] = json.loads(p.stdout.strip().split("\n")[-1])
        print(step, doc[step], flush=True)
    out_dir = os.path.join(ROOT, "profiles", "depth")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, f"bench_depth_{human(args.rows)}.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", path)
    print(baseline_row(doc))
    if args.baseline:
        write_baseline(doc)


if __name__ == "__main__":
    main()
