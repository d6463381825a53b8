#!/usr/bin/env python3
"""Time consensus and multi_intersect over F = 2, 8 and 64 uniform frames, device API, index builds included.

    python tools/bench_multi.py [--rows 16000000] [--contigs 24] [--steps 5] [--warmup 2] [--frames 2 8 64] [--baseline]

--rows is the TOTAL over the F frames (every frame holds rows / F), so the three frame counts sort the same number of rows.
The driver (no --step) starts one child process per frame count, each under its own `timeout -k 10`, and stops at the first
one that fails: nothing more is started on a device that has just faulted or hung.  Every child builds its uniform frames
in-process from polars_bio_amd.synth (nothing is read from outside the tree), uploads them once and times

  consensus        DeviceJoin.multi_inter(frames, ceil(F / 2), consensus=True)
  multi_intersect  DeviceJoin.multi_inter(frames, 1)
  depth_concat     DeviceJoin.depth over the concatenated rows of all frames: the same amount of sorting in one index
  union_chain      F - 1 DeviceJoin.setop(.., "union") calls folded over the frames: what a user without these calls writes
                   for the N-way union (and cannot write for "at least k of N")

One more multi_intersect call with the engine's per-kernel HIP events on splits the call into the per-frame run extraction
(`depth_*` kernels), the walk (`multi_*` kernels) and the index builds (every other kernel); a further one over prebuilt frame
indexes leaves the index of the RUNS as the only build, which separates it from the F frame index builds.  What the kernels do
not account for is host time: launches, allocations and the waits for the totals (one per frame in the run extraction).

Result: profiles/multi/bench_multi.json and, with --baseline, the rows of the subsection "N frames as position sets" of
BASELINE.md."""
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
MARK = "<!-- bench_multi -->"


def human(n):
    return f"{n // 1_000_000}M" if n % 1_000_000 == 0 else str(n)


def timed(call, steps, warmup, sync):
    for _ in range(warmup):
        res = call()
    sync()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        res = call()
        sync()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return {"ms_median": round(times[len(times) // 2], 3), "ms_min": round(times[0], 3), "ms_max": round(times[-1], 3)}, res


def kernel_split(dj, call):
    """one call with the engine's per-kernel events on -> ms of the run extraction, the walk and everything else"""
    dj.engine.enable_timing(2)
    t0 = time.perf_counter()
    call()
    dj.torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    ms = {k: v["ms"] for k, v in dj.engine.timings().items()}
    dj.engine.enable_timing(0)
    extract = sum(v for k, v in ms.items() if k.startswith("depth_"))
    walk = sum(v for k, v in ms.items() if k.startswith("multi_"))
    other = sum(ms.values()) - extract - walk
    return {"wall_ms": round(wall, 3), "extract_ms": round(extract, 3), "walk_ms": round(walk, 3), "index_ms": round(other, 3),
            "host_ms": round(wall - sum(ms.values()), 3)}


def run_step(args):
    import numpy as np
    import torch
    from polars_bio_amd import synth
    from polars_bio_amd._engine import make_opts
    from polars_bio_amd.device_api import DeviceJoin, DeviceSide

    F = args.step
    per = args.rows // F
    dj = DeviceJoin(0)
    sync = torch.cuda.synchronize
    up = lambda side: DeviceSide(*(torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in side))
    frames = [up(synth.make_side(per, 42 + f, synth.BUILD_LEN, args.contigs)) for f in range(F)]
    concat = DeviceSide(*(torch.cat([getattr(s, name) for s in frames]) for name in ("contig", "start", "end")))
    cap = 2 * per * F
    out4 = tuple(torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(3)) + (torch.empty(cap, dtype=torch.int64, device="cuda"),)
    outd = tuple(torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(4))
    k = (F + 1) // 2
    rec = {"frames": F, "rows_per_frame": per, "contigs": args.contigs, "consensus_min_frames": k, "calls": args.steps}

    rec["consensus"], res = timed(lambda: dj.multi_inter(frames, k, True, args.contigs, consensus=True, out=out4[:3]), args.steps, args.warmup, sync)
    rec["consensus"]["regions"] = int(res[0].numel())
    seg = lambda: dj.multi_inter(frames, 1, True, args.contigs, out=out4)
    rec["multi_intersect"], res = timed(seg, args.steps, args.warmup, sync)
    rec["multi_intersect"]["regions"] = int(res[0].numel())
    rec["depth_concat"], res = timed(lambda: dj.depth(concat, True, args.contigs, out=outd), args.steps, args.warmup, sync)
    rec["depth_concat"]["regions"] = int(res[0].numel())

    def chain():
        acc = frames[0]
        for other in frames[1:]:
            acc = DeviceSide(*dj.setop(acc, other, "union", True, args.contigs))
        return (acc.contig,)
    rec["union_chain"], res = timed(chain, max(1, args.steps // 2), 1, sync)
    rec["union_chain"]["regions"] = int(res[0].numel())
    rec["union_regions_of_consensus_1"] = int(dj.multi_inter(frames, 1, True, args.contigs, consensus=True, out=out4[:3])[0].numel())

    rec["split_whole_call"] = kernel_split(dj, seg)
    opts = make_opts(True, args.contigs)
    ixs = [dj.engine.index_build_dev(s.as_c(), opts, True, sweep_only=True) for s in frames]
    try:
        rec["split_prebuilt_indexes"] = kernel_split(dj, lambda: dj.multi_inter(frames, 1, True, args.contigs, indexes=ixs, out=out4))
    finally:
        for ix in ixs:
            ix.close()
    print(json.dumps(rec))


def baseline_rows(doc):
    rows = []
    for F in sorted(int(k) for k in doc):
        r = doc[str(F)]
        w, p = r["split_whole_call"], r["split_prebuilt_indexes"]
        share = lambda x: f"{x / w['wall_ms'] * 100:.0f} %"
        rows.append(
            f"| F = {F} x {human(r['rows_per_frame'])} rows {MARK} | {r['consensus']['ms_median']:.2f} (k = {r['consensus_min_frames']}, {r['consensus']['regions']:,} regions) | "
            f"{r['multi_intersect']['ms_median']:.2f} ({r['multi_intersect']['regions']:,} segments) | {r['depth_concat']['ms_median']:.2f} | "
            f"{r['union_chain']['ms_median']:.2f} | run extraction {w['extract_ms']:.2f} ms ({share(w['extract_ms'])}), frame index builds "
            f"{w['index_ms'] - p['index_ms']:.2f} ms ({share(w['index_ms'] - p['index_ms'])}), run index build {p['index_ms']:.2f} ms ({share(p['index_ms'])}), "
            f"walk {w['walk_ms']:.2f} ms ({share(w['walk_ms'])}), host (launches, allocations, {F} + 1 waits) {w['host_ms']:.2f} ms ({share(w['host_ms'])}) "
            f"of a {w['wall_ms']:.2f} ms call |")
    return rows


def write_baseline(doc):
    path = os.path.join(ROOT, "BASELINE.md")
    lines = open(path).read().split("\n")
    keep = [l for l in lines if MARK not in l]
    at = max(i for i, l in enumerate(keep) if l.startswith("| frames") and "multi_intersect" in l) + 2
    keep[at:at] = baseline_rows(doc)
    open(path, "w").write("\n".join(keep))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16_000_000, help="rows of all frames together (every frame holds rows / F)")
    ap.add_argument("--contigs", type=int, default=24)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, nargs="+", default=[2, 8, 64])
    ap.add_argument("--step", type=int, help="(child) the frame count to run")
    ap.add_argument("--baseline", action="store_true", help="also write the rows into BASELINE.md")
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    doc = {}
    for F in args.frames:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", str(F), "--rows", str(args.rows),
               "--contigs", str(args.contigs), "--steps", str(args.steps), "--warmup", str(args.warmup)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.exit(f"F = {F} ended with status {p.returncode}: nothing more is started")
        doc[str(F)] = json.loads(p.stdout.strip().split("\n")[-1])
        print(F, doc[str(F)], flush=True)
    out_dir = os.path.join(ROOT, "profiles", "multi")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "bench_multi.json")
    with open(path, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print("wrote", path)
    print("\n".join(baseline_rows(doc)))
    if args.baseline:
        write_baseline(doc)


if __name__ == "__main__":
    main()
