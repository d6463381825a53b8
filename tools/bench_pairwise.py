#!/usr/bin/env python3
"""Time pairwise_jaccard's two matrices over F = 4, 16 and 64 frames against the two routes a user had before it.

    python tools/bench_pairwise.py [--rows 300000] [--contigs 24] [--steps 5] [--warmup 2] [--frames 4 16 64] [--sets sparse dense]

--rows is the rows of EVERY frame.  Two frame sets:

  sparse   F independent uniform frames (polars_bio_amd.synth): few positions are shared, most masks hold one bit
  dense    F replicates of one peak set (the rows of one uniform frame, every start and end jittered per replicate): nearly every
           segment is covered by most frames, a mask of p bits costs p (p + 1) / 2 updates

The driver (no --step) starts one child process per (frame set, frame count), each under its own `timeout -k 10`, and stops at
the first one that fails: nothing more is started on a device that has just faulted or hung.  Every child uploads its frames,
builds their indexes once (all three routes start from prebuilt indexes) and times

  pairwise     DeviceJoin.multi_pairwise(frames, indexes=...): one walk, both matrices; one further call with the engine's
               per-kernel HIP events on gives the share of the reduction (`pairwise_*` kernels), of the walk that produces the
               segments (`multi_*`, `depth_*`) and of the index of the runs (every other kernel)
  set_stats    F (F - 1) / 2 + F Engine.set_stats_dev calls, one per unordered pair and one per frame (run once)
  bit_loop     DeviceJoin.multi_inter(frames, 1), the four columns copied to the host, then numpy per pair: the segments with
               both bits, their summed lengths and their run starts.  The loop is timed over at most --loop-pairs pairs and
               scaled to all of them (`pairs_timed` / `pairs` say so).

With IVJ_PAIRWISE_THREADS=256 in the environment the reduction runs with 4 wavefronts a workgroup instead of 16.
Prints one JSON document; --out also writes it to a file."""
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

STEP_TIMEOUT_S = 280


def timed(call, steps, warmup, sync):
    for _ in range(warmup):
        call()
    sync()
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        call()
        sync()
        times.append((time.perf_counter() - t0) * 1e3)
    times.sort()
    return {"ms_median": round(times[len(times) // 2], 3), "ms_min": round(times[0], 3), "ms_max": round(times[-1], 3), "calls": steps}


def make_frames(kind, F, rows, contigs):
    import numpy as np
    from polars_bio_amd import synth
    if kind == "sparse":
        return [synth.make_side(rows, 42 + f, synth.BUILD_LEN, contigs) for f in range(F)]
    c, s, e = synth.make_side(rows, 42, synth.BUILD_LEN, contigs)
    frames = []
    for f in range(F):
        rng = np.random.default_rng(1000 + f)
        js, je = rng.integers(0, 50, rows), rng.integers(0, 50, rows)
        frames.append((c, (s.astype(np.int64) + js).astype(np.int32), (e.astype(np.int64) + 50 + je).astype(np.int32)))
    return frames


def run_step(args):
    import numpy as np
    import torch
    from polars_bio_amd._engine import make_opts
    from polars_bio_amd.device_api import DeviceJoin, DeviceSide

    kind, F = args.step[0], int(args.step[1])
    dj = DeviceJoin(0)
    sync = torch.cuda.synchronize
    host = make_frames(kind, F, args.rows, args.contigs)
    frames = [DeviceSide(*(torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in side)) for side in host]
    opts = make_opts(True, args.contigs)
    ixs = [dj.engine.index_build_dev(s.as_c(), opts, True, sweep_only=True) for s in frames]
    rec = {"set": kind, "frames": F, "rows_per_frame": args.rows, "contigs": args.contigs,
           "reduction_threads": int(os.environ.get("IVJ_PAIRWISE_THREADS", "1024"))}
    try:
        out = tuple(torch.empty((F, F), dtype=torch.int64, device="cuda") for _ in range(2))
        call = lambda: dj.multi_pairwise(frames, True, args.contigs, indexes=ixs, out=out)
        rec["pairwise"] = timed(call, args.steps, args.warmup, sync)
        bases, runs = (t.cpu().numpy().copy() for t in out)
        dj.engine.enable_timing(2)
        t0 = time.perf_counter()
        call()
        sync()
        wall = (time.perf_counter() - t0) * 1e3
        ms = {k: v["ms"] for k, v in dj.engine.timings().items()}
        dj.engine.enable_timing(0)
        reduce_ms = sum(v for k, v in ms.items() if k.startswith("pairwise_"))
        walk_ms = sum(v for k, v in ms.items() if k.startswith(("multi_", "depth_")))
        rec["pairwise"]["split"] = {"wall_ms": round(wall, 3), "reduction_ms": round(reduce_ms, 3), "walk_ms": round(walk_ms, 3),
                                    "index_ms": round(sum(ms.values()) - reduce_ms - walk_ms, 3), "host_ms": round(wall - sum(ms.values()), 3),
                                    "kernels": {k: round(v, 3) for k, v in ms.items() if k.startswith("pairwise_")}}

        pairs = [(i, j) for i in range(F) for j in range(i, F)]
        t0 = time.perf_counter()
        stats = {(i, j): dj.engine.set_stats_dev(ixs[i], ixs[j], opts) for i, j in pairs}
        rec["set_stats"] = {"ms": round((time.perf_counter() - t0) * 1e3, 3), "calls": len(pairs)}
        same = all((int(bases[i, j]), int(runs[i, j])) == (st[2], st[3]) for (i, j), st in stats.items())

        cap = 2 * F * args.rows
        out4 = tuple(torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(3)) + (torch.empty(cap, dtype=torch.int64, device="cuda"),)
        t0 = time.perf_counter()
        c, s, e, mask = (t.cpu().numpy() for t in dj.multi_inter(frames, 1, True, args.contigs, indexes=ixs, out=out4))
        fetch_ms = (time.perf_counter() - t0) * 1e3
        mask = mask.view(np.uint64)
        length = e.astype(np.int64) - s
        follows = np.concatenate([[False], (c[1:] == c[:-1]) & (e[:-1] == s[1:])])
        some = pairs[:: max(1, len(pairs) // args.loop_pairs)][:args.loop_pairs]
        t0 = time.perf_counter()
        for i, j in some:
            both = ((mask >> np.uint64(i)) & (mask >> np.uint64(j)) & np.uint64(1)).astype(bool)
            starts = both & ~(follows & np.concatenate([[False], both[:-1]]))
            same = same and (int(length[both].sum()), int(starts.sum())) == (int(bases[i, j]), int(runs[i, j]))
        loop_ms = (time.perf_counter() - t0) * 1e3
        rec["bit_loop"] = {"segments": int(len(c)), "multi_inter_and_d2h_ms": round(fetch_ms, 3), "pairs": len(pairs), "pairs_timed": len(some),
                           "loop_ms_scaled": round(loop_ms * len(pairs) / len(some), 3), "ms": round(fetch_ms + loop_ms * len(pairs) / len(some), 3)}
        sample = np.ascontiguousarray(mask[:: max(1, len(mask) // 1_000_000)])
        rec["mean_bits_per_segment"] = round(float(np.unpackbits(sample.view(np.uint8)).sum()) / max(len(sample), 1), 2)
        rec["routes_agree"] = bool(same)
    finally:
        for ix in ixs:
            ix.close()
    print(json.dumps(rec))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=300_000, help="rows of every frame")
    ap.add_argument("--contigs", type=int, default=24)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--frames", type=int, nargs="+", default=[4, 16, 64])
    ap.add_argument("--sets", nargs="+", default=["sparse", "dense"], choices=["sparse", "dense"])
    ap.add_argument("--loop-pairs", type=int, default=12, help="pairs the numpy bit loop is timed over")
    ap.add_argument("--out", help="also write the JSON document to this file")
    ap.add_argument("--step", nargs=2, metavar=("SET", "FRAMES"), help="(child) the frame set and frame count to run")
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    doc = []
    for kind in args.sets:
        for F in args.frames:
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", kind, str(F), "--rows", str(args.rows),
                   "--contigs", str(args.contigs), "--steps", str(args.steps), "--warmup", str(args.warmup), "--loop-pairs", str(args.loop_pairs)]
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:
                sys.exit(f"{kind} F = {F} ended with status {p.returncode}: nothing more is started")
            doc.append(json.loads(p.stdout.strip().split("\n")[-1]))
            print(json.dumps(doc[-1]), file=sys.stderr, flush=True)
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
