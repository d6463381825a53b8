#!/usr/bin/env python3
"""Time depth_profile (per window row and bin the summed overlap bases) on a built index, next to overlap_bases on the explicit
n x B bin frame already resident on the device, and against the route a user had before it: the bin frame built in numpy, pushed
through pb.mean_depth and reshaped.

    python tools/bench_depth_profile.py [--steps 10] [--warmup 3] [--scale 1.0] [--baseline]

60 000 windows of 2 - 6 kb x {50, 400} bins over the build side of config 3 (5 M rows, 24 contigs).  The driver (no --step) starts
one child process per GPU step -- the kernels, then the host route -- each under its own `timeout -k 10`, and stops at the first
step that fails: nothing more is started on a device that has just faulted or hung.  Every child builds its tables in-process
from polars_bio_amd.synth (nothing is read from outside the tree).

The kernel step builds ONE index (end order and position sums included), then per bin count times with HIP events on the engine's
stream, after warm-up (median of --steps calls):
  profile_ms         depth_profile_dev: the windows (12 bytes per row) in, the n x B matrix out
  explicit_bins_ms   overlap_bases_dev on the n x B bin frame, uploaded beforehand (its 12 bytes per BIN are not timed)
and checks that the two results are equal.  The host-route step times end to end, per call: numpy bin frame -> Arrow table ->
pb.mean_depth -> reshape, against pb.depth_profile on the 60 000-row frame (index build and transfers included on both sides).

Result: one JSON line (also profiles/depth_profile/bench_depth_profile.json) and, with --baseline, a row in BASELINE.md."""
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
MARK = "<!-- bench_depth_profile -->"
N_WINDOWS = 60_000
WINDOW_LEN = (2000, 6000)
BUILD_ROWS = 5_000_000
N_CONTIGS = 24
BINS = (50, 400)


def _tables(scale):
    from polars_bio_amd import synth
    windows = synth.make_side(max(1, int(N_WINDOWS * scale)), 7, WINDOW_LEN, N_CONTIGS)
    build = synth.make_rows(max(1, int(BUILD_ROWS * scale)), 43, synth.BUILD_LEN, N_CONTIGS)[0]
    return windows, build


def _bin_frame(windows, n_bins):
    """the explicit n x B bin frame of 0-based half-open windows: bin j of a window of L positions from S is
    [S + floor(j L / B), S + floor((j + 1) L / B))"""
    import numpy as np
    c, s, e = (np.asarray(a, np.int64) for a in windows)
    x = s[:, None] + (e - s)[:, None] * np.arange(n_bins + 1, dtype=np.int64)[None, :] // n_bins
    return (np.repeat(c, n_bins).astype(np.int32), x[:, :-1].reshape(-1).astype(np.int32), x[:, 1:].reshape(-1).astype(np.int32))


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


def run_kernels(args):
    import numpy as np
    import torch
    from polars_bio_amd._engine import make_opts
    from polars_bio_amd.device_api import DeviceJoin, DeviceSide
    windows, build = _tables(args.scale)
    up = lambda side: DeviceSide(*(torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in side))
    w, b = up(windows), up(build)
    dj = DeviceJoin(0)
    eng = dj.engine
    opts = make_opts(True, N_CONTIGS)
    ix = eng.index_build_dev(b.as_c(), opts, True)
    rec = {"step": "kernels", "windows": w.n, "build_rows": b.n, "contigs": N_CONTIGS, "calls": args.steps}
    try:
        for n_bins in BINS:
            bins = up(_bin_frame(windows, n_bins))
            out_p = torch.empty((w.n, n_bins), dtype=torch.int64, device="cuda")
            out_b = torch.empty(bins.n, dtype=torch.int64, device="cuda")
            ws, bs = w.as_c(), bins.as_c()
            eng.depth_profile_dev(ix, ws, 0, n_bins, opts, out_p.data_ptr())       # the first call on the index builds the position sums
            eng.overlap_bases_dev(ix, bs, opts, out_b.data_ptr())
            torch.cuda.synchronize()
            assert torch.equal(out_p.reshape(-1), out_b), f"{n_bins} bins: the two routes disagree"
            r = {"bins": n_bins, "checksum": int(out_p.sum().item())}
            r["profile_ms"] = _event_ms(torch, lambda: eng.depth_profile_dev(ix, ws, 0, n_bins, opts, out_p.data_ptr()), args.steps, args.warmup)
            r["explicit_bins_ms"] = _event_ms(torch, lambda: eng.overlap_bases_dev(ix, bs, opts, out_b.data_ptr()), args.steps, args.warmup)
            r["profile_over_explicit"] = round(r["profile_ms"]["median"] / r["explicit_bins_ms"]["median"], 3)
            r["bins_per_s"] = round(w.n * n_bins / r["profile_ms"]["median"] * 1e3)
            rec[f"bins_{n_bins}"] = r
            del bins, out_p, out_b
    finally:
        ix.close()
    print(json.dumps(rec))


def run_host_route(args):
    import numpy as np
    import pyarrow as pa
    import torch
    import polars_bio_amd as pb
    from polars_bio_amd import synth
    windows, build = _tables(args.scale)
    names = pa.array(synth.CONTIG_NAMES[:N_CONTIGS])
    meta = {"coordinate_system_zero_based": "true"}

    def table(side):
        c, s, e = side
        return pa.table({"chrom": pa.DictionaryArray.from_arrays(pa.array(c, pa.int32()), names), "start": pa.array(s, pa.int32()),
                         "end": pa.array(e, pa.int32())}).replace_schema_metadata(meta)

    t_w, t_b = table(windows), table(build)
    rec = {"step": "host_route", "windows": len(windows[0]), "build_rows": len(build[0])}

    def wall(fn, calls):
        fn()
        times = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = fn()
            times.append((time.perf_counter() - t0) * 1e3)
        times.sort()
        return res, round(times[len(times) // 2], 3)

    for n_bins in BINS:
        def bins_route():
            md = pb.mean_depth(table(_bin_frame(windows, n_bins)), t_b, output_type="pyarrow.Table")
            return md.column("bases").to_numpy().reshape(len(windows[0]), n_bins)

        def profile_route():
            return pb.depth_profile(t_w, t_b, n_bins=n_bins, output="bases", output_type="numpy.ndarray")

        calls = max(2, args.steps // 3)
        a, bins_ms = wall(bins_route, calls)
        b, profile_ms = wall(profile_route, calls)
        assert (a == b).all(), f"{n_bins} bins: the two routes disagree"
        rec[f"bins_{n_bins}"] = {"bins": n_bins, "bin_frame_mean_depth_ms": bins_ms, "depth_profile_ms": profile_ms,
                                 "speedup": round(bins_ms / profile_ms, 2)}
    print(json.dumps(rec))


def baseline_row(doc):
    k, h = doc["kernels"], doc["host_route"]
    def one(b):
        d = k[f"bins_{b}"]
        return (f"{b} bins: depth_profile_dev {d['profile_ms']['median']:.3f} ms, overlap_bases_dev on the resident {k['windows'] * b / 1e6:.0f} M-row bin frame "
                f"{d['explicit_bins_ms']['median']:.3f} ms (ratio {d['profile_over_explicit']:.2f})")
    def host(b):
        d = h[f"bins_{b}"]
        return f"{b} bins: {d['depth_profile_ms']:.0f} ms against {d['bin_frame_mean_depth_ms']:.0f} ms for numpy bin frame -> pb.mean_depth -> reshape (x{d['speedup']:.1f})"
    worst = max(k[f"bins_{b}"]["profile_over_explicit"] for b in BINS)
    verdict = "the expectation (no slower than overlap_bases_dev over the explicit bins) holds" if worst <= 1.0 else \
        "the expectation (no slower than overlap_bases_dev over the explicit bins) FAILS for at least one bin count"
    d = k[f"bins_{BINS[-1]}"]
    return (f"| depth_profile, {k['windows'] // 1000}k windows x {{50, 400}} bins over {k['build_rows'] // 1_000_000}M build rows, kernel on a built index (device API, HIP events) {MARK} | "
            f"{d['profile_ms']['median']:.3f} | {d['bins_per_s']:.2e} bins/s | {one(BINS[0])}; {one(BINS[1])}: {verdict} | "
            f"end to end through the front door: {host(BINS[0])}; {host(BINS[1])} | - |")


def write_baseline(doc):
    path = os.path.join(ROOT, "BASELINE.md")
    lines = open(path).read().split("\n")
    row = baseline_row(doc)
    hit = [i for i, l in enumerate(lines) if MARK in l]
    if hit:
        lines[hit[0]] = row
    else:
        at = min(i for i, l in enumerate(lines) if "<!-- bench_mean_depth -->" in l)           # next to mean_depth's row
        lines.insert(at + 1, row)
    open(path, "w").write("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="scale the windows' and the build side's rows (a quick check at a small size)")
    ap.add_argument("--step", choices=("kernels", "host_route"))
    ap.add_argument("--baseline", action="store_true", help="also write the row into BASELINE.md")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "depth_profile"), help="directory of bench_depth_profile.json")
    args = ap.parse_args()
    if args.step:
        return run_host_route(args) if args.step == "host_route" else run_kernels(args)
    doc = {}
    for step in ("kernels", "host_route"):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", step, "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--scale", str(args.scale)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.exit(f"step {step} ended with status {p.returncode}: nothing more is started")
        doc[step] = json.loads(p.stdout.strip().split("\n")[-1])
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "bench_depth_profile.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if args.baseline:
        write_baseline(doc)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
