#!/usr/bin/env python3
"""Time the distance-window join (pb.window's device entries) against the thresholded join it was modelled on and against what a
user did before it existed: pad df1, join, copy the pairs back, compute distances and filter on the host.

    python tools/bench_window.py [--steps 10] [--warmup 3] [--scale 1.0] [--baseline] [--from-json FILE]

The driver (no --step) starts ONE child process for the GPU step under its own `timeout -k 10` and stops when it fails.  The child
builds 10 M x 1 M uniform rows on 24 contigs from polars_bio_amd.synth, uploads them once, builds one index and times, after
warm-up, whole calls on the device API (median of --steps calls; HIP events around the call AND host wall clock, because the pair
routes end with the host waiting for the pair count).  At window 0, 1 000 and 100 000:
  count        ivj_count_window_dev                        per-probe counts only
  pairs        ivj_overlap_window_dev, dist_dev = NULL      count -> scan -> emit, 8 bytes per pair
  pairs_dist   ivj_overlap_window_dev with distances        16 bytes per pair
and the two yardsticks
  a  thresh    ivj_overlap_thresh_dev / ivj_count_overlaps_thresh_dev with min_overlap = 1 on the same index and probes, compared at
               window 0 (thresh.hip.h is the parent commit's: this tree does not touch it; its candidate set is that of window 0 up
               to touching rows)
  b  host      the route users had, per window: pad df1 by the window in torch (int64, clamped to int32), the fused overlap into
               preallocated buffers, D2H of the pairs, numpy distance and filter (wall clock); not attempted for a window with more
               than HOST_ROUTE_MAX_PAIRS pairs, whose host temporaries would run to tens of GB
Rates: matches per second for every line.  The kernels do not export how many candidates they tested; every match is a candidate, so
matches / s is a lower bound of candidates / s (tight at small windows, where the loose range holds about one row more than the
exact one).

Result: one JSON line (also profiles/window/bench_window.json) and, with --baseline, the `<!-- bench_window -->` section of
BASELINE.md.  --from-json FILE writes both from the JSON of an earlier run, without a GPU."""
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
N_PROBE, N_BUILD, N_CONTIGS = 10_000_000, 1_000_000, 24
WINDOWS = (0, 1_000, 100_000)
HOST_ROUTE_MAX_PAIRS = 128_000_000      # above this the host route's numpy temporaries (ten int64 columns of the pairs) are not attempted
MARK_BEGIN, MARK_END = "<!-- bench_window -->", "<!-- /bench_window -->"


def _timed(torch, fn, steps, warmup):
    """-> (HIP-event stats, wall-clock stats) in ms of whole calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev, wall = [], []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        b.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        ev.append(a.elapsed_time(b))
    stats = lambda v: {"median": round(sorted(v)[len(v) // 2], 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    return stats(ev), stats(wall)


def run_step(args):
    import numpy as np
    import torch
    from polars_bio_amd import synth
    from polars_bio_amd._engine import make_opts, make_thresholds, make_window
    from polars_bio_amd.device_api import DeviceJoin, DeviceSide
    n_probe, n_build = max(int(N_PROBE * args.scale), 1), max(int(N_BUILD * args.scale), 1)
    probe = synth.make_rows(n_probe, 42, synth.PROBE_LEN, N_CONTIGS)[0]
    build = synth.make_rows(n_build, 43, synth.BUILD_LEN, N_CONTIGS)[0]
    p, b = (DeviceSide(*(torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in side)) for side in (probe, build))
    dj = DeviceJoin(0)
    eng = dj.engine
    opts = make_opts(True, N_CONTIGS)
    ix = eng.index_build_dev(b.as_c(), opts, False)
    rec = {"probe_rows": n_probe, "build_rows": n_build, "contigs": N_CONTIGS, "calls": args.steps, "windows": {}}
    try:
        side = p.as_c()
        counts = torch.empty(n_probe, dtype=torch.int64, device="cuda")
        totals = {w: eng.overlap_window_dev(ix, side, opts, make_window(w, w), 0, 0, 0, 0)[0] for w in WINDOWS}
        cap = max(totals.values()) + 1024
        out = [torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(2)]
        dist = torch.empty(cap, dtype=torch.int64, device="cuda")
        ptrs = (out[0].data_ptr(), out[1].data_ptr())
        rate = lambda n, ms: round(n / (ms * 1e-3)) if ms > 0 else 0
        for w in WINDOWS:
            win = make_window(w, w)
            n = totals[w]
            r = {"pairs": int(n)}
            forms = (("count", lambda: eng.count_window_dev(ix, side, opts, win, counts.data_ptr())),
                     ("pairs", lambda: eng.overlap_window_dev(ix, side, opts, win, *ptrs, 0, cap)),
                     ("pairs_dist", lambda: eng.overlap_window_dev(ix, side, opts, win, *ptrs, dist.data_ptr(), cap)))
            for name, fn in forms:
                r[f"{name}_ms"], r[f"{name}_wall_ms"] = _timed(torch, fn, args.steps, args.warmup)
                r[f"{name}_matches_per_s"] = rate(n, r[f"{name}_ms"]["median"])

            def host_route():
                pad = lambda t, d: torch.clamp(t.to(torch.int64) + d, -(1 << 31), (1 << 31) - 1).to(torch.int32)
                padded = DeviceSide(p.contig, pad(p.start, -w - 1), pad(p.end, w + 1))
                pi, bi = dj.overlap(padded, b, True, N_CONTIGS, index=ix, out=out)
                pi, bi = pi.cpu().numpy(), bi.cpu().numpy()
                ps, pe, bs, be = (a.astype(np.int64) for a in (probe[1][pi], probe[2][pi], build[1][bi], build[2][bi]))
                ov = (bs < pe) & (ps < be)
                d = np.where(ov, 0, np.maximum(bs - pe, ps - be))
                keep = (d <= w) & (ps < pe) & (bs < be)
                r["host_pairs"] = int(keep.sum())
                r["host_padded_pairs"] = len(pi)

            if n <= HOST_ROUTE_MAX_PAIRS:
                _, r["host_wall_ms"] = _timed(torch, host_route, max(3, args.steps // 3), 1)
                r["host_matches_per_s"] = rate(r["host_pairs"], r["host_wall_ms"]["median"])
                assert r["host_pairs"] == n, (w, r["host_pairs"], n)
                r["pairs_dist_over_host"] = round(r["pairs_dist_wall_ms"]["median"] / r["host_wall_ms"]["median"], 4)
            rec["windows"][str(w)] = r
        thr = make_thresholds(1)
        t = {"pairs": int(eng.overlap_thresh_dev(ix, side, opts, thr, 0, 0, 0)[0])}
        t["count_ms"], t["count_wall_ms"] = _timed(torch, lambda: eng.count_overlaps_thresh_dev(ix, side, opts, thr, counts.data_ptr()), args.steps, args.warmup)
        t["pairs_ms"], t["pairs_wall_ms"] = _timed(torch, lambda: eng.overlap_thresh_dev(ix, side, opts, thr, *ptrs, cap), args.steps, args.warmup)
        for name in ("count", "pairs"):
            t[f"{name}_matches_per_s"] = rate(t["pairs"], t[f"{name}_ms"]["median"])
        rec["thresh_min_overlap_1"] = t
        w0 = rec["windows"]["0"]
        rec["window0_over_thresh"] = {k: round(w0[f"{k}_ms"]["median"] / t[f"{j}_ms"]["median"], 3)
                                      for k, j in (("count", "count"), ("pairs", "pairs"), ("pairs_dist", "pairs"))}
        eng.enable_timing(2)
        eng.overlap_window_dev(ix, side, opts, make_window(0, 0), *ptrs, dist.data_ptr(), cap)
        rec["window0_kernel_ms"] = {k: round(v["ms"], 4) for k, v in eng.timings().items()}
        eng.enable_timing(0)
    finally:
        ix.close()
    print(json.dumps(rec))


def baseline_section(d):
    m = lambda r, k: r[k]["median"]
    t = d["thresh_min_overlap_1"]
    lines = [
        MARK_BEGIN,
        "### Distance window: `ivj_overlap_window_dev` / `ivj_count_window_dev` against the thresholded join and the host route",
        "",
        f"`tools/bench_window.py`, {d['probe_rows'] / 1e6:g} M x {d['build_rows'] / 1e6:g} M rows on {d['contigs']} contigs, one index, device API, "
        f"median of {d['calls']} whole calls after warm-up (JSON: `profiles/window/bench_window.json`).  HIP events, ms (matches / s); the "
        "host route in wall clock.  The rate is matches per second, NOT candidates per second: the kernels do not export how many "
        "candidates they tested, every match is a candidate, so the figure is a lower bound of the candidate rate.  The host route is "
        f"not run for a window with more than {HOST_ROUTE_MAX_PAIRS} pairs (its numpy temporaries would take tens of GB of host memory).",
        "",
        "| window | number of pairs | count form | pairs form | pairs + distance form | host route: pad, fused overlap, D2H, numpy (wall) | pairs + distance / host (wall) |",
        "|---|---|---|---|---|---|---|",
    ]
    for w, r in d["windows"].items():
        cell = lambda k: f"{m(r, k + '_ms'):.3f} ({r[k + '_matches_per_s']:.3g})"
        host = (f"{m(r, 'host_wall_ms'):.3f} ({r['host_matches_per_s']:.3g}; {r['host_padded_pairs']} padded pairs copied) | {r['pairs_dist_over_host']:.4f}"
                if "host_wall_ms" in r else f"not run (more than {HOST_ROUTE_MAX_PAIRS} pairs) | -")
        lines.append(f"| {w} | {r['pairs']} | {cell('count')} | {cell('pairs')} | {cell('pairs_dist')} | {host} |")
    o = d["window0_over_thresh"]
    lines += [
        "",
        f"Yardstick a, `ivj_overlap_thresh_dev` with `min_overlap = 1` on the same index and probes: {t['pairs']} pairs, count "
        f"{m(t, 'count_ms'):.3f} ms, pairs {m(t, 'pairs_ms'):.3f} ms.  Window 0 over it: count {o['count']:.3f}, pairs {o['pairs']:.3f}, "
        f"pairs + distance {o['pairs_dist']:.3f} (16 bytes per pair against 8).  Kernels of one window-0 call with distances: "
        + ", ".join(f"{k} {v:.3f}" for k, v in d["window0_kernel_ms"].items()) + " ms.",
        MARK_END,
    ]
    return "\n".join(lines)


def write_baseline(d):
    path = os.path.join(ROOT, "BASELINE.md")
    text = open(path).read()
    sec = baseline_section(d)
    if MARK_BEGIN in text and MARK_END in text:
        text = text[:text.index(MARK_BEGIN)] + sec + text[text.index(MARK_END) + len(MARK_END):]
    else:
        at = text.index("<!-- bench_signal -->")                               # the newest subsection of the results comes first
        text = text[:at] + sec + "\n\n" + text[at:]
    open(path, "w").write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="scale both tables' rows (a quick check at a small size)")
    ap.add_argument("--step", action="store_true", help="run the GPU step in this process")
    ap.add_argument("--baseline", action="store_true", help="also write the subsection into BASELINE.md")
    ap.add_argument("--from-json", default=None, help="take the result of an earlier run from this file instead of running")
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    if args.from_json:
        doc = json.load(open(args.from_json))
    else:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--scale", str(args.scale)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.exit(f"the GPU step ended with status {p.returncode}")
        doc = json.loads(p.stdout.strip().split("\n")[-1])
    out_dir = os.path.join(ROOT, "profiles", "window")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bench_window.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if args.baseline:
        write_baseline(doc)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
