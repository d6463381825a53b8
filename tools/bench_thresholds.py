#!/usr/bin/env python3
"""Time the thresholded overlap join (min_overlap / min_frac1) against the plain join of the same candidate-test design and
against what a user did before it existed: join everything, copy the pairs back, filter on the host.

    python tools/bench_thresholds.py [--steps 10] [--warmup 3] [--scale 1.0] [--baseline]

The driver (no --step) starts ONE child process for the GPU step under its own `timeout -k 10` and stops when it fails.  The child
builds 10 M x 1 M uniform rows on 24 contigs from polars_bio_amd.synth, uploads them once, builds one index and times, after
warm-up, whole calls on the device API (median of --steps calls; HIP events around the call AND host wall clock, because every
route ends with the host waiting for the pair count):
  a  thresh_min_overlap_1   ivj_overlap_thresh_dev with min_overlap = 1: a threshold that removes nothing (count -> scan -> emit)
  b  thresh_min_frac1_0.5   ivj_overlap_thresh_dev with probe_min = min_bases(len, 0.5), the minima computed once outside the timed region
  c  fused_flat             ivj_overlap_fused_dev with partition_mode = 5 on the same input: the plain run of the same design (one pass)
  d  plain_d2h_numpy        the automatic plain path (DeviceJoin.overlap into preallocated buffers) + D2H of the pairs + a numpy
                            filter ov / len >= 0.5 over host copies of the columns: the route users had (wall clock)
and the ratios a / c (events) and b / d (wall clock).  The pair counts of a and c, and of b and d, are compared.

Result: one JSON line (also profiles/thresholds/bench_thresholds.json) and, with --baseline, a subsection in BASELINE.md."""
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
MARK_BEGIN, MARK_END = "<!-- bench_thresholds -->", "<!-- /bench_thresholds -->"


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
    from polars_bio_amd._engine import make_opts, make_thresholds
    from polars_bio_amd.device_api import DeviceJoin, DeviceSide
    from polars_bio_amd.range_op import min_bases
    n_probe, n_build = max(int(N_PROBE * args.scale), 1), max(int(N_BUILD * args.scale), 1)
    probe = synth.make_rows(n_probe, 42, synth.PROBE_LEN, N_CONTIGS)[0]
    build = synth.make_rows(n_build, 43, synth.BUILD_LEN, N_CONTIGS)[0]
    p, b = (DeviceSide(*(torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in side)) for side in (probe, build))
    dj = DeviceJoin(0)
    eng = dj.engine
    opts, opts_flat = make_opts(True, N_CONTIGS), make_opts(True, N_CONTIGS, partition_mode=5)
    ix = eng.index_build_dev(b.as_c(), opts, False)
    rec = {"probe_rows": n_probe, "build_rows": n_build, "contigs": N_CONTIGS, "calls": args.steps}
    try:
        side = p.as_c()
        total, _ = eng.overlap_thresh_dev(ix, side, opts, make_thresholds(1), 0, 0, 0)
        cap = total + total // 8 + 1024
        out = [torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(2)]
        ptrs = (out[0].data_ptr(), out[1].data_ptr())
        pm_host = min_bases(probe[2].astype(np.int64) - probe[1].astype(np.int64), 0.5)
        pm = torch.from_numpy(pm_host.view(np.int32).copy()).cuda()
        thr_a, thr_b = make_thresholds(1), make_thresholds(0, pm.data_ptr())
        got = {}

        def call_a():
            got["a"] = eng.overlap_thresh_dev(ix, side, opts, thr_a, *ptrs, cap)[0]

        def call_b():
            got["b"] = eng.overlap_thresh_dev(ix, side, opts, thr_b, *ptrs, cap)[0]

        def call_c():
            got["c"] = eng.overlap_fused_dev(ix, side, opts_flat, *ptrs, cap)[0]

        def call_d():
            pi, bi = dj.overlap(p, b, True, N_CONTIGS, index=ix, out=out)
            pi, bi = pi.cpu().numpy(), bi.cpu().numpy()
            ps, pe, bs, be = probe[1][pi], probe[2][pi], build[1][bi], build[2][bi]
            ov = np.minimum(pe, be).astype(np.int64) - np.maximum(ps, bs)
            keep = (ov >= 1) & (ov / (pe.astype(np.int64) - ps) >= 0.5)
            got["d"] = int(keep.sum())
            got["d_plain"] = len(pi)

        for name, fn in (("a", call_a), ("b", call_b), ("c", call_c)):
            rec[f"{name}_ms"], rec[f"{name}_wall_ms"] = _timed(torch, fn, args.steps, args.warmup)
        _, rec["d_wall_ms"] = _timed(torch, call_d, max(3, args.steps // 2), 1)
        eng.enable_timing(2)
        call_a()
        rec["a_kernel_ms"] = {k: round(v["ms"], 4) for k, v in eng.timings().items()}
        call_c()
        rec["c_kernel_ms"] = {k: round(v["ms"], 4) for k, v in eng.timings().items()}
        eng.enable_timing(0)
        rec["pairs"] = {k: int(v) for k, v in got.items()}
        assert got["a"] == got["c"] == got["d_plain"], got       # every synthetic row covers a position: min_overlap = 1 removes nothing
        assert got["b"] == got["d"], got
    finally:
        ix.close()
    rec["a_over_c"] = round(rec["a_ms"]["median"] / rec["c_ms"]["median"], 3)
    rec["b_over_d"] = round(rec["b_wall_ms"]["median"] / rec["d_wall_ms"]["median"], 4)
    print(json.dumps(rec))


def baseline_section(d):
    m = lambda k: d[k]["median"]
    return "\n".join([
        MARK_BEGIN,
        "### Overlap thresholds: the thresholded join against the plain join and the host filter",
        "",
        f"`tools/bench_thresholds.py`, {d['probe_rows'] // 1_000_000} M x {d['build_rows'] // 1_000_000} M rows on {d['contigs']} contigs, one index, device API, "
        f"median of {d['calls']} whole calls after warm-up (JSON: `profiles/thresholds/bench_thresholds.json`).",
        "",
        "| route | pairs | HIP events, ms | wall clock, ms |",
        "|---|---|---|---|",
        f"| a `ivj_overlap_thresh_dev`, `min_overlap = 1` (removes nothing; count, scan, emit) | {d['pairs']['a']} | {m('a_ms'):.3f} | {m('a_wall_ms'):.3f} |",
        f"| b `ivj_overlap_thresh_dev`, `min_frac1 = 0.5` | {d['pairs']['b']} | {m('b_ms'):.3f} | {m('b_wall_ms'):.3f} |",
        f"| c `ivj_overlap_fused_dev`, `partition_mode = 5` (the plain run of the same design, one pass) | {d['pairs']['c']} | {m('c_ms'):.3f} | {m('c_wall_ms'):.3f} |",
        f"| d automatic plain path + D2H + numpy filter `ov / len >= 0.5` | {d['pairs']['d']} of {d['pairs']['d_plain']} | - | {m('d_wall_ms'):.3f} |",
        "",
        f"a / c = {d['a_over_c']:.3f} (events), b / d = {d['b_over_d']:.4f} (wall clock).  Kernels of one call of a: "
        + ", ".join(f"{k} {v:.3f}" for k, v in d["a_kernel_ms"].items()) + " ms; of c: "
        + ", ".join(f"{k} {v:.3f}" for k, v in d["c_kernel_ms"].items()) + " ms.",
        MARK_END,
    ])


def write_baseline(d):
    path = os.path.join(ROOT, "BASELINE.md")
    text = open(path).read()
    sec = baseline_section(d)
    if MARK_BEGIN in text and MARK_END in text:
        text = text[:text.index(MARK_BEGIN)] + sec + text[text.index(MARK_END) + len(MARK_END):]
    else:
        at = text.index("### N frames as position sets")                     # the newest subsection of the results comes first
        text = text[:at] + sec + "\n\n" + text[at:]
    open(path, "w").write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="scale both tables' rows (a quick check at a small size)")
    ap.add_argument("--step", action="store_true", help="run the GPU step in this process")
    ap.add_argument("--baseline", action="store_true", help="also write the subsection into BASELINE.md")
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--scale", str(args.scale)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit(f"the GPU step ended with status {p.returncode}")
    doc = json.loads(p.stdout.strip().split("\n")[-1])
    out_dir = os.path.join(ROOT, "profiles", "thresholds")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bench_thresholds.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if args.baseline:
        write_baseline(doc)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
