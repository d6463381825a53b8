#!/usr/bin/env python3
"""Time pb.map_overlaps on the device (ivj_overlap_agg_dev) against the same sweep without values and against what a user had before.

    python tools/bench_overlap_agg.py [--steps 10] [--warmup 3] [--scale 1.0] [--shape big|small|both] [--baseline]

The driver (no --step) starts ONE child process per shape for the GPU step under its own `timeout -k 10` and stops when one fails.
A child builds uniform rows on 24 contigs from polars_bio_amd.synth (100 M x 5 M, or 10 M x 1 M), uploads them once, builds ONE
index and times, after --warmup calls, --steps whole calls between HIP events (median, min .. max):
  map          ivj_overlap_agg_dev, one int64 and one double value column, all five operations each, plain predicate
  map_thr      the same under min_overlap = 1 (the thresholded predicate)
  count_thr    ivj_count_overlaps_thresh_dev with min_overlap = 1 on the same index: the same candidate sweep without values
  old          the route users had: fused pairs on the device -> D2H of both pair columns -> numpy group-by (np.add.at /
               np.minimum.at / np.maximum.at over the probe index) for the same two columns                      (wall clock)
and, from the context's kernel timers, the gather and the reduce kernel of one call separately.  The columns of map and old are
compared (integer columns bit for bit; double sums to the bound of a reordered sum).  No ratio is fixed in advance: the claim to
check is "one call beats pairs + host group-by", and a ratio below 1 is written down as such.

Result: one JSON line per shape (also profiles/overlap_agg/bench_overlap_agg.json) and, with --baseline, a subsection in BASELINE.md."""
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
SHAPES = {"big": (100_000_000, 5_000_000), "small": (10_000_000, 1_000_000)}
N_CONTIGS = 24
MARK_BEGIN, MARK_END = "<!-- bench_overlap_agg -->", "<!-- /bench_overlap_agg -->"
OPS = ("sum", "min", "max", "mean", "count")


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
    from polars_bio_amd._engine import AGG_F64, AGG_I64, make_opts, make_thresholds
    from polars_bio_amd.device_api import DeviceJoin, DeviceSide
    n_probe, n_build = (max(int(n * args.scale), 1) for n in SHAPES[args.shape])
    probe = synth.make_rows(n_probe, 42, synth.PROBE_LEN, N_CONTIGS)[0]
    build = synth.make_rows(n_build, 43, synth.BUILD_LEN, N_CONTIGS)[0]
    rng = np.random.default_rng(44)
    vi = rng.integers(-1000, 1000, n_build).astype(np.int64)
    vf = rng.standard_normal(n_build)
    p, b = (DeviceSide(*(torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in side)) for side in (probe, build))
    dvi, dvf = torch.from_numpy(vi).cuda(), torch.from_numpy(vf).cuda()
    dj = DeviceJoin(0)
    eng = dj.engine
    opts = make_opts(True, N_CONTIGS)
    ix = eng.index_build_dev(b.as_c(), opts, True)
    rec = {"shape": args.shape, "probe_rows": n_probe, "build_rows": n_build, "contigs": N_CONTIGS, "calls": args.steps}
    try:
        side = p.as_c()
        kinds = lambda dt: {"sum": dt, "min": dt, "max": dt, "mean": torch.float64, "count": torch.int64}
        outs = [{op: torch.empty(n_probe, dtype=dt, device="cuda") for op, dt in kinds(d).items()} for d in (torch.int64, torch.float64)]
        cols = [(dvi.data_ptr(), 0, AGG_I64, 31), (dvf.data_ptr(), 0, AGG_F64, 31)]
        ptrs = [{op: t.data_ptr() for op, t in o.items()} for o in outs]
        counts = torch.empty(n_probe, dtype=torch.int64, device="cuda")
        thr = make_thresholds(1)
        calls = {
            "map": lambda: eng.overlap_agg_dev(ix, side, opts, None, n_build, cols, ptrs),
            "map_thr": lambda: eng.overlap_agg_dev(ix, side, opts, thr, n_build, cols, ptrs),
            "count_thr": lambda: eng.count_overlaps_thresh_dev(ix, side, opts, thr, counts.data_ptr()),
        }
        for name, fn in calls.items():
            rec[f"{name}_ms"], rec[f"{name}_wall_ms"] = _timed(torch, fn, args.steps, args.warmup)
        eng.enable_timing(2)
        calls["map"]()
        rec["map_kernel_ms"] = {k: round(v["ms"], 4) for k, v in eng.timings().items()}
        eng.enable_timing(0)
        calls["map"]()
        torch.cuda.synchronize()
        got = [{op: t.cpu().numpy() for op, t in o.items()} for o in outs]
        n_pairs = eng.overlap_count_dev(ix, side, opts)
        cap = n_pairs + n_pairs // 8 + 1024
        out = [torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(2)]
        old = {}

        def old_route():
            pi, bi = dj.overlap(p, b, True, N_CONTIGS, index=ix, out=out)
            pi, bi = pi.cpu().numpy(), bi.cpu().numpy()
            cnt = np.bincount(pi, minlength=n_probe).astype(np.int64)
            res = []
            for v in (vi, vf):
                x = v[bi]
                s = np.zeros(n_probe, v.dtype)
                np.add.at(s, pi, x)
                lo, hi = np.full(n_probe, np.inf), np.full(n_probe, -np.inf)
                np.minimum.at(lo, pi, x)
                np.maximum.at(hi, pi, x)
                with np.errstate(divide="ignore", invalid="ignore"):
                    res.append({"sum": s, "min": lo, "max": hi, "mean": s.astype(np.float64) / cnt, "count": cnt})
            old["res"] = res

        few = max(3, args.steps // 3)
        _, rec["old_wall_ms"] = _timed(torch, old_route, few, 1)
        some = got[0]["count"] > 0
        for k in range(2):
            assert (got[k]["count"] == old["res"][k]["count"]).all(), "counts differ from the old route"
            assert (got[k]["min"][some] == old["res"][k]["min"][some]).all() and (got[k]["max"][some] == old["res"][k]["max"][some]).all()
        assert (got[0]["sum"] == old["res"][0]["sum"]).all(), "integer sums differ from the old route"
        tol = np.maximum(got[1]["count"], 1) * 2.0 ** -52 * np.maximum(np.abs(old["res"][1]["max"]), np.abs(old["res"][1]["min"]))[some].max() * 64
        assert (np.abs(got[1]["sum"] - old["res"][1]["sum"]) <= tol).all(), "double sums differ from the old route beyond reordering"
        rec["pairs"] = int(n_pairs)
    finally:
        ix.close()
    m = lambda k: rec[k]["median"]
    rec["map_over_count_thr"] = round(m("map_thr_ms") / m("count_thr_ms"), 3)
    rec["map_over_old"] = round(m("map_wall_ms") / m("old_wall_ms"), 5)
    print(json.dumps(rec))


def baseline_section(docs):
    lines = [MARK_BEGIN, "### map_overlaps: one call against the sweep without values and against pairs + host group-by", "",
             "`tools/bench_overlap_agg.py`, uniform rows on 24 contigs, one index per shape, one int64 and one double value column with all five "
             "operations, median (min .. max) of whole calls after warm-up (JSON: `profiles/overlap_agg/bench_overlap_agg.json`).", "",
             "| shape | route | HIP events, ms | wall clock, ms |", "|---|---|---|---|"]
    f = lambda d, k: "-" if k is None else f"{d[k]['median']:.3f} ({d[k]['min']:.3f} .. {d[k]['max']:.3f})"
    for d in docs:
        shape = f"{d['probe_rows'] / 1e6:g} M x {d['build_rows'] / 1e6:g} M, {d['pairs'] / 1e6:.1f} M pairs"
        lines += [f"| {shape} | `ivj_overlap_agg_dev`, plain | {f(d, 'map_ms')} | {f(d, 'map_wall_ms')} |",
                  f"| | `ivj_overlap_agg_dev`, `min_overlap = 1` | {f(d, 'map_thr_ms')} | {f(d, 'map_thr_wall_ms')} |",
                  f"| | `ivj_count_overlaps_thresh_dev`, `min_overlap = 1` (no values) | {f(d, 'count_thr_ms')} | {f(d, 'count_thr_wall_ms')} |",
                  f"| | old: fused pairs + D2H + numpy group-by | - | {f(d, 'old_wall_ms')} |"]
    lines.append("")
    for d in docs:
        lines.append(f"{d['probe_rows'] / 1e6:g} M x {d['build_rows'] / 1e6:g} M: map (two columns) / thresholded count = {d['map_over_count_thr']:.3f}, "
                     f"map / old route = {d['map_over_old']:.5f} (wall clock); kernels of one call: "
                     + ", ".join(f"{k} {v:.3f}" for k, v in d["map_kernel_ms"].items()) + " ms.")
    lines.append(MARK_END)
    return "\n".join(lines)


def write_baseline(docs):
    path = os.path.join(ROOT, "BASELINE.md")
    text = open(path).read()
    sec = baseline_section(docs)
    if MARK_BEGIN in text and MARK_END in text:
        text = text[:text.index(MARK_BEGIN)] + sec + text[text.index(MARK_END) + len(MARK_END):]
    else:
        at = text.index("<!-- bench_join_kinds -->")                          # the newest subsection of the results comes first
        text = text[:at] + sec + "\n\n" + text[at:]
    open(path, "w").write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="scale both tables' rows (a quick check at a small size)")
    ap.add_argument("--shape", choices=["big", "small", "both"], default="both")
    ap.add_argument("--step", action="store_true", help="run the GPU step of one shape in this process")
    ap.add_argument("--baseline", action="store_true", help="also write the subsection into BASELINE.md")
    ap.add_argument("--from-json", default=None, help="write the BASELINE.md subsection from a result file instead of running")
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    if args.from_json:
        return write_baseline(json.load(open(args.from_json)))
    docs = []
    for shape in (["small", "big"] if args.shape == "both" else [args.shape]):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", "--shape", shape,
               "--steps", str(args.steps), "--warmup", str(args.warmup), "--scale", str(args.scale)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.exit(f"the GPU step of shape {shape} ended with status {p.returncode}")
        docs.append(json.loads(p.stdout.strip().split("\n")[-1]))
    out_dir = os.path.join(ROOT, "profiles", "overlap_agg")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bench_overlap_agg.json"), "w") as f:
        json.dump(docs, f, indent=1)
        f.write("\n")
    if args.baseline:
        write_baseline(docs)
    for d in docs:
        print(json.dumps(d))


if __name__ == "__main__":
    main()
