#!/usr/bin/env python3
"""Time the semi / anti / left outer join kinds of pb.overlap against their floor (count_overlaps alone) and against what a user
did before they existed.

    python tools/bench_join_kinds.py [--steps 10] [--warmup 3] [--scale 1.0] [--baseline]

The driver (no --step) starts ONE child process for the GPU step under its own `timeout -k 10` and stops when it fails.  The child
builds 10 M x 1 M uniform rows on 24 contigs from polars_bio_amd.synth, uploads them once, builds one index and times, after
warm-up, whole calls (median, min and max of --steps calls; HIP events around the call AND host wall clock, because every
selection ends with the host waiting for the row count):
  count        ivj_count_overlaps_dev alone: the floor -- the selection adds two passes over the counts and one write of the row ids
  semi / anti  ivj_overlap_select_dev into a preallocated buffer (count kernel + select_count + scan + 8-byte D2H + select_emit)
  count_thr    ivj_count_overlaps_thresh_dev with min_overlap = 1           the same pair for the thresholded predicate
  semi_thr     ivj_overlap_select_dev with min_overlap = 1
  old_semi     the route users had: inner join on the device + D2H of all pairs + np.unique(probe_idx)            (wall clock)
  old_anti     count_overlaps on the device + D2H of the int64 counts + np.flatnonzero(counts == 0)              (wall clock)
  inner_host   Engine.overlap  (host entry: uploads, index build, count, fill, D2H)                               (wall clock)
  left_host    Engine.overlap_outer (host entry: the same plus the counts, the selection and the (row, -1) tail)  (wall clock)
count_overlaps and the inner join are the code of the parent commit, unchanged: their times in this run are the parent's.  The row
sets of semi / old_semi and anti / old_anti are compared, as are the pair counts of left_host and inner_host + anti.

Result: one JSON line (also profiles/join_kinds/bench_join_kinds.json) and, with --baseline, a subsection in BASELINE.md."""
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
MARK_BEGIN, MARK_END = "<!-- bench_join_kinds -->", "<!-- /bench_join_kinds -->"


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
    from polars_bio_amd._engine import SELECT_ANTI, SELECT_SEMI, make_opts, make_thresholds
    from polars_bio_amd.device_api import DeviceJoin, DeviceSide
    n_probe, n_build = max(int(N_PROBE * args.scale), 1), max(int(N_BUILD * args.scale), 1)
    probe = synth.make_rows(n_probe, 42, synth.PROBE_LEN, N_CONTIGS)[0]
    build = synth.make_rows(n_build, 43, synth.BUILD_LEN, N_CONTIGS)[0]
    p, b = (DeviceSide(*(torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in side)) for side in (probe, build))
    dj = DeviceJoin(0)
    eng = dj.engine
    opts = make_opts(True, N_CONTIGS)
    ix = eng.index_build_dev(b.as_c(), opts, True)
    rec = {"probe_rows": n_probe, "build_rows": n_build, "contigs": N_CONTIGS, "calls": args.steps}
    try:
        side = p.as_c()
        rows = torch.empty(n_probe, dtype=torch.int32, device="cuda")
        counts = torch.empty(n_probe, dtype=torch.int64, device="cuda")
        n_pairs = eng.overlap_count_dev(ix, side, opts)
        cap = n_pairs + n_pairs // 8 + 1024
        out = [torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(2)]
        thr = make_thresholds(1)
        got = {}

        def select(mode, t=None):
            return eng.overlap_select_dev(ix, side, opts, t, mode, rows.data_ptr(), 0, n_probe)[0]

        calls = {
            "count": lambda: eng.count_overlaps_dev(ix, side, opts, counts.data_ptr()),
            "semi": lambda: got.__setitem__("semi", select(SELECT_SEMI)),
            "anti": lambda: got.__setitem__("anti", select(SELECT_ANTI)),
            "count_thr": lambda: eng.count_overlaps_thresh_dev(ix, side, opts, thr, counts.data_ptr()),
            "semi_thr": lambda: got.__setitem__("semi_thr", select(SELECT_SEMI, thr)),
        }
        for name, fn in calls.items():
            rec[f"{name}_ms"], rec[f"{name}_wall_ms"] = _timed(torch, fn, args.steps, args.warmup)
        semi_rows = rows[:select(SELECT_SEMI)].cpu().numpy().copy()
        anti_rows = rows[:select(SELECT_ANTI)].cpu().numpy().copy()

        def old_semi():
            pi, _ = dj.overlap(p, b, True, N_CONTIGS, index=ix, out=out)
            got["old_semi"] = np.unique(pi.cpu().numpy())

        def old_anti():
            eng.count_overlaps_dev(ix, side, opts, counts.data_ptr())
            got["old_anti"] = np.flatnonzero(counts.cpu().numpy() == 0)

        few = max(3, args.steps // 3)
        _, rec["old_semi_wall_ms"] = _timed(torch, old_semi, few, 1)
        _, rec["old_anti_wall_ms"] = _timed(torch, old_anti, few, 1)
        assert (got["old_semi"] == semi_rows).all() and len(semi_rows) == got["semi"], "semi differs from the old route"
        assert (got["old_anti"] == anti_rows).all() and len(anti_rows) == got["anti"], "anti differs from the old route"

        def inner_host():
            got["inner_host"] = len(eng.overlap(probe, build, True, N_CONTIGS)[0])

        def left_host():
            got["left_host"] = len(eng.overlap_outer(probe, build, True, N_CONTIGS)[0])

        _, rec["inner_host_wall_ms"] = _timed(torch, inner_host, few, 1)
        _, rec["left_host_wall_ms"] = _timed(torch, left_host, few, 1)
        assert got["inner_host"] == n_pairs and got["left_host"] == n_pairs + got["anti"], got
        eng.enable_timing(2)
        select(SELECT_SEMI)
        rec["semi_kernel_ms"] = {k: round(v["ms"], 4) for k, v in eng.timings().items()}
        select(SELECT_SEMI, thr)
        rec["semi_thr_kernel_ms"] = {k: round(v["ms"], 4) for k, v in eng.timings().items()}
        eng.enable_timing(0)
        rec["rows"] = {"semi": int(got["semi"]), "anti": int(got["anti"]), "semi_thr": int(got["semi_thr"]), "inner_pairs": int(n_pairs),
                       "left_pairs": int(got["left_host"])}
    finally:
        ix.close()
    m = lambda k: rec[k]["median"]
    rec["semi_minus_count_ms"] = round(m("semi_ms") - m("count_ms"), 4)
    rec["semi_thr_minus_count_thr_ms"] = round(m("semi_thr_ms") - m("count_thr_ms"), 4)
    rec["semi_over_old_semi"] = round(m("semi_wall_ms") / m("old_semi_wall_ms"), 5)
    rec["anti_over_old_anti"] = round(m("anti_wall_ms") / m("old_anti_wall_ms"), 5)
    rec["left_over_inner_host"] = round(m("left_host_wall_ms") / m("inner_host_wall_ms"), 4)
    print(json.dumps(rec))


def baseline_section(d):
    def row(label, n, ev, wall):
        f = lambda k: "-" if k is None else f"{d[k]['median']:.3f} ({d[k]['min']:.3f} .. {d[k]['max']:.3f})"
        return f"| {label} | {n} | {f(ev)} | {f(wall)} |"
    r = d["rows"]
    return "\n".join([
        MARK_BEGIN,
        "### Join kinds: semi, anti and left outer against `count_overlaps`, the inner join and the routes users had",
        "",
        f"`tools/bench_join_kinds.py`, {d['probe_rows'] // 1_000_000} M x {d['build_rows'] // 1_000_000} M rows on {d['contigs']} contigs, one index, "
        f"median (min .. max) of {d['calls']} whole calls after warm-up, the host routes of fewer (JSON: `profiles/join_kinds/bench_join_kinds.json`).  "
        "`count_overlaps` and the inner join are the parent commit's code, unchanged, timed in the same run.",
        "",
        "| route | rows / pairs | HIP events, ms | wall clock, ms |",
        "|---|---|---|---|",
        row("`ivj_count_overlaps_dev` alone (the floor; parent commit)", d["probe_rows"], "count_ms", "count_wall_ms"),
        row("semi, `ivj_overlap_select_dev`", r["semi"], "semi_ms", "semi_wall_ms"),
        row("anti, `ivj_overlap_select_dev`", r["anti"], "anti_ms", "anti_wall_ms"),
        row("`ivj_count_overlaps_thresh_dev`, `min_overlap = 1` (parent commit)", d["probe_rows"], "count_thr_ms", "count_thr_wall_ms"),
        row("semi under `min_overlap = 1`", r["semi_thr"], "semi_thr_ms", "semi_thr_wall_ms"),
        row("old semi: inner join + D2H of the pairs + `np.unique`", r["semi"], None, "old_semi_wall_ms"),
        row("old anti: `count_overlaps` + D2H of the counts + host filter", r["anti"], None, "old_anti_wall_ms"),
        row("inner join, host entry `ivj_overlap` (parent commit)", r["inner_pairs"], None, "inner_host_wall_ms"),
        row("left outer join, host entry `ivj_overlap_outer`", r["left_pairs"], None, "left_host_wall_ms"),
        "",
        f"semi - count = {d['semi_minus_count_ms']:.3f} ms (events; thresholded: {d['semi_thr_minus_count_thr_ms']:.3f} ms), "
        f"semi / old semi = {d['semi_over_old_semi']:.5f}, anti / old anti = {d['anti_over_old_anti']:.5f}, "
        f"left / inner (host entries) = {d['left_over_inner_host']:.4f} (wall clock).  Kernels of one semi call: "
        + ", ".join(f"{k} {v:.3f}" for k, v in d["semi_kernel_ms"].items()) + " ms; under `min_overlap = 1`: "
        + ", ".join(f"{k} {v:.3f}" for k, v in d["semi_thr_kernel_ms"].items()) + " ms.",
        MARK_END,
    ])


def write_baseline(d):
    path = os.path.join(ROOT, "BASELINE.md")
    text = open(path).read()
    sec = baseline_section(d)
    if MARK_BEGIN in text and MARK_END in text:
        text = text[:text.index(MARK_BEGIN)] + sec + text[text.index(MARK_END) + len(MARK_END):]
    else:
        at = text.index("<!-- bench_thresholds -->")                          # the newest subsection of the results comes first
        text = text[:at] + sec + "\n\n" + text[at:]
    open(path, "w").write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="scale both tables' rows (a quick check at a small size)")
    ap.add_argument("--step", action="store_true", help="run the GPU step in this process")
    ap.add_argument("--baseline", action="store_true", help="also write the subsection into BASELINE.md")
    ap.add_argument("--from-json", default=None, help="write the BASELINE.md subsection from a result file instead of running")
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    out_dir = os.path.join(ROOT, "profiles", "join_kinds")
    if args.from_json:
        return write_baseline(json.load(open(args.from_json)))
    cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--scale", str(args.scale)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit(f"the GPU step ended with status {p.returncode}")
    doc = json.loads(p.stdout.strip().split("\n")[-1])
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bench_join_kinds.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if args.baseline:
        write_baseline(doc)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
