#!/usr/bin/env python3
"""Time pb.map_quantiles on the device (ivj_overlap_quantiles_dev) against one walk without a select and against what a user had before.

    python tools/bench_map_quantiles.py [--steps 10] [--warmup 3] [--scale 1.0] [--shape big|small|both] [--lib PATH] [--no-old] [--baseline]

The driver (no --step) starts ONE child process per shape for the GPU step under its own `timeout -k 10` and stops when one fails.
A child builds uniform rows on 24 contigs from polars_bio_amd.synth (100 M x 5 M, or 10 M x 1 M: the shapes of
tools/bench_overlap_agg.py), uploads them once, builds ONE index and times, after --warmup calls, --steps whole calls between HIP
events (median, min .. max), for three value columns -- small integer scores (int64 in 0 .. 999), float32 values widened to double,
arbitrary doubles -- and n_q = 1 (q = 0.5, lower) and n_q = 2 (q = 0.5, lower and upper: what map_median sends):
  quant     ivj_overlap_quantiles_dev
  count     (a) ivj_overlap_agg_dev with `count` on the same column: the same walk, once; quant / count says what the passes cost
  old       (b) the route users had: fused pairs on the device -> D2H of both pair columns -> numpy sort by (probe, value) and
            group-by for the lower median                                                                        (wall clock)
(c) a second library compiled with another digit width (make CXXFLAGS+=-DIVJ_OVQ_BITS=8 into a directory of its own) is timed by
running the tool again with --lib PATH; the result records the library it ran.  The lower medians of quant and old are compared
exactly.  No ratio is fixed in advance.

Result: one JSON line per shape (also profiles/map_quantiles/bench_map_quantiles.json) and, with --baseline, a subsection in BASELINE.md."""
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
MARK_BEGIN, MARK_END = "<!-- bench_map_quantiles -->", "<!-- /bench_map_quantiles -->"
COLUMNS = ("scores", "float32", "doubles")


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
    from polars_bio_amd import _engine, synth
    if args.lib:
        _engine.LIB_PATH = os.path.abspath(args.lib)
    from polars_bio_amd._engine import AGG_COUNT, AGG_F64, AGG_I64, make_opts
    from polars_bio_amd.device_api import DeviceJoin, DeviceSide
    n_probe, n_build = (max(int(n * args.scale), 1) for n in SHAPES[args.shape])
    probe = synth.make_rows(n_probe, 42, synth.PROBE_LEN, N_CONTIGS)[0]
    build = synth.make_rows(n_build, 43, synth.BUILD_LEN, N_CONTIGS)[0]
    rng = np.random.default_rng(44)
    host = {"scores": rng.integers(0, 1000, n_build).astype(np.int64), "float32": rng.standard_normal(n_build).astype(np.float32).astype(np.float64),
            "doubles": rng.standard_normal(n_build) * np.exp(rng.uniform(-300, 300, n_build))}
    p, b = (DeviceSide(*(torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in side)) for side in (probe, build))
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    dj = DeviceJoin(0)
    eng = dj.engine
    opts = make_opts(True, N_CONTIGS)
    ix = eng.index_build_dev(b.as_c(), opts, True)
    rec = {"shape": args.shape, "probe_rows": n_probe, "build_rows": n_build, "contigs": N_CONTIGS, "calls": args.steps,
           "library": os.path.relpath(_engine.LIB_PATH, ROOT), "columns": {}}
    try:
        side = p.as_c()
        out = torch.empty((n_probe, 2), dtype=torch.int64, device="cuda")
        cnt = torch.empty(n_probe, dtype=torch.int64, device="cuda")
        n_pairs = eng.overlap_count_dev(ix, side, opts)
        rec["pairs"] = int(n_pairs)
        pairs_out = None
        for name in COLUMNS:
            dtype = AGG_I64 if host[name].dtype == np.int64 else AGG_F64
            col = (dev[name].data_ptr(), 0, dtype)
            r = {}
            calls = {"quant_1": lambda: eng.overlap_quantiles_dev(ix, side, opts, None, n_build, col, [0.5], [0], out.data_ptr(), cnt.data_ptr()),
                     "quant_2": lambda: eng.overlap_quantiles_dev(ix, side, opts, None, n_build, col, [0.5, 0.5], [0, 1], out.data_ptr(), cnt.data_ptr()),
                     "count": lambda: eng.overlap_agg_dev(ix, side, opts, None, n_build, [col + (AGG_COUNT,)], [{"count": cnt.data_ptr()}])}
            for what, fn in calls.items():
                r[f"{what}_ms"], r[f"{what}_wall_ms"] = _timed(torch, fn, args.steps, args.warmup)
            eng.enable_timing(2)
            calls["quant_1"]()
            r["quant_1_kernel_ms"] = {k: round(v["ms"], 4) for k, v in eng.timings().items()}
            eng.enable_timing(0)
            calls["quant_1"]()
            torch.cuda.synchronize()
            got = out.cpu().numpy().reshape(-1)[:n_probe].view(host[name].dtype).copy()      # n_q = 1: the first n_probe cells
            got_n = cnt.cpu().numpy().copy()
            for k in ("quant_1", "quant_2"):
                r[f"{k}_over_count"] = round(r[f"{k}_ms"]["median"] / r["count_ms"]["median"], 3)
            if not args.no_old:
                if pairs_out is None:
                    cap = n_pairs + n_pairs // 8 + 1024
                    pairs_out = [torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(2)]
                old = {}

                def old_route():
                    pi, bi = dj.overlap(p, b, True, N_CONTIGS, index=ix, out=pairs_out)
                    pi, bi = pi.cpu().numpy(), bi.cpu().numpy()
                    x = host[name][bi]
                    order = np.lexsort((x, pi))
                    pi, x = pi[order], x[order]
                    m = np.bincount(pi, minlength=n_probe).astype(np.int64)
                    first = np.cumsum(m) - m
                    some = m > 0
                    med = np.zeros(n_probe, x.dtype)
                    med[some] = x[first[some] + (m[some] - 1) // 2]
                    old["med"], old["m"] = med, m

                _, r["old_wall_ms"] = _timed(torch, old_route, max(2, args.steps // 5), 0)
                assert (got_n == old["m"]).all(), f"{name}: counts differ from the old route"
                assert (got == old["med"]).all(), f"{name}: lower medians differ from the old route"
                r["quant_1_over_old"] = round(r["quant_1_wall_ms"]["median"] / r["old_wall_ms"]["median"], 5)
            rec["columns"][name] = r
    finally:
        ix.close()
    print(json.dumps(rec))


def baseline_section(docs):
    lines = [MARK_BEGIN, "### map_quantiles: the select against one walk and against pairs + host sort", "",
             "`tools/bench_map_quantiles.py`, uniform rows on 24 contigs, one index per shape, median (min .. max) of whole calls after warm-up "
             "(JSON: `profiles/map_quantiles/bench_map_quantiles.json`).  `count` is `ivj_overlap_agg_dev` with `count` on the same column: "
             "the same walk, once.", "",
             "| shape, library | column | n_q = 1, ms | n_q = 2, ms | count, ms | n_q = 1 / count | n_q = 2 / count | old route (wall), ms | n_q = 1 / old (wall) |",
             "|---|---|---|---|---|---|---|---|---|"]
    f = lambda d, k: f"{d[k]['median']:.3f} ({d[k]['min']:.3f} .. {d[k]['max']:.3f})" if k in d else "not run"
    for d in docs:
        shape = f"{d['probe_rows'] / 1e6:g} M x {d['build_rows'] / 1e6:g} M, {d['pairs'] / 1e6:.1f} M pairs, `{d['library']}`"
        for name, r in d["columns"].items():
            lines.append(f"| {shape} | {name} | {f(r, 'quant_1_ms')} | {f(r, 'quant_2_ms')} | {f(r, 'count_ms')} | {r['quant_1_over_count']:.3f} | "
                         f"{r['quant_2_over_count']:.3f} | {f(r, 'old_wall_ms')} | {r.get('quant_1_over_old', 'not run')} |")
            shape = ""
    lines += ["", "A shape or a library (`--lib`: a build with another `IVJ_OVQ_BITS`) that has no row here is unmeasured.", MARK_END]
    return "\n".join(lines)


def write_baseline(docs):
    path = os.path.join(ROOT, "BASELINE.md")
    text = open(path).read()
    sec = baseline_section(docs)
    if MARK_BEGIN in text and MARK_END in text:
        text = text[:text.index(MARK_BEGIN)] + sec + text[text.index(MARK_END) + len(MARK_END):]
    else:
        at = text.index("<!-- bench_window -->")                               # the newest subsection of the results comes first
        text = text[:at] + sec + "\n\n" + text[at:]
    open(path, "w").write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="scale both tables' rows (a quick check at a small size)")
    ap.add_argument("--shape", choices=["big", "small", "both"], default="both")
    ap.add_argument("--lib", default=None, help="time this libivjoin_hip.so (a build with another IVJ_OVQ_BITS) instead of the package's")
    ap.add_argument("--no-old", action="store_true", help="leave out the pairs + host sort route")
    ap.add_argument("--step", action="store_true", help="run the GPU step of one shape in this process")
    ap.add_argument("--baseline", action="store_true", help="also write the subsection into BASELINE.md")
    ap.add_argument("--from-json", default=None, help="write the BASELINE.md subsection from a result file instead of running")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_quantiles", "bench_map_quantiles.json"))
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    if args.from_json:
        return write_baseline(json.load(open(args.from_json)))
    docs = []
    for shape in (["small", "big"] if args.shape == "both" else [args.shape]):
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", "--shape", shape,
               "--steps", str(args.steps), "--warmup", str(args.warmup), "--scale", str(args.scale)]
        cmd += (["--lib", args.lib] if args.lib else []) + (["--no-old"] if args.no_old else [])
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.exit(f"the GPU step of shape {shape} ended with status {p.returncode}")
        docs.append(json.loads(p.stdout.strip().split("\n")[-1]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(docs, f, indent=1)
        f.write("\n")
    if args.baseline:
        write_baseline(docs)
    for d in docs:
        print(json.dumps(d))


if __name__ == "__main__":
    main()
