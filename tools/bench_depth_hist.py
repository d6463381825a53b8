#!/usr/bin/env python3
"""Time depth_hist (per probe row, and per contig, the positions at each depth 0 .. max_depth) on a built index: its per-call build
share against its two kernels, and the region form against the two routes a user had before.

    python tools/bench_depth_hist.py [--steps 10] [--warmup 3] [--scale 1.0] [--baseline | --from-json FILE]

The driver (no --step) starts one child process per GPU step, each under its own `timeout -k 10`, and stops at the first step
that fails: nothing more is started on a device that has just faulted or hung.  Both steps share one build side, 4 M reads of
100 .. 150 positions on 24 contigs of 1 M positions (mean depth ~ 20, ~ 8 M depth blocks):
  targets   200 k probe rows of 200 .. 2000 positions (reads over targets: a few hundred blocks under a row)
  contigs   24 probe rows, each a whole contig (every block of the contig under one row)

A step builds ONE index of the build side (end order included) and reports per max_depth in (8, 100, 1000), after warm-up:
  kernel_ms          the engine's own HIP events of one depth_hist_dev call, per launch name
  build_share_ms     of those, everything but the histogram kernel: the blocks (depth_*), the block index, the records
  hist_kernel_ms     the depth_hist launch alone;  contigs_kernel_ms: the depth_hist_contigs launch of one contig-form call
  call_ms            the whole depth_hist_dev call (HIP events around it, median of --steps calls), contigs_call_ms likewise
  lds128_call_ms     the same call with IVJ_HIST_LDS_KB=128: one resident workgroup per CU with twice the rows, against two
  chained_ms         ceil(max_depth / 8) depth_summary_dev calls on the same index and the differencing of their columns (torch,
                     on the device); chained_speedup = chained / call.  The two routes' matrices are compared.
  numpy_ms           (targets, max_depth 100 only) DeviceJoin.depth -> D2H -> numpy searchsorted / repeat / bincount

Result: one JSON line (also profiles/depth_hist/bench_depth_hist.json) and, with --baseline, a section in BASELINE.md."""
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
MARK = "<!-- bench_depth_hist -->"
STEPS = ("targets", "contigs")
DEPTHS = (8, 100, 1000)
N_CONTIGS, CONTIG_LEN, N_READS, N_TARGETS = 24, 1_000_000, 4_000_000, 200_000


def _tables(step, scale):
    import numpy as np
    rng = np.random.default_rng(77)
    nb = max(int(N_READS * scale), 1000)
    bc = rng.integers(0, N_CONTIGS, nb)
    bs = rng.integers(0, CONTIG_LEN - 150, nb)
    build = (bc, bs, bs + rng.integers(100, 151, nb))
    if step == "targets":
        n = max(int(N_TARGETS * scale), 100)
        ps = rng.integers(0, CONTIG_LEN - 2000, n)
        probe = (rng.integers(0, N_CONTIGS, n), ps, ps + rng.integers(200, 2001, n))
    else:
        probe = (np.arange(N_CONTIGS), np.zeros(N_CONTIGS), np.full(N_CONTIGS, CONTIG_LEN))
    return tuple(np.ascontiguousarray(a, np.int32) for a in probe), tuple(np.ascontiguousarray(a, np.int32) for a in build)


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


def _numpy_route(dj, b, probe, md):
    """the block list to the host, then the region histogram in numpy -> (matrix, seconds)"""
    import numpy as np
    t0 = time.perf_counter()
    kc, ks, ke, kd = (x.cpu().numpy().astype(np.int64) for x in dj.depth(b, True, N_CONTIGS))
    pc, ps, pe = (a.astype(np.int64) for a in probe)
    span = np.int64(1) << 34
    i0 = np.searchsorted(kc * span + ke, pc * span + ps, "right")
    i1 = np.searchsorted(kc * span + ks, pc * span + pe, "left")
    cnt = np.maximum(i1 - i0, 0)
    row = np.repeat(np.arange(len(pc)), cnt)
    blk = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(i0, cnt)
    ln = np.minimum(ke[blk], pe[row]) - np.maximum(ks[blk], ps[row])
    flat = np.bincount(row * (md + 1) + np.minimum(kd[blk], md), weights=ln, minlength=len(pc) * (md + 1))
    hist = flat.astype(np.int64).reshape(len(pc), md + 1)
    hist[:, 0] = np.maximum(pe - ps, 0) - hist.sum(axis=1)
    return hist, time.perf_counter() - t0


def run_step(args):
    import numpy as np
    import torch
    from polars_bio_amd._engine import make_opts
    from polars_bio_amd.device_api import DeviceJoin, DeviceSide
    probe, build = _tables(args.step, args.scale)
    p, b = (DeviceSide(*(torch.from_numpy(a).cuda() for a in side)) for side in (probe, build))
    dj = DeviceJoin(0)
    eng = dj.engine
    opts = make_opts(True, N_CONTIGS)
    ix = eng.index_build_dev(b.as_c(), opts, True)
    rec = {"step": args.step, "probe_rows": p.n, "build_rows": b.n, "contigs": N_CONTIGS, "calls": args.steps, "depths": {}}
    try:
        side = p.as_c()
        for md in DEPTHS:
            d = {}
            out = torch.empty((p.n, md + 1), dtype=torch.int64, device="cuda")
            cout = torch.empty((N_CONTIGS, md + 1), dtype=torch.int64, device="cuda")
            call = lambda: eng.depth_hist_dev(ix, side, opts, md, out.data_ptr())
            ccall = lambda: eng.depth_hist_contigs_dev(ix, opts, md, cout.data_ptr())
            for _ in range(args.warmup):
                call()
                ccall()
            torch.cuda.synchronize()
            eng.enable_timing(2)
            call()
            kern = {k: round(v["ms"], 4) for k, v in eng.timings().items()}
            ccall()
            ckern = {k: round(v["ms"], 4) for k, v in eng.timings().items()}
            eng.enable_timing(0)
            d["kernel_ms"] = kern
            d["hist_kernel_ms"] = kern.get("depth_hist", 0.0)
            d["build_share_ms"] = round(sum(v for k, v in kern.items() if k != "depth_hist"), 4)
            d["contigs_kernel_ms"] = ckern.get("depth_hist_contigs", 0.0)
            d["call_ms"] = _event_ms(torch, call, args.steps, args.warmup)
            d["contigs_call_ms"] = _event_ms(torch, ccall, args.steps, args.warmup)
            mine = out.clone()
            os.environ["IVJ_HIST_LDS_KB"] = "128"
            try:
                d["lds128_call_ms"] = _event_ms(torch, call, args.steps, args.warmup)
                eng.enable_timing(2)
                call()
                d["lds128_hist_kernel_ms"] = round(eng.timings().get("depth_hist", {"ms": 0.0})["ms"], 4)
                eng.enable_timing(0)
                assert torch.equal(out, mine), "the LDS budget changed the result"
            finally:
                del os.environ["IVJ_HIST_LDS_KB"]
            d["lds128_over_lds64"] = round(d["lds128_call_ms"]["median"] / d["call_ms"]["median"], 3)
            # the route through depth_summary: groups of 8 thresholds, columns differenced on the device
            groups = [tuple(range(lo, min(lo + 8, md + 1))) for lo in range(1, md + 1, 8)]
            bgs = [torch.empty((len(g), p.n), dtype=torch.int64, device="cuda") for g in groups]
            length = (p.end.to(torch.int64) - p.start.to(torch.int64)).clamp_(min=0)
            res = {}

            def chained():
                for g, bg in zip(groups, bgs):
                    eng.depth_summary_dev(ix, side, opts, g, 0, bg.data_ptr())
                ge = torch.cat(bgs, dim=0)
                h = torch.empty((p.n, md + 1), dtype=torch.int64, device="cuda")
                h[:, 1:md] = (ge[:-1] - ge[1:]).T
                h[:, md] = ge[md - 1]
                h[:, 0] = length - ge[0]
                res["h"] = h
            few = max(2, args.steps // 3) if md > 100 else args.steps
            d["chained_calls"] = len(groups)
            d["chained_ms"] = _event_ms(torch, chained, few, 1)
            assert torch.equal(res["h"], mine), f"the two routes disagree at max_depth {md}"
            d["chained_speedup"] = round(d["chained_ms"]["median"] / d["call_ms"]["median"], 3)
            if args.step == "targets" and md == 100:
                hist, sec = _numpy_route(dj, b, probe, md)
                assert (hist == mine.cpu().numpy()).all(), "the numpy route disagrees"
                d["numpy_ms"] = round(sec * 1e3, 1)
                d["numpy_speedup"] = round(sec * 1e3 / d["call_ms"]["median"], 1)
            d["checksum"] = int((mine * torch.arange(md + 1, device="cuda")).sum().item())
            rec["depths"][str(md)] = d
            del out, mine, bgs, res
    finally:
        ix.close()
    print(json.dumps(rec))


def baseline_section(doc):
    lines = [f"## depth_hist: the depth histogram per row and per contig {MARK}", "",
             f"`tools/bench_depth_hist.py`: one index of {doc['targets']['build_rows']:,} reads (100 .. 150 positions, {N_CONTIGS} contigs of "
             f"{CONTIG_LEN:,} positions), device API, HIP events, medians of {doc['targets']['calls']} calls; ms.", "",
             "| probes | max_depth | call | build share | depth_hist kernel | contig form call (kernel) | LDS 128 KiB call (kernel) | "
             "chained depth_summary (calls) | depth -> D2H -> numpy |", "|---|---|---|---|---|---|---|---|---|"]
    for step in STEPS:
        s = doc[step]
        for md in DEPTHS:
            d = s["depths"][str(md)]
            lines.append(f"| {step}: {s['probe_rows']:,} rows | {md} | {d['call_ms']['median']:.2f} | {d['build_share_ms']:.2f} | {d['hist_kernel_ms']:.2f} | "
                         f"{d['contigs_call_ms']['median']:.2f} ({d['contigs_kernel_ms']:.3f}) | {d['lds128_call_ms']['median']:.2f} "
                         f"({d['lds128_hist_kernel_ms']:.2f}), x{d['lds128_over_lds64']:.2f} | {d['chained_ms']['median']:.2f} ({d['chained_calls']}), "
                         f"x{d['chained_speedup']:.2f} | " + (f"{d['numpy_ms']:.0f}, x{d['numpy_speedup']:.0f} |" if "numpy_ms" in d else "- |"))
    return lines


def write_baseline(doc):
    path = os.path.join(ROOT, "BASELINE.md")
    text = open(path).read().rstrip("\n").split("\n")
    hit = [i for i, l in enumerate(text) if MARK in l]
    if hit:
        end = next((i for i in range(hit[0] + 1, len(text)) if text[i].startswith("## ")), len(text))
        notes = [l for l in text[hit[0]:end] if l.startswith("Residency") or l.startswith("Against")]
        text[hit[0]:end] = baseline_section(doc) + [""] + [x for l in notes for x in (l, "")]          # the hand-written notes stay
    else:
        text += [""] + baseline_section(doc) + [""]
    open(path, "w").write("\n".join(text).rstrip("\n") + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="scale every table's rows (a quick check at a small size)")
    ap.add_argument("--step", choices=STEPS)
    ap.add_argument("--baseline", action="store_true", help="also write the section into BASELINE.md")
    ap.add_argument("--from-json", help="write BASELINE.md's section from a result file of an earlier run, without a GPU")
    args = ap.parse_args()
    if args.from_json:
        return write_baseline(json.load(open(args.from_json)))
    if args.step:
        return run_step(args)
    doc = {}
    for step in STEPS:
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", step, "--steps", str(args.steps),
               "--warmup", str(args.warmup), "--scale", str(args.scale)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if p.returncode != 0:
            sys.exit(f"step {step} ended with status {p.returncode}: nothing more is started")
        doc[step] = json.loads(p.stdout.strip().split("\n")[-1])
    out_dir = os.path.join(ROOT, "profiles", "depth_hist")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bench_depth_hist.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if args.baseline:
        write_baseline(doc)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
