#!/usr/bin/env python3
"""Time the overlap-weighted walk (pb.signal_summary / pb.signal_profile) on the device against its unweighted form and against
what a user had before.

    python tools/bench_signal.py [--steps 10] [--warmup 3] [--scale 1.0] [--baseline]

The driver (no --step) starts ONE child process for the GPU step under its own `timeout -k 10`.  The child builds a signal track
of short rows (a tiling of 24 contigs into runs of 1 .. 50 positions, as a bedGraph has them) and uniform probe rows and windows,
uploads them once, builds ONE index and times, after --warmup calls, --steps whole calls between HIP events
(median, min .. max):
  wagg          ivj_overlap_wagg_dev, one int64 and one double value column, all five operations each
  agg_thr       ivj_overlap_agg_dev under min_overlap = 1 on the same call: the same walk, every row weighing 1
  old           the route users had: fused pairs on the device -> D2H of both pair columns -> numpy clip / multiply / group-by
                (np.add.at over the probe index) for the same two columns                                       (wall clock)
  profile       ivj_signal_profile_dev: windows (12 bytes per row) in, one double column, sum / mean / bases matrices out
  profile_flat  ivj_overlap_wagg_dev over the explicit bin frame of the same windows, built with numpy and uploaded (the upload
                is not timed; the frame's bytes are reported)
The columns of wagg and old and of profile and profile_flat are compared (integers bit for bit; double sums to the bound of a
reordered sum).  No ratio is fixed in advance; a ratio above 1 is written down as such.

Result: one JSON line (also profiles/signal/bench_signal.json) and, with --baseline, a subsection in BASELINE.md."""
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
N_PROBE, N_TRACK, N_WINDOWS, N_BINS = 5_000_000, 20_000_000, 50_000, 100
N_CONTIGS = 24
MARK_BEGIN, MARK_END = "<!-- bench_signal -->", "<!-- /bench_signal -->"


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


def _track(np, n, seed):
    """n rows tiling N_CONTIGS contigs without gaps: runs of 1 .. 50 positions, half-open."""
    rng = np.random.default_rng(seed)
    per = n // N_CONTIGS
    c = np.repeat(np.arange(N_CONTIGS, dtype=np.int32), per)
    ln = rng.integers(1, 51, len(c))
    e = ln.reshape(N_CONTIGS, per).cumsum(axis=1).reshape(-1)
    return c, (e - ln).astype(np.int32), e.astype(np.int32), int(e.reshape(N_CONTIGS, per)[:, -1].min())


def run_step(args):
    import numpy as np
    import torch
    from polars_bio_amd import range_op
    from polars_bio_amd._engine import AGG_F64, AGG_I64, make_opts, make_thresholds
    from polars_bio_amd.device_api import DeviceJoin, DeviceSide
    n_probe, n_track, n_win = (max(int(n * args.scale), N_CONTIGS) for n in (N_PROBE, N_TRACK, N_WINDOWS))
    bc, bs, be, span = _track(np, n_track, 43)
    n_track = len(bc)
    rng = np.random.default_rng(44)
    rows = lambda n, max_len: (rng.integers(0, N_CONTIGS, n).astype(np.int32), rng.integers(0, span - max_len, n).astype(np.int32), rng.integers(1, max_len, n))
    pc, ps, pl = rows(n_probe, 400)
    wc, ws, wl = rows(n_win, 5000)
    probe, windows = (pc, ps, (ps + pl).astype(np.int32)), (wc, ws, (ws + wl).astype(np.int32))
    vi = rng.integers(-1000, 1000, n_track).astype(np.int64)
    vf = rng.standard_normal(n_track)
    dev_side = lambda side: DeviceSide(*(torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda() for a in side))
    p, b, w = dev_side(probe), dev_side((bc, bs, be)), dev_side(windows)
    dvi, dvf = torch.from_numpy(vi).cuda(), torch.from_numpy(vf).cuda()
    dj = DeviceJoin(0)
    eng = dj.engine
    opts = make_opts(True, N_CONTIGS)
    ix = eng.index_build_dev(b.as_c(), opts, True)
    rec = {"probe_rows": n_probe, "track_rows": n_track, "windows": n_win, "bins": N_BINS, "contigs": N_CONTIGS, "calls": args.steps}
    try:
        kinds = lambda dt: {"sum": dt, "min": dt, "max": dt, "mean": torch.float64, "count": torch.int64}
        new = lambda n, d: {op: torch.empty(n, dtype=dt, device="cuda") for op, dt in kinds(d).items()}
        ptrs = lambda outs: [{op: t.data_ptr() for op, t in o.items()} for o in outs]
        outs = [new(n_probe, torch.int64), new(n_probe, torch.float64)]
        cols = [(dvi.data_ptr(), 0, AGG_I64, 31), (dvf.data_ptr(), 0, AGG_F64, 31)]
        side, thr = p.as_c(), make_thresholds(1)
        calls = {"wagg": lambda: eng.overlap_wagg_dev(ix, side, opts, None, n_track, cols, ptrs(outs)),
                 "agg_thr": lambda: eng.overlap_agg_dev(ix, side, opts, thr, n_track, cols, ptrs(outs))}
        for name in ("agg_thr", "wagg"):
            rec[f"{name}_ms"], rec[f"{name}_wall_ms"] = _timed(torch, calls[name], args.steps, args.warmup)
        torch.cuda.synchronize()
        got = [{op: t.cpu().numpy() for op, t in o.items()} for o in outs]
        n_pairs = eng.overlap_count_dev(ix, side, opts)
        cap = n_pairs + n_pairs // 8 + 1024
        pair_out = [torch.empty(cap, dtype=torch.int32, device="cuda") for _ in range(2)]
        old = {}

        def old_route():
            pi, bi = dj.overlap(p, b, True, N_CONTIGS, index=ix, out=pair_out)
            pi, bi = pi.cpu().numpy(), bi.cpu().numpy()
            ov = np.minimum(probe[2][pi], be[bi]).astype(np.int64) - np.maximum(probe[1][pi], bs[bi])
            keep = ov >= 1
            pi, bi, ov = pi[keep], bi[keep], ov[keep]
            bases = np.zeros(n_probe, np.int64)
            np.add.at(bases, pi, ov)
            res = []
            for v in (vi, vf):
                s = np.zeros(n_probe, v.dtype)
                np.add.at(s, pi, v[bi] * ov.astype(v.dtype))
                res.append({"sum": s, "count": bases})
            old["res"] = res

        _, rec["old_wall_ms"] = _timed(torch, old_route, max(3, args.steps // 3), 1)
        assert (got[0]["count"] == old["res"][0]["count"]).all() and (got[0]["sum"] == old["res"][0]["sum"]).all(), "integers differ from the old route"
        tol = np.maximum(got[1]["count"], 1) * 2.0 ** -52 * 50 * np.abs(vf).max() * 64
        assert (np.abs(got[1]["sum"] - old["res"][1]["sum"]) <= tol).all(), "double sums differ from the old route beyond reordering"
        rec["pairs"] = int(n_pairs)

        # the profile against the explicit bin frame
        lens = range_op.profile_bin_lengths(windows[1], windows[2], True, N_BINS)
        edges = windows[1].astype(np.int64)[:, None] + np.concatenate([np.zeros((n_win, 1), np.int64), np.cumsum(lens, axis=1)], axis=1)
        frame = (np.repeat(wc, N_BINS), edges[:, :-1].reshape(-1), edges[:, 1:].reshape(-1))
        f = dev_side(frame)
        rec["bin_frame_bytes"], rec["window_bytes"] = 12 * n_win * N_BINS, 12 * n_win
        pcols = [(dvf.data_ptr(), 0, AGG_F64, 1 | 8 | 16)]
        pm, fm = new(n_win * N_BINS, torch.float64), new(n_win * N_BINS, torch.float64)
        fside, wside = f.as_c(), w.as_c()
        calls = {"profile": lambda: eng.signal_profile_dev(ix, wside, 0, N_BINS, opts, n_track, pcols, ptrs([pm])),
                 "profile_flat": lambda: eng.overlap_wagg_dev(ix, fside, opts, None, n_track, pcols, ptrs([fm]))}
        for name in ("profile_flat", "profile"):
            rec[f"{name}_ms"], rec[f"{name}_wall_ms"] = _timed(torch, calls[name], args.steps, args.warmup)
        torch.cuda.synchronize()
        # (a large probe side is bucketed by position, so the two calls fold a bin's rows in different tile geometries: the bases are
        # identical, the double sums agree to the bound of a reordered sum of at most 64 products)
        assert torch.equal(pm["count"], fm["count"]), "profile bases differ from the explicit bin frame"
        some = pm["count"] > 0
        ptol = pm["count"].double() * (2.0 ** -52 * 64 * float(np.abs(vf).max()))
        assert bool(((pm["sum"] - fm["sum"]).abs() <= ptol).all()), "profile sums differ from the explicit bin frame beyond reordering"
        rec["bins_with_signal"] = int(some.sum())
    finally:
        ix.close()
    m = lambda k: rec[k]["median"]
    rec["wagg_over_agg_thr"] = round(m("wagg_ms") / m("agg_thr_ms"), 3)
    rec["wagg_over_old"] = round(m("wagg_wall_ms") / m("old_wall_ms"), 5)
    rec["profile_over_flat"] = round(m("profile_ms") / m("profile_flat_ms"), 3)
    print(json.dumps(rec))


def baseline_section(d):
    f = lambda k: "-" if k is None else f"{d[k]['median']:.3f} ({d[k]['min']:.3f} .. {d[k]['max']:.3f})"
    return "\n".join([
        MARK_BEGIN, "### signal_summary / signal_profile: the weighted walk against the unweighted one, pairs + host group-by, and an explicit bin frame", "",
        f"`tools/bench_signal.py`: a track of {d['track_rows'] / 1e6:g} M rows tiling {d['contigs']} contigs in runs of 1 .. 50 positions, "
        f"{d['probe_rows'] / 1e6:g} M probe rows of 1 .. 399 positions ({d['pairs'] / 1e6:.1f} M pairs), {d['windows']} windows of 1 .. 4999 "
        f"positions x {d['bins']} bins; one index, one int64 and one double value column with all five operations (the profile: one double "
        f"column, sum / mean / bases); median (min .. max) of {d['calls']} whole calls after warm-up (JSON: `profiles/signal/bench_signal.json`).  "
        "One machine, one run series: the ratios are what this series gave, not targets.", "",
        "| route | HIP events, ms | wall clock, ms |", "|---|---|---|",
        f"| `ivj_overlap_wagg_dev` | {f('wagg_ms')} | {f('wagg_wall_ms')} |",
        f"| `ivj_overlap_agg_dev`, `min_overlap = 1` (unweighted, same call) | {f('agg_thr_ms')} | {f('agg_thr_wall_ms')} |",
        f"| old: fused pairs + D2H + numpy clip / multiply / group-by | - | {f('old_wall_ms')} |",
        f"| `ivj_signal_profile_dev` ({d['window_bytes'] / 1e6:g} MB of windows in) | {f('profile_ms')} | {f('profile_wall_ms')} |",
        f"| `ivj_overlap_wagg_dev` over the explicit bin frame ({d['bin_frame_bytes'] / 1e6:g} MB, upload not timed) | {f('profile_flat_ms')} | {f('profile_flat_wall_ms')} |",
        "", f"weighted / unweighted = {d['wagg_over_agg_thr']:.3f}; weighted / old route = {d['wagg_over_old']:.5f} (wall clock); "
        f"profile / explicit bin frame = {d['profile_over_flat']:.3f}; {d['bins_with_signal']} of {d['windows'] * d['bins']} bins hold signal.", MARK_END])


def write_baseline(d):
    path = os.path.join(ROOT, "BASELINE.md")
    text = open(path).read()
    sec = baseline_section(d)
    if MARK_BEGIN in text and MARK_END in text:
        text = text[:text.index(MARK_BEGIN)] + sec + text[text.index(MARK_END) + len(MARK_END):]
    else:
        at = text.index("<!-- bench_merge_agg -->")                           # the newest subsection of the results comes first
        text = text[:at] + sec + "\n\n" + text[at:]
    open(path, "w").write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="scale every table's rows (a quick check at a small size)")
    ap.add_argument("--step", action="store_true", help="run the GPU step in this process")
    ap.add_argument("--baseline", action="store_true", help="also write the subsection into BASELINE.md")
    ap.add_argument("--from-json", default=None, help="write the BASELINE.md subsection from a result file instead of running")
    args = ap.parse_args()
    if args.step:
        return run_step(args)
    if args.from_json:
        return write_baseline(json.load(open(args.from_json)))
    cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step",
           "--steps", str(args.steps), "--warmup", str(args.warmup), "--scale", str(args.scale)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    if p.returncode != 0:
        sys.exit(f"the GPU step ended with status {p.returncode}")
    doc = json.loads(p.stdout.strip().split("\n")[-1])
    out_dir = os.path.join(ROOT, "profiles", "signal")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bench_signal.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if args.baseline:
        write_baseline(doc)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
