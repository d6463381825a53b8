#!/usr/bin/env python3
"""Time depth_quantiles (per probe row and per rank the order statistic of the build side's depth) on a built index: the call's
build share against the radix-select kernel, for 1 and 3 ranks, against the route a user had before, and at 4 against 6 bits
per pass.

    python tools/bench_depth_quantiles.py [--steps 10] [--warmup 3] [--scale 1.0] [--lib-b6 PATH] [--baseline | --from-json FILE]

The driver (no --step) starts one child process per GPU step, each under its own `timeout -k 10`, and stops at the first step
that fails: nothing more is started on a device that has just faulted or hung.  A step is (rows, bits):
  exons   200 k probe rows of 100 .. 300 positions (a few blocks under a row)
  genes   2 000 probe rows of 20 000 .. 200 000 positions (thousands of blocks under a row)
  bits    4: the in-tree library; 6: a second library compiled with -DIVJ_QUANT_BITS=6.  --lib-b6 names it; without the option
          the driver compiles it once with hipcc next to the in-tree one (about as long as the library's own build).
Each step runs three build sides on 24 contigs of 1 M positions, reads of 100 .. 150 positions:
  shallow   0.8 M reads (mean depth ~ 4, below 16: one pass at 4 bits)
  typical   8 M reads (mean depth ~ 40: two passes at 4 bits)
  pile      the typical reads plus 100 000 identical reads on contig 0 (17 bits: five passes at 4 bits in the tiles under it)
and reports per build side and K in (1, 3) (the lower median; the three lower quartiles), after warm-up:
  kernel_ms          the engine's own HIP events of one depth_quantiles_dev call, per launch name
  quant_kernel_ms    the depth_quant launch alone;  build_share_ms: everything else (the blocks, the block index, the records)
  call_ms            the whole call (HIP events around it, median of --steps calls)
  hist_route_ms      (bits 4, K 1 only) depth_hist_dev(max_depth = 1023) -> D2H of the (n, 1024) matrix -> numpy cumulative search,
                     host clock around it; hist_route_speedup = hist_route / call.  Where no depth exceeds 1023 the two are compared.

Result: one JSON line (also profiles/depth_quant/bench_depth_quantiles.json) and, with --baseline, a section in BASELINE.md."""
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
MARK = "<!-- bench_depth_quantiles -->"
ROWS = ("exons", "genes")
BITS = (4, 6)
SIDES = ("shallow", "typical", "pile")
KS = (1, 3)
N_CONTIGS, CONTIG_LEN = 24, 1_000_000
N_READS = {"shallow": 800_000, "typical": 8_000_000, "pile": 8_000_000}
PILE = 100_000


def _probe(rows, scale):
    import numpy as np
    rng = np.random.default_rng(78)
    if rows == "exons":
        n, lo, hi = max(int(200_000 * scale), 100), 100, 301
    else:
        n, lo, hi = max(int(2_000 * scale), 10), 20_000, 200_001
    ps = rng.integers(0, CONTIG_LEN - hi, n)
    return tuple(np.ascontiguousarray(a, np.int32) for a in (rng.integers(0, N_CONTIGS, n), ps, ps + rng.integers(lo, hi, n)))


def _build(side, scale):
    import numpy as np
    rng = np.random.default_rng(79)
    nb = max(int(N_READS[side] * scale), 1000)
    bc = rng.integers(0, N_CONTIGS, nb)
    bs = rng.integers(0, CONTIG_LEN - 150, nb)
    be = bs + rng.integers(100, 151, nb)
    if side == "pile":
        m = max(int(PILE * scale), 70_000)                     # 17 bits at any scale
        bc, bs, be = (np.concatenate([a, np.full(m, v)]) for a, v in ((bc, 0), (bs, 500_000), (be, 500_120)))
    return tuple(np.ascontiguousarray(a, np.int32) for a in (bc, bs, be))


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


def _hist_route(torch, eng, ix, side, opts, n, rank):
    """depth_hist at the largest max_depth, the matrix to the host, the first bin whose cumulative count exceeds the rank
    -> (values, the clamped bin's total, seconds)"""
    import numpy as np
    t0 = time.perf_counter()
    out = torch.empty((n, 1024), dtype=torch.int64, device="cuda")
    eng.depth_hist_dev(ix, side, opts, 1023, out.data_ptr())
    hist = out.cpu().numpy()
    val = np.empty(n, np.int64)
    for lo in range(0, n, 20_000):                               # (the cumulative matrix in slabs: 8 KiB per row)
        cum = np.cumsum(hist[lo:lo + 20_000], axis=1)
        val[lo:lo + 20_000] = (cum <= rank[lo:lo + 20_000, None]).sum(axis=1)
    return val, int(hist[:, 1023].sum()), time.perf_counter() - t0


def run_step(args):
    import numpy as np
    import torch
    from polars_bio_amd import _engine
    if args.lib:
        _engine.LIB_PATH = os.path.abspath(args.lib)           # before the first load
    from polars_bio_amd._engine import make_opts
    from polars_bio_amd.device_api import DeviceJoin, DeviceSide
    probe = _probe(args.rows, args.scale)
    p = DeviceSide(*(torch.from_numpy(a).cuda() for a in probe))
    L = probe[2].astype(np.int64) - probe[1].astype(np.int64)
    ranks = {1: ((L - 1) // 2)[:, None], 3: np.stack([np.floor(q * (L - 1)).astype(np.int64) for q in (0.25, 0.5, 0.75)], axis=1)}
    dj = DeviceJoin(0)
    eng = dj.engine
    opts = make_opts(True, N_CONTIGS)
    rec = {"rows": args.rows, "bits": args.bits, "probe_rows": p.n, "contigs": N_CONTIGS, "calls": args.steps, "sides": {}}
    for name in SIDES:
        b = DeviceSide(*(torch.from_numpy(a).cuda() for a in _build(name, args.scale)))
        ix = eng.index_build_dev(b.as_c(), opts, True)
        s = {"build_rows": b.n}
        try:
            side = p.as_c()
            for k in KS:
                d = {}
                r = torch.from_numpy(np.ascontiguousarray(ranks[k])).cuda()
                out = torch.empty((p.n, k), dtype=torch.int32, device="cuda")
                call = lambda: eng.depth_quantiles_dev(ix, side, opts, k, r.data_ptr(), out.data_ptr())
                for _ in range(args.warmup):
                    call()
                torch.cuda.synchronize()
                eng.enable_timing(2)
                call()
                kern = {n: round(v["ms"], 4) for n, v in eng.timings().items()}
                eng.enable_timing(0)
                d["kernel_ms"] = kern
                d["quant_kernel_ms"] = kern.get("depth_quant", 0.0)
                d["build_share_ms"] = round(sum(v for n, v in kern.items() if n != "depth_quant"), 4)
                d["call_ms"] = _event_ms(torch, call, args.steps, args.warmup)
                mine = out.cpu().numpy().astype(np.int64)
                d["checksum"] = int(mine.sum())
                d["max_value"] = int(mine.max())
                if args.bits == 4 and k == 1:
                    val, clamped, sec = _hist_route(torch, eng, ix, side, opts, p.n, ranks[1][:, 0])
                    if clamped == 0:
                        assert (val == mine[:, 0]).all(), f"the two routes disagree on {name}"
                    d["hist_route_compared"] = clamped == 0
                    d["hist_route_ms"] = round(sec * 1e3, 1)
                    d["hist_route_speedup"] = round(sec * 1e3 / d["call_ms"]["median"], 1)
                s[f"k{k}"] = d
        finally:
            ix.close()
        rec["sides"][name] = s
        del b
    print(json.dumps(rec))


def baseline_section(doc):
    any_step = doc[f"{ROWS[0]}_b4"]
    lines = [f"## depth_quantiles: exact per-row depth quantiles {MARK}", "",
             f"`tools/bench_depth_quantiles.py`: reads of 100 .. 150 positions on {N_CONTIGS} contigs of {CONTIG_LEN:,} positions, device API, HIP "
             f"events, medians of {any_step['calls']} calls; ms.  B = bits per pass (`IVJ_QUANT_BITS`).", "",
             "| probes | build side | K | B=4 call | build share | depth_quant kernel | B=6 call | B=6 kernel | B=6 / B=4 kernel | "
             "depth_hist(1023) -> D2H -> numpy |", "|---|---|---|---|---|---|---|---|---|---|"]
    for rows in ROWS:
        b4, b6 = doc[f"{rows}_b4"], doc.get(f"{rows}_b6")
        for name in SIDES:
            for k in KS:
                d = b4["sides"][name][f"k{k}"]
                e = b6["sides"][name][f"k{k}"] if b6 else None
                assert e is None or e["checksum"] == d["checksum"], "the two libraries disagree"
                lines.append(f"| {rows}: {b4['probe_rows']:,} rows | {name}: {b4['sides'][name]['build_rows']:,} reads | {k} | {d['call_ms']['median']:.2f} | "
                             f"{d['build_share_ms']:.2f} | {d['quant_kernel_ms']:.2f} | "
                             + (f"{e['call_ms']['median']:.2f} | {e['quant_kernel_ms']:.2f} | x{e['quant_kernel_ms'] / max(d['quant_kernel_ms'], 1e-9):.2f} | " if e
                                else "unmeasured | unmeasured | unmeasured | ")
                             + (f"{d['hist_route_ms']:.0f}, x{d['hist_route_speedup']:.0f} |" if "hist_route_ms" in d else "- |"))
    return lines


def write_baseline(doc):
    path = os.path.join(ROOT, "BASELINE.md")
    text = open(path).read().rstrip("\n").split("\n")
    hit = [i for i, l in enumerate(text) if MARK in l]
    if hit:
        end = next((i for i in range(hit[0] + 1, len(text)) if text[i].startswith("## ")), len(text))
        notes = [l for l in text[hit[0]:end] if l.startswith("Bits per pass") or l.startswith("Against")]
        text[hit[0]:end] = baseline_section(doc) + [""] + [x for l in notes for x in (l, "")]          # the hand-written notes stay
    else:
        text += [""] + baseline_section(doc) + [""]
    open(path, "w").write("\n".join(text).rstrip("\n") + "\n")


def build_b6():
    """the library with 6 bits per pass, next to the in-tree one"""
    pkg = os.path.join(ROOT, "polars-bio_amd")
    out = os.path.join(pkg, "polars_bio_amd", "lib", "libivjoin_hip_qb6.so")
    src = os.path.join(pkg, "csrc", "ivjoin.hip")
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(os.path.join(pkg, "csrc", f)) for f in os.listdir(os.path.join(pkg, "csrc"))):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-DIVJ_QUANT_BITS=6", "-shared", "-o", out, src], check=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="scale every table's rows (a quick check at a small size)")
    ap.add_argument("--rows", choices=ROWS)
    ap.add_argument("--bits", type=int, choices=BITS, default=4)
    ap.add_argument("--step", action="store_true", help="run one (rows, bits) step in this process")
    ap.add_argument("--lib", help="the library a step loads instead of the in-tree one")
    ap.add_argument("--lib-b6", help="a library compiled with -DIVJ_QUANT_BITS=6 (compiled here when absent)")
    ap.add_argument("--only-b6-build", action="store_true", help="compile the 6-bit library and stop (no GPU needed)")
    ap.add_argument("--baseline", action="store_true", help="also write the section into BASELINE.md")
    ap.add_argument("--from-json", help="write BASELINE.md's section from a result file of an earlier run, without a GPU")
    args = ap.parse_args()
    if args.from_json:
        return write_baseline(json.load(open(args.from_json)))
    if args.step:
        return run_step(args)
    lib6 = args.lib_b6 or build_b6()
    if args.only_b6_build:
        return print(lib6)
    doc = {}
    for rows in ROWS:
        for bits in BITS:
            cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", "--rows", rows, "--bits", str(bits),
                   "--steps", str(args.steps), "--warmup", str(args.warmup), "--scale", str(args.scale)] + (["--lib", lib6] if bits == 6 else [])
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:
                sys.exit(f"step {rows} / {bits} bits ended with status {p.returncode}: nothing more is started")
            doc[f"{rows}_b{bits}"] = json.loads(p.stdout.strip().split("\n")[-1])
    out_dir = os.path.join(ROOT, "profiles", "depth_quant")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bench_depth_quantiles.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    if args.baseline:
        write_baseline(doc)
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
