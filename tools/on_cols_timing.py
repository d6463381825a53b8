#!/usr/bin/env python3
"""on_cols timing: the group-id passes (ivj_group_ids_dev) and a stranded join against the plain join.

  device     device API, 100M x 5M (synth overlap_100M_5M_24contig) + a seeded strand column: DeviceJoin.group wall time and
             per-kernel times, plain vs stranded overlap (fused pass into preallocated buffers)
  frontdoor  pb.overlap, 10M x 1M (synth overlap_10M_1M_1contig) as pandas frames, plain vs on_cols=["strand"]

usage: python tools/on_cols_timing.py [--out FILE]          runs each step in a child process under `timeout -k 10`
       python tools/on_cols_timing.py --step device|frontdoor
"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "polars-bio_amd")):
    sys.path.insert(0, p)

STEPS = {"device": 300, "frontdoor": 300}       # seconds each step may take


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def step_device():
    import numpy as np
    import torch
    from polars_bio_amd import synth
    from polars_bio_amd.device_api import DeviceJoin, DeviceSide
    dj = DeviceJoin(0)
    probe, build, nc = synth.workload("overlap_100M_5M_24contig")
    rng = np.random.default_rng(7)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    P, B = DeviceSide(*(t(a) for a in probe)), DeviceSide(*(t(a) for a in build))
    ps, bs = t(rng.integers(0, 2, len(probe[0]))), t(rng.integers(0, 2, len(build[0])))
    out = {"probe_rows": len(probe[0]), "build_rows": len(build[0])}

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return _median(ts), r

    ms, (p2, b2, g, _) = timed(lambda: dj.group(P, B, [ps], [bs], [2], nc), 10)
    out["group_wall_ms"] = round(ms, 4)
    out["groups"] = g
    # bytes the passes must move: contig + code in, gid out, both sides (the bitmap and scan words are a few KiB here)
    out["group_bytes"] = 12 * (len(probe[0]) + len(build[0]))
    dj.engine.enable_timing(2)
    dj.group(P, B, [ps], [bs], [2], nc)
    torch.cuda.synchronize()
    out["group_kernels"] = {k: round(v["ms"], 4) for k, v in dj.engine.timings().items()}
    out["group_kernel_ms"] = round(sum(out["group_kernels"].values()), 4)
    dj.engine.enable_timing(0)
    for name, (pp, bb, n) in {"plain": (P, B, nc), "stranded": (p2, b2, g)}.items():
        pairs = dj.overlap(pp, bb, True, n)
        total = int(pairs[0].numel())
        del pairs
        buf = (torch.empty(total + 1024, dtype=torch.int32, device="cuda"), torch.empty(total + 1024, dtype=torch.int32, device="cuda"))
        ms, r = timed(lambda: dj.overlap(pp, bb, True, n, out=buf), 7)
        out[f"{name}_overlap_ms"] = round(ms, 4)
        out[f"{name}_pairs"] = int(r[0].numel())
        del buf, r
        torch.cuda.empty_cache()
    print(json.dumps(out), flush=True)


def step_frontdoor():
    import numpy as np
    import pandas as pd
    import polars_bio_amd as pb
    from polars_bio_amd import synth
    probe, build, nc = synth.workload("overlap_10M_1M_1contig")
    rng = np.random.default_rng(8)
    strands = np.array(["+", "-"], dtype=object)

    def frame(side):
        df = pd.DataFrame({"chrom": np.array(synth.CONTIG_NAMES, dtype=object)[side[0]], "start": side[1].astype(np.int64),
                           "end": side[2].astype(np.int64), "strand": strands[rng.integers(0, 2, len(side[0]))]})
        df.attrs["coordinate_system_zero_based"] = True
        return df
    df1, df2 = frame(probe), frame(build)
    out = {"probe_rows": len(df1), "build_rows": len(df2)}
    for name, kw in {"plain": {}, "stranded": {"on_cols": ["strand"]}}.items():
        pb.overlap(df1.head(1000), df2, output_type="pyarrow.Table", **kw)
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            r = pb.overlap(df1, df2, output_type="pyarrow.Table", **kw)
            ts.append((time.perf_counter() - t0) * 1e3)
        out[f"{name}_ms"] = round(_median(ts), 2)
        out[f"{name}_rows"] = r.num_rows
        del r
    print(json.dumps(out), flush=True)


def main():
    if "--step" in sys.argv:
        {"device": step_device, "frontdoor": step_frontdoor}[sys.argv[sys.argv.index("--step") + 1]]()
        return 0
    dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    res = {}
    for step, limit in STEPS.items():
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step],
                           capture_output=True, text=True)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-4000:] + r.stderr[-4000:])
            print(f"step {step} failed with exit status {r.returncode}; no further steps", file=sys.stderr)
            return r.returncode
        res[step] = json.loads(r.stdout.strip().splitlines()[-1])
        print(step, json.dumps(res[step]), flush=True)
    if dest:
        with open(dest, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
