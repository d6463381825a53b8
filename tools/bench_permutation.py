#!/usr/bin/env python3
"""Time pb.permutation_test's device entry (ivj_permute_overlaps_dev) against the composition the device API offered before it.

    python tools/bench_permutation.py [--steps 10] [--warmup 3] [--scale 1.0] [--shape small|big|both] [--baseline]

One process.  Per shape -- df1 1 M x df2 200 k rows with 1000 permutations, df1 5 M x df2 5 M with 100, uniform rows on 24 contigs
from polars_bio_amd.synth -- the rows are uploaded once, ONE index is built and, after --warmup calls, --steps whole calls are timed
between HIP events (median, min .. max):
  permute      ivj_permute_overlaps_dev over all permutations: one call
  composed     per permutation a torch shift-and-split of the device-resident df1 columns (first pieces in rows [0, n), second
               pieces of the wrapped rows in rows [n, 2 n), contig -1 where a row does not wrap), then
               ivj_count_overlaps_thresh_dev(min_overlap = 1) on the same index and torch sums -- nothing leaves the device
  count        plain ivj_count_overlaps_dev of the unshifted rows: what ONE permutation's lookups cost as a stand-alone call
The two integer arrays of both routes are compared.  No ratio is fixed in advance: the claim to check is "the one call is not slower
than the composition", and a ratio below 1 is written down as such.

Result: one JSON line per shape (also profiles/permutation/bench_permutation.json) and, with --baseline, a subsection in BASELINE.md."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "polars-bio_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = {"small": (1_000_000, 200_000, 1000), "big": (5_000_000, 5_000_000, 100)}
N_CONTIGS = 24
MARK_BEGIN, MARK_END = "<!-- bench_permutation -->", "<!-- /bench_permutation -->"


def _timed(torch, fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ev.append(a.elapsed_time(b))
    return {"median": round(sorted(ev)[len(ev) // 2], 4), "min": round(min(ev), 4), "max": round(max(ev), 4)}


def run_shape(shape, args):
    import numpy as np
    import torch
    from polars_bio_amd import synth
    from polars_bio_amd._engine import Engine, make_opts, make_thresholds
    from polars_bio_amd.device_api import DeviceJoin, DeviceSide
    n_probe, n_build, n_perm = SHAPES[shape]
    n_probe, n_build = max(int(n_probe * args.scale), 1), max(int(n_build * args.scale), 1)
    probe = synth.make_rows(n_probe, 42, synth.PROBE_LEN, N_CONTIGS)[0]
    build = synth.make_rows(n_build, 43, synth.BUILD_LEN, N_CONTIGS)[0]
    assert min(int(probe[1].min()), int(build[1].min())) >= 0
    length = max(int(probe[2].max()), int(build[2].max())) + 1000
    lengths = np.full(N_CONTIGS, length, np.int32)
    off = np.random.default_rng(44).integers(0, lengths[None, :].astype(np.int64), size=(n_perm, N_CONTIGS)).astype(np.int32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    p, b = DeviceSide(*map(dev, probe)), DeviceSide(*map(dev, build))
    d_len, d_off = dev(lengths), dev(off)
    dj = DeviceJoin(0)
    eng = dj.engine
    opts = make_opts(True, N_CONTIGS)
    ix = eng.index_build_dev(b.as_c(), opts, True)
    rec = {"shape": shape, "probe_rows": n_probe, "build_rows": n_build, "n_perm": n_perm, "contigs": N_CONTIGS, "contig_len": length,
           "calls": args.steps}
    try:
        side = p.as_c()
        pairs = torch.zeros(n_perm, dtype=torch.int64, device="cuda")
        rows = torch.zeros(n_perm, dtype=torch.int64, device="cuda")
        new = lambda: eng.permute_overlaps_dev(ix, side, opts, d_len.data_ptr(), d_off.data_ptr(), n_perm, pairs.data_ptr(), rows.data_ptr())
        # the composition: columns of 2 n rows, reused by every permutation
        n = n_probe
        pc64, ps64, ln64 = p.contig.long(), p.start.long(), (p.end - p.start).long()
        c2 = torch.empty(2 * n, dtype=torch.int32, device="cuda")
        s2 = torch.zeros(2 * n, dtype=torch.int32, device="cuda")
        e2 = torch.empty(2 * n, dtype=torch.int32, device="cuda")
        c2[:n] = p.contig
        counts = torch.empty(2 * n, dtype=torch.int64, device="cuda")
        side2 = Engine.dev_side(c2.data_ptr(), s2.data_ptr(), e2.data_ptr(), 2 * n, 0)
        thr = make_thresholds(1)
        c_pairs, c_rows = torch.zeros_like(pairs), torch.zeros_like(rows)
        off64, minus1 = d_off.long(), torch.full((n,), -1, dtype=torch.int32, device="cuda")

        def composed():
            for k in range(n_perm):
                s1 = (ps64 + off64[k][pc64]) % length
                e1 = s1 + ln64
                wrap = e1 > length
                s2[:n] = s1.int()
                e2[:n] = torch.clamp(e1, max=length).int()
                c2[n:] = torch.where(wrap, p.contig, minus1)
                e2[n:] = (e1 - length).int()                   # (start of a second piece is 0: s2[n:] stays)
                eng.count_overlaps_thresh_dev(ix, side2, opts, thr, counts.data_ptr())
                c_pairs[k] = counts.sum()
                c_rows[k] = ((counts[:n] + counts[n:]) > 0).sum()

        plain = torch.empty(n, dtype=torch.int64, device="cuda")
        rec["permute_ms"] = _timed(torch, new, args.steps, args.warmup)
        rec["composed_ms"] = _timed(torch, composed, args.steps, args.warmup)
        rec["count_ms"] = _timed(torch, lambda: eng.count_overlaps_dev(ix, side, opts, plain.data_ptr()), args.steps, args.warmup)
        eng.enable_timing(2)
        new()
        rec["permute_kernel_ms"] = {k: round(v["ms"], 4) for k, v in eng.timings().items()}
        eng.enable_timing(0)
        torch.cuda.synchronize()
        rec["results_equal"] = bool(torch.equal(pairs, c_pairs) and torch.equal(rows, c_rows))
        rec["n_pairs_first"], rec["n_rows_first"] = int(pairs[0]), int(rows[0])
        rec["ratio_composed_over_permute"] = round(rec["composed_ms"]["median"] / rec["permute_ms"]["median"], 2)
        rec["permute_ms_per_permutation"] = round(rec["permute_ms"]["median"] / n_perm, 5)
    finally:
        ix.close()
    return rec


def baseline_section(recs):
    lines = [MARK_BEGIN, "### Permutation test (tools/bench_permutation.py)", "",
             "HIP events, median of the timed calls (min .. max), one index per shape, 24 contigs; `composed` = per permutation a torch",
             "shift-and-split + `count_overlaps_thresh_dev(min_overlap=1)` + torch sums on the same index; `count` = one plain",
             "`count_overlaps_dev` of the unshifted df1 rows.", "",
             "| df1 x df2 rows | permutations | permute ms | composed ms | composed / permute | permute ms per permutation | count ms | results equal |",
             "|---|---|---|---|---|---|---|---|"]
    f = lambda s: f"{s['median']} ({s['min']} .. {s['max']})"
    for r in recs:
        lines.append(f"| {r['probe_rows']:,} x {r['build_rows']:,} | {r['n_perm']} | {f(r['permute_ms'])} | {f(r['composed_ms'])} | "
                     f"{r['ratio_composed_over_permute']} | {r['permute_ms_per_permutation']} | {f(r['count_ms'])} | {r['results_equal']} |")
    return "\n".join(lines + ["", MARK_END, ""])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--shape", choices=["small", "big", "both"], default="both")
    ap.add_argument("--baseline", action="store_true")
    args = ap.parse_args()
    import torch  # noqa: F401  (before the engine library: it brings its own runtime)
    recs = []
    for shape in (("small", "big") if args.shape == "both" else (args.shape,)):
        t0 = time.time()
        rec = run_shape(shape, args)
        rec["wall_s"] = round(time.time() - t0, 1)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    out = os.path.join(ROOT, "profiles", "permutation")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "bench_permutation.json"), "w") as fh:
        for r in recs:
            fh.write(json.dumps(r) + "\n")
    if args.baseline:
        path = os.path.join(ROOT, "BASELINE.md")
        text = open(path).read()
        sec = baseline_section(recs)
        if MARK_BEGIN in text and MARK_END in text:
            text = text[:text.index(MARK_BEGIN)] + sec.rstrip("\n") + text[text.index(MARK_END) + len(MARK_END):]
        else:
            text = text.rstrip("\n") + "\n\n" + sec
        open(path, "w").write(text)
    if not all(r["results_equal"] for r in recs):
        sys.exit("the two routes disagree")


if __name__ == "__main__":
    main()
