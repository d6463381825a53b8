#!/bin/bash
# Round-2 GPU session driver.  usage: tools/gpu_r02.sh <tag> <stage>...   (run through gpurun; everything lands in gpurun_out/<tag>_*)
#   tests:    fast (pytest -m gpu without the full-size configs) | full (full-size configs + multi-GPU tests) | k=<expr> (pytest -k)
#   benches:  c3 c3nopmc c2 c4 c5 c3two c3dense c3rows c3m1 (256-bucket window-scan path) c3m6 (slice path) sortscan
#   profiles: prof (rocprofv3 --kernel-trace --stats of config 3) | ktab (per-kernel HIP-event table, config 3)
cd "${GRAFT_REPO_ROOT:-/root/repo}"
mkdir -p gpurun_out
export TMPDIR=/tmp
tag=$1; shift
B="python bench.py --full"
for stage in "$@"; do
  o=gpurun_out/${tag}_${stage//[^A-Za-z0-9_=-]/_}
  case "$stage" in
    fast) echo "== pytest gpu (fast)"; timeout 1500 python -m pytest tests -m gpu -q -x -k "not full_size and not two_rank and not self_spawn" 2>&1 | tee $o.log | tail -15 ;;
    full) echo "== pytest gpu (full-size + multi-GPU)"; timeout 2400 python -m pytest tests -m gpu -q -x -k "full_size or two_rank or self_spawn" --durations=8 2>&1 | tee $o.log | tail -25 ;;
    k=*) echo "== pytest -k ${stage#k=}"; timeout 1500 python -m pytest tests -m gpu -q -x -k "${stage#k=}" 2>&1 | tee $o.log | tail -25 ;;
    c3) echo "== bench config3 (default run: PMC passes, CPU baseline, extras)"; timeout 1500 $B --steps 10 --warmup 2 2>$o.err | tee $o.json | cut -c1-1500; tail -5 $o.err ;;
    c3nopmc) timeout 900 $B --steps 10 --warmup 2 --no-pmc --no-cpu-baseline --kernel-table 2>$o.err | tee $o.json | cut -c1-600; tail -30 $o.err ;;
    c3m1) timeout 900 $B --steps 10 --warmup 2 --no-pmc --no-cpu-baseline --no-extras --partition-mode 1 --kernel-table 2>$o.err | tee $o.json | cut -c1-600; tail -24 $o.err ;;
    c3m6) timeout 900 $B --steps 10 --warmup 2 --no-pmc --no-cpu-baseline --partition-mode 6 --kernel-table 2>$o.err | tee $o.json | cut -c1-600; tail -24 $o.err ;;
    c3two) timeout 900 $B --steps 10 --warmup 2 --no-pmc --no-cpu-baseline --no-extras --two-pass --kernel-table 2>$o.err | tee $o.json | cut -c1-600; tail -24 $o.err ;;
    c2) timeout 900 $B --workload overlap_10M_1M_1contig --steps 10 --warmup 2 --no-pmc --kernel-table 2>$o.err | tee $o.json | cut -c1-600; tail -24 $o.err ;;
    c4) timeout 900 $B --workload nearest_50M_2M_24contig --steps 10 --warmup 2 --no-pmc --kernel-table 2>$o.err | tee $o.json | cut -c1-600; tail -24 $o.err ;;
    c5) timeout 900 $B --workload count_200M_200k_24contig --steps 10 --warmup 2 --no-pmc --kernel-table 2>$o.err | tee $o.json | cut -c1-600; tail -24 $o.err ;;
    c3dense) timeout 900 $B --workload overlap_100M_5M_24contig_dense --steps 3 --warmup 1 --no-pmc --no-cpu-baseline --no-extras --kernel-table 2>$o.err | tee $o.json | cut -c1-600; tail -24 $o.err ;;
    c3rows) timeout 900 $B --steps 10 --warmup 2 --materialize --no-pmc --no-cpu-baseline --no-extras --kernel-table 2>$o.err | tee $o.json | cut -c1-600; tail -24 $o.err ;;
    sortscan) for w in coverage_100M_5M_24contig subtract_20M_5M_24contig merge_100M_24contig; do
        timeout 900 $B --workload $w --steps 5 --warmup 2 --no-pmc --kernel-table 2>${o}_$w.err | tee ${o}_$w.json | cut -c1-400; grep -A12 "per-kernel" ${o}_$w.err | head -14; done ;;
    prof) echo "== rocprofv3 --kernel-trace --stats (config 3)";
      (cd /tmp && timeout 1200 rocprofv3 --kernel-trace --stats -d "$OLDPWD/${o}_dir" -o c3 --output-format csv -- python "$OLDPWD/bench.py" --steps 5 --warmup 2 --no-cpu-baseline --no-pmc --no-extras > "$OLDPWD/$o.out" 2> "$OLDPWD/$o.err");
      tail -2 $o.out | cut -c1-400; f=$(find ${o}_dir -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && { cp "$f" $o.kernel_stats.csv; head -25 "$f"; } ;;
    pmcsq*) echo "== PMC SQ/TCP/LDS breakdown (config 3${stage#pmcsq}; extra bench args in \$PMCARGS)";
      i=0; dirs="";
      for set in "SQ_WAVES SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_VALU SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_WAVE_CYCLES" "SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_LDS SQ_INSTS_VMEM_WR SQ_THREAD_CYCLES_VALU SQ_INSTS_BRANCH" "TCP_TCC_READ_REQ_sum TCP_TOTAL_CACHE_ACCESSES_sum TCP_TCC_READ_REQ_LATENCY_sum TCP_PENDING_STALL_CYCLES_sum" "SQ_INSTS_VMEM_RD SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS SQ_INST_LEVEL_VMEM SQ_INST_LEVEL_LDS GRBM_GUI_ACTIVE"; do
        i=$((i+1));
        (cd /tmp && timeout 300 rocprofv3 --kernel-trace --pmc $set -d "$OLDPWD/${o}_$i" -o pmc --output-format csv -- python "$OLDPWD/bench.py" --steps 2 --warmup 1 --no-cpu-baseline --no-pmc --no-extras $PMCARGS > "$OLDPWD/${o}_$i.out" 2> "$OLDPWD/${o}_$i.err");
        tail -1 ${o}_$i.err | cut -c1-160; dirs="$dirs ${o}_$i";
      done;
      python tools/pmc_summary.py $dirs > $o.summary.json 2> $o.summary.err; tail -3 $o.summary.err;
      python - "$o.summary.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
for k, v in d.items():
    if "slice" not in k and "overlap" not in k and "part_" not in k:
        continue
    g = lambda n: v.get(n, {}).get("sum", 0.0) / max(v.get(n, {}).get("rows", 1), 1)
    wc = g("SQ_WAVE_CYCLES") or 1
    print(k[:60])
    print("   waves %.0f  VALU insts %.1fM SALU %.1fM LDS %.1fM VMEM_RD %.2fM VMEM_WR %.2fM BRANCH %.1fM" % (g("SQ_WAVES"), g("SQ_INSTS_VALU")/1e6, g("SQ_INSTS_SALU")/1e6, g("SQ_INSTS_LDS")/1e6, g("SQ_INSTS_VMEM_RD")/1e6, g("SQ_INSTS_VMEM_WR")/1e6, g("SQ_INSTS_BRANCH")/1e6))
    print("   wave_cycles %.0fM busy_cycles %.1fM  wait_any/wave %.2f wait_inst_any/wave %.2f active_valu/wave %.3f active_lds/wave %.3f active_vmem/wave %.3f lanes/valu %.1f" % (wc/1e6, g("SQ_BUSY_CYCLES")/1e6, g("SQ_WAIT_ANY")/wc, g("SQ_WAIT_INST_ANY")/wc, g("SQ_ACTIVE_INST_VALU")/wc, g("SQ_ACTIVE_INST_LDS")/wc, g("SQ_ACTIVE_INST_VMEM")/wc, g("SQ_THREAD_CYCLES_VALU")/max(g("SQ_ACTIVE_INST_VALU"),1)*1.0))
    print("   LDS idx_active %.1fM bank_conflict %.1fM wait_inst_lds/wave %.3f  TCP reads %.1fM accesses %.1fM GUI_ACTIVE %.2fM" % (g("SQ_LDS_IDX_ACTIVE")/1e6, g("SQ_LDS_BANK_CONFLICT")/1e6, g("SQ_WAIT_INST_LDS")/wc, g("TCP_TCC_READ_REQ_sum")/1e6, g("TCP_TOTAL_CACHE_ACCESSES_sum")/1e6, g("GRBM_GUI_ACTIVE")/1e6))
PY
      ;;
    smoke) python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -3 ;;
    *) echo "unknown stage $stage" ;;
  esac
done
