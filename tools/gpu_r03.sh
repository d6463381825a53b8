#!/bin/bash
# Round-3 GPU session driver.  usage: tools/gpu_r03.sh <tag> <stage>...   (run through gpurun; everything lands in gpurun_out/<tag>_*)
#   tests:    fast (pytest -m gpu without the full-size configs) | full (full-size configs + multi-GPU tests) | k=<expr> (pytest -k)
#   benches:  c3 (default run) c3q (no PMC / baseline / extras, kernel table) c3old (IVJ_CS=0: round-2 slice kernels) c2 c4 c5 c1 c3two c3dense c3rows sortscan
#             env=<VAR=val,...>:<stage> runs a stage under extra environment variables (A/B knobs)
#   profiles: prof (rocprofv3 --kernel-trace --stats of config 3) | pmcsq (SQ / TCP / LDS counter passes of config 3)
cd "${GRAFT_REPO_ROOT:-/root/repo}"
mkdir -p gpurun_out
export TMPDIR=/tmp
tag=$1; shift
B="python bench.py --full"
Q="--no-pmc --no-cpu-baseline --no-extras --kernel-table"
run_stage() {
  local stage=$1 sfx=$2
  local o=gpurun_out/${tag}_${stage//[^A-Za-z0-9_=-]/_}$sfx
  case "$stage" in
    fast) echo "== pytest gpu (fast)"; timeout 1500 python -m pytest tests -m gpu -q -x -k "not full_size and not two_rank and not self_spawn" 2>&1 | tee $o.log | tail -15 ;;
    full) echo "== pytest gpu (full-size + multi-GPU)"; timeout 2400 python -m pytest tests -m gpu -q -x -k "full_size or two_rank or self_spawn" --durations=8 2>&1 | tee $o.log | tail -25 ;;
    k=*) echo "== pytest -k ${stage#k=}"; timeout 1500 python -m pytest tests -m gpu -q -x -k "${stage#k=}" 2>&1 | tee $o.log | tail -25 ;;
    c3) echo "== bench config3 (default run: PMC passes, CPU baseline, extras)"; timeout 1500 $B --steps 10 --warmup 2 2>$o.err | tee $o.json | cut -c1-1500; tail -5 $o.err ;;
    c3q) timeout 900 $B --steps 10 --warmup 2 $Q 2>$o.err | tee $o.json | cut -c1-400; grep -A16 "per-kernel" $o.err ;;
    c3old) IVJ_CS=0 timeout 900 $B --steps 10 --warmup 2 $Q 2>$o.err | tee $o.json | cut -c1-400; grep -A16 "per-kernel" $o.err ;;
    c3two) timeout 900 $B --steps 10 --warmup 2 $Q --two-pass 2>$o.err | tee $o.json | cut -c1-400; grep -A16 "per-kernel" $o.err ;;
    c1) timeout 600 $B --workload overlap_1k_1k_1contig --steps 20 --warmup 3 --no-pmc --kernel-table 2>$o.err | tee $o.json | cut -c1-600; grep -A12 "per-kernel" $o.err ;;
    c2) timeout 900 $B --workload overlap_10M_1M_1contig --steps 10 --warmup 2 --kernel-table 2>$o.err | tee $o.json | cut -c1-600; grep -A16 "per-kernel" $o.err ;;
    c4) timeout 900 $B --workload nearest_50M_2M_24contig --steps 10 --warmup 2 --kernel-table 2>$o.err | tee $o.json | cut -c1-600; grep -A16 "per-kernel" $o.err ;;
    c5) timeout 900 $B --workload count_200M_200k_24contig --steps 10 --warmup 2 --kernel-table 2>$o.err | tee $o.json | cut -c1-600; grep -A16 "per-kernel" $o.err ;;
    c3fd) echo "== bench config3 through the N > 1 code path on one rank (library communicator, world 1)"; timeout 900 $B --force-dist --steps 5 --warmup 2 $Q 2>$o.err | tee $o.json | cut -c1-900 ;;
    frontend) timeout 600 python tools/frontend_e2e.py 2>&1 | tee $o.txt | tail -12 ;;
    c3dense) timeout 900 $B --workload overlap_100M_5M_24contig_dense --steps 3 --warmup 1 $Q 2>$o.err | tee $o.json | cut -c1-600; grep -A16 "per-kernel" $o.err ;;
    c3rows) timeout 900 $B --steps 10 --warmup 2 --materialize $Q 2>$o.err | tee $o.json | cut -c1-600; grep -A16 "per-kernel" $o.err ;;
    sortscan) for w in coverage_100M_5M_24contig subtract_20M_5M_24contig merge_100M_24contig; do
        timeout 900 $B --workload $w --steps 5 --warmup 2 --kernel-table 2>${o}_$w.err | tee ${o}_$w.json | cut -c1-400; grep -A12 "per-kernel" ${o}_$w.err | head -14; done ;;
    prof) echo "== rocprofv3 --kernel-trace --stats (config 3)";
      (cd /tmp && timeout 1200 rocprofv3 --kernel-trace --stats -d "$OLDPWD/${o}_dir" -o c3 --output-format csv -- python "$OLDPWD/bench.py" --steps 5 --warmup 2 --no-cpu-baseline --no-pmc --no-extras > "$OLDPWD/$o.out" 2> "$OLDPWD/$o.err");
      tail -2 $o.out | cut -c1-400; f=$(find ${o}_dir -name "*kernel_stats.csv" | head -1); [ -n "$f" ] && { cp "$f" $o.kernel_stats.csv; head -25 "$f"; } ;;
    pmcsq*) echo "== PMC SQ/TCP/LDS breakdown (config 3${stage#pmcsq}; extra bench args in \$PMCARGS)";
      i=0; dirs="";
      for set in "SQ_WAVES SQ_INSTS_SALU SQ_INSTS_SMEM SQ_INSTS_VALU SQ_ACTIVE_INST_ANY SQ_ACTIVE_INST_VALU SQ_ACTIVE_INST_SCA SQ_WAVE_CYCLES" "SQ_BUSY_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_VMEM SQ_ACTIVE_INST_LDS SQ_INSTS_VMEM_WR SQ_THREAD_CYCLES_VALU SQ_INSTS_BRANCH" "SQ_INSTS_VMEM_RD SQ_INSTS_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_INST_LDS SQ_INST_LEVEL_VMEM SQ_INST_LEVEL_LDS GRBM_GUI_ACTIVE"; do
        i=$((i+1));
        (cd /tmp && timeout 300 rocprofv3 --kernel-trace --pmc $set -d "$OLDPWD/${o}_$i" -o pmc --output-format csv -- python "$OLDPWD/bench.py" --steps 2 --warmup 1 --no-cpu-baseline --no-pmc --no-extras $PMCARGS > "$OLDPWD/${o}_$i.out" 2> "$OLDPWD/${o}_$i.err");
        tail -1 ${o}_$i.err | cut -c1-160; dirs="$dirs ${o}_$i";
      done;
      python tools/pmc_summary.py $dirs > $o.summary.json 2> $o.summary.err; tail -3 $o.summary.err;
      python tools/pmc_print.py $o.summary.json ;;
    smoke) python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -3 ;;
    *) echo "unknown stage $stage" ;;
  esac
}
for stage in "$@"; do
  case "$stage" in
    env=*:*) kv=${stage#env=}; st=${kv#*:}; kv=${kv%%:*}; sfx=_${kv//[^A-Za-z0-9]/_};
             ( IFS=,; for a in $kv; do export "$a"; done; echo "== [$kv] $st"; run_stage "$st" "$sfx" ) ;;
    *) run_stage "$stage" "" ;;
  esac
done
