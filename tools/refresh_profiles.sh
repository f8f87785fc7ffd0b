#!/bin/bash
# Re-take the profiles/ evidence of a list of workloads on the binary in the tree, on ONE box:
#   gpurun --timeout 1500 -- 'bash tools/refresh_profiles.sh r05 g1_c3 g1_full shadow_c4'
# Per workload: the seven --pmc passes and the kernel-trace pass of tools/profile.sh (each its own rocprofv3 run), the summaries
# copied into profiles/ on the box so that the bench line of the same binary replays them, then that bench line
# (<tag>_<config>_b<B>_bench.json, with the --full legs; the CPU legs only for the headline).  Last: the default bench line with
# --full, every other workload as `other_configs` (<tag>_default_bench.json).  Everything lands in $MKH_RESULTS_DIR (default:
# results/); copy <tag>_* from there into profiles/ afterwards.
set -u
TAG=$1; shift
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
export MKH_RESULTS_DIR=$(mkdir -p "${MKH_RESULTS_DIR:-$R/results}" && cd "${MKH_RESULTS_DIR:-$R/results}" && pwd)
RES=$MKH_RESULTS_DIR
cd "$R"
for CFG in "$@"; do
  B=$(python -c "import sys; sys.path.insert(0, '$R'); from mink_amd import workloads as w; print(w.BENCH_CONFIGS['$CFG']['batch'])")
  NAME=${CFG}_b${B}
  MKH_PROFILE_PMC_ONLY=1 bash tools/profile.sh "$TAG" "$CFG" > /dev/null 2>&1
  MKH_PROFILE_TRACE_ONLY=1 bash tools/profile.sh "$TAG" "$CFG" > /dev/null 2>&1
  cp "$RES/${TAG}_${NAME}_pmc.json" "$RES/${TAG}_${NAME}_kernel_stats.csv" profiles/ 2>/dev/null
  EXTRA="--full --no-cpu-baseline"; [ "$CFG" = g1_c3 ] && EXTRA="--full"
  timeout 300 python bench.py --config "$CFG" --batch "$B" --steps 20 --warmup 3 $EXTRA > "$RES/${TAG}_${NAME}_bench.json" 2> "$RES/${TAG}_${NAME}_bench.err"
  python - <<PY
import json
try:
    d = json.load(open("$RES/${TAG}_${NAME}_bench.json")); r = d["roofline"]
    print("$CFG", "%.2f M/s" % (d["value"] / 1e6), r["kernel"], "kernel %.4f ms" % r["kernel_ms"], "traffic", r.get("traffic"), "stale", r.get("stale_profile"))
except Exception as e:
    print("$CFG", "FAILED", e)
PY
done
timeout 600 python bench.py --full > "$RES/${TAG}_default_bench.json" 2> "$RES/${TAG}_default_bench.err"
head -c 300 "$RES/${TAG}_default_bench.json"; echo
