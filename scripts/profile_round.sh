#!/bin/bash
# Collects one round's rocprofv3 evidence on the GPU box (run through gpurun from the repo root):
#   scripts/profile_round.sh r02a
# writes $RESULTS_DIR/<tag>_{kernel_stats.csv,hip_event_table.csv,concurrency.txt,pmc_FETCH_SIZE.csv,
# pmc_WRITE_SIZE.csv,pmc_sq_counters.csv,bench_line.json,hip_event_table_1stream.csv} (RESULTS_DIR: results/ under the
# repository root by default); scripts/assemble_profiles.py <tag> then turns them into profiles/<tag>_*.
# Every GPU step runs once, under a time limit of its own: a step that fails, crashes, runs out of time or leaves no
# (or an empty) result file ends the script with a non-zero status -- nothing more starts on the GPU after it, and no
# stale file passes for evidence.
set -u
TAG=${1:-round}
R=${GRAFT_REPO_ROOT:-$(pwd)}
OUT=${RESULTS_DIR:-results}
case $OUT in /*) ;; *) OUT=$R/$OUT ;; esac
cd /tmp && export TMPDIR=/tmp
cd "$R"
mkdir -p "$OUT"
rm -f "$OUT"/${TAG}_*

fail() { echo "profile_round: $*" >&2; exit 1; }
need() { [ -s "$1" ] || fail "missing or empty: $1"; }
# profiled <seconds> <dir> -- rocprofv3 ...: one attempt in a fresh output directory; true only if it exited 0 and wrote CSVs
profiled() {
  local limit=$1 dir=$2; shift 3
  rm -rf "$dir"
  timeout -k 10 "$limit" "$@" > "$dir.log" 2>&1 && ls "$dir"/*/*.csv > /dev/null 2>&1
}

# (nothing behind the timed steps in this run: trace_concurrency.py looks at the last 60 % of the traced window)
export MM3D_BENCH_NO_ISOLATED=1
profiled 900 /tmp/prof_kt -- rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof_kt -- python3 bench.py --steps 5 --warmup 3 --no-pcie --no-pair-stage \
    --no-cpu-baseline --kernel-table "$OUT/${TAG}_hip_event_table.csv" || fail "kernel trace (see /tmp/prof_kt.log)"
cp /tmp/prof_kt/*/*kernel_stats.csv "$OUT/${TAG}_kernel_stats.csv" || fail "no kernel_stats.csv"
need "$OUT/${TAG}_kernel_stats.csv"; need "$OUT/${TAG}_hip_event_table.csv"
python3 scripts/trace_concurrency.py /tmp/prof_kt/*/*kernel_trace.csv > "$OUT/${TAG}_concurrency.txt" || fail "trace_concurrency"
unset MM3D_BENCH_NO_ISOLATED
for cnt in FETCH_SIZE WRITE_SIZE; do
  profiled 600 /tmp/prof_pmc -- rocprofv3 --kernel-trace --pmc $cnt --output-format csv -d /tmp/prof_pmc -- python3 bench.py --full --steps 1 --warmup 1 \
      --streams 1 --no-cpu-baseline || fail "pmc $cnt (see /tmp/prof_pmc.log)"
  python3 scripts/pmc_summary.py /tmp/prof_pmc/*/*counter_collection.csv > "$OUT/${TAG}_pmc_${cnt}.csv" || fail "pmc_summary $cnt"
  need "$OUT/${TAG}_pmc_${cnt}.csv"
done
profiled 600 /tmp/prof_sqA -- rocprofv3 --kernel-trace --pmc SQ_WAVES SQ_WAVE_CYCLES SQ_BUSY_CYCLES SQ_INSTS_VALU SQ_ACTIVE_INST_VALU SQ_WAIT_ANY \
    SQ_WAIT_INST_ANY SQ_INSTS_LDS --output-format csv -d /tmp/prof_sqA -- python3 scripts/pmc_driver.py pair || fail "pmc SQ pass A (see /tmp/prof_sqA.log)"
profiled 600 /tmp/prof_sqB -- rocprofv3 --kernel-trace --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_THREAD_CYCLES_VALU SQ_ACTIVE_INST_LDS \
    SQ_INSTS_SALU SQ_ACTIVE_INST_ANY SQ_INSTS_VMEM_RD SQ_INSTS_SMEM --output-format csv -d /tmp/prof_sqB -- python3 scripts/pmc_driver.py pair \
    || fail "pmc SQ pass B (see /tmp/prof_sqB.log)"
python3 scripts/pmc_summary.py /tmp/prof_sqA/*/*counter_collection.csv /tmp/prof_sqB/*/*counter_collection.csv \
    > "$OUT/${TAG}_pmc_sq_counters.csv" || fail "pmc_summary SQ"
need "$OUT/${TAG}_pmc_sq_counters.csv"
timeout -k 10 600 python3 bench.py --steps 2 --warmup 1 --streams 1 --no-cpu-baseline --kernel-table "$OUT/${TAG}_hip_event_table_1stream.csv" \
    > /tmp/one_stream.log 2>&1 || fail "one-stream bench"
need "$OUT/${TAG}_hip_event_table_1stream.csv"
timeout -k 10 900 python3 bench.py --full > /tmp/bench.out 2> /tmp/bench.err || fail "full bench (see /tmp/bench.err)"
tail -1 /tmp/bench.out > "$OUT/${TAG}_bench_line.json"
python3 -c "import json,sys; json.load(open(sys.argv[1]))" "$OUT/${TAG}_bench_line.json" || fail "bench line is not JSON (see /tmp/bench.err)"
cut -c1-260 "$OUT/${TAG}_bench_line.json"
cat "$OUT/${TAG}_concurrency.txt"
