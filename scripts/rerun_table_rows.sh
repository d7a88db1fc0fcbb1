#!/bin/bash
# Re-measures single rows of BASELINE.md's table after a change that only concerns them (same commands as
# scripts/baseline_table.sh):   scripts/rerun_table_rows.sh r03 4 4indoor
# Each row runs once under a time limit; the first that fails, crashes or runs out of time ends the script.
cd "${GRAFT_REPO_ROOT:-$(pwd)}"
TAG=$1; shift
OUT=${RESULTS_DIR:-results}
mkdir -p "$OUT"
run() {
  local cfg=$1; shift
  local line="$OUT/${TAG}_table_cfg$cfg.json" err="/tmp/table_cfg$cfg.err"
  timeout -k 10 1500 python3 bench.py "$@" > "/tmp/table_cfg$cfg.out" 2> "$err"
  local rc=$?
  if [ $rc -ne 0 ]; then echo "cfg$cfg failed (exit $rc), stopping:"; tail -5 "$err"; exit 1; fi
  tail -1 "/tmp/table_cfg$cfg.out" > "$line"
  python3 -c "import json, sys; d=json.load(open(sys.argv[1])); print('cfg$cfg', d['value'], d['cpu_baseline']['value'], d['cpu_baseline_all_cores']['value'], (d.get('parity_check') or {}).get('ok'))" "$line" \
    || { echo "cfg$cfg: no bench line, stopping:"; tail -5 "$err"; exit 1; }
}
for row in "$@"; do
  case $row in
    1) run 1 --full --maps 2 --points 10000 --steps 10 --warmup 2 ;;
    2) run 2 --full --maps 4 --points 200000 --steps 5 --warmup 1 ;;
    3) run 3 --full ;;
    5) run 5 --full --maps 64 --points 50000 --steps 2 --warmup 1 ;;
    4) run 4 --full --maps 8 --points 2000000 --descriptor SHOT --steps 2 --warmup 1 ;;
    4indoor) run 4indoor --full --maps 8 --points 2000000 --descriptor SHOT --window 30 --resolution 0.05 --steps 1 --warmup 1 ;;
    2lattice) run 2lattice --full --maps 4 --points 200000 --scenes lattice --overlap-step 0.25 --sac-iterations 20000 --steps 3 --warmup 1 ;;
  esac
done
