#!/bin/bash
# BASELINE.md's results table: the five BASELINE.json configurations on one GPU, each with the CPU baselines
# B1 (one thread) and B2 (all cores) timed in the same run on the same box.  Run from the repository root on the GPU box:
#   scripts/baseline_table.sh r02        -> $RESULTS_DIR/r02_table_cfg{1..5}.json (results/ by default)
# scripts/fill_baseline_table.py r02 then writes the table into BASELINE.md and copies the lines to profiles/.
# Each row is one `bench.py --full` run under a time limit of its own; the first row that fails, crashes or runs out of
# time ends the script (nothing more starts on the GPU after it).
set -u
TAG=${1:-round}
R=${GRAFT_REPO_ROOT:-$(pwd)}
cd "$R"
OUT=${RESULTS_DIR:-results}
mkdir -p "$OUT"
run() {   # run <cfg> <bench args...>       (ONLY="5 1": just those rows)
  local cfg=$1; shift
  if [ -n "${ONLY:-}" ] && [[ " $ONLY " != *" $cfg "* ]]; then return; fi
  local line="$OUT/${TAG}_table_cfg$cfg.json" err="/tmp/table_cfg$cfg.err"
  timeout -k 10 1500 python3 bench.py --full "$@" > "/tmp/table_cfg$cfg.out" 2> "$err"
  local rc=$?
  if [ $rc -ne 0 ]; then echo "cfg$cfg failed (exit $rc), stopping:"; tail -5 "$err"; exit 1; fi
  tail -1 "/tmp/table_cfg$cfg.out" > "$line"
  python3 -c "import json, sys; d=json.load(open(sys.argv[1])); print('cfg$cfg', d['value'], (d.get('cpu_baseline') or {}).get('value'), (d.get('cpu_baseline_all_cores') or {}).get('value'), (d.get('parity_check') or {}).get('ok'), d.get('icp_iterations_histogram'), d.get('gt_error', {}).get('recovered_within_0.5'))" "$line" \
    || { echo "cfg$cfg: no bench line, stopping:"; tail -5 "$err"; exit 1; }
}
# (steps of 4 and 14 ms: enough of them that one late host thread does not show -- five steps of row 2 gave 358 ... 435)
run 1 --maps 2 --points 10000 --steps 30 --warmup 3
run 2 --maps 4 --points 200000 --steps 15 --warmup 3
run 3
run 5 --maps 64 --points 50000 --steps 5 --warmup 1
run 4 --maps 8 --points 2000000 --descriptor SHOT --steps 2 --warmup 1
# configs[3] as SURVEY 8d words it: dense indoor -- 30 m windows, resolution 0.05 (the radii keep the reference's defaults)
run 4indoor --maps 8 --points 2000000 --descriptor SHOT --window 30 --resolution 0.05 --steps 1 --warmup 1
# the 'lattice' scene family with enough SAC-IA hypotheses for the algorithm to find the basin: ICP iterates, gt_error is small
run 2lattice --maps 4 --points 200000 --scenes lattice --overlap-step 0.25 --sac-iterations 20000 --steps 3 --warmup 1
# the headline size on the 'lattice' family with 20 000 hypotheses: poses worth refining, so "Mpoints/s (ICP)" is measured on an ICP
# that iterates (CPU baselines + parity_check on a sample of two maps and ONE pair: a pair with 20 000 hypotheses is ~ 50 s of one core)
# (four warm-up steps: a step moves 1.26 GB of hypothesis errors per pair through the memory pools, which keep growing through the
# first three -- with two warm-up steps the row scattered between 131 and 188 map-pairs/s, with four it is 186 - 187)
run 3lattice --maps 16 --points 500000 --scenes lattice --overlap-step 0.25 --sac-iterations 20000 --steps 3 --warmup 4
