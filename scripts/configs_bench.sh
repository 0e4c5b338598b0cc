#!/bin/bash
# One bench line + one rocprofv3 kernel-trace summary per BASELINE config:
#   $OUT/${TAG}_<config>.json and $OUT/${TAG}_<config>_prof/run_kernel_stats.csv
# Every GPU step has its own time limit; a fault / abort / timeout stops the script.
set -u
cd "${GRAFT_REPO_ROOT:-/root/repo}"
REPO=$PWD; OUT=${OUT:-$PWD/bench_out}; mkdir -p "$OUT"
mkdir -p "$OUT"
TAG=${1:-cfg}
CFGS=${CFGS:-"c2_trusted c3_group c5_mixed c6_256"}
stop() { local rc=$1 what=$2; echo "[configs] $what exit $rc"; if [ "$rc" -ne 0 ]; then exit "$rc"; fi; }
for c in $CFGS; do
  timeout -k 10 400 python bench.py --full --config $c --no-host-modes > $OUT/${TAG}_$c.json 2> $OUT/${TAG}_$c.err
  stop $? "bench $c"
  tail -c 600 $OUT/${TAG}_$c.json
  (cd /tmp && export TMPDIR=/tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$OUT/${TAG}_${c}_prof" \
     -o run --output-format csv -- python3 "$REPO/bench.py" --full --config $c --steps 10 --no-cpu-baseline --no-host-modes \
     > "$OUT/${TAG}_${c}_prof.log" 2>&1)
  stop $? "prof $c"
done
echo "[configs] done"
