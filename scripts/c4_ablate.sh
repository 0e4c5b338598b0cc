#!/bin/bash
# C4 ablations of the current build (KW_TILE_DEBUG bits, diagnostics only: verdicts wrong): kernel ms.
set -u
cd "$(dirname "$0")/.."; OUT=${OUT:-$PWD/bench_out}; mkdir -p "$OUT"
for rep in 1 2; do
  for dbg in 0 1 2 4 1024 2048 4096 8192 16384 65536; do
    KW_TILE_DEBUG=$dbg timeout -k 10 300 python bench.py --full --steps 20 --no-cpu-baseline --no-host-modes > $OUT/c4ab_$dbg.json 2> /dev/null || exit $?
    echo "[c4] debug=$dbg kernel_ms=$(python -c "import json;print('%.4f' % json.load(open('$OUT/c4ab_$dbg.json'))['kernel_ms']['evaluate'])")"
  done
done
