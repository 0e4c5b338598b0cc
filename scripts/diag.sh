#!/bin/bash
# Diagnostics of the tile kernel on one box: phase clocks (KW_TILE_DEBUG 512), then the kernel time
# with phases / sub-phases ablated (KW_TILE_DEBUG bits, knobs.hpp / plan.cpp), all at C4 unless CFG is set.
set -u
cd "$(dirname "$0")/.."; OUT=${OUT:-$PWD/bench_out}; mkdir -p "$OUT"
TAG=${1:-diag}
CFG=${CFG:-c4_64}
KW_TILE_DEBUG=768 timeout -k 10 300 python bench.py --full --config $CFG --steps 2 --warmup 1 --no-cpu-baseline --no-host-modes > /dev/null 2> $OUT/${TAG}_phase.err || exit $?
grep -E "kw phase|kw tile\] launch" $OUT/${TAG}_phase.err | head -8
for d in ${DEBUGS:-0 1 2 4 6 7 1024 2048 4096}; do
  KW_TILE_DEBUG=$d timeout -k 10 300 python bench.py --full --config $CFG --steps 10 --warmup 2 --no-cpu-baseline --no-host-modes > $OUT/${TAG}_d$d.json 2>$OUT/${TAG}_d$d.err
  rc=$?; echo "debug=$d rc=$rc $(python -c "import json;d=json.load(open('$OUT/${TAG}_d$d.json'));print('%.4f' % d['kernel_ms']['evaluate'])" 2>/dev/null)"
  if [ $rc -ne 0 ]; then exit $rc; fi
done
