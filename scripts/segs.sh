#!/bin/bash
# Phase and per-wave segment clocks of the timing instantiation (KW_TILE_DEBUG=512) per config:
# where a tile's critical path goes (P1 / P2 item segments, each phase's busy time and barrier wait).
set -u
cd "$(dirname "$0")/.."; OUT=${OUT:-$PWD/bench_out}; mkdir -p "$OUT"
TAG=${1:-seg}
for CFG in ${CFGS:-c4_64 c3_group c2_trusted}; do
  KW_TILE_DEBUG=512 timeout -k 10 300 python bench.py --full --config $CFG --steps 2 --warmup 1 --no-cpu-baseline --no-host-modes > /dev/null 2> $OUT/${TAG}_${CFG}.err || exit $?
  echo "[$CFG] $(grep -E 'kw phase' $OUT/${TAG}_${CFG}.err | tail -1)"
  echo "[$CFG] $(grep -E 'kw seg' $OUT/${TAG}_${CFG}.err | tail -1)"
done
echo "[seg] done"
