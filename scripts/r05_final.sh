#!/bin/bash
# r05 closing record, part A: the GPU suite, smoke(), the default bench line (C4: HBM-resident value,
# roofline, CPU baseline, timing modes), then every other BASELINE config's line.
set -u
cd "$(dirname "$0")/.."; OUT=${OUT:-$PWD/bench_out}; mkdir -p "$OUT"
TAG=${1:-r05f}
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q -p no:cacheprovider --timeout 500 --timeout-method thread > $OUT/${TAG}_gpu_tests.log 2>&1
rc=$?; tail -1 $OUT/${TAG}_gpu_tests.log; if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1 || exit $?
echo "[final] smoke ok"
timeout -k 10 600 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || exit $?
tail -c 300 $OUT/${TAG}_bench.json
for cfg in c2_trusted c3_group c5_mixed c6_256 c1_namespace; do
  timeout -k 10 400 python bench.py --full --config $cfg --steps 20 --warmup 3 --no-cpu-baseline > $OUT/${TAG}_${cfg}_bench.json 2> $OUT/${TAG}_${cfg}_bench.err || exit $?
  python3 -c "import json;d=json.load(open('$OUT/${TAG}_${cfg}_bench.json'));print('[final] $cfg', round(d['value']/1e6,1), 'M req/s kernel', round(d['kernel_ms']['evaluate'],4), 'ms frac', round(d['roofline']['frac'],4))"
done
