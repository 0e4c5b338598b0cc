#!/bin/bash
# r04 closing record after the bulk-path changes: the GPU suite, smoke(), then the default bench
# line (HBM-resident value, roofline, CPU baseline and the timing modes).
set -u
cd "$(dirname "$0")/.."; OUT=${OUT:-$PWD/bench_out}; mkdir -p "$OUT"
TAG=${1:-r04z}
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/${TAG}_gpu_tests.log 2>&1
rc=$?; tail -1 $OUT/${TAG}_gpu_tests.log; if [ $rc -ne 0 ]; then exit $rc; fi
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1 || exit $?
echo "[final] smoke ok"
timeout -k 10 600 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || exit $?
tail -c 400 $OUT/${TAG}_bench.json
