#!/bin/bash
# The tile kernel built without the (never-run) next-tile L2-prefetch code (-DKW_PREFETCH=0,
# variants/nopf.so) against the r05 final build (variants/cur.so, lib 7fda9efd): parity subset on
# nopf, then kernel times per config, alternating, twice (the r04 gain depended on it).
set -u
cd "$(dirname "$0")/.."; OUT=${OUT:-$PWD/bench_out}; mkdir -p "$OUT"
KWGPU_LIB=$PWD/policy-server_amd/variants/nopf.so timeout -k 10 600 python -u -m pytest -q --timeout 300 --timeout-method thread -m gpu tests/test_parity_gpu.py tests/test_ctr_scan.py > $OUT/nopf_tests.log 2>&1; rc=$?
tail -2 $OUT/nopf_tests.log; [ $rc -eq 0 ] || exit $rc
run() {  # name lib args...
  local n=$1 lib=$2; shift 2
  KWGPU_LIB=$PWD/policy-server_amd/variants/$lib.so timeout -k 10 300 python bench.py --full "$@" --no-cpu-baseline --no-host-modes > $OUT/nopf_ab.json 2>/dev/null || exit $?
  python3 -c "import json;d=json.load(open('$OUT/nopf_ab.json'));print('[nopf_ab] $n $* kernel_ms=%.4f step_ms=%.4f' % (d['kernel_ms']['evaluate'], d['ms_per_step']))"
}
for rep in 1 2; do
  for a in "--config c4_64 --steps 20" "--config c5_mixed --steps 10" "--config c2_trusted --steps 20" "--config c3_group --steps 20" "--config c6_256 --steps 10"; do
    run cur cur $a
    run nopf nopf $a
  done
done
