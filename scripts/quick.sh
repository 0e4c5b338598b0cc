#!/bin/bash
# Quick GPU check: parity tests, a short bench and one PMC pass (LDS / wave-state counters).
set -u
cd "$(dirname "$0")/.."; REPO=$PWD; OUT=${OUT:-$PWD/bench_out}; mkdir -p "$OUT"
TAG=${1:-q}
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q -p no:cacheprovider --timeout 120 --timeout-method thread > $OUT/${TAG}_tests.log 2>&1
rc=$?; echo "tests rc=$rc"; tail -2 $OUT/${TAG}_tests.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full --steps 10 --warmup 2 --no-cpu-baseline > $OUT/${TAG}_bench.json 2>/dev/null || exit $?
python -c "import json;d=json.load(open('$OUT/${TAG}_bench.json'));print('bench', round(d['value']/1e6,1), 'Mreq/s', d['kernel_ms'])"
KW_TILE_DEBUG=256 timeout -k 10 300 python bench.py --full --steps 1 --warmup 0 --no-cpu-baseline > /dev/null 2> $OUT/${TAG}_tile.log || exit $?
grep -m10 "kw tile" $OUT/${TAG}_tile.log || true
[ -n "${NOPMC:-}" ] && exit 0
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_INSTS_LDS SQ_INSTS_VALU SQ_INSTS_SALU SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_ACTIVE_INST_ANY --kernel-trace -d "$OUT/${TAG}_pmc" -o run --output-format csv -- python3 "$REPO/bench.py" --full --steps 3 --warmup 1 --no-cpu-baseline > "$OUT/${TAG}_pmc.log" 2>&1 || exit $?
cd "$REPO" && python3 scripts/pmc_summary.py $OUT/${TAG}_pmc
