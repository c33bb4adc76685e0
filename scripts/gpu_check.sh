#!/bin/bash
# GPU box check: parity tests, smoke, bench lines, rocprof kernel summary.
# Every GPU step has its own time limit; the script stops at the first failure.
# Usage: scripts/gpu_check.sh [OUT_DIR] (logs and lines; a fresh temporary directory by default)
set -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$(mktemp -d)}
mkdir -p $OUT
OUT=$(cd $OUT && pwd)
echo "output in $OUT"
cd $R
export TMPDIR=/tmp
step() { echo "== $1"; }
step pytest
timeout -k 10 900 python -u -m pytest tests -m gpu -x -q --timeout 300 --timeout-method thread > $OUT/pytest_gpu.log 2>&1; rc=$?
tail -3 $OUT/pytest_gpu.log
[ $rc -eq 0 ] || { grep -E "Error|assert|FAILED" $OUT/pytest_gpu.log | head -30; exit 1; }
step smoke
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" || exit 1
step bench-2p20
timeout -k 10 300 python bench.py --full --steps 20 --warmup 3 --cpu-budget 5 > $OUT/bench.json 2> $OUT/bench.err || { tail -20 $OUT/bench.err; exit 1; }
cat $OUT/bench.json
step bench-2p24
for P in default; do
  if [ $P = default ]; then unset PBF_NTT_PASSES; else export PBF_NTT_PASSES=$P; fi
  timeout -k 10 300 python bench.py --log-n 24 --batch 2 --steps 20 --warmup 3 > $OUT/bench24_$P.json 2>> $OUT/bench.err || exit 1
  python -c "import json;d=json.load(open('$OUT/bench24_$P.json'));print('$P', d['ms_per_step'], d['roofline']['achieved'], d['roofline']['frac'])"
done
unset PBF_NTT_PASSES
step rocprof
cd /tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof -o ntt2p20 --output-format csv -- python3 $R/bench.py --full --steps 20 --warmup 3 --no-cpu --no-traffic > $OUT/rocprof.log 2>&1 || { tail -20 $OUT/rocprof.log; exit 1; }
cd $R
find $OUT/prof -name "*stats*" | head
for f in $(find $OUT/prof -name "*kernel_stats.csv"); do head -8 $f; done
