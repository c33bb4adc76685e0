#!/bin/bash
# rocprofv3 kernel statistics of the default bench (no PMC children under the profiler)
set -o pipefail
OUT=${OUT:-out}  # where the logs and lines of this script go
mkdir -p $OUT/r05
export TMPDIR=/tmp
TAG=${1:-r05z}
start=$(date +%s)
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d $OUT/r05/bprof_$TAG -o b -- python bench.py --full --no-traffic > $OUT/r05/bench_prof_$TAG.json 2> $OUT/r05/bench_prof_$TAG.err &
pid=$!
while kill -0 $pid 2>/dev/null; do sleep 50; echo "profiled bench running $(( $(date +%s) - start )) s"; done
wait $pid || { tail -20 $OUT/r05/bench_prof_$TAG.err; exit 1; }
f=$(find $OUT/r05/bprof_$TAG -name "*.db" | head -1)
python scripts/kstats.py "$f" 60 > $OUT/r05/bench_kstats_$TAG.txt
head -30 $OUT/r05/bench_kstats_$TAG.txt
