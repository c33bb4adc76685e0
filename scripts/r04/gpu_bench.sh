#!/bin/bash
# Round-4 evidence: batch-affine microbenchmark, then the default bench line (N = 1).
set -o pipefail
OUT=${OUT:-out}  # where the logs and lines of this script go
mkdir -p $OUT/r04
timeout -k 10 120 scripts/ubench/batch_affine > $OUT/r04/batch_affine.log 2>&1 || exit $?
timeout -k 10 900 python -u bench.py --full > $OUT/r04/bench.json 2> $OUT/r04/bench.err || exit $?
