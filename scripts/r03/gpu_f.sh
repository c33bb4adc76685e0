#!/bin/bash
# Round 3 (session 2): full GPU test suite, smoke, default bench line, kernel stats of the bench.
set -o pipefail
OUT=${OUT:-out}  # where the logs and lines of this script go
cd "$GRAFT_REPO_ROOT" || exit 1
O=$OUT/r03f; mkdir -p $O
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $O/pytest_gpu.log 2>&1
rc=$?; tail -3 $O/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 || exit 1
timeout -k 10 600 python -u bench.py --full > $O/bench.json 2> $O/bench.err || { tail -20 $O/bench.err; exit 1; }
cat $O/bench.json
