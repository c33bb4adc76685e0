#!/bin/bash
# Round 3 final-tree evidence: full GPU test suite, smoke, default bench line, kernel stats
# of the bench's NTT and extra workloads.
set -o pipefail
OUT=${OUT:-out}  # where the logs and lines of this script go
cd "$GRAFT_REPO_ROOT" || exit 1
O=$OUT/${R03OUT:-r03g}; mkdir -p $O
export TMPDIR=/tmp
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread > $O/pytest_gpu.log 2>&1
rc=$?; tail -3 $O/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1 || { tail $O/smoke.log; exit 1; }
timeout -k 10 700 python -u bench.py --full > $O/bench.json 2> $O/bench.err || { tail -20 $O/bench.err; exit 1; }
cat $O/bench.json
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $O/prof -o k -- python bench.py --full --no-cpu --no-traffic --prove-log-n 20 > /dev/null 2>&1 || exit 1
echo done
