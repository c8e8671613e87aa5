#!/bin/bash
# GPU-box check used during development: parity tests, a short full bench, a rocprofv3 kernel summary.
# usage: [OUT=dir] scripts/gpu_check.sh <tag> [bench args...]   (files go to $OUT, default out/)
set -o pipefail
TAG=${1:-dev}; shift
OUT=${OUT:-out}
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 400 python -m pytest tests -q -m gpu -p no:cacheprovider -x > $OUT/${TAG}_tests.log 2>&1 || { echo "tests failed"; tail -30 $OUT/${TAG}_tests.log; exit 1; }
tail -1 $OUT/${TAG}_tests.log
timeout -k 10 400 python bench.py --full --steps 2 --warmup 1 --no-cpu-baseline "$@" > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || { echo "bench failed"; tail -30 $OUT/${TAG}_bench.err; exit 1; }
timeout -k 10 500 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -o prof -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline "$@" > $OUT/${TAG}_prof.log 2>&1 || { echo "rocprof failed"; tail -30 $OUT/${TAG}_prof.log; exit 1; }
echo done
