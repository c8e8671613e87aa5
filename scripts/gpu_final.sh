#!/bin/bash
# Round-end check: smoke(), the GenRecV1 and sports-shaped full bench lines (the DiffMM baby line and
# the parity suite come from scripts/gpu_round.sh).  Files go to $OUT (default out/).
set -o pipefail
TAG=${1:-fin}
OUT=${OUT:-out}
export TMPDIR=/tmp
mkdir -p "$OUT"
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > $OUT/${TAG}_smoke.log 2>&1 || { tail -30 $OUT/${TAG}_smoke.log; exit 1; }
tail -1 $OUT/${TAG}_smoke.log
timeout -k 10 500 python bench.py --full --model genrecv1 --steps 2 --warmup 1 > $OUT/${TAG}_genrec_bench.json 2> $OUT/${TAG}_genrec_bench.err || { tail -30 $OUT/${TAG}_genrec_bench.err; exit 1; }
cut -c1-300 $OUT/${TAG}_genrec_bench.json
timeout -k 10 500 python bench.py --full --shape sports --steps 2 --warmup 1 --no-cpu-baseline > $OUT/${TAG}_sports_bench.json 2> $OUT/${TAG}_sports_bench.err || { tail -30 $OUT/${TAG}_sports_bench.err; exit 1; }
cut -c1-300 $OUT/${TAG}_sports_bench.json
echo all-done
