#!/bin/bash
# Full round check: parity tests + bench + rocprof (gpu_check.sh), the default full bench (with the
# CPU-baseline leg), and a 2-rank gloo data-parallel rehearsal on the single GPU.
# Files go to $OUT (default out/).
set -o pipefail
TAG=${1:-dev}
export OUT=${OUT:-out}
export TMPDIR=/tmp
bash scripts/gpu_check.sh "$TAG" || exit 1
timeout -k 10 600 python bench.py --full > $OUT/${TAG}_bench_default.json 2> $OUT/${TAG}_bench_default.err || { echo "default bench failed"; tail -30 $OUT/${TAG}_bench_default.err; exit 1; }
cat $OUT/${TAG}_bench_default.json
GMR_DIST_BACKEND=gloo timeout -k 10 600 python -m torch.distributed.run --nnodes=1 --nproc-per-node 2 --master-addr 127.0.0.1 --master-port 29511 bench.py --full --gpus 2 --steps 1 --warmup 1 --no-cpu-baseline > $OUT/${TAG}_dp2.json 2> $OUT/${TAG}_dp2.err || { echo "dp2 failed"; tail -30 $OUT/${TAG}_dp2.err; exit 1; }
cat $OUT/${TAG}_dp2.json
echo all-done
