#!/bin/bash
# Memory-side traffic and MFMA busy cycles per kernel class of one bench workload, on the current
# build.  Three separate rocprofv3 --pmc passes (FETCH_SIZE and WRITE_SIZE do not fit one pass on
# gfx950; MFMA busy + GRBM active in a third), each over the same short serial bench command, then
# scripts/pmc_summary.py writes $OUT/<tag>_pmc_<model>.json (OUT defaults to out/) stamped with the
# library's SHA-256 (bench.py uses a summary only when that hash equals the loaded library's).
# usage: [OUT=dir] scripts/pmc_collect.sh <tag> <model> [extra bench args]
set -o pipefail
TAG=${1:-dev}; MODEL=${2:-diffmm}; shift 2
OUT=${OUT:-out}
export TMPDIR=/tmp
mkdir -p "$OUT"
CMD="bench.py --full --model $MODEL --steps 1 --warmup 1 --no-cpu-baseline --no-probe --no-legs --eval-passes 1 $*"
export GMR_SERIAL=1
timeout -k 10 -s KILL 300 rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/${TAG}_pmcf_${MODEL} -o pmc -- python3 $CMD > $OUT/${TAG}_pmcf_${MODEL}.log 2>&1 || { echo "fetch pass failed"; tail -20 $OUT/${TAG}_pmcf_${MODEL}.log; exit 1; }
timeout -k 10 -s KILL 300 rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/${TAG}_pmcw_${MODEL} -o pmc -- python3 $CMD > $OUT/${TAG}_pmcw_${MODEL}.log 2>&1 || { echo "write pass failed"; tail -20 $OUT/${TAG}_pmcw_${MODEL}.log; exit 1; }
timeout -k 10 -s KILL 300 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE --output-format csv -d $OUT/${TAG}_pmcm_${MODEL} -o pmc -- python3 $CMD > $OUT/${TAG}_pmcm_${MODEL}.log 2>&1 || { echo "mfma pass failed"; tail -20 $OUT/${TAG}_pmcm_${MODEL}.log; exit 1; }
python3 scripts/pmc_summary.py $OUT/${TAG}_pmcf_${MODEL}/pmc_counter_collection.csv $OUT/${TAG}_pmcw_${MODEL}/pmc_counter_collection.csv $OUT/${TAG}_pmcm_${MODEL}/pmc_counter_collection.csv "$CMD" > $OUT/${TAG}_pmc_${MODEL}.json && cat $OUT/${TAG}_pmc_${MODEL}.json
