#!/bin/bash
# Everything a profiles/<TAG>_* checkpoint holds for the Kuka step, in one run on the GPU box (from the repo root):
#   kernel stats + timeline of the default bench under rocprofv3, the default bench, the driver-style short bench (all three
#   with --full, as the checkpoint records roofline and CPU baseline), one PMC pass for MFMA-busy / LDS conflicts, the two
#   HBM-traffic PMC passes.  Output under $OUT (default profiling_out/).
# usage:  bash tools/checkpoint_profiles.sh r03_mid   then   python tools/collect_profiles.py r03_mid
TAG=$1
R=$PWD
OUT=$(realpath -m "${OUT:-profiling_out}")
mkdir -p $OUT && rm -rf $OUT/prof_$TAG $OUT/pmc_$TAG && (cd "${TMPDIR:-/tmp}" &&
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -- python3 $R/bench.py --full --no-cpu-baseline > $OUT/bench_prof_$TAG.log 2>&1 &&
  timeout -k 10 300 rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_LDS_BANK_CONFLICT SQ_ACTIVE_INST_LDS --output-format csv -d $OUT/pmc_$TAG -- python3 $R/bench.py --steps 6 --warmup 3 --no-cpu-baseline --no-roofline --no-graph --streams 67 > $OUT/pmc_$TAG.log 2>&1) &&
  OUT=$OUT bash tools/pmc_traffic.sh $TAG > $OUT/traffic_$TAG.log 2>&1 &&
  timeout -k 10 400 python bench.py --full > $OUT/bench_$TAG.log 2>&1 &&
  timeout -k 10 400 python bench.py --full --steps 20 --warmup 5 > $OUT/bench20_$TAG.log 2>&1 &&
  tail -1 $OUT/bench20_$TAG.log | cut -c1-400
