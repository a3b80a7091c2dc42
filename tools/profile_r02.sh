#!/bin/bash
# Four rocprofv3 passes of the headline bench (counters in their own passes) -> gpurun_out/prof_r02/{trace,sq,fetch,write}.
# Run on the GPU box from the repo root:  bash tools/profile_r02.sh [extra bench flags]
set -o pipefail
ROOT=$(pwd); OUT=$ROOT/gpurun_out/prof_r02; rm -rf $OUT; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
B="python3 $ROOT/bench.py --full --steps 1 --warmup 1 --cpu-outfits 0 $@"
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace -- $B > $OUT/trace.log 2>&1 || { tail -5 $OUT/trace.log; exit 1; }
rocprofv3 --kernel-trace --output-format csv --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE SQ_INSTS_VALU_MFMA_MOPS_F16 SQ_INSTS_VALU_MFMA_MOPS_BF16 SQ_BUSY_CYCLES -d $OUT/sq -- $B > $OUT/sq.log 2>&1 || { tail -5 $OUT/sq.log; exit 1; }
rocprofv3 --kernel-trace --output-format csv --pmc FETCH_SIZE -d $OUT/fetch -- $B > $OUT/fetch.log 2>&1 || { tail -5 $OUT/fetch.log; exit 1; }
rocprofv3 --kernel-trace --output-format csv --pmc WRITE_SIZE -d $OUT/write -- $B > $OUT/write.log 2>&1 || { tail -5 $OUT/write.log; exit 1; }
cd $ROOT
python3 tools/pmc_mfma_util.py $OUT > $OUT/mfma_util.json && cp $(find $OUT/trace -name "*kernel_stats.csv" | head -1) $OUT/kernel_stats.csv
# keep the merge-back small: drop the raw per-dispatch csv files
find $OUT -name "*counter_collection.csv" -delete; find $OUT -name "*kernel_trace.csv" -delete; find $OUT -name "*agent_info.csv" -delete
ls -la $OUT; head -c 1500 $OUT/mfma_util.json
