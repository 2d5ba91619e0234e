#!/bin/bash
# kernel-level profile of the bs8 (configs[1]) step:  bash tools/prof_c2.sh <tag>
TAG=${1:-rXX}
export TMPDIR=/tmp
OUT=${OUT:-profile_out}
mkdir -p $OUT
rm -rf $OUT/prof_c2_$TAG
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_c2_$TAG -- python3 bench.py --workload c2 --steps 5 --warmup 2 --no-cpu-baseline > $OUT/prof_c2_$TAG.log 2>&1
python3 tools/step_breakdown.py $OUT/prof_c2_$TAG > $OUT/${TAG}_bench_c2_step_breakdown.txt 2>&1
cp $(ls $OUT/prof_c2_$TAG/*/*_kernel_stats.csv | head -1) $OUT/${TAG}_bench_c2_kernel_stats.csv
rm -rf $OUT/prof_c2_$TAG
head -40 $OUT/${TAG}_bench_c2_step_breakdown.txt
