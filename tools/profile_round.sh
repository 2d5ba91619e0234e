# Run on the GPU box: the evidence set of one round for the bs64 bench step.
#   usage: bash tools/profile_round.sh r03     (writes $OUT/<tag>_*, default profile_out/;
#   copy what is to be judged into profiles/)
TAG=${1:-rXX}
export OUT=${OUT:-profile_out}   # bench_pmc.sh and prof_c2.sh write there as well
mkdir -p $OUT
export TMPDIR=/tmp
rm -rf $OUT/prof_$TAG
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_$TAG -- python3 bench.py --steps 5 --warmup 2 --no-cpu-baseline > $OUT/prof_$TAG.log 2>&1
python3 tools/step_breakdown.py $OUT/prof_$TAG > $OUT/${TAG}_bench_bs64_step_breakdown.txt 2>&1
cp $(ls $OUT/prof_$TAG/*/*_kernel_stats.csv | head -1) $OUT/${TAG}_bench_bs64_kernel_stats.csv
rm -rf $OUT/prof_$TAG
bash tools/bench_pmc.sh
cp $OUT/pmc_summary.csv $OUT/${TAG}_bench_bs64_pmc_summary.csv
cp $OUT/gemm128_hbm_traffic.json $OUT/${TAG}_gemm128_hbm_traffic.json
rm -rf $OUT/pmc
bash tools/prof_c2.sh $TAG > /dev/null 2>&1
for w in c2 c5 c5_hs512 defaults defaults_seg; do
  python3 bench.py --full --workload $w > $OUT/${TAG}_bench_$w.json 2> $OUT/${TAG}_bench_$w.err
done
python3 bench.py --full --workload c2 --batch 64 --no-cpu-baseline > $OUT/${TAG}_bench_c2_bs64.json 2> $OUT/${TAG}_bench_c2_bs64.err
python3 bench.py --full > $OUT/${TAG}_bench_line.json 2> $OUT/${TAG}_bench_line.err
tail -3 $OUT/${TAG}_bench_line.err
head -12 $OUT/${TAG}_bench_bs64_step_breakdown.txt
