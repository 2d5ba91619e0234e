# Run on the GPU box: hardware-counter passes over one bench step (separate rocprofv3 --pmc runs, no tracing domains).
#   pass f: FETCH_SIZE   pass w: WRITE_SIZE   pass s: SQ / GRBM cycle counters
# Summaries: python3 tools/pmc_summary.py $OUT/pmc -> profiles/
export TMPDIR=/tmp
OUT=${OUT:-profile_out}
mkdir -p $OUT
rm -rf $OUT/pmc
rocprofv3 --pmc FETCH_SIZE --output-format csv -d $OUT/pmc/f -- python3 bench.py --steps 1 --warmup 1 --no-cpu-baseline > $OUT/pmc_f.log 2>&1
rocprofv3 --pmc WRITE_SIZE --output-format csv -d $OUT/pmc/w -- python3 bench.py --steps 1 --warmup 1 --no-cpu-baseline > $OUT/pmc_w.log 2>&1
rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY GRBM_GUI_ACTIVE --output-format csv -d $OUT/pmc/s -- python3 bench.py --steps 1 --warmup 1 --no-cpu-baseline > $OUT/pmc_s.log 2>&1
python3 tools/pmc_summary.py $OUT/pmc $OUT/pmc_summary.csv $OUT/gemm128_hbm_traffic.json $OUT/gemm128_traffic_by_launch.csv
