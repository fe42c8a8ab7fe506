# Round profiles: kernel-trace summary of a training-step run and of the bench command, PMC passes (MFMA utilisation, HBM traffic).
# Run on the GPU box from the repo root:  bash tools/collect_profiles.sh r02
R=${1:-r06}
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
OUT=${OUT:-bench_out}; mkdir -p $OUT
export HD_COMMIT=${HD_COMMIT:-unknown}
STEPS=20 rocprofv3 --kernel-trace --stats -d $OUT/prof_step --output-format csv -- python3 tools/bench_step.py > $OUT/prof_step.log 2>&1
rocprofv3 --kernel-trace --stats -d $OUT/prof_bench --output-format csv -- python3 bench.py --steps 10 --warmup 3 --full --no-cpu-baseline > $OUT/prof_bench.log 2>&1
STEPS=3 rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_INST_LDS SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAIT_ANY SQ_WAIT_INST_ANY --kernel-trace -d $OUT/pmc_mfma --output-format csv -- python3 tools/bench_step.py > $OUT/pmc_mfma.log 2>&1
STEPS=3 rocprofv3 --pmc GRBM_GUI_ACTIVE SQ_INSTS_MFMA SQ_ACTIVE_INST_ANY --kernel-trace -d $OUT/pmc_gui --output-format csv -- python3 tools/bench_step.py > $OUT/pmc_gui.log 2>&1
STEPS=3 rocprofv3 --pmc FETCH_SIZE --kernel-trace -d $OUT/pmc_fetch --output-format csv -- python3 tools/bench_step.py > $OUT/pmc_fetch.log 2>&1
STEPS=3 rocprofv3 --pmc WRITE_SIZE --kernel-trace -d $OUT/pmc_write --output-format csv -- python3 tools/bench_step.py > $OUT/pmc_write.log 2>&1
python3 tools/pmc_mfma.py $OUT/pmc_mfma $OUT/pmc_gui $OUT/${R}_conv_mfma_util.json > /dev/null
F=$(ls $OUT/pmc_fetch/*/*counter_collection.csv | head -1); W=$(ls $OUT/pmc_write/*/*counter_collection.csv | head -1)
python3 tools/pmc_traffic.py $F $W conv_igemm_kernel,gemm_w8_kernel,conv3x3_small_kernel,conv3x3_w8_kernel,conv3x3_m160_kernel,conv3x3_c64_kernel,conv7x7s2_stem_kernel,conv3x3_c32to128_kernel,conv3x3_cat128to32_kernel $OUT/${R}_conv_traffic.json > /dev/null
STEPS=12 rocprofv3 --kernel-trace -d $OUT/trace_ss --output-format csv -- python3 tools/bench_step.py > $OUT/trace_ss.log 2>&1
python3 tools/trace_gaps.py $(ls $OUT/trace_ss/*/*kernel_trace.csv | head -1) 0.5 --table --aten > $OUT/${R}_steady_state.txt 2>&1
rm -rf $OUT/trace_ss
python3 tools/conv_table.py all > $OUT/${R}_conv_table.txt 2>&1
# the bench line quotes the PMC summaries from profiles/: put this run's there first (else the line marks them stale)
cp $OUT/${R}_conv_mfma_util.json $OUT/${R}_conv_traffic.json profiles/
python3 bench.py --full > $OUT/${R}_bench_line.json 2> $OUT/${R}_bench_line.err
cp $(ls $OUT/prof_step/*/*kernel_stats.csv | head -1) $OUT/${R}_train_step_kernel_stats.csv
cp $(ls $OUT/prof_bench/*/*kernel_stats.csv | head -1) $OUT/${R}_bench_kernel_stats.csv
rm -rf $OUT/prof_step $OUT/prof_bench $OUT/pmc_mfma $OUT/pmc_gui $OUT/pmc_fetch $OUT/pmc_write
tail -2 $OUT/prof_step.log; tail -c 600 $OUT/prof_bench.log; cat $OUT/${R}_conv_mfma_util.json | head -40
