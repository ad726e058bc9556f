# usage: bash tools/final_measurements.sh OUT_DIR  -> the --full bench line, kernel trace + stats and MFMA counters in OUT_DIR
R=$PWD
O=$(mkdir -p "${1:?usage: bash tools/final_measurements.sh OUT_DIR}" && cd "$1" && pwd)
# (the rocprofv3 output directories are hundreds of MB: always removed, whatever fails in between)
trap 'rm -rf $O/trace $O/pmc' EXIT
timeout -k 10 500 python bench.py --full > $O/bench_line.json 2> $O/bench_stderr.log
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $O/trace -- python $R/bench.py --steps 10 --warmup 5 --no-cpu-baseline --no-roofline --no-host-fed > $O/trace.log 2>&1
cd $R
python tools/trace_steps.py $O/trace/*/*kernel_trace.csv --steps 10 --top 60 --md $O/step_kernels.md > $O/trace_steps.log 2>&1
cp $O/trace/*/*kernel_stats.csv $O/kernel_stats_whole_run.csv
rm -rf $O/trace
cd /tmp
timeout -k 10 400 rocprofv3 --pmc SQ_INSTS_VALU_MFMA_MOPS_BF16 SQ_INSTS_VALU_MFMA_MOPS_F32 SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE --kernel-trace --output-format csv -d $O/pmc -- python $R/bench.py --steps 4 --warmup 3 --no-cpu-baseline --no-roofline --no-host-fed > $O/pmc.log 2>&1
cd $R
python tools/pmc_mfma.py $O/pmc/*/*counter_collection.csv --steps 3 --md $O/pmc_mfma.md > $O/pmc_mfma.log 2>&1
rm -rf $O/pmc
