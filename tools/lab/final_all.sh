# usage: bash tools/lab/final_all.sh OUT_DIR  -> the round's final artefacts in OUT_DIR
O=$(mkdir -p "${1:?usage: bash tools/lab/final_all.sh OUT_DIR}" && cd "$1" && pwd)
bash tools/final_measurements.sh $O > $O/final.log 2>&1
bash tools/config_table.sh > $O/config_table.txt 2>&1
timeout -k 10 500 python tools/hot_replay.py --roofline 30 > $O/hot_replay.txt 2>&1
timeout -k 10 300 python tools/sink_census.py 40 > $O/sink_census.txt 2>&1
bash tools/profile_step.sh r04_z > /dev/null 2>&1
cat $O/bench_line.json; cat $O/config_table.txt; head -5 $O/step_kernels.md
