# usage: bash tools/run_round_profiles.sh OUT_DIR   (bench lines, kernel traces and their tables are written under OUT_DIR)
set -x
REPO=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "${1:?usage: run_round_profiles.sh OUT_DIR}" && cd "$1" && pwd)
cd $REPO
python bench.py --full > $OUT/bench_v9.json 2> $OUT/bench_v9.err
python bench.py --full --workload posegraph --steps 10 --warmup 2 > $OUT/bench_pg4_v5.json 2> $OUT/bench_pg4_v5.err
python bench.py --full --workload posegraph --six-dof --steps 10 --warmup 2 > $OUT/bench_pg6_v5.json 2> $OUT/bench_pg6_v5.err
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats -d $OUT/prof_v9 -o b -- python $REPO/bench.py --full --no-cpu-baseline > $OUT/prof_v9.log 2>&1
rocprofv3 --kernel-trace --stats -d $OUT/prof_pg4_v5 -o b -- python $REPO/bench.py --workload posegraph --steps 10 --warmup 2 --no-cpu-baseline > $OUT/prof_pg4_v5.log 2>&1
rocprofv3 --kernel-trace --stats -d $OUT/prof_pg6_v5 -o b -- python $REPO/bench.py --workload posegraph --six-dof --steps 10 --warmup 2 --no-cpu-baseline > $OUT/prof_pg6_v5.log 2>&1
rocprofv3 --kernel-trace --stats -d $OUT/prof_slide -o b -- python $REPO/tools/margtime.py --rig-v2 > $OUT/prof_slide.log 2>&1
cd $REPO
for d in prof_slide prof_v9 prof_pg4_v5 prof_pg6_v5; do python tools/prof_summary.py $OUT/$d/b_results.db > $OUT/$d.txt 2>&1; done
tail -c 600 $OUT/bench_v9.json; echo; tail -c 1500 $OUT/bench_pg4_v5.json; echo; tail -c 800 $OUT/bench_pg6_v5.json
