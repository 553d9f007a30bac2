# Round artifact set: full GPU test suite, default bench, rocprofv3 kernel stats + PMC passes of the same bench command,
# secondary benches.  usage (on the GPU box): bash tools/round_artifacts.sh <tag> [outdir]   -> <outdir>/<tag>/ (default artifacts/<tag>/)
set -e
TAG=${1:-r02_v1}
cd $GRAFT_REPO_ROOT
OUT=${2:-artifacts}/$TAG
mkdir -p $OUT
timeout -k 10 1000 python -m pytest tests -m gpu -x -q > $OUT/pytest_gpu.log 2>&1; tail -3 $OUT/pytest_gpu.log
timeout -k 10 400 python bench.py --full > $OUT/bench.json 2> $OUT/bench.err; tail -c 900 $OUT/bench.json
export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof -- python3 bench.py --steps 40 --warmup 5 --no-cpu-baseline --no-a8 --no-int8 --no-verify > $OUT/bench_under_rocprof.json 2> $OUT/prof.err
python tools/trace_step.py $OUT/prof > $OUT/step_timeline.txt 2>&1 || true
find $OUT/prof -name "*kernel_trace.csv" -delete
echo prof done
bash tools/pmc.sh $OUT/pmc > $OUT/pmc.log 2>&1; tail -30 $OUT/pmc.log
find $OUT/pmc -name "*.csv" -size +1M -delete
timeout -k 10 700 python tools/bench_ops.py all > $OUT/bench_ops.json 2> $OUT/bench_ops.err; wc -l $OUT/bench_ops.json
timeout -k 10 200 python tools/moe_stage_sweep.py 64 128 256 512 768 1024 1536 2048 3929 4096 8192 16384 2> /dev/null > $OUT/stage_sweep.json; wc -l $OUT/stage_sweep.json
