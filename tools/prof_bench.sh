# rocprofv3 kernel trace + stats of the full bench (writes under <out dir>/prof_bench_<tag>)
#   usage: bash tools/prof_bench.sh <tag> <out dir>
R=$(cd "$(dirname "$0")/.." && pwd)
TAG=${1:-r1}
O=$(realpath -m "${2:?usage: bash tools/prof_bench.sh <tag> <out dir>}")/prof_bench_$TAG
cd /tmp && export TMPDIR=/tmp
rm -rf $O; mkdir -p $(dirname $O)
rocprofv3 --kernel-trace --stats --output-format csv -d $O -o run -- python $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > $O.log 2>&1
tail -1 $O.log | cut -c1-200
python $R/tools/layer_report.py $O/run_kernel_trace.csv | tail -12
head -40 $O/run_kernel_stats.csv | cut -c1-150
