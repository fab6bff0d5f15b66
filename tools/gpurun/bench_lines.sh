# full bench lines (with cpu_baseline) of every workload on one box. usage: bash tools/gpurun/bench_lines.sh <tag>
OUT=${OUT:-build/runs}; mkdir -p $OUT   # folder of this run's files
tag=${1:-bl}
timeout 900 python bench.py --full --steps 20 --warmup 5 2> $OUT/${tag}_bench_config3.err > $OUT/${tag}_bench_config3.json; cut -c1-200 $OUT/${tag}_bench_config3.json
for wl in config5 config2 config3k64; do
  timeout 900 python bench.py --full --workload $wl --no-e2e 2> $OUT/${tag}_bench_$wl.err > $OUT/${tag}_bench_$wl.json; cut -c1-200 $OUT/${tag}_bench_$wl.json
done
