# round-4 development iteration: GPU test tier (optionally a -k subset), then bench lines of config 3 and config 5
# usage: bash tools/gpurun/r4_iter.sh <tag> [pytest -k expression]
OUT=${OUT:-build/runs}; mkdir -p $OUT   # folder of this run's files
tag=$1; kexpr=$2
mkdir -p $OUT
if [ -n "$kexpr" ]; then
  python -m pytest tests -m gpu -x -q -k "$kexpr" 2>&1 | tail -15 > $OUT/${tag}_pytest.txt
else
  python -m pytest tests -m gpu -x -q 2>&1 | tail -15 > $OUT/${tag}_pytest.txt
fi
cat $OUT/${tag}_pytest.txt
timeout 900 python bench.py --full --no-e2e 2> $OUT/${tag}_c3.err > $OUT/${tag}_c3.json; cut -c1-1200 $OUT/${tag}_c3.json; tail -3 $OUT/${tag}_c3.err
timeout 900 python bench.py --full --workload config5 --no-e2e 2> $OUT/${tag}_c5.err > $OUT/${tag}_c5.json; cut -c1-600 $OUT/${tag}_c5.json; tail -3 $OUT/${tag}_c5.err
