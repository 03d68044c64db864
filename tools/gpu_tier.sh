#!/bin/bash
# the full GPU tier (no -x: every failure is listed), then the default bench command with every section (--full):
#   OUT=<dir> tools/gpu_tier.sh <tag>      (outputs: <dir>/<tag>_*, default out/)
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
TAG=${1:-r06}
OUT=${OUT:-$R/out}   # where the outputs go
cd $R; mkdir -p $OUT
( time python -m pytest tests -m gpu -q > $OUT/${TAG}_pytest_gpu.txt 2>&1 ) 2>&1 | grep real
tail -12 $OUT/${TAG}_pytest_gpu.txt
( time python bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/${TAG}_bench_default.txt 2> $OUT/${TAG}_bench_default.err ) 2>&1 | grep real
tail -1 $OUT/${TAG}_bench_default.txt | wc -c
tail -1 $OUT/${TAG}_bench_default.txt | python -c "import sys, json; r = json.loads(sys.stdin.read()); print(r['value'], r['roofline']['frac'], json.dumps(r['summary']))"
cp bench_sections.json $OUT/${TAG}_bench_sections.json 2>/dev/null
tail -3 $OUT/${TAG}_bench_default.err
