#!/bin/bash
# One GPU check: smoke, GPU parity tests, bench (--full), rocprof kernel stats.  bash tools/gpu_check.sh [TAG [OUTDIR]]
# (outputs in OUTDIR, default out/TAG)
TAG=${1:-r02}
ROOT=$PWD
OUT=$(realpath -m ${2:-out/$TAG})
mkdir -p $OUT
export TMPDIR=/tmp
echo "== smoke"; timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | tail -4
echo "== pytest gpu"; timeout 1800 python -m pytest tests -m gpu -x -q 2>&1 | tail -15
echo "== bench"; timeout 900 python bench.py --full 2>&1 | tail -1 | tee $OUT/bench_$TAG.json | cut -c1-600
echo "== rocprof stats"; cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o s -- python $ROOT/bench.py --full --steps 5 --warmup 1 --no-cpu-baseline > $OUT/prof_$TAG.log 2>&1; cd $ROOT
python tools/prof_summary.py $(find $OUT/prof_$TAG -name "*results.db" | head -1) | tee $OUT/kernel_stats_$TAG.txt | head -24
