#!/bin/bash
# kernel trace of the all-rows headline configuration ALONE (no class-rows-only region, no config 3 / 4)
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/out}; export OUT; mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp && rm -rf $OUT/prof_head && rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_head -- python3 $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-extra-configs --no-class-rows > $OUT/bench_head.log 2>&1
cd $R; tail -1 $OUT/bench_head.log | cut -c1-300; f=$(ls -t $OUT/prof_head/*/*kernel_stats.csv | head -1); head -8 $f | cut -c1-150
