#!/bin/bash
# Round-2 GPU check (run through gpurun): new scale / chunk tests, bench line with the per-kernel table, kernel trace.
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/out}; export OUT; mkdir -p $OUT
timeout 1500 python -m pytest tests/test_gpu_scale.py -m gpu -x -q > $OUT/scale_test.log 2>&1; tail -5 $OUT/scale_test.log
python bench.py --full --steps 20 --warmup 5 > $OUT/bench_r2.log 2>&1; tail -1 $OUT/bench_r2.log | cut -c1-6000
cd /tmp && export TMPDIR=/tmp && rm -rf $OUT/prof_r2 && rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_r2 -- python3 $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-extra-configs > $OUT/bench_prof_r2.log 2>&1
cd $R; f=$(find $OUT/prof_r2 -name "*kernel_stats.csv" | head -1); head -12 $f | cut -c1-160
