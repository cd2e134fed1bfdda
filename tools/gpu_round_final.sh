#!/bin/bash
# end-of-round collection: GPU test suite, full bench line, kernel trace of the all-rows headline alone, kernel trace of the default run
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/out}; export OUT; mkdir -p $OUT; cd $R
timeout 1500 python -m pytest tests -m gpu -x -q > $OUT/final_gputests.log 2>&1; tail -2 $OUT/final_gputests.log
python bench.py --full > $OUT/bench_final.log 2>&1; tail -1 $OUT/bench_final.log | cut -c1-300
bash tools/gpu_trace_headline.sh > $OUT/trace_headline.log 2>&1; tail -9 $OUT/trace_headline.log | cut -c1-200
cd /tmp && export TMPDIR=/tmp && rm -rf $OUT/prof_full && rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/prof_full -- python3 $R/bench.py --full --steps 10 --warmup 3 --no-cpu-baseline > $OUT/bench_prof_full.log 2>&1
cd $R; f=$(ls -t $OUT/prof_full/*/*kernel_stats.csv | head -1); test -n "$f" && head -10 "$f" | cut -c1-160
