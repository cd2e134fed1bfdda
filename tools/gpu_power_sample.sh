#!/bin/bash
# power / clock samples of the GPU while bench.py runs (is the step power-limited?)
R=$(cd "$(dirname "$0")/.." && pwd); OUT=${OUT:-$R/out}; export OUT; mkdir -p $OUT
python3 bench.py --full --steps 2500 --warmup 20 > $OUT/power_bench.log 2>&1 &
BP=$!
for i in $(seq 1 120); do
  rocm-smi --showpower --showclocks 2>&1 | grep -E "Package Power|sclk" | sed 's/.*: //' | tr '\n' ' '
  echo
  sleep 0.25
  kill -0 $BP 2>/dev/null || break
done | sort | uniq -c | sort -k1,1nr | head -40
wait $BP
tail -1 $OUT/power_bench.log | cut -c1-160
