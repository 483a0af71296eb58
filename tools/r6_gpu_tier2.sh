#!/bin/bash
export OUT=${OUT:-bench_logs}      # where the logs of this script go
mkdir -p $OUT/r6e
( timeout 3000 python -m pytest tests -m gpu -q -x 2>&1 | tail -40 ) > $OUT/r6e/gpu_tier.log 2>&1
( timeout 900 python bench.py --full --steps 20 --warmup 5 2>&1 | grep -v amdgpu.ids | tail -2 ) > $OUT/r6e/bench_full.log 2>&1; echo rc=$? >> $OUT/r6e/bench_full.log
( timeout 300 python -c "import __graft_entry__ as g; g.smoke()" 2>&1 | grep -v amdgpu.ids | tail -2 ) > $OUT/r6e/smoke.log 2>&1
tail -12 $OUT/r6e/gpu_tier.log; cat $OUT/r6e/smoke.log; tail -c 600 $OUT/r6e/bench_full.log
