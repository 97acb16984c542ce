#!/bin/bash
# end-of-round refresh of profiles/: every rocprofv3 summary and the single-GPU bench lines of the large BASELINE configs (those under OUT, the first argument)
cd "$(dirname "$0")/.."
OUT=${1:?"usage: tools/final_profiles.sh OUTDIR"}
mkdir -p "$OUT"
bash tools/profile_run.sh 8192 2 half_tank ic0_tile > /dev/null 2>&1
bash tools/profile_run.sh 8192 2 half_tank ic0 > /dev/null 2>&1
bash tools/profile_run.sh 1024 10 dam_break ic0 > /dev/null 2>&1
bash tools/profile_run.sh 4096 4 waterfall ic0_tile > /dev/null 2>&1
bash tools/profile_run.sh 4096 4 waterfall ic0 > /dev/null 2>&1
bash tools/profile_run.sh 16384 1 half_tank ic0_tile > /dev/null 2>&1
for p in ic0_tile ic0; do
  python bench.py --full --size 16384 --workload dam_break --precond $p --steps 2 --no-secondary --no-pmc > "$OUT/bench_16384_dam_break_$p.json" 2> "$OUT/bench_16384_dam_break_$p.err"
  python bench.py --full --size 4096 --workload waterfall --precond $p --steps 10 --no-secondary --no-pmc > "$OUT/bench_4096_waterfall_$p.json" 2> "$OUT/bench_4096_waterfall_$p.err"
done
ls gpurun_out/prof_*/summary.md
