#!/bin/bash
# end-of-round check on the GPU box: smoke, the whole GPU suite, the full bench line; everything goes under OUT (the first argument)
cd "$(dirname "$0")/.."
OUT=${1:?"usage: tools/final_batch.sh OUTDIR"}
mkdir -p "$OUT"
python -c "import __graft_entry__ as g; g.smoke(); print('smoke ok')" > "$OUT/smoke.txt" 2>&1
python -m pytest tests -m gpu -q -x 2>&1 | tail -5 > "$OUT/gputest_head.txt"
python bench.py --full > "$OUT/bench_default.json" 2> "$OUT/bench_default.err"
tail -2 "$OUT/smoke.txt"; cat "$OUT/gputest_head.txt"; tail -c 300 "$OUT/bench_default.json"
