#!/bin/bash
# resample phase clocks (GH_RS_STAMPS variant) for the C2 and C4 sizes;
# "full" as first argument: also the GPU suite and the whole bench lines.
# Output under GH_RS_OUT (default out/rs).
set -e
O=${GH_RS_OUT:-out/rs}
mkdir -p "$O"
export TMPDIR=/tmp
timeout -k 10 120 python tools/rs_stamps.py lg10 20 > "$O/stamps_lg10.txt" 2>&1
timeout -k 10 120 python tools/rs_stamps.py kit 21 > "$O/stamps_kit.txt" 2>&1
if [ "$1" = "full" ]; then
  timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$O/pytest_gpu.log" 2>&1
  timeout -k 10 300 python bench.py --full --no-cpu-baseline > "$O/bench.json" 2> "$O/bench.err"
  timeout -k 10 300 python bench.py --full --no-cpu-baseline --model kitagawa --particles 2097152 > "$O/bench_kit.json" 2> "$O/bench_kit.err"
fi
