#!/bin/bash
# Run the bench on every A/B variant (GPU box): tools/ab_run.sh name1 name2 ...
# Logs and summary.txt go to $AB_OUT (default build/ab under the repository).
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${AB_OUT:-$ROOT/build/ab}
mkdir -p "$OUT"
for name in "$@"; do
  # --full: the summary reads the roofline's kernel time and integrator steps
  PCK_LIB=$ROOT/pycatkin_amd/_ab/lib_$name.so timeout -k 10 120 python "$ROOT/bench.py" --steps 5 --warmup 1 \
      --full --no-cpu-baseline > "$OUT/$name.log" 2>&1 || exit $?
  echo "$name $(tail -1 "$OUT/$name.log" | python -c 'import json,sys; d=json.loads(sys.stdin.read()); print(d["value"], d["roofline"]["kernel_ms"], d["roofline"]["integrator_steps"], d["status"])')" >> "$OUT/summary.txt"
done
