#!/bin/bash
# A/B of library builds on ONE box: scripts/ab/lib*.so, each through the same bench command.
# usage: [AB_OUT=dir] scripts/ab_bench.sh [bench.py flags...]   (results: $AB_OUT/<name>.<rep>.json, default ab_out/)
OUT=${AB_OUT:-ab_out}
mkdir -p "$OUT"
for rep in 1 2; do
for lib in scripts/ab/lib*.so; do
  name=$(basename $lib .so)
  SWIMMER_HIP_LIB=$PWD/$lib python bench.py --full --no-cpu-baseline --no-aux --steps 100 --warmup 5 "$@" > "$OUT/$name.$rep.json" 2> "$OUT/$name.$rep.err" || exit 1
  python - <<P
import json
j = json.load(open("$OUT/$name.$rep.json"))
print("$name rep$rep: ms/iter %.4f kernel_ms %.4f (post %.4f) value %.4e" % (j["ms_per_step"], j["roofline"]["kernel_ms_timed_region"], j["roofline"]["kernel_ms_postpass"], j["value"]))
P
done
done
