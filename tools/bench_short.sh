#!/bin/bash
# usage: tools/bench_short.sh <tag>   (run on the GPU box) - bench line + top kernels
tag=${1:-x}
mkdir -p tools/tmp
timeout 500 python bench.py --full --steps 50 --warmup 10 --no-cpu-baseline > tools/tmp/bench_$tag.json 2> tools/tmp/bench_$tag.err || exit
python - <<EOF2
import json
d=json.load(open("bench_detail.json"))
print(d["value"], d["ms_per_step"], d["step_mfma_frac"])
for k in d["kernels"][:${2:-9}]: print(k["tag"], k["launches_per_step"], k["avg_us"], k["per_step_ms"])
EOF2
