#!/bin/bash
# quick A/B on the GPU box: the k = 32 route's tests, then the default bench line's headline figures.  usage: tools/qbench.sh tag [bench args]
# (the bench line lands in $BENCH_OUT, default bench_out/)
tag=$1; shift
out=${BENCH_OUT:-bench_out}
mkdir -p $out
python -m pytest tests/test_gpu_bs.py tests/test_gpu_fuzz.py -x -q 2>&1 | tail -3
python bench.py --full --steps 20 --warmup 5 --no-end-to-end --no-cpu-baseline --no-repeats "$@" > $out/qb_$tag.json 2> $out/qb_$tag.err
python - "$out/qb_$tag.json" <<'PY'
import json, sys
d = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
print(d["value"], d["ms_per_step"], d.get("kernels", {}).get("ms_per_step"))
PY
