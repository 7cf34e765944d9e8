#!/bin/bash
cd ${GRAFT_REPO_ROOT:-.}
export O=${FG_BENCH_OUT:-bench_out}; mkdir -p $O
timeout -k 10 900 python -m pytest tests -x -q -m gpu 2>&1 | tail -5 &&
timeout -k 10 600 python bench.py --full --steps 20 --warmup 5 --full-out $O/r4_bench_c_full.json > $O/r4_bench_c.json 2> $O/r4_bench_c.err && wc -c $O/r4_bench_c.json && python - <<'PY'
import json, os
d=json.load(open(os.path.join(os.environ['O'], 'r4_bench_c.json')))
print(d['value'], d['roofline']['frac'], d['cpu_baseline']['value'])
for k,v in d['legs'].items(): print(k, v)
PY
