#!/bin/bash
cd ${GRAFT_REPO_ROOT:-.}
O=${FG_BENCH_OUT:-bench_out}; mkdir -p $O
timeout -k 10 900 python bench.py --full --full-out $O/r4_bench_default_full.json > $O/r4_bench_default.json 2> $O/r4_bench_default.err && wc -c $O/r4_bench_default.json &&
timeout -k 10 600 python bench.py --full --steps 20 --warmup 5 --full-out $O/r4_bench_s20_full.json > $O/r4_bench_s20.json 2> $O/r4_bench_s20.err && wc -c $O/r4_bench_s20.json
