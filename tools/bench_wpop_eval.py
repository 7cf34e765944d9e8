"""Times the predictive checks and WAIC / IS-LOO of a weighted population on the device (fg_wpop_eval.hip) on the GPU:

    python tools/bench_wpop_eval.py [--particles 1048576] [--rows 64] [--obs 64] [--reps 3] [--out FILE]

A table [rows][N] of doubles and Dirichlet-like weights are uploaded once.  Each call is made once to warm up, then `reps` times; the
figures are medians of whole calls on the host clock (every call ends in a download, so it is synchronous):
    copy_ms            a device copy of the same table (`cells_f64` with f64 tags: every cell read once and written once): the yardstick
    loglik_ms          `WeightedPopulation.loglik(table, rows)`: the cells once, three staged words written and read twice, the trees
    checks_marginal_ms `WeightedPopulation.checks`: one marginal check (mean) per row, `rows` slots
    checks_all_ms      one check over every row with all five statistics, 5 slots
    moments_ms         `WeightedPopulation.moments(table, rows)`: what the checks' scratch round trip costs per slot
    table_bytes, and each of the above as GB/s of the table (`*_table_gbs`: table_bytes over the time, not the traffic)
and the summary driver on `workloads.ridge_regression` with `obs` observations (p = 8):
    summary_plain_ms      `adaptive_smc_summary(seed, N, model)`, whole call: what the parent commit's summary costs
    summary_eval_ms       the same with `pointwise=True, checks=True`
    population_plain_ms / population_eval_ms   `population_summary` of one engine that holds the final population, without / with the options
    population_sliced_ms  the same with `stage_words=N`: one statement per slice, so fg_predict_eval runs once per statement
No threshold: DESIGN 3.21 states the expected bound before the measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fugue_amd import engine as E       # noqa: E402
from fugue_amd import inference as I    # noqa: E402
from fugue_amd import model as M        # noqa: E402
from fugue_amd import workloads as W    # noqa: E402


def median_ms(call, reps):
    call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1048576)
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--obs", type=int, default=64)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, R, seed = a.particles, a.rows, a.seed
    rng = np.random.default_rng(seed)
    row = dict(particles=N, rows=R, reps=a.reps, table_bytes=R * N * 8)
    eng = E.Engine(E.compile_model(W.normal_sites(1)), N, seed=seed)     # N chains: `cells_f64` copies [1][rows][chains]
    g = rng.gamma(0.7, size=N)
    d_w = eng.upload(g / g.sum())
    d_x = eng.device_alloc(R * N * 8)
    block = max(1, (1 << 24) // N)
    for r0 in range(0, R, block):                    # uploaded in pieces: the host never holds the table
        eng.upload(rng.normal(-3.0, 1.0, (min(block, R - r0), N)), d_x + r0 * N * 8)
    d_y = eng.device_alloc(R * N * 8)
    wp = eng.wpop(N, d_w)

    def copy():
        eng.cells_f64(d_x, 1, R, list(range(R)), [M.F64] * R, out=d_y)
        eng.synchronize()

    marginal = [([k], ["mean"], [-3.0]) for k in range(R)]
    whole = [(list(range(R)), list(E.PPC_STATS), [-3.0] * R)]
    row["copy_ms"] = median_ms(copy, a.reps)
    row["loglik_ms"] = median_ms(lambda: wp.loglik(d_x, R), a.reps)
    row["checks_marginal_ms"] = median_ms(lambda: wp.checks(d_x, [M.F64] * R, marginal), a.reps)
    row["checks_all_ms"] = median_ms(lambda: wp.checks(d_x, [M.F64] * R, whole), a.reps)
    row["moments_ms"] = median_ms(lambda: wp.moments(d_x, R), a.reps)
    for k in ("copy", "loglik", "checks_marginal", "checks_all", "moments"):
        row[k + "_table_gbs"] = row["table_bytes"] / (row[k + "_ms"] * 1e-3) / 1e9
    wp.close()
    for b in (d_w, d_x, d_y):
        eng.device_free(b)
    eng.close()

    X, y, _ = W.ridge_data(n=a.obs, p=8)[:3]
    cp = E.compile_model(W.ridge_regression(X, y))
    row["observe_statements"] = cp.O
    row["summary_plain_ms"] = median_ms(lambda: I.adaptive_smc_summary(seed, N, cp), a.reps)
    row["summary_eval_ms"] = median_ms(lambda: I.adaptive_smc_summary(seed, N, cp, pointwise=True, checks=True), a.reps)
    eng = E.Engine(cp, N, seed=seed)
    r = eng.smc_run(download=False)
    row["population_plain_ms"] = median_ms(lambda: I.population_summary(eng, r["log_evidence"], r["betas"]), a.reps)
    row["population_eval_ms"] = median_ms(lambda: I.population_summary(eng, r["log_evidence"], r["betas"], pointwise=True, checks=True), a.reps)
    row["population_sliced_ms"] = median_ms(lambda: I.population_summary(eng, r["log_evidence"], r["betas"], pointwise=True, checks=True, stage_words=N), a.reps)
    eng.close()
    print("N=%d rows=%d (%.0f MB): copy %.2f ms; loglik %.2f ms; checks marginal %.2f ms, all-rows %.2f ms; moments %.2f ms; summary plain %.1f ms, with pointwise + checks %.1f ms; "
          "on a held population: plain %.1f, eval %.1f, one statement per slice %.1f ms" % (
              N, R, row["table_bytes"] / 1e6, row["copy_ms"], row["loglik_ms"], row["checks_marginal_ms"], row["checks_all_ms"], row["moments_ms"], row["summary_plain_ms"],
              row["summary_eval_ms"], row["population_plain_ms"], row["population_eval_ms"], row["population_sliced_ms"]), flush=True)
    line = json.dumps(row)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
