"""Times the ABC kernels (fg_abc.hip) on the GPU:

    python tools/bench_abc.py [--n 4096,65536] [--reps 5] [--out FILE]

Per population size n, at d = 4 (x#i ~ N(0, 1), y#i ~ N(x#i, 0.5) observed, i < 4; simulator = the four observe statements, Euclidean):
    rejection   one round of B = n prior attempts through `fg_abc_round_prior` (prior draw, simulate, cells to f64, distance, ordered
                compaction, the count back to the host): attempts per second;
    mixture     `fg_abc_mixture` of m = n particles against n centers (table, k_abc_mixture, finish, the call's own allocation and
                synchronise): microseconds per call, (particle, center) pairs per second, and the time as a multiple of what the pairs
                cost at the f64 vector rate alone, counting 2 d + 3 operations and a 30-operation exp per pair.
Host clock around `reps` calls after 2 warm-up calls; median of 3 such windows."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fugue_amd import abc as A          # noqa: E402
from fugue_amd import engine as E       # noqa: E402
from fugue_amd import model as M        # noqa: E402

D = 4
F64_VECTOR_FLOPS = 1024 * 64 * 2.2e9 / 4.3   # f64 lane-operations per second: 1 024 SIMDs, one v_fma_f64 / v_add_f64 per ~4.3 cycles per SIMD at
#                                              ~2.2 GHz (profiles/round1_f64_issue_microbench.txt), an FMA counted as one operation


def model():
    P = M.Program()
    for i in range(D):
        x = P.sample(M.addr("x", i), M.Normal(0.0, 1.0))
        P.observe(M.addr("y", i), M.Normal(x, 0.5), 0.2 * i - 0.3)
    return P


def window(fn, reps):
    for _ in range(2):
        fn()
    out = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        out.append((time.perf_counter() - t0) / reps)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", default="4096,65536")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    cp = E.compile_model(model())
    rows = []
    for n in [int(v) for v in a.n.split(",")]:
        eng = E.Engine(cp, n, seed=1)
        h = A.ABCHandle(eng, A.SIM_OBSERVE, list(range(D)), A._observed(cp, A.SIM_OBSERVE, list(range(D)), None), A.EuclideanDistance(), n)
        t_round = window(lambda: h.round_prior(1.0, n), a.reps)
        acc, _ = h.round_prior(1.0, n)
        h.close()
        rng = np.random.default_rng(n)
        centers = rng.normal(0.0, 1.0, (D, n))
        x = centers + rng.normal(0.0, 0.3, (D, n))
        w = np.full(n, 1.0 / n)
        std = np.full(D, 0.4)
        d_x, d_c, d_o = eng.upload(x), eng.upload(centers), eng.device_alloc(n * 8)
        t_mix = window(lambda: E._check(E.lib().fg_abc_mixture(eng.h, d_x, n, d_c, n, D, E._dp(w), E._dp(std), d_o)), a.reps)
        for p in (d_x, d_c, d_o):
            eng.device_free(p)
        eng.close()
        pairs = float(n) * n
        alu_s = pairs * (2 * D + 3 + 30) / F64_VECTOR_FLOPS
        row = {"n": n, "d": D, "rejection_round_us": t_round * 1e6, "attempts_per_s": n / t_round, "accepted_of_round": acc,
               "mixture_us": t_mix * 1e6, "pairs_per_s": pairs / t_mix, "mixture_over_f64_alu_bound": t_mix / alu_s}
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
