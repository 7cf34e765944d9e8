"""Mean-field VI throughput on one MI355X: the fused ELBO batch (k_vi_elbo + k_vi_reduce, fg_vi.hip) against the same batch composed
from the parent API (host draws, Engine.set_values, Engine.log_joint), and the optimizer's time per iteration.

    python tools/bench_vi.py [--n 65536] [--iters 20] [--warmup 3] [--out FILE.json]

N = samples per ELBO evaluation.  One optimizer iteration of a P-factor guide is 1 + 4P evaluations of N samples: a "sample-score" is one
sample of one evaluation (P draws, P guide densities, one ScoreGivenTrace).  Times are host clocks around calls that end in a device
synchronise; every shape is warmed up first; the two paths alternate inside one process.  Without a GPU the script fails (no fallback)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fugue_amd import engine as E, vi as V, workloads as W   # noqa: E402


def batch_rows(cp, eps=0.01):
    """The 1 + 4P guides of one optimizer iteration from for_support(Real, 0.0), and their stream ids."""
    P = cp.S
    base = [(0, j, 0.0, V.init_log_sigma(0.0)) for j in range(P)]
    rows, sids = [base], [0]
    for j in range(2 * P):
        for sg in (eps, -eps):
            r = list(base)
            f, s, a, b = r[j // 2]
            r[j // 2] = (f, s, a + sg, b) if j % 2 == 0 else (f, s, a, b + sg)
            rows.append(r)
            sids.append(1 + j)
    return rows, sids


def composed_batch(eng, cp, rows, sids, N, seed):
    """The same ELBO batch from the parent commit's API: draws and log q on the host (numpy), 8 S N bytes over the host link per
    evaluation (Engine.set_values), one k_log_joint launch per evaluation (Engine.log_joint)."""
    out = np.zeros(len(rows))
    for k, (row, sid) in enumerate(zip(rows, sids)):
        rng = np.random.default_rng([seed, sid])
        z = rng.standard_normal((cp.S, N))
        mu = np.array([q[2] for q in row])[:, None]
        sg = np.exp(np.array([q[3] for q in row]))[:, None]
        x = mu + sg * z
        log_q = (-0.5 * z * z - np.log(sg) - 0.9189385332046727).sum(axis=0)
        eng.set_values(np.ascontiguousarray(x).view(np.int64))
        acc = eng.log_joint()
        out[k] = ((acc[0] + acc[1] + acc[2]) - log_q).mean()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--composed-iters", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    results = []
    for name, prog in (("normal_sites(32)", W.normal_sites(32)), ("reference_model(8)", W.reference_model(8))):
        cp = E.compile_model(prog)
        rows, sids = batch_rows(cp)
        n_eval, N = len(rows), a.n
        eng = E.Engine(cp, N, seed=1)
        for _ in range(a.warmup):
            fused = eng.vi_elbo_batch(rows, sids)
        t = []
        for _ in range(a.iters):
            t0 = time.perf_counter(); fused = eng.vi_elbo_batch(rows, sids); t.append(time.perf_counter() - t0)
        composed_batch(eng, cp, rows[:2], sids[:2], N, 1)                       # warm-up of the composed path's shapes
        tc = []
        for _ in range(a.composed_iters):
            t0 = time.perf_counter(); comp = composed_batch(eng, cp, rows, sids, N, 1); tc.append(time.perf_counter() - t0)
        guide = [(0, j, 0.0, V.init_log_sigma(0.0)) for j in range(cp.S)]
        cfg = V.VIConfig(n_iterations=a.iters, n_samples_per_iter=N, convergence_window=0).raw()
        eng.vi_optimize(guide, V.VIConfig(n_iterations=a.warmup, n_samples_per_iter=N, convergence_window=0).raw())
        t0 = time.perf_counter(); eng.vi_optimize(guide, cfg); t_opt = (time.perf_counter() - t0) / a.iters
        eng.close()
        t_f, t_c = float(np.median(t)), float(np.median(tc))
        r = dict(model=name, n_factors=cp.S, n_eval=n_eval, n_samples=N,
                 fused_batch_ms=1e3 * t_f, fused_batch_ms_min_max=[1e3 * min(t), 1e3 * max(t)], fused_sample_scores_per_s=n_eval * N / t_f,
                 composed_batch_ms=1e3 * t_c, composed_sample_scores_per_s=n_eval * N / t_c, fused_over_composed=t_c / t_f,
                 optimizer_ms_per_iteration=1e3 * t_opt, monitor_elbo_fused=float(fused[0]), monitor_elbo_composed=float(comp[0]))
        print(json.dumps(r), flush=True)
        results.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
