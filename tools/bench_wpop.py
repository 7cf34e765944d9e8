"""Times the weighted-population summary on the device (fg_wpop.hip behind `adaptive_smc_summary`) against the path it replaces --
`adaptive_smc`'s download of the population and a numpy summary on the host -- on the GPU:

    python tools/bench_wpop.py [--particles 1048576] [--sites 32] [--reps 3] [--out FILE]

The model is `workloads.reference_model(sites)`.  Each driver is called once to warm up (compilation at run time, allocations), then
`reps` times; the figures are medians of whole calls on the host clock:
    summary_ms        `adaptive_smc_summary(seed, N, model)`: the run, then mean / std / mcse / five exact quantiles of every site on the device
    download_ms       `adaptive_smc(seed, N, model)`: the same run, then [S][N] cells and both weight vectors copied to the host
    host_numpy_ms     the host's summary of that download: weighted mean / std / mcse per site and the five weighted quantiles by
                      argsort + cumulative sum (float64; not the exact units of the device path)
    download_plus_host_ms  the two together: what a caller of the parent commit pays for the same figures
and, on one engine that holds the final population (`smc_run(download=False)` once), the pieces of the device path alone:
    smc_run_ms, wpop_new_ms (the copy of the weights and their units), gather_ms (`cells_f64` of the sites), moments_ms, quantiles_ms,
    copy_back_ms (`get_values` + `smc_weights`, the copy the summary avoids);
    spread_moments_ms, spread_quantiles_ms, spread_passes_max: the same rows under Dirichlet-like weights uploaded by the caller, which keep
    every particle alive (the final weights of the run itself may leave few: `ess` and `n_zero` say how many), so the selection needs its
    histogram pass.
No threshold: the comparison is against the download path of the same commit."""
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

PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)


def host_summary(res):
    w = res.weights
    W_ = w.sum()
    out = {}
    for a, v in zip(res.sites, res.vtypes):
        if v != M.F64:
            continue
        x = res.get_f64(a)
        mean = float((w * x).sum() / W_)
        dev = x - mean
        order = np.argsort(x, kind="stable")
        cum = np.cumsum(w[order])
        idx = np.minimum(np.searchsorted(cum, np.asarray(PROBS) * cum[-1], side="left"), x.size - 1)
        out[a] = (mean, float(np.sqrt((w * dev * dev).sum() / W_)), float(np.sqrt((w * w * dev * dev).sum())) / W_, x[order][idx])
    return out


def median_ms(call, reps):
    call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--particles", type=int, default=1048576)
    ap.add_argument("--sites", type=int, default=32)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    N, seed = a.particles, a.seed
    cp = E.compile_model(W.reference_model(a.sites))
    row = dict(particles=N, sites=cp.S, f64_sites=cp.d, reps=a.reps, population_bytes=(cp.S + 2) * N * 8)

    keep = {}
    row["summary_ms"], row["summary_calls"] = median_ms(lambda: keep.__setitem__("s", I.adaptive_smc_summary(seed, N, cp)), a.reps)
    row["download_ms"], row["download_calls"] = median_ms(lambda: keep.__setitem__("r", I.adaptive_smc(seed, N, cp)), a.reps)
    row["host_numpy_ms"], row["host_numpy_calls"] = median_ms(lambda: keep.__setitem__("h", host_summary(keep["r"])), a.reps)
    row["download_plus_host_ms"] = row["download_ms"] + row["host_numpy_ms"]
    s, h = keep["s"], keep["h"]
    row["max_abs_mean_diff"] = max(abs(s.mean[s.row(k)] - v[0]) for k, v in h.items())
    row["max_abs_median_diff"] = max(abs(s.quantiles[s.row(k)][2] - v[3][2]) for k, v in h.items())
    row["ess"], row["n_zero"], row["passes_max"] = s.ess, s.n_zero, int(s.passes.max())

    eng = E.Engine(cp, N, seed=seed)
    row["smc_run_ms"], _ = median_ms(lambda: eng.smc_run(download=False), a.reps)
    values = E.lib().fg_engine_values_device(eng.h)
    x = eng.device_alloc(cp.d * N * 8)

    def new_pop():
        wp = eng.wpop()
        wp.close()

    def gather():
        eng.cells_f64(values, 1, cp.S, cp.f64_sites, [M.F64] * cp.d, out=x)
        eng.synchronize()

    row["wpop_new_ms"], _ = median_ms(new_pop, a.reps)
    row["gather_ms"], _ = median_ms(gather, a.reps)
    wp = eng.wpop()
    row["moments_ms"], _ = median_ms(lambda: wp.moments(x, cp.d), a.reps)
    row["quantiles_ms"], _ = median_ms(lambda: wp.quantiles(x, cp.d, PROBS), a.reps)
    row["copy_back_ms"], _ = median_ms(lambda: (eng.get_values(), eng.smc_weights()), a.reps)
    wp.close()
    # the same rows under weights that keep every particle alive (a tempered run of a 32-site model leaves few): a Dirichlet-like vector
    g = np.random.default_rng(seed).gamma(0.7, size=N)
    d_w = eng.upload(g / g.sum())
    wp = eng.wpop(N, d_w)
    row["spread_n_zero"] = wp.units()["n_zero"]
    row["spread_moments_ms"], _ = median_ms(lambda: wp.moments(x, cp.d), a.reps)
    row["spread_quantiles_ms"], _ = median_ms(lambda: keep.__setitem__("q", wp.quantiles(x, cp.d, PROBS)), a.reps)
    row["spread_passes_max"] = int(keep["q"][1].max())
    wp.close()
    eng.device_free(d_w)
    eng.device_free(x)
    eng.close()
    print("N=%d sites=%d: summary %.1f ms; download %.1f ms + numpy %.1f ms = %.1f ms; pieces: smc_run %.2f, wpop_new %.2f, gather %.2f, moments %.2f, quantiles %.2f, copy back %.1f ms; spread weights: moments %.2f, quantiles %.2f ms in %d passes" % (
        N, cp.S, row["summary_ms"], row["download_ms"], row["host_numpy_ms"], row["download_plus_host_ms"], row["smc_run_ms"], row["wpop_new_ms"], row["gather_ms"],
        row["moments_ms"], row["quantiles_ms"], row["copy_back_ms"], row["spread_moments_ms"], row["spread_quantiles_ms"], row["spread_passes_max"]), flush=True)
    line = json.dumps(row)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
