"""Exact Gibbs sweeps on one MI355X: k_gibbs_sweep (fg_gibbs.hip behind `Engine.gibbs`) on C5, the mixture of `workloads.mixture` with
64 labels of K = 4 values beside four means, against the same move composed from the parent API and against single-site MH.

    python tools/bench_gibbs.py [--chains 32768,262144] [--reps 5] [--composed-sites 4] [--mix-chains 1024] [--mix-samples 200] [--out FILE]

Per chain count, medians of whole calls on the host clock, every call ending in a device synchronise, every path warmed first:
    sweep_ms          `gibbs.sweep(1)`: all 64 labels of every chain, 256 scoring runs a chain, one launch
    composed_ms       the same sweep from the parent commit's entry points: per label and candidate the cells are written on the host,
                      uploaded (`Engine.set_values`) and scored (`Engine.log_joint`), and numpy normalises and picks.  Measured on
                      `--composed-sites` labels and scaled to 64 (every label costs the same); composed_over_sweep is the ratio
    mh_pass_ms        `mh_step(S)` on the same engine: S single-site proposals a chain, the count that visits every site once
    hmc_step_ms       `hmc_step(1)`; sweep_share = sweep / (hmc_step + sweep), the sweep's share of an HMC-within-Gibbs iteration
Mixing, at `--mix-chains` chains: multi-chain ESS of mu#0 per second of wall time under `hmc_gibbs_chain` against `adaptive_mcmc_chain`
with the same number of samples and warmup iterations (an MH iteration is one single-site proposal).  No threshold is attached to any
of these figures.  Without a GPU the script fails (no fallback)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fugue_amd as F   # noqa: E402
from fugue_amd import engine as E, workloads as W   # noqa: E402
from fugue_amd.diagnostics import effective_sample_size_multichain   # noqa: E402

K = 4


def timed(call, eng=None):
    t0 = time.perf_counter()
    r = call()
    if eng is not None:
        eng.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def composed_sites(eng, sites, rng):
    """the move of `sites` [(site, lo, K)] from set_values + log_joint, numpy for the rest"""
    v = eng.get_values()
    for site, lo, k_n in sites:
        l = np.empty((k_n, eng.C))
        for k in range(k_n):
            v[site] = lo + k
            eng.set_values(v)
            acc = eng.log_joint()
            l[k] = (acc[0] + acc[1]) + acc[2]
        w = np.exp(l - l.max(axis=0))
        s = np.cumsum(w, axis=0)
        x = rng.random(eng.C) * s[-1]
        v[site] = lo + np.minimum((x[None] >= s).sum(axis=0), k_n - 1)
    eng.set_values(v)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="32768,262144")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--composed-sites", type=int, default=4)
    ap.add_argument("--mix-chains", type=int, default=1024)
    ap.add_argument("--mix-samples", type=int, default=200)
    ap.add_argument("--out", default=None)
    a_ = ap.parse_args()
    prog = W.mixture(W.mixture_data(64)[0], K=K)
    cp = E.compile_model(prog)
    rows = []
    for Cn in (int(v) for v in a_.chains.split(",")):
        eng = E.Engine(cp, Cn, seed=1)
        eng.hmc_init(E.hmc_config(), 0)
        g = eng.gibbs()
        n_sites = g.n_sites
        sites = list(zip(g.layout["sites"], g.layout["lo"], g.layout["K"]))
        rng = np.random.default_rng(1)
        g.sweep(1); eng.hmc_step(1); eng.synchronize()                                    # warm-up of every path
        t_s = [timed(lambda: g.sweep(1), eng)[0] for _ in range(a_.reps)]
        t_h = [timed(lambda: eng.hmc_step(1), eng)[0] for _ in range(a_.reps)]
        g.close(); eng.close()
        ec = E.Engine(cp, Cn, seed=1)                                                     # no sampler session: set_values re-scores nothing
        ec.prior_init()
        composed_sites(ec, sites[:1], rng)
        t_c = [timed(lambda: composed_sites(ec, sites[:a_.composed_sites], rng), ec)[0] * n_sites / a_.composed_sites for _ in range(max(1, a_.reps // 2))]
        ec.close()
        em = E.Engine(cp, Cn, seed=1)
        em.mh_init(0)
        em.mh_step(cp.S); em.synchronize()
        t_m = [timed(lambda: em.mh_step(cp.S), em)[0] for _ in range(a_.reps)]
        em.close()
        s, h, c, m = (statistics.median(t) for t in (t_s, t_h, t_c, t_m))
        row = dict(chains=Cn, labels=n_sites, K=K, sweep_ms=s, scoring_runs_per_s=Cn * n_sites * K / (s * 1e-3), composed_ms=c, composed_over_sweep=c / s, mh_pass_ms=m,
                   hmc_step_ms=h, sweep_share=s / (s + h))
        print("C5 %7d chains: sweep %8.2f ms = %.3g scoring runs/s; composed %10.1f ms (x%.0f); mh_step(%d) %8.2f ms; hmc_step(1) %8.2f ms, the sweep is %4.1f%% of an iteration"
              % (Cn, s, row["scoring_runs_per_s"], c, c / s, cp.S, m, h, 100.0 * row["sweep_share"]), flush=True)
        rows.append(row)
    n, Cm = a_.mix_samples, a_.mix_chains
    for name, run in (("hmc_gibbs_chain", lambda: F.hmc_gibbs_chain(1, cp, n, n, n_chains=Cm)), ("adaptive_mcmc_chain", lambda: F.adaptive_mcmc_chain(1, cp, n, n, n_chains=Cm))):
        run()                                                                             # warm-up: run-time compilation, allocations
        ms, b = timed(run)
        ess = effective_sample_size_multichain(b.get_f64("mu#0"))
        row = dict(driver=name, chains=Cm, samples=n, warmup=n, wall_ms=ms, ess_mu0=ess, ess_per_s=ess / (ms * 1e-3))
        print("mixing %-20s %d chains x %d draws: %9.1f ms, ESS(mu#0) %.4g = %.4g per second" % (name, Cm, n, ms, ess, row["ess_per_s"]), flush=True)
        rows.append(row)
    line = json.dumps(rows)
    print(line)
    if a_.out:
        os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
        with open(a_.out, "w") as f_:
            f_.write(line + "\n")


if __name__ == "__main__":
    main()
