"""Times the particle filter bank on the device (fg_pf.hip behind `ParticleFilterBank`) on the GPU:

    python tools/bench_pf.py [--particles 256,1024,5000] [--filters 1,256,4096] [--steps 256] [--reps 3] [--host-steps 8] [--out FILE]

For every bank shape (n particles x B filters, T steps) one bank is built and called once to warm up (code object, allocations), then
`reps` times; the figures are medians of whole calls on the host clock, every call ending in the library's own synchronise:
    run_ms            `bank.run(obs)`: T steps in ceil(T / steps_per_launch) launches, the five [T][B] summaries copied back
    filter_steps_per_s, particle_steps_per_s   B T and B T n over run_ms
    steps_ms          the same T steps as T `bank.step(obs_t, record=False)` calls: one launch, one upload and one copy back each
    step_recorded_ms  one `bank.step(obs_t)` with StepOut's five [B][n] arrays copied back
and, beside them, the restatement (tests/pf_restatement.py, the reference's sequential order) on the host:
    host_filter_steps_per_s, host_particle_steps_per_s   one filter of n particles over `--host-steps` steps
No threshold is attached to any of these figures."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fugue_amd import pf as PF                 # noqa: E402
from tests import pf_restatement as R          # noqa: E402


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
    ap.add_argument("--particles", default="256,1024,5000")
    ap.add_argument("--filters", default="1,256,4096")
    ap.add_argument("--steps", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-steps", type=int, default=8)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    T = a.steps
    obs = np.cumsum(np.random.default_rng(1).normal(0.0, 0.5, T))
    rows = []
    for n in [int(v) for v in a.particles.split(",")]:
        f = R.Filter(n, 1.0, 0.5, 0.7, 0.5, 1, clamp=False)
        t0 = time.perf_counter()
        for y in obs[:a.host_steps]:
            f.step(float(y))
        host_s = (time.perf_counter() - t0) / max(1, min(T, a.host_steps))
        for B in [int(v) for v in a.filters.split(",")]:
            row = dict(particles=n, filters=B, steps=T, reps=a.reps, steps_per_launch=PF.steps_per_launch(n), host_filter_steps_per_s=1.0 / host_s,
                       host_particle_steps_per_s=n / host_s)
            with PF.ParticleFilterBank(n, 1.0, 0.5, 0.7, 0.5, np.arange(B, dtype=np.uint64) + 1) as bank:
                row["run_ms"] = median_ms(lambda: bank.run(obs), a.reps)
                row["filter_steps_per_s"] = B * T / (row["run_ms"] * 1e-3)
                row["particle_steps_per_s"] = row["filter_steps_per_s"] * n
                row["steps_ms"] = median_ms(lambda: [bank.step(float(y), record=False) for y in obs], a.reps)
                row["step_recorded_ms"] = median_ms(lambda: bank.step(float(obs[0])), a.reps)
            print("n=%d B=%d T=%d: run %.2f ms = %.3g filter-steps/s, %.3g particle-steps/s; as %d step calls %.1f ms; one recorded step %.2f ms; host restatement %.3g "
                  "filter-steps/s" % (n, B, T, row["run_ms"], row["filter_steps_per_s"], row["particle_steps_per_s"], T, row["steps_ms"], row["step_recorded_ms"],
                                      row["host_filter_steps_per_s"]), flush=True)
            rows.append(row)
    line = json.dumps(rows)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
