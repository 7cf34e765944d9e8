"""Times the streamed quantile selector (fg_diag_qstream.hip) on the GPU:

    python tools/bench_diag_qstream.py [--chains 65536] [--d 32] [--chunk 64] [--n 256] [--capacity 65536] [--reps 3] [--e2e N_SAMPLES] [--out FILE]

Uploaded iid N(0, 1) draws [n][d][C] are presented to a stream pass after pass until it is done.  Per pass: ms per `update` of one
chunk [chunk][d][C] (host clock around all updates of the pass, ended by a synchronise; median over reps after one warm-up run),
the GB/s that makes of the chunk's bytes, and the ms of `end_pass` (counters and collected keys to the host, the planner's step).
With the defaults the passes are: a first histogram pass (one group per coordinate), a second histogram pass (up to five groups),
a collect pass.  Beside them, for the same chunk: `DiagStream.update` at K = 64 and `hmc_step(chunk)` of the headline model
(normal_sites(d), default HMC configuration, after 20 warm-up transitions).

--e2e N: `hmc_chain_summary` on normal_sites(d) with N samples, 20 warm-up transitions, with and without quantiles=True: seconds,
their ratio and the pass count."""
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
from fugue_amd import workloads as W    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--capacity", type=int, default=65536)
    ap.add_argument("--digit-bits", type=int, default=12)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--e2e", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    C, d, chunk, n = a.chains, a.d, a.chunk, a.n
    assert n % chunk == 0
    row = d * C * 8
    res = dict(chains=C, d=d, chunk=chunk, n=n, chunk_bytes=chunk * row, capacity=a.capacity, digit_bits=a.digit_bits)
    eng = E.Engine(E.compile_model(W.normal_sites(d)), C, seed=1)
    buf = eng.device_alloc(n * row)
    rng = np.random.default_rng(11)
    for k in range(n // chunk):
        eng.upload(rng.standard_normal((chunk, d, C)), buf + k * chunk * row)
    per_pass = {}
    for rep in range(a.reps + 1):
        s = eng.diag_qstream(n, d, digit_bits=a.digit_bits, capacity=a.capacity)
        done, p = False, 0
        while not done:
            eng.synchronize()
            t0 = time.perf_counter()
            for k in range(n // chunk):
                s.update(buf + k * chunk * row, chunk)
            eng.synchronize()
            t1 = time.perf_counter()
            done = s.end_pass()
            t2 = time.perf_counter()
            if rep:                                      # the first run warms up
                per_pass.setdefault(p, []).append(((t1 - t0) * 1e3 / (n // chunk), (t2 - t1) * 1e3))
            p += 1
        vals, sp = s.result()
        res["passes"], res["slot_passes_min_max"] = s.passes, [int(sp.min()), int(sp.max())]
        s.close()
    res["quantiles_coordinate_0"] = vals[0].tolist()
    res["qstream"] = []
    for p in sorted(per_pass):
        ms = statistics.median(v[0] for v in per_pass[p])
        res["qstream"].append(dict(pass_index=p + 1, ms_per_update=ms, ms_per_update_all=[v[0] for v in per_pass[p]], gb_per_s=chunk * row / ms / 1e6,
                                   ms_end_pass=statistics.median(v[1] for v in per_pass[p])))
    upd = []
    for rep in range(a.reps + 1):
        s = eng.diag_stream(n, d, 64)
        eng.synchronize()
        t0 = time.perf_counter()
        for k in range(n // chunk):
            s.update(buf + k * chunk * row, chunk)
        eng.synchronize()
        if rep:
            upd.append((time.perf_counter() - t0) * 1e3 / (n // chunk))
        s.close()
    res["diag_stream_K64_ms_per_update"] = statistics.median(upd)
    eng.hmc_init(E.hmc_config(), 20)
    eng.hmc_step(20)
    step = []
    for rep in range(a.reps + 1):
        eng.synchronize()
        t0 = time.perf_counter()
        eng.hmc_step(chunk, buf)
        eng.synchronize()
        if rep:
            step.append((time.perf_counter() - t0) * 1e3)
    res["hmc_step_chunk_ms"] = statistics.median(step)
    eng.device_free(buf)
    eng.close()
    if a.e2e:
        kw = dict(seed=7, model_fn=W.normal_sites(d), n_samples=a.e2e, n_warmup=20, n_chains=C, chunk=chunk)
        t0 = time.perf_counter()
        plain = I.hmc_chain_summary(**kw)
        t1 = time.perf_counter()
        quant = I.hmc_chain_summary(quantiles=True, quantile_capacity=a.capacity, **kw)
        t2 = time.perf_counter()
        res["e2e"] = dict(n_samples=a.e2e, s_without=t1 - t0, s_with=t2 - t1, ratio=(t2 - t1) / (t1 - t0), passes=quant.passes,
                          same_figures=bool(all(np.array_equal(getattr(plain, k), getattr(quant, k)) for k in ("mean", "std", "r_hat", "ess"))),
                          quantiles_site_0=quant.quantiles[0].tolist())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
