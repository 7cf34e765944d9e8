"""Times the chunked diagnostics (fg_diag_stream.hip) next to the stored-draws call, on the GPU:

    python tools/bench_diag_stream.py [--chains 65536] [--d 32] [--chunk 64] [--n 256] [--lags 64,256] [--reps 5] [--out FILE]

Per K: ms per `update` of one chunk [chunk][d][C] (host clock around all updates of a run of n draws, ended by a synchronise;
median over reps after one warm-up run), the bytes the pass has to move -- (K / 32 + 1) reads of the chunk plus the state traffic
(P read and written, head written once, ring read and written) -- and the GB/s that makes; then the read-out (`rhat_ess` on the
finished stream) and, beside it, `fg_diag_rhat_ess` on a stored buffer of the same n draws.  Draws are iid N(0, 1) from a seed."""
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
from fugue_amd import workloads as W    # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--chunk", type=int, default=64)
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--lags", default="64,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    C, d, chunk, n = a.chains, a.d, a.chunk, a.n
    assert n % chunk == 0
    eng = E.Engine(E.compile_model(W.normal_sites(1)), C, seed=1)
    row = d * C * 8
    buf = eng.device_alloc(n * row)
    rng = np.random.default_rng(11)
    for k in range(n // chunk):
        eng.upload(rng.standard_normal((chunk, d, C)), buf + k * chunk * row)
    res = dict(chains=C, d=d, chunk=chunk, n=n, chunk_bytes=chunk * row, runs=[])
    for K in [int(v) for v in a.lags.split(",")]:
        per_update, readout = [], []
        for rep in range(a.reps + 1):
            s = eng.diag_stream(n, d, K)
            eng.synchronize()
            t0 = time.perf_counter()
            for k in range(n // chunk):
                s.update(buf + k * chunk * row, chunk)
            eng.synchronize()
            t1 = time.perf_counter()
            r = s.rhat_ess()
            t2 = time.perf_counter()
            s.close()
            if rep:                                      # the first run warms up
                per_update.append((t1 - t0) * 1e3 / (n // chunk))
                readout.append((t2 - t1) * 1e3)
        ms = statistics.median(per_update)
        state = (2 * K + min(K, chunk) + 2 * min(K, chunk)) * row          # steady state: P in and out, ring in and out; head only at the start
        moved = (K // 32 + 1) * chunk * row + state
        res["runs"].append(dict(K=s.K, ms_per_update=ms, ms_per_update_all=per_update, bytes_per_update=moved, gb_per_s=moved / ms / 1e6,
                                state_bytes=(3 * s.K + 7) * row, ms_readout=statistics.median(readout),
                                r_hat_max=float(np.max(r["r_hat"])), ess_min=float(np.min(r["ess"]))))
    stored = []
    for rep in range(a.reps + 1):
        t0 = time.perf_counter()
        r = eng.diag_rhat_ess(buf, n, d)
        if rep:
            stored.append((time.perf_counter() - t0) * 1e3)
    res["stored"] = dict(ms_rhat_ess=statistics.median(stored), ms_all=stored, buffer_bytes=n * row, r_hat_max=float(np.max(r["r_hat"])), ess_min=float(np.min(r["ess"])))
    eng.device_free(buf)
    eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
