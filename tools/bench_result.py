"""Times the result kernel (fg_result.hip: k_result_eval behind `Engine.result_eval`) on the GPU:

    python tools/bench_result.py [--chains 65536,8192] [--d 32] [--draws 64] [--reps 20] [--out FILE]

Model: normal_sites(d).  One chunk of iid N(0, 1) draws [draws][d][C] in the HMC draw layout is uploaded once.  Three result sets:
    exp1     one result, exp of one site                      (1 row in, 1 result out per draw and chain)
    lin32    one result, a d-term linear predictor            (d rows in, 1 out)
    mixed8   eight results: four exps, four d-term predictors (d rows in, 8 out)
Per set and chain count: ms per call (host clock around `reps` calls ended by one synchronise, after 3 warm-up calls; median of 5
such windows), the bytes the streaming bound counts -- 8 (rows read + R) per draw and chain -- the GB/s that makes, and the share of
the measured HBM copy rate (6.29 TB/s, MI355X float4 copy) that is.  Beside it the route without the kernel: downloading the chunk
and evaluating the same expressions in numpy (seconds, once), with the largest relative difference between the two."""
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
from fugue_amd import model as M        # noqa: E402
from fugue_amd import workloads as W    # noqa: E402

HBM_COPY_BYTES_PER_S = 6.29e12


def result_sets(prog, d):
    x = [M.Expr("site", a=h) for h in range(prog.n_samples)]

    def lin(shift):
        e = M.as_expr(0.25 + shift)
        for j in range(d):
            e = e + x[j] * (0.5 + 0.03125 * ((j + shift) % 7))
        return e
    return {"exp1": [M.exp(x[0])], "lin32": [lin(0)], "mixed8": [M.exp(x[j]) for j in range(4)] + [lin(s) for s in range(1, 5)]}


def host_route(name, draws, order, d):
    """The same results from downloaded draws [n][d][C] in numpy; order[h] = coordinate of handle h."""
    col = lambda h: draws[:, order[h]]

    def lin(shift):
        e = np.full(draws[:, 0].shape, 0.25 + shift)
        for j in range(d):
            e = e + col(j) * (0.5 + 0.03125 * ((j + shift) % 7))
        return e
    if name == "exp1":
        return np.stack([np.exp(col(0))], axis=1)
    if name == "lin32":
        return np.stack([lin(0)], axis=1)
    return np.stack([np.exp(col(j)) for j in range(4)] + [lin(s) for s in range(1, 5)], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="65536,8192")
    ap.add_argument("--d", type=int, default=32)
    ap.add_argument("--draws", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    d, n = a.d, a.draws
    res = dict(d=d, draws=n, reps=a.reps, hbm_copy_bytes_per_s=HBM_COPY_BYTES_PER_S, rows=[])
    for C in (int(c) for c in a.chains.split(",")):
        x = np.random.default_rng(11).standard_normal((n, d, C))
        for name in ("exp1", "lin32", "mixed8"):
            prog = W.normal_sites(d)
            prog.result = result_sets(prog, d)[name]
            cp = E.compile_model(prog)
            order = {h: cp.f64_sites.index(cp.site_of_handle(h)) for h in range(prog.n_samples)}
            eng = E.Engine(cp, C, seed=1)
            buf = eng.upload(x)
            out = eng.device_alloc(n * cp.R * C * 8)
            for _ in range(3):
                eng.result_eval(buf, n, out=out)
            eng.synchronize()
            windows = []
            for _ in range(5):
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    eng.result_eval(buf, n, out=out)
                eng.synchronize()
                windows.append((time.perf_counter() - t0) * 1e3 / a.reps)
            ms = statistics.median(windows)
            nbytes = 8 * (len(cp.result_sites) + cp.R) * n * C
            t0 = time.perf_counter()
            host = host_route(name, eng.download(buf, (n, d, C)), order, d)
            host_s = time.perf_counter() - t0
            dev = eng.download(out, (n, cp.R, C))
            with np.errstate(all="ignore"):
                rel = float(np.nanmax(np.abs(dev - host) / np.abs(host)))
            res["rows"].append(dict(chains=C, results=name, R=cp.R, rows_read=len(cp.result_sites),
                                    ms_per_call=ms, ms_windows=windows, bytes=nbytes, gb_per_s=nbytes / ms / 1e6,
                                    share_of_hbm_copy_rate=nbytes / (ms * 1e-3) / HBM_COPY_BYTES_PER_S, host_route_s=host_s,
                                    speedup_over_host_route=host_s / (ms * 1e-3), max_rel_diff_vs_numpy=rel))
            eng.device_free(buf)
            eng.device_free(out)
            eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
