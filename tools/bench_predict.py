"""Times the predictive kernel (fg_predict.hip: k_predict_eval behind `Engine.predict_eval`) on the GPU:

    python tools/bench_predict.py [--chains 65536,8192] [--reps 5] [--out FILE]

One chunk of draws [draws][d][C] in the HMC draw layout is uploaded once per shape.  Shapes:
    readme        mu ~ N(0, 1), y ~ N(mu, 0.5): 1 row in, 1 replicate out per draw and chain                      (64 draws)
    readme+ll     the same with the pointwise log-likelihood table as a second output
    reg32x1024    32 coefficients, 1 024 observations y#i ~ N(sum_j beta#j x_ij, 0.5); sel = 16 rows / all rows  (4 draws)
    pois_gamma    rate ~ Gamma, shape ~ Gamma; 8 Poisson(rate) and 8 Gamma(shape, 1.5) observes: rejection samplers (64 draws)
Per shape and chain count: microseconds per chunk (host clock around `reps` calls ended by one synchronise, after 2 warm-up calls;
median of 3 such windows), the bytes the streaming bound counts -- 8 (rows read + tables' rows written) per draw and chain -- and that
time as a multiple of a plain device-to-device copy that moves the same number of bytes (half read, half written), measured in the
same process.  Beside it the host route of tests/test_gpu_reference_integration.py:78-79 on the same draws: download, then numpy's
generators (seconds, once)."""
import argparse
import ctypes as C
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


def regression(p=32, n_obs=1024):
    X, y, _ = W.ridge_data(n_obs, p)
    return W.ridge_regression(X, y), np.asarray(X)


def pois_gamma():
    P = M.Program()
    rate = P.sample(M.addr("rate"), M.Gamma(2.0, 1.0))
    shape = P.sample(M.addr("shape"), M.Gamma(3.0, 2.0))
    for i in range(8):
        P.observe(M.addr("count", i), M.Poisson(rate), 2)
    for i in range(8):
        P.observe(M.addr("wait", i), M.Gamma(shape, 1.5), 1.0 + 0.1 * i)
    return P


def _hip():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            h = C.CDLL(name)
            h.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
            return h
        except OSError:
            continue
    raise RuntimeError("libamdhip64.so not found")


def copy_us(eng, nbytes, reps):
    """A device-to-device copy on the engine's stream that moves nbytes in all (nbytes / 2 read, nbytes / 2 written): microseconds,
    median of 3 windows."""
    hip, half = _hip(), max(8, nbytes // 2)
    src, dst = eng.device_alloc(half), eng.device_alloc(half)
    stream = E.lib().fg_engine_stream(eng.h)

    def copy():
        rc = hip.hipMemcpyDtoDAsync(dst, src, half, stream)
        assert rc == 0, rc
    for _ in range(2):
        copy()
    eng.synchronize()
    w = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            copy()
        eng.synchronize()
        w.append((time.perf_counter() - t0) * 1e6 / reps)
    eng.device_free(src)
    eng.device_free(dst)
    return statistics.median(w)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", default="65536,8192")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    reg_prog, X = regression()
    shapes = [  # name, program, draws, selection, pointwise, positive draws, host route
        ("readme", W.readme_normal(), 64, None, False, False, lambda dr, g: dr[:, 0] + 0.5 * g.standard_normal(dr[:, 0].shape)),
        ("readme+ll", W.readme_normal(), 64, None, True, False, None),
        ("reg32x1024 sel=16", reg_prog, 4, list(range(0, 1024, 64)), False, False,
         lambda dr, g: np.einsum("ij,tjc->tic", X[0:1024:64], dr) + 0.5 * g.standard_normal((dr.shape[0], 16, dr.shape[2]))),
        ("reg32x1024 all", reg_prog, 4, None, False, False,
         lambda dr, g: np.einsum("ij,tjc->tic", X, dr) + 0.5 * g.standard_normal((dr.shape[0], 1024, dr.shape[2]))),
        ("pois_gamma", pois_gamma(), 64, None, False, True,
         lambda dr, g: (g.poisson(np.broadcast_to(dr[:, 0][:, None], (dr.shape[0], 8, dr.shape[2]))), g.gamma(np.broadcast_to(dr[:, 1][:, None], (dr.shape[0], 8, dr.shape[2])), 1.0 / 1.5))),
    ]
    res = dict(reps=a.reps, rows=[])
    for C in (int(c) for c in a.chains.split(",")):
        for name, prog, n, sel, ll, positive, host in shapes:
            cp = E.compile_model(prog)
            n_sel = cp.O if sel is None else len(sel)
            g = np.random.default_rng(11)
            x = g.standard_normal((n, cp.d, C))
            if positive:
                x = np.exp(0.5 * x)
            eng = E.Engine(cp, C, seed=1)
            buf = eng.upload(x)
            out = eng.device_alloc(n * n_sel * C * 8)
            lbuf = eng.device_alloc(n * n_sel * C * 8) if ll else False
            call = lambda: eng.predict_eval(buf, n, sel=sel, out=out, loglik=lbuf)
            for _ in range(2):
                call()
            eng.synchronize()
            windows = []
            for _ in range(3):
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    call()
                eng.synchronize()
                windows.append((time.perf_counter() - t0) * 1e6 / a.reps)
            us = statistics.median(windows)
            nbytes = 8 * (cp.d + n_sel * (2 if ll else 1)) * n * C
            cus = copy_us(eng, nbytes, a.reps)
            host_s = None
            if host is not None:
                t0 = time.perf_counter()
                host(eng.download(buf, (n, cp.d, C)), np.random.default_rng(42))
                host_s = time.perf_counter() - t0
            row = dict(chains=C, shape=name, draws=n, observes=cp.O, n_sel=n_sel, instructions=cp.n_instructions, n_slots=cp.n_slots, us_per_chunk=us, us_windows=windows,
                       bytes=nbytes, gb_per_s=nbytes / us / 1e3, copy_us_same_bytes=cus, times_the_copy=us / cus,
                       ns_per_replicate=us * 1e3 / (n * cp.O * C), host_route_s=host_s, speedup_over_host_route=None if host_s is None else host_s / (us * 1e-6))
            res["rows"].append(row)
            print("%-20s C=%-6d draws=%-3d O=%-5d sel=%-5d %10.1f us/chunk  %8.1f MB  copy %8.1f us  x%-8.1f %6.3f ns/replicate  host %s" % (
                name, C, n, cp.O, n_sel, us, nbytes / 1e6, cus, us / cus, row["ns_per_replicate"], "-" if host_s is None else "%.3f s (x%.0f)" % (host_s, row["speedup_over_host_route"])), flush=True)
            eng.device_free(buf)
            eng.device_free(out)
            if lbuf:
                eng.device_free(lbuf)
            eng.close()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
