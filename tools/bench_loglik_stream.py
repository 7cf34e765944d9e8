"""Times the log-likelihood stream (fg_loglik_stream.hip: k_loglik_stream_update behind `LoglikStream.update`) on the GPU:

    python tools/bench_loglik_stream.py [--chains 65536] [--chunk 16] [--n-sel 64] [--reps 5] [--out FILE]

One chunk of the pointwise log-likelihood [chunk][n_sel][C] is made by `Engine.predict_eval` (a regression with 8 coefficients and
n_sel observations, loglik only) from draws uploaded once.  Reported, each the median of 3 windows of `reps` calls ended by one
synchronise (host clock, after 2 warm-up calls):
    update_ms        one `LoglikStream.update` of the chunk (two exp and the moment sums per cell; reads the chunk once, reads and
                     writes 80 bytes of state per column)
    copy_ms          a device-to-device copy of the same chunk (chunk bytes read, chunk bytes written): the streaming yardstick
    predict_eval_ms  the `predict_eval` call that produced the chunk
    result_ms        one read-out (the pooling tree, two levels at C = 65 536, and the download), once
No threshold: the copy and predict_eval are the yardsticks."""
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
from fugue_amd import workloads as W    # noqa: E402


def _hip():
    for name in ("libamdhip64.so", "/opt/rocm/lib/libamdhip64.so"):
        try:
            h = C.CDLL(name)
            h.hipMemcpyDtoDAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
            return h
        except OSError:
            continue
    raise RuntimeError("libamdhip64.so not found")


def timed(eng, call, reps):
    for _ in range(2):
        call()
    eng.synchronize()
    w = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        eng.synchronize()
        w.append((time.perf_counter() - t0) * 1e3 / reps)
    return statistics.median(w), w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=65536)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--n-sel", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    Cn, n, n_sel = a.chains, a.chunk, a.n_sel
    X, y, _ = W.ridge_data(n_sel, 8)
    cp = E.compile_model(W.ridge_regression(X, y))
    assert cp.O == n_sel
    eng = E.Engine(cp, Cn, seed=1)
    draws = eng.upload(np.random.default_rng(11).standard_normal((n, cp.d, Cn)))
    nbytes = n * n_sel * Cn * 8
    ll, dst = eng.device_alloc(nbytes), eng.device_alloc(nbytes)
    calls = 2 + 3 * a.reps
    stream = eng.loglik_stream(n * calls, n_sel)
    hip, hstream = _hip(), E.lib().fg_engine_stream(eng.h)

    def copy():
        rc = hip.hipMemcpyDtoDAsync(dst, ll, nbytes, hstream)
        assert rc == 0, rc

    pe_ms, pe_w = timed(eng, lambda: eng.predict_eval(draws, n, out=False, loglik=ll), a.reps)
    up_ms, up_w = timed(eng, lambda: stream.update(ll, n), a.reps)
    cp_ms, cp_w = timed(eng, copy, a.reps)
    t0 = time.perf_counter()
    res = stream.result()
    result_ms = (time.perf_counter() - t0) * 1e3
    cells = n * n_sel * Cn
    row = dict(chains=Cn, chunk=n, n_sel=n_sel, reps=a.reps, chunk_bytes=nbytes, state_bytes=80 * n_sel * Cn, update_ms=up_ms, update_windows=up_w,
               copy_ms=cp_ms, copy_windows=cp_w, predict_eval_ms=pe_ms, predict_eval_windows=pe_w, result_ms=result_ms,
               update_ns_per_cell=up_ms * 1e6 / cells, update_times_the_copy=up_ms / cp_ms, update_over_predict_eval=up_ms / pe_ms,
               elpd_loo_total=float(np.sum(res["elpd_loo"])), min_is_ess=float(np.min(res["is_ess"])))
    print("C=%d chunk=%d n_sel=%d: update %.3f ms (%.4f ns/cell), copy %.3f ms (x%.2f), predict_eval %.3f ms, result %.3f ms" % (
        Cn, n, n_sel, up_ms, row["update_ns_per_cell"], cp_ms, up_ms / cp_ms, pe_ms, result_ms), flush=True)
    stream.free()
    for b in (draws, ll, dst):
        eng.device_free(b)
    eng.close()
    line = json.dumps(row)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
