"""Times the posterior predictive check stream (fg_ppc_stream.hip: k_ppc_stream_stats and k_ppc_stream_update behind
`PpcStream.update`) on the GPU:

    python tools/bench_ppc.py [--chains 65536] [--chunk 16] [--rows 64] [--reps 5] [--out FILE]

One chunk of replicated data [chunk][rows][C] is made by `Engine.predict_eval` (a regression with 8 coefficients and `rows`
observations, cells only) from draws uploaded once.  Two forms of checks over it:
    one_check   one check over all rows with the five statistics (5 slots; the variance pass reads the chunk a second time)
    marginal    one check per row with the statistic "mean" (rows slots, K = 1)
Reported per form, each the median of 3 windows of `reps` calls ended by one synchronise (host clock, after 2 warm-up calls):
    update_ms             one `PpcStream.update` of the chunk
    update_times_the_copy update_ms over copy_ms, a device-to-device copy of the same chunk timed in the same process (chunk bytes
                          read, chunk bytes written): the streaming yardstick, not the code under test
    implied_bytes_per_cell  16 x that ratio: the bytes per 8-byte cell the update would move if it ran at the copy's rate
    model_bytes_per_cell  what DESIGN 3.17 counts: the cells read once (twice with the variance), the scratch table written and read,
                          2 x 48 bytes of state per (slot, chain) and piece
    pooled_ms             one read-out (the pooling tree and the download), once
No threshold: the copy is the yardstick."""
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
    ap.add_argument("--rows", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    Cn, n, rows = a.chains, a.chunk, a.rows
    X, y, _ = W.ridge_data(rows, 8)
    cp = E.compile_model(W.ridge_regression(X, y))
    assert cp.O == rows and all(v is not None for v in cp.observe_values)
    eng = E.Engine(cp, Cn, seed=1)
    draws = eng.upload(np.random.default_rng(11).standard_normal((n, cp.d, Cn)))
    nbytes = n * rows * Cn * 8
    yrep, dst = eng.device_alloc(nbytes), eng.device_alloc(nbytes)
    eng.predict_eval(draws, n, out=yrep, loglik=False)
    hip, hstream = _hip(), E.lib().fg_engine_stream(eng.h)

    def copy():
        rc = hip.hipMemcpyDtoDAsync(dst, yrep, nbytes, hstream)
        assert rc == 0, rc

    calls = 2 + 3 * a.reps
    cells = n * rows * Cn
    forms = dict(one_check=[(list(range(rows)), list(range(5)), cp.observe_values)],
                 marginal=[([k], [0], [cp.observe_values[k]]) for k in range(rows)])
    cp_ms, cp_w = timed(eng, copy, a.reps)
    lines = []
    for name, checks in forms.items():
        stream = eng.ppc_stream(n * calls, cp.observe_vtypes, checks)
        up_ms, up_w = timed(eng, lambda: stream.update(yrep, n), a.reps)
        t0 = time.perf_counter()
        res = stream.pooled()
        pooled_ms = (time.perf_counter() - t0) * 1e3
        n_slots, reads = stream.n_slots, 2 if name == "one_check" else 1
        pieces = -(-n // E.PPC_SCRATCH_DRAWS)
        model = (reads * cells * 8 + 2 * n * n_slots * Cn * 8 + pieces * 2 * 48 * n_slots * Cn) / cells
        row = dict(form=name, chains=Cn, chunk=n, rows=rows, n_slots=n_slots, reps=a.reps, chunk_bytes=nbytes, state_bytes=48 * n_slots * Cn, update_ms=up_ms,
                   update_windows=up_w, copy_ms=cp_ms, copy_windows=cp_w, copy_TB_per_s=2 * nbytes / cp_ms / 1e9, pooled_ms=pooled_ms,
                   update_times_the_copy=up_ms / cp_ms, implied_bytes_per_cell=16.0 * up_ms / cp_ms, model_bytes_per_cell=model,
                   model_ms_at_the_copy_rate=model * cells / (2 * nbytes / cp_ms), p_mid_first=float((2 * res["n_gt"][0] + res["n_eq"][0]) / (2.0 * n * calls * Cn)))
        print("%s: C=%d chunk=%d rows=%d slots=%d: update %.3f ms, copy %.3f ms (x%.2f), %.1f bytes/cell implied, %.1f by the model (%.3f ms), pooled %.3f ms" % (
            name, Cn, n, rows, n_slots, up_ms, cp_ms, up_ms / cp_ms, row["implied_bytes_per_cell"], model, row["model_ms_at_the_copy_rate"], pooled_ms), flush=True)
        stream.free()
        lines.append(json.dumps(row))
    for b in (draws, yrep, dst):
        eng.device_free(b)
    eng.close()
    for line in lines:
        print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
