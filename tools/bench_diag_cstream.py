"""Times the discrete-site streams (fg_diag_cstream.hip) on the GPU:

    python tools/bench_diag_cstream.py [--chains 262144] [--rows 68] [--watch 64] [--k 4] [--chunk 16] [--reps 5] [--e2e] [--out FILE]

The shape is C5 (workloads.mixture: 4 means, 64 Categorical assignments): one uploaded chunk [chunk][rows][C] of cells whose first
rows - watch rows are f64 and whose last `watch` rows hold integers uniform over [0, k).  Per form -- the default (NARROW at k <= 8)
and FG_DIAG_CSTREAM_FORM=wide on the same input -- ms per `update` of the chunk (host clock around `reps` updates ended by a
synchronise, after one warm-up update; the median over 3 such regions) and the GB/s that makes of the bytes the kernel reads (the
watched rows).  Beside them `cells_f64` of the f64 rows (what the driver gathers) and of every row, and the yardstick: a
hipMemcpyDtoDAsync of as many bytes as the count kernel reads, timed the same way.

--e2e: `adaptive_mcmc_chain_summary` on a small C5 (8 192 chains, 256 samples, 64 warm-up steps) with and without discrete=True:
seconds and their ratio, and whether every membership table sums to n_samples x n_chains."""
import argparse
import ctypes
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

FG_F64, FG_USIZE = 0, 3


def timed(eng, fn, reps, regions=3):
    """ms per call of fn: one warm-up call, then the median over `regions` regions of `reps` calls each."""
    fn()
    eng.synchronize()
    out = []
    for _ in range(regions):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        eng.synchronize()
        out.append((time.perf_counter() - t0) * 1e3 / reps)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=262144)
    ap.add_argument("--rows", type=int, default=68)
    ap.add_argument("--watch", type=int, default=64)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--chunk", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--e2e", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    C, n_rec, nw, K, chunk = a.chains, a.rows, a.watch, a.k, a.chunk
    nf = n_rec - nw
    assert 0 <= nf and 1 <= nw
    chunk_bytes, read_bytes = chunk * n_rec * C * 8, chunk * nw * C * 8
    res = dict(chains=C, rows=n_rec, watched=nw, k=K, chunk=chunk, chunk_bytes=chunk_bytes, bytes_read_by_count=read_bytes)
    eng = E.Engine(E.compile_model(W.normal_sites(1)), C, seed=1)
    rng = np.random.default_rng(11)
    buf = eng.device_alloc(chunk_bytes)
    for t in range(chunk):                                    # one draw at a time: the host never holds the whole chunk
        cells = np.zeros((n_rec, C), dtype=np.int64)
        cells[:nf] = rng.standard_normal((nf, C)).view(np.int64)
        cells[nf:] = rng.integers(0, K, size=(nw, C))
        eng.upload(cells, buf + t * n_rec * C * 8)
    rows, vt = list(range(nf, n_rec)), [FG_USIZE] * nw
    reps_total = 1 + 3 * a.reps
    for form in ("default", "wide"):
        if form == "wide":
            os.environ["FG_DIAG_CSTREAM_FORM"] = "wide"
        s = eng.diag_cstream(reps_total * chunk, n_rec, rows, vt, [0] * nw, [K] * nw)
        ms, every = timed(eng, lambda: s.update(buf, chunk), a.reps)
        tab = s.result()
        s.close()
        os.environ.pop("FG_DIAG_CSTREAM_FORM", None)
        ok = all(int(c.sum()) == reps_total * chunk * C for c in tab["counts"])
        res[form] = dict(ms_per_chunk=ms, ms_all=every, gb_per_s=read_bytes / ms / 1e6, tables_complete=ok, counts_row_0=tab["counts"][0].tolist())
    # the gathers of the same chunk
    if nf:
        out = eng.device_alloc(chunk * nf * C * 8)
        ms, every = timed(eng, lambda: eng.cells_f64(buf, chunk, n_rec, list(range(nf)), [FG_F64] * nf, out=out), a.reps)
        res["cells_f64_f64_rows"] = dict(rows=nf, ms_per_chunk=ms, ms_all=every, gb_per_s=2 * chunk * nf * C * 8 / ms / 1e6)
        eng.device_free(out)
    out = eng.device_alloc(chunk_bytes)
    every_vt = [FG_F64] * nf + vt
    ms, every = timed(eng, lambda: eng.cells_f64(buf, chunk, n_rec, list(range(n_rec)), every_vt, out=out), a.reps)
    res["cells_f64_every_row"] = dict(rows=n_rec, ms_per_chunk=ms, ms_all=every, gb_per_s=2 * chunk_bytes / ms / 1e6)
    # the yardstick: a device-to-device copy of as many bytes as the count kernel reads, on the engine's stream
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpyDtoDAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    stream = E.lib().fg_engine_stream(eng.h)

    def copy():
        rc = hip.hipMemcpyDtoDAsync(out, buf, read_bytes, stream)
        assert rc == 0, rc

    ms, every = timed(eng, copy, a.reps)
    res["memcpy_dtod"] = dict(bytes=read_bytes, ms=ms, ms_all=every, gb_per_s_read=read_bytes / ms / 1e6)
    eng.device_free(out)
    eng.device_free(buf)
    eng.close()
    if a.e2e:
        data, _ = W.mixture_data(64)
        kw = dict(seed=7, n_samples=256, n_warmup=64, n_chains=8192, chunk=chunk, max_lag=256)
        cp = E.compile_model(W.mixture(data, K=4))
        for flag in (False, True):                                # warm-up: whatever is compiled at run time
            I.adaptive_mcmc_chain_summary(model_fn=cp, discrete=flag, **dict(kw, n_samples=16, n_warmup=4))
        t0 = time.perf_counter()
        plain = I.adaptive_mcmc_chain_summary(model_fn=cp, **kw)
        t1 = time.perf_counter()
        disc = I.adaptive_mcmc_chain_summary(model_fn=cp, discrete=True, **kw)
        t2 = time.perf_counter()
        d = disc.discrete
        res["e2e"] = dict(kw, s_without=t1 - t0, s_with=t2 - t1, ratio=(t2 - t1) / (t1 - t0), discrete_sites=len(d.sites),
                          tables_sum_to_draws=bool(all(int(c.sum()) == 256 * 8192 for c in d.counts)),
                          same_f64_figures=bool(all(np.array_equal(getattr(plain, k), getattr(disc, k)) for k in ("mean", "std", "r_hat", "ess"))),
                          probs_z0=d.probs()[0].tolist())
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
