"""Times Pareto-smoothed LOO on a stored table (`Engine.psis_loo`, fg_psis.hip) on the GPU:

    python tools/bench_psis.py [--reps 5] [--out FILE]

at n_sel = 16, n = 64, C = 65 536 (S = 4.2e6 pooled draws per statement, M = 6 144) and at n_sel = 1 024, n = 16, C = 4 096 (S = 65 536,
M = 768): 537 MB of table each, uploaded once draw by draw.  Each call is made once to warm up, then `reps` times; the figures are
medians of whole calls on the host clock (every call ends in a download or a synchronisation), with no other process on the device:
    copy_ms     a device copy of the same table (`cells_f64` with f64 tags: every cell read once and written once): the yardstick
    loglik_ms   the log-likelihood stream's update on the table as one chunk, with its read-out (WAIC / raw IS-LOO)
    psis_ms     `Engine.psis_loo`: six radix passes and the collect pass over the table, then the fit
    table_bytes, and each of the above as GB/s of the table (`*_table_gbs`: table_bytes over the time, not the traffic)
One JSON line per shape.  No threshold: nothing exists to compare the call to but the copy rate."""
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

SHAPES = ((16, 64, 65536), (1024, 16, 4096))          # n_sel, n, C


def median_ms(call, reps):
    call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def one(n_sel, n, C, reps, seed):
    rng = np.random.default_rng(seed)
    row = dict(n_sel=n_sel, n=n, C=C, reps=reps, table_bytes=n * n_sel * C * 8)
    eng = E.Engine(E.compile_model(W.normal_sites(1)), C, seed=seed)
    d_x, d_y = eng.device_alloc(row["table_bytes"]), eng.device_alloc(row["table_bytes"])
    for t in range(n):                                # uploaded draw by draw: the host never holds the table
        eng.upload(rng.normal(-3.0, 1.0, (n_sel, C)), d_x + t * n_sel * C * 8)
    res = {}

    def copy():
        eng.cells_f64(d_x, n, n_sel, list(range(n_sel)), [M.F64] * n_sel, out=d_y)
        eng.synchronize()

    def loglik():
        s = eng.loglik_stream(n, n_sel)
        try:
            s.update(d_x, n)
            s.result()
        finally:
            s.free()

    def psis():
        res["psis"] = eng.psis_loo(d_x, n, n_sel)

    row["copy_ms"], row["loglik_ms"], row["psis_ms"] = median_ms(copy, reps), median_ms(loglik, reps), median_ms(psis, reps)
    for k in ("copy", "loglik", "psis"):
        row[k + "_table_gbs"] = row["table_bytes"] / (row[k + "_ms"] * 1e-3) / 1e9
    r = res["psis"]
    row.update(tail_len=int(r["tail_len"][0]), n_fitted=int((r["status"] == 0).sum()), khat_mean=float(np.mean(r["khat"])), khat_max=float(np.max(r["khat"])))
    eng.device_free(d_x)
    eng.device_free(d_y)
    eng.close()
    print("n_sel=%d n=%d C=%d (%.0f MB, M=%d): copy %.2f ms; loglik stream %.2f ms; psis_loo %.2f ms (%.1f x the copy); khat mean %.3f" % (
        n_sel, n, C, row["table_bytes"] / 1e6, row["tail_len"], row["copy_ms"], row["loglik_ms"], row["psis_ms"], row["psis_ms"] / row["copy_ms"], row["khat_mean"]), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [json.dumps(one(n_sel, n, C, a.reps, a.seed)) for n_sel, n, C in SHAPES]
    for line in lines:
        print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
