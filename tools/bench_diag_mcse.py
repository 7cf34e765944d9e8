"""Times the MCSE / ESS figures of the mean, the sd and quantiles (`Engine.diag_mcse`, fg_diag_mcse.hip) on the GPU:

    python tools/bench_diag_mcse.py [--reps 5] [--out FILE] [--small]

at n = 1 000, C = 65 536 (S = 6.6e7 pooled draws per coordinate) and at n = 200, C = 8 192 (S = 1.6e6) -- tools/bench_diag_rank.py's
shapes -- two coordinates of iid N(0, 1) draws each, uploaded once draw by draw, the probabilities (0.05, 0.5, 0.95); `--small` runs
the second shape only.  Each call is made once to warm up, then `reps` times; the figures are medians of whole calls on the host clock
(every call ends in a download), per coordinate, with no other process on the device:
    mcse_ms        `Engine.diag_mcse` (fg_diag_mcse): the plain figures, two sorts, the rows, the combination on the rows, the Beta rule
    transform_ms   `Engine.diag_mcse_transform` into a device buffer of the caller's: the two sorts, the rows and the gathers
    rank_ms        `Engine.diag_rank` of the same buffer in the same session: the call this one is measured against (its kernels are
                   the same code before and after fg_diag_mcse.hip was added)
    plain_ms       `Engine.diag_rhat_ess` of the raw draws
The split of a call comes from a child process of this tool under `rocprofv3 --kernel-trace` (kernel time per coordinate, summed over
the launches of one call): key_ms (k_rank_keys), rows_ms (k_mcse_rows: the rows and the folded key pass), radix_ms (k_rank_count,
k_rank_scan, k_rank_scatter), gather_ms (k_mcse_gather), combine_ms (the kernels of fg_diag_rhat_ess, raw draws and rows).
One JSON line per shape.  No threshold: nobody had measured these numbers."""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((1000, 65536), (200, 8192))          # n, C
D = 2
PROBS = (0.05, 0.5, 0.95)
GROUPS = (("key_ms", ("k_rank_keys",)), ("rows_ms", ("k_mcse_rows",)), ("radix_ms", ("k_rank_count", "k_rank_scan", "k_rank_scatter")), ("gather_ms", ("k_mcse_gather",)),
          ("combine_ms", ("k_diag_",)))


def median_ms(call, reps):
    call()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def setup(n, C, seed):
    from fugue_amd import engine as E, workloads as W
    rng = np.random.default_rng(seed)
    eng = E.Engine(E.compile_model(W.normal_sites(1)), C, seed=seed)
    d_x = eng.device_alloc(n * D * C * 8)
    for t in range(n):                                # uploaded draw by draw: the host never holds the table
        eng.upload(rng.normal(size=(D, C)), d_x + t * D * C * 8)
    return eng, d_x


def child(n, C, reps, seed):
    """what the profiled process runs: the warm call and `reps` calls of diag_mcse"""
    eng, d_x = setup(n, C, seed)
    for _ in range(reps + 1):
        eng.diag_mcse(d_x, n, D, probs=PROBS)
    eng.device_free(d_x)
    eng.close()


def split(n, C, reps, seed):
    """kernel time per coordinate of one call, by group, from a child under rocprofv3; {} when the profiler is missing"""
    prof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if not prof:
        return {}
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([prof, "--kernel-trace", "--output-format", "csv", "-d", tmp, "--", sys.executable, os.path.abspath(__file__), "--child", str(n), str(C), "--reps", str(reps), "--seed", str(seed)],
                           capture_output=True, text=True)
        if r.returncode != 0:
            print("the profiled child failed:\n" + r.stderr[-1500:])
            return {}
        tot = {k: 0.0 for k, _ in GROUPS}
        for f in glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(f)):
                for k, names in GROUPS:
                    if any(nm in row["Kernel_Name"] for nm in names):
                        tot[k] += (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-6
    return {k: v / ((reps + 1) * D) for k, v in tot.items()}


def one(n, C, reps, seed, pre):
    row = dict(n=n, C=C, d=D, S=n * C, reps=reps, probs=list(PROBS))
    eng, d_x = setup(n, C, seed)
    d_out = eng.device_alloc(n * (2 + len(PROBS)) * C * 8)
    res = {}

    def mcse():
        res["mcse"] = eng.diag_mcse(d_x, n, D, probs=PROBS)

    def transform():
        for j in range(D):
            eng.diag_mcse_transform(d_x, n, D, res["mcse"]["mean"][j:j + 1], j0=j, n_j=1, probs=PROBS, d_out=d_out)

    def rank():
        res["rank"] = eng.diag_rank(d_x, n, D)

    def plain():
        res["plain"] = eng.diag_rhat_ess(d_x, n, D)

    row["mcse_ms"], row["transform_ms"], row["rank_ms"], row["plain_ms"] = (median_ms(f, reps) / D for f in (mcse, transform, rank, plain))
    r = res["mcse"]
    row.update(n_passes=int(r["n_passes"][0]), mcse_mean=float(r["mcse_mean"][0]), mcse_sd=float(r["mcse_sd"][0]), mcse_quantile=[float(v) for v in r["mcse_quantile"][0]],
               ess_quantile=[float(v) for v in r["ess_quantile"][0]])
    eng.device_free(d_out)
    eng.device_free(d_x)
    eng.close()
    row.update(pre)
    print("n=%d C=%d (S=%.3g): diag_mcse %.2f ms per coordinate (transform %.2f ms; %d radix passes); diag_rank %.2f ms; plain diag_rhat_ess %.2f ms; split %s" % (
        n, C, n * C, row["mcse_ms"], row["transform_ms"], row["n_passes"], row["rank_ms"], row["plain_ms"], {k: round(row[k], 3) for k, _ in GROUPS if k in row}), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--child", nargs=2, type=int, default=None, metavar=("N", "C"))
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.reps, a.seed)
        return
    shapes = SHAPES[1:] if a.small else SHAPES
    pre = [split(n, C, a.reps, a.seed) for n, C in shapes]          # the profiled children run before this process opens the device
    lines = [json.dumps(one(n, C, a.reps, a.seed, p)) for (n, C), p in zip(shapes, pre)]
    for line in lines:
        print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
