"""Log-joint surfaces on one MI355X: the fused path (k_grid_eval and the reductions of fg_grid.hip behind `Engine.grid`) against the same
surfaces composed from the parent API -- host-built trace cells, `Engine.set_values`, `Engine.log_joint` -- on an engine sized to the grid.

    python tools/bench_grid.py [--shapes 128x128x1,128x128x256,128x128x4096,2048x2048x1] [--models readme,refmodel8,logistic] [--reps 3] [--out FILE]

A shape is n_a x n_b x bases; a model run is one cell of one base.  Per (model, shape), medians of whole calls on the host clock, every
call ending in a device synchronise, every shape warmed first, the two paths alternating inside one process:
    fused_ms          `grid.eval(0, bases, keep=False)`: scoring, the per-base reductions, the mixture, the n_a + n_b + 6 words per base
                      copied back; nothing of size cells x bases leaves the device
    score_only_ms     the same call with FG_GRID_REDUCE=0 (no reduction kernel, nothing copied back): reduce_share = 1 - score_only / fused
    fused_table_ms    `grid.eval(0, bases)`: the same plus the table [bases][n_b][n_a] through a device buffer to the host (tables up to 256 MiB)
    composed_ms       the cells [S][chains] built with numpy, uploaded (8 S bytes a model run) and scored in engines of at most 2^22 chains;
                      the surface is the sum of the three accumulators on the host.  No normaliser, marginal or mode: those would be numpy's.
`readme` has one f64 site: both axes name it (the second wins, grid.rs:52-57), which scores as many model runs.  No threshold is attached
to any of these figures.  Without a GPU the script fails (no fallback)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fugue_amd import engine as E, workloads as W   # noqa: E402

COMPOSED_CHAINS = 1 << 22
MODELS = {
    "readme": lambda: W.readme_normal(),
    "refmodel8": lambda: W.reference_model(8),
    "logistic": lambda: W.logistic_regression(*W.classification_data()[:2]),
}


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


def composed(ref, values, n_bases, ja, a, jb, b):
    """every surface of the bases from the parent commit's API -> [n_bases][n_b][n_a]"""
    n_a, n_b = a.size, b.size
    cells, total = n_a * n_b, n_a * n_b * n_bases
    out = np.empty(total)
    ab, bb = bits(a), bits(b)
    for start in range(0, total, ref.C):
        idx = np.arange(start, min(total, start + ref.C))
        cell = idx % cells
        cols = np.empty((values.shape[0], ref.C), dtype=np.int64)
        cols[:, :idx.size] = values[:, idx // cells]
        cols[:, idx.size:] = values[:, :1]
        cols[ja, :idx.size] = ab[cell % n_a]
        cols[jb, :idx.size] = bb[cell // n_a]
        ref.set_values(cols)
        acc = ref.log_joint()
        out[idx] = ((acc[0] + acc[1]) + acc[2])[:idx.size]
    return out.reshape(n_bases, n_b, n_a)


def timed(call):
    t0 = time.perf_counter()
    r = call()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="128x128x1,128x128x256,128x128x4096,2048x2048x1")
    ap.add_argument("--models", default="readme,refmodel8,logistic")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a_ = ap.parse_args()
    rows = []
    for name in a_.models.split(","):
        cp = E.compile_model(MODELS[name]())
        ja = cp.f64_sites[0]
        jb = cp.f64_sites[1] if cp.d > 1 else ja
        for shape in a_.shapes.split(","):
            n_a, n_b, n_bases = (int(v) for v in shape.split("x"))
            runs = n_a * n_b * n_bases
            a, b = np.linspace(-2.0, 2.0, n_a), np.linspace(-1.5, 2.5, n_b)
            eng = E.Engine(cp, n_bases, seed=1)
            ref = E.Engine(cp, min(runs, COMPOSED_CHAINS), seed=1)
            eng.prior_init()
            values = eng.get_values().copy()
            g = eng.grid(ja, a, jb, b)
            os.environ["FG_GRID_REDUCE"] = "0"
            g0 = eng.grid(ja, a, jb, b)
            del os.environ["FG_GRID_REDUCE"]
            table = runs * 8 <= (256 << 20)
            reps_c = a_.reps if runs < (1 << 24) else 1
            g.eval(0, n_bases, keep=False); g0.eval(0, n_bases, keep=False)                       # warm-up of every path's shapes
            comp = composed(ref, values, min(n_bases, 2), ja, a, jb, b)
            t_f, t_s, t_t, t_c = [], [], [], []
            for rep in range(a_.reps):
                t_f.append(timed(lambda: g.eval(0, n_bases, keep=False))[0])
                t_s.append(timed(lambda: g0.eval(0, n_bases, keep=False))[0])
                if table:
                    ms, lj = timed(lambda: g.eval(0, n_bases))
                    t_t.append(ms)
                if rep < reps_c:
                    ms, comp = timed(lambda: composed(ref, values, n_bases, ja, a, jb, b))
                    t_c.append(ms)
            same = bool(np.array_equal(lj, comp, equal_nan=True)) if table else None
            g.close(); g0.close(); eng.close(); ref.close()
            f, s, c = statistics.median(t_f), statistics.median(t_s), statistics.median(t_c)
            row = dict(model=name, sites=cp.S, n_a=n_a, n_b=n_b, bases=n_bases, model_runs=runs, fused_ms=f, fused_runs_per_s=runs / (f * 1e-3), score_only_ms=s,
                       reduce_share=1.0 - s / f, fused_table_ms=statistics.median(t_t) if table else None, composed_ms=c, composed_runs_per_s=runs / (c * 1e-3),
                       composed_over_fused=c / f, composed_reps=reps_c, same_bits=same)
            print("%-9s %4d x %4d x %4d: fused %9.2f ms = %.3g runs/s (score only %9.2f ms, reductions %4.1f%%)%s; composed %10.1f ms = %.3g runs/s; x%.1f%s"
                  % (name, n_a, n_b, n_bases, f, row["fused_runs_per_s"], s, 100.0 * row["reduce_share"], "; with the table %.2f ms" % row["fused_table_ms"] if table else "",
                     c, row["composed_runs_per_s"], c / f, "" if same is None else "; same bits: %s" % same), flush=True)
            rows.append(row)
    line = json.dumps(rows)
    print(line)
    if a_.out:
        os.makedirs(os.path.dirname(os.path.abspath(a_.out)), exist_ok=True)
        with open(a_.out, "w") as f_:
            f_.write(line + "\n")


if __name__ == "__main__":
    main()
