"""Times the rank-normalised diagnostics (`Engine.diag_rank`, fg_diag_rank.hip) on the GPU:

    python tools/bench_diag_rank.py --build-yardstick        (no GPU: compiles tools/bin/rank_yardstick, if rocPRIM's headers are installed)
    python tools/bench_diag_rank.py [--reps 5] [--out FILE]  (on the GPU)

at n = 1 000, C = 65 536 (S = 6.6e7 pooled draws per coordinate) and at n = 200, C = 8 192 (S = 1.6e6), two coordinates of iid N(0, 1)
draws each, uploaded once draw by draw.  Each call is made once to warm up, then `reps` times; the figures are medians of whole calls
on the host clock (every call ends in a download), per coordinate, with no other process on the device:
    rank_ms        `Engine.diag_rank` (fg_diag_rank_rhat_ess): the transform and the combination
    transform_ms   `Engine.diag_rank_transform` into a device buffer of the caller's: the two sorts, the run passes and the scatters
    plain_ms       `Engine.diag_rhat_ess` of the raw draws of the same shape: the parent's cost of the plain figures
The split of a call comes from a child process of this tool under `rocprofv3 --kernel-trace` (kernel time per coordinate, summed
over the launches of one call): key_ms (k_rank_keys), radix_ms (k_rank_count, k_rank_scan, k_rank_scatter), run_ms (k_rank_runs,
k_rank_carry: the run pass with the normal scores and the scatters by cell index), combine_ms (the kernels of fg_diag_rhat_ess on the
transformed rows).  yardstick_ms: `rocprim::radix_sort_pairs` of S (u64, u32) pairs of the same keys, one sort (the transform runs
two), by tools/bin/rank_yardstick when it was built -- in the tool only; the library does not call rocPRIM.
One JSON line per shape.  No threshold: nobody had measured either number."""
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
YARD = os.path.join(ROOT, "tools", "bin", "rank_yardstick")
YARD_SRC = r"""
#include <string.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>
#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
int main(int argc, char **argv) {
    const size_t S = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 1u << 20;
    const int reps = argc > 2 ? std::atoi(argv[2]) : 5;
    std::vector<unsigned long long> k(S);
    std::vector<unsigned int> v(S);
    std::mt19937_64 g(42);
    std::normal_distribution<double> nd(0.0, 1.0);
    for (size_t i = 0; i < S; ++i) { const double x = nd(g); unsigned long long u; std::memcpy(&u, &x, 8); k[i] = (u >> 63) ? ~u : (u | 0x8000000000000000ull); v[i] = (unsigned int)i; }
    unsigned long long *ki, *ko; unsigned int *vi, *vo; void *tmp = nullptr; size_t tb = 0;
    CHECK(hipMalloc(&ki, S * 8)); CHECK(hipMalloc(&ko, S * 8)); CHECK(hipMalloc(&vi, S * 4)); CHECK(hipMalloc(&vo, S * 4));
    CHECK(hipMemcpy(ki, k.data(), S * 8, hipMemcpyHostToDevice)); CHECK(hipMemcpy(vi, v.data(), S * 4, hipMemcpyHostToDevice));
    CHECK(rocprim::radix_sort_pairs(tmp, tb, ki, ko, vi, vo, S));
    CHECK(hipMalloc(&tmp, tb));
    std::vector<double> ms;
    for (int r = 0; r <= reps; ++r) {
        CHECK(hipDeviceSynchronize());
        const auto t0 = std::chrono::steady_clock::now();
        CHECK(rocprim::radix_sort_pairs(tmp, tb, ki, ko, vi, vo, S));
        CHECK(hipDeviceSynchronize());
        if (r) ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    std::printf("%.6f\n", ms[ms.size() / 2]);
    return 0;
}
"""


def build_yardstick():
    from fugue_amd import build as B
    os.makedirs(os.path.dirname(YARD), exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "rank_yardstick.hip")
        with open(src, "w") as f:
            f.write(YARD_SRC)
        r = subprocess.run([B.hipcc(), "-O3", "-std=c++17", "--offload-arch=gfx950", "-x", "hip", src, "-o", YARD], capture_output=True, text=True)
    if r.returncode != 0:
        print("the yardstick did not compile (are rocPRIM's headers installed?): none will be reported\n" + r.stderr[-2000:])
        return None
    return YARD


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
    """what the profiled process runs: the warm call and `reps` calls of diag_rank"""
    eng, d_x = setup(n, C, seed)
    for _ in range(reps + 1):
        eng.diag_rank(d_x, n, D)
    eng.device_free(d_x)
    eng.close()


GROUPS = (("key_ms", ("k_rank_keys",)), ("radix_ms", ("k_rank_count", "k_rank_scan", "k_rank_scatter")), ("run_ms", ("k_rank_runs", "k_rank_carry")), ("combine_ms", ("k_diag_",)))


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


def children(n, C, reps, seed):
    """the figures that other processes measure: the profiled child's split and the yardstick.  They run before this process opens
    the device, one at a time."""
    out = split(n, C, reps, seed)
    if os.path.exists(YARD):
        y = subprocess.run([YARD, str(n * C), str(reps)], capture_output=True, text=True)
        if y.returncode == 0:
            out["yardstick_ms"] = float(y.stdout.strip().splitlines()[-1])
        else:
            print("the yardstick failed:\n" + y.stderr[-800:])
    return out


def one(n, C, reps, seed, pre):
    row = dict(n=n, C=C, d=D, S=n * C, reps=reps)
    eng, d_x = setup(n, C, seed)
    d_out = eng.device_alloc(n * 4 * C * 8)
    res = {}

    def rank():
        res["rank"] = eng.diag_rank(d_x, n, D)

    def transform():
        for j in range(D):
            eng.diag_rank_transform(d_x, n, D, j0=j, n_j=1, d_out=d_out)

    def plain():
        res["plain"] = eng.diag_rhat_ess(d_x, n, D)

    row["rank_ms"], row["transform_ms"], row["plain_ms"] = (median_ms(f, reps) / D for f in (rank, transform, plain))
    r = res["rank"]
    row.update(n_passes=int(r["n_passes"][0]), rhat_rank=float(r["rhat_rank"][0]), ess_bulk=float(r["ess_bulk"][0]), ess_tail=float(r["ess_tail"][0]), plain_rhat=float(res["plain"]["r_hat"][0]))
    eng.device_free(d_out)
    eng.device_free(d_x)
    eng.close()
    row.update(pre)
    print("n=%d C=%d (S=%.3g): diag_rank %.2f ms per coordinate (transform %.2f ms; %d radix passes); plain diag_rhat_ess %.2f ms; split %s; one rocprim sort %s ms" % (
        n, C, n * C, row["rank_ms"], row["transform_ms"], row["n_passes"], row["plain_ms"], {k: round(row[k], 3) for k, _ in GROUPS if k in row}, row.get("yardstick_ms")), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--out", default=None)
    ap.add_argument("--build-yardstick", action="store_true")
    ap.add_argument("--child", nargs=2, type=int, default=None, metavar=("N", "C"))
    a = ap.parse_args()
    if a.build_yardstick:
        print(build_yardstick())
        return
    if a.child:
        child(a.child[0], a.child[1], a.reps, a.seed)
        return
    pre = [children(n, C, a.reps, a.seed) for n, C in SHAPES]
    lines = [json.dumps(one(n, C, a.reps, a.seed, p)) for (n, C), p in zip(SHAPES, pre)]
    for line in lines:
        print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
