// fg_grid_plan.h -- the host side of the log-joint surfaces (fg_grid.hip) ahead of their launches: the cells of a launch, the cut of the
// launch grid, how many bases one chunk table holds, the shapes of the reductions, and the refusals.
// Plain C++ (no HIP): tests/test_grid_cpu.py drives it through tests/cpp/grid_plan_driver.cpp under -fsanitize=address,undefined.
//
// A surface has n_b rows of n_a cells, cell = j n_a + i (row-major, log_joint_grid's `out[j * a_values.len() + i]`, grid.rs:19-20).
// k_grid_eval: grid x = the waves of 64 consecutive cells, grid y = the bases of the chunk; it fills the chunk table [base_chunk][n_b][n_a].
//
// THE SUMMATION ORDERS, functions of (n_a, n_b) alone (tests/grid_restatement.py restates them):
//   log_marg_a[i]  log_sum_exp (numerical.rs:15-38) of column i: one thread; max by fmax over j = 0, 1, ..., n_b - 1 from -inf; -inf when the
//                  max is -inf; else sum of exp(x - max) over j in that sequence from +0.0; -inf when the sum is 0, else max + ln sum.
//   log_marg_b[j]  log_sum_exp of row j by one workgroup of `row_threads` threads: the max is exact (fmax, any order gives the same value);
//                  -inf when it is -inf; else the sum of exp(x - max) is `plan_row_sum`:
//                    1. thread t adds its cells t, t + row_threads, t + 2 row_threads, ... (< n_a) in that sequence, starting from +0.0;
//                    2. each wave of 64 threads folds its 64 partials by halves: lane l takes v[l] + v[l ^ 32], then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1;
//                    3. the wave totals are added in wave order 0, 1, ..., row_threads / 64 - 1, starting from +0.0.
//   log_norm       log_sum_exp of log_marg_b[0 .. n_b) by one thread, in index order as log_marg_a.
//   max, argmax    the fold of the reference's own test (crates/fugue-wasm/tests/wasm.rs:115-124): strict > from -inf over the flat index.
//                  Comparisons round nothing: the workgroups take the larger value and, between equal values, the smaller index.
//   n_nan, n_neg_inf, n_pos_inf   integers.
//   mix[cell]      += exp(lj[c][cell] - log_norm[c]) for the bases c of finite log_norm in arrival order, one thread per cell.
// None depends on the number of bases, on base_chunk, on the cut of the bases into eval calls, or on whether the caller takes the table.
#pragma once
#include <cstddef>

#include "../../include/fugue_amd.h"

#define FG_GRID_WAVE 64
#define FG_GRID_ROW_MAX_THREADS 256               /* the workgroup of one row: 1, 2 or 4 waves */
#define FG_GRID_ROW_TARGET_PER_THREAD 4           /* cells per thread before the workgroup grows */
#define FG_GRID_COL_THREADS 256                   /* columns per workgroup of the column kernel; cells per workgroup of the mixture kernel */
#define FG_GRID_MAX_CELLS 0x7fffffffLL            /* cells below 2^31: the flat index is an int, grid x (waves) is below 2^25 */
#define FG_GRID_MAX_GRID_Y 65535                  /* bases of one launch */
#define FG_GRID_CHUNK_BYTES (256LL << 20)         /* the chunk table the handle owns stays under this (one base at least) */

struct FgGridPlan {
    long long n_a, n_b, cells;
    unsigned waves;          // k_grid_eval: grid x, ceil(cells / 64); grid y = the bases of a chunk
    long long base_chunk;    // bases per chunk table: in [1, FG_GRID_MAX_GRID_Y]
    int row_threads;         // workgroup of the row kernel: 64, 128 or 256; grid (n_b, bases)
    int row_per_thread;      // ceil(n_a / row_threads)
    unsigned col_blocks;     // the column kernel: grid (col_blocks, bases) of FG_GRID_COL_THREADS threads
    unsigned mix_blocks;     // the mixture kernel: ceil(cells / FG_GRID_COL_THREADS) workgroups
};

// FG_E_BAD_ARG: n_a < 1, n_b < 1 or base_chunk < 0; FG_E_LIMIT: 2^31 cells or more.  base_chunk 0: the largest under FG_GRID_CHUNK_BYTES.
inline int fg_grid_plan(long long n_a, long long n_b, long long base_chunk, FgGridPlan *out) {
    if (n_a < 1 || n_b < 1 || base_chunk < 0) return FG_E_BAD_ARG;
    if (n_a > FG_GRID_MAX_CELLS || n_b > FG_GRID_MAX_CELLS || n_a > FG_GRID_MAX_CELLS / n_b) return FG_E_LIMIT;
    FgGridPlan p;
    p.n_a = n_a; p.n_b = n_b; p.cells = n_a * n_b;
    p.waves = (unsigned)((p.cells + FG_GRID_WAVE - 1) / FG_GRID_WAVE);
    long long bc = base_chunk > 0 ? base_chunk : FG_GRID_CHUNK_BYTES / (p.cells * 8);
    if (bc < 1) bc = 1;
    if (bc > FG_GRID_MAX_GRID_Y) bc = FG_GRID_MAX_GRID_Y;
    p.base_chunk = bc;
    p.row_threads = FG_GRID_WAVE;
    while (p.row_threads < FG_GRID_ROW_MAX_THREADS && (long long)p.row_threads * FG_GRID_ROW_TARGET_PER_THREAD < n_a) p.row_threads *= 2;
    p.row_per_thread = (int)((n_a + p.row_threads - 1) / p.row_threads);
    p.col_blocks = (unsigned)((n_a + FG_GRID_COL_THREADS - 1) / FG_GRID_COL_THREADS);
    p.mix_blocks = (unsigned)((p.cells + FG_GRID_COL_THREADS - 1) / FG_GRID_COL_THREADS);
    *out = p;
    return FG_OK;
}
// the bases of one eval call: engine chains [chain0, chain0 + n_bases) of C
inline int fg_grid_check_bases(long long C, long long chain0, long long n_bases) {
    if (chain0 < 0 || n_bases < 1 || chain0 > C || n_bases > C - chain0) return FG_E_BAD_ARG;
    return FG_OK;
}
// chunk k of a call of n_bases takes bases [first, first + count); count = 0 past the last chunk
inline void fg_grid_chunk(const FgGridPlan &p, long long n_bases, long long k, long long *first, long long *count) {
    *first = k * p.base_chunk;
    const long long left = n_bases - *first;
    *count = left <= 0 ? 0 : (left < p.base_chunk ? left : p.base_chunk);
}
inline long long fg_grid_n_chunks(const FgGridPlan &p, long long n_bases) { return n_bases <= 0 ? 0 : (n_bases + p.base_chunk - 1) / p.base_chunk; }
// the cell of (wave, lane) in k_grid_eval, or -1 (a dead lane of the tail wave)
inline long long fg_grid_cell(const FgGridPlan &p, unsigned wave, int lane) {
    const long long c = (long long)wave * FG_GRID_WAVE + lane;
    return c < p.cells ? c : -1;
}
// the cell of row j that (thread, slot) of the row workgroup adds, or -1: cell i belongs to thread i % row_threads, slot i / row_threads
inline long long fg_grid_row_owner(const FgGridPlan &p, int thread, int slot) {
    const long long i = (long long)slot * p.row_threads + thread;
    return i < p.n_a ? i : -1;
}
