// fg_predict_plan.h -- the host side of k_predict_eval (fg_predict.hip) ahead of the launch: waves per workgroup, draws per wave,
// the grid, the LDS bytes and which instantiation runs.  Plain C++ (no HIP, no engine): tests/test_predict_cpu.py walks the plan
// over a grid of shapes through a stand-alone build of tests/cpp/predict_plan_driver.cpp, and the kernel takes a wave's work from
// the same fg_predict_item, so what the driver proves about the ownership of (tile, draw) pairs holds for the launch.
//
// The kernel draws replicated data from the observe statements of a model with the latent sites pinned to a draw -- what the
// reference's workflows do by hand after a run (tests/inference_integration.rs:717-740) -- with one lane per chain.  A wave owns one
// 64-chain tile and a run of consecutive draws; its working set is the program's [n_slots][64] slice of 8-byte cells.  While four,
// two or one slice fit a workgroup's LDS (one alone may take the 160 KB of a CU) the slices are in LDS, otherwise in a global
// scratch [waves][n_slots][64]: no program size is refused.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/fugue_amd.h"

#if defined(__HIPCC__)
#define FG_PRED_HD __host__ __device__
#else
#define FG_PRED_HD
#endif

#define FG_PRED_WAVE 64                    /* = FG_WAVE (fg_interp.h) */
#define FG_PRED_LDS_MAX (160 * 1024)       /* LDS of a CU: one slice may take all of it (fg_launch raises the kernel's limit above 64 KB) */
#define FG_PRED_LDS_PLAIN (64 * 1024)      /* what a workgroup gets without raising the limit: several slices share at most this */
#define FG_PRED_WAVES_PER_CU 16            /* waves the grid aims at per CU (4 per SIMD): draws are split between waves until it is reached */
#define FG_PRED_WAVES_PER_CU_GLOBAL 4      /* the global form pays 512 n_slots bytes of scratch per wave */

struct FgPredictPlan {
    int W;                                // waves per workgroup
    long long draws_per_wave;             // consecutive draws of one tile a wave evaluates
    long long tiles, chunks, items;       // 64-chain tiles, runs of draws per tile, tiles x chunks = waves with work
    unsigned grid;                        // workgroups (x); the block is 64 W threads.  0: n == 0, nothing to launch
    size_t lds;                           // dynamic LDS bytes of a workgroup (0: global form)
    int global_tile;                      // 1: k_predict_eval<true>, slices in the global scratch
    size_t scratch_bytes;                 // ... of this many bytes
};

// Work item g (= workgroup x W + wave) of a plan: its tile and its draws [t0, t1).  Items >= plan.items have no work.
FG_PRED_HD inline void fg_predict_item(long long g, long long tiles, long long draws_per_wave, long long n, long long *tile, long long *t0, long long *t1) {
    const long long chunk = g / tiles;
    *tile = g - chunk * tiles;
    *t0 = chunk * draws_per_wave;
    const long long end = *t0 + draws_per_wave;
    *t1 = end < n ? end : n;
}

// Cell of the draws [n][n_rows][C] and of the tables [n][n_sel][C] a lane touches: 64-bit throughout ([chunk][O][C] passes 2^32 cells
// in ordinary runs).
FG_PRED_HD inline long long fg_predict_draw_index(long long t, long long n_rows, long long row, long long C, long long c) { return (t * n_rows + row) * C + c; }
FG_PRED_HD inline long long fg_predict_out_index(long long t, long long n_sel, long long r, long long C, long long c) { return (t * n_sel + r) * C + c; }

// FG_E_BAD_ARG: C, n_slots or n_ins below 1, n below 0; FG_E_LIMIT: more workgroups than a grid's x dimension holds.
// n == 0 is a plan without work (grid 0): the caller launches nothing.
inline int fg_predict_plan(long long C, long long n, int n_slots, int n_ins, int n_cu, bool force_global, FgPredictPlan *out) {
    if (C < 1 || n < 0 || n_slots < 1 || n_ins < 1 || !out) return FG_E_BAD_ARG;
    if (n_cu < 1) n_cu = 1;
    FgPredictPlan P;
    const size_t slice = (size_t)n_slots * FG_PRED_WAVE * sizeof(double);
    P.global_tile = (force_global || slice > FG_PRED_LDS_MAX) ? 1 : 0;
    if (P.global_tile) P.W = 4;
    else P.W = 4 * slice <= FG_PRED_LDS_PLAIN ? 4 : (2 * slice <= FG_PRED_LDS_PLAIN ? 2 : 1);
    P.lds = P.global_tile ? 0 : (size_t)P.W * slice;
    P.tiles = (C + FG_PRED_WAVE - 1) / FG_PRED_WAVE;
    if (n == 0) { P.draws_per_wave = 0; P.chunks = 0; P.items = 0; P.grid = 0; P.scratch_bytes = 0; *out = P; return FG_OK; }
    // Few tiles (C = 64: one) leave the card empty unless the draws are split: as many runs of draws per tile as it takes to reach
    // the aimed-at number of waves, never more than n.  Many tiles: one run, every wave streams all n draws of its tile.
    const long long want = (long long)n_cu * (P.global_tile ? FG_PRED_WAVES_PER_CU_GLOBAL : FG_PRED_WAVES_PER_CU);
    long long chunks = (want + P.tiles - 1) / P.tiles;
    if (chunks > n) chunks = n;
    if (chunks < 1) chunks = 1;
    P.draws_per_wave = (n + chunks - 1) / chunks;
    P.chunks = (n + P.draws_per_wave - 1) / P.draws_per_wave;
    P.items = P.tiles * P.chunks;
    const long long groups = (P.items + P.W - 1) / P.W;
    if (groups > 0x7fffffffLL) return FG_E_LIMIT;
    P.grid = (unsigned)groups;
    P.scratch_bytes = P.global_tile ? (size_t)groups * P.W * slice : 0;
    *out = P;
    return FG_OK;
}
