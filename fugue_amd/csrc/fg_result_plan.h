// fg_result_plan.h -- the host side of k_result_eval (fg_result.hip) ahead of the launch: waves per workgroup, draws per wave, the
// grid, the LDS bytes and which instantiation runs.  Plain C++ (no HIP, no engine): tests/test_result_cpu.py walks the plan over a
// grid of shapes through a g++ build of tests/cpp/result_plan_driver.cpp, and the kernel takes a wave's work from the same
// fg_result_item, so what the driver proves about the ownership of (tile, draw) pairs holds for the launch.
//
// The kernel evaluates the model's return value -- the `A` of `Model<A>` (src/core/model.rs `pure`; hmc.rs:566-583 returns it per
// draw) -- with one lane per chain.  A wave owns one 64-chain tile and a run of consecutive draws; its working set is a
// [n_slots][64] slice of 8-byte cells.  While four, two or one slice fit a workgroup's LDS (one alone may take the 160 KB of a CU)
// the slices are in LDS, otherwise in a global scratch [waves][n_slots][64]: no program size is refused.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/fugue_amd.h"

#if defined(__HIPCC__)
#define FG_RES_HD __host__ __device__
#else
#define FG_RES_HD
#endif

#define FG_RES_WAVE 64                    /* = FG_WAVE (fg_interp.h) */
#define FG_RES_LDS_MAX (160 * 1024)       /* LDS of a CU: one slice may take all of it (fg_launch raises the kernel's limit above 64 KB) */
#define FG_RES_LDS_PLAIN (64 * 1024)      /* what a workgroup gets without raising the limit: several slices share at most this */
#define FG_RES_WAVES_PER_CU 16            /* waves the grid aims at per CU (4 per SIMD): draws are split between waves until it is reached */
#define FG_RES_WAVES_PER_CU_GLOBAL 4      /* the global form pays 512 n_slots bytes of scratch per wave */

struct FgResultPlan {
    int W;                                // waves per workgroup
    long long draws_per_wave;             // consecutive draws of one tile a wave evaluates
    long long tiles, chunks, items;       // 64-chain tiles, runs of draws per tile, tiles x chunks = waves with work
    unsigned grid;                        // workgroups (x); the block is 64 W threads
    size_t lds;                           // dynamic LDS bytes of a workgroup (0: global form)
    int global_tile;                      // 1: k_result_eval<true>, slices in the global scratch
    size_t scratch_bytes;                 // ... of this many bytes
};

// Work item g (= workgroup x W + wave) of a plan: its tile and its draws [t0, t1).  Items >= plan.items have no work.
FG_RES_HD inline void fg_result_item(long long g, long long tiles, long long draws_per_wave, long long n, long long *tile, long long *t0, long long *t1) {
    const long long chunk = g / tiles;
    *tile = g - chunk * tiles;
    *t0 = chunk * draws_per_wave;
    const long long end = *t0 + draws_per_wave;
    *t1 = end < n ? end : n;
}

// Cell of the draws [n][n_rows][C] and of the results [n][R][C] a lane touches: 64-bit throughout (n R C passes 2^32 in ordinary runs).
FG_RES_HD inline long long fg_result_draw_index(long long t, long long n_rows, long long row, long long C, long long c) { return (t * n_rows + row) * C + c; }
FG_RES_HD inline long long fg_result_out_index(long long t, long long R, long long r, long long C, long long c) { return (t * R + r) * C + c; }

// FG_E_BAD_ARG: C, n, n_slots or n_ins below 1; FG_E_LIMIT: more workgroups than a grid's x dimension holds.
inline int fg_result_plan(long long C, long long n, int n_slots, int n_ins, int n_cu, bool force_global, FgResultPlan *out) {
    if (C < 1 || n < 1 || n_slots < 1 || n_ins < 1 || !out) return FG_E_BAD_ARG;
    if (n_cu < 1) n_cu = 1;
    FgResultPlan P;
    const size_t slice = (size_t)n_slots * FG_RES_WAVE * sizeof(double);
    P.global_tile = (force_global || slice > FG_RES_LDS_MAX) ? 1 : 0;
    if (P.global_tile) P.W = 4;
    else P.W = 4 * slice <= FG_RES_LDS_PLAIN ? 4 : (2 * slice <= FG_RES_LDS_PLAIN ? 2 : 1);
    P.lds = P.global_tile ? 0 : (size_t)P.W * slice;
    P.tiles = (C + FG_RES_WAVE - 1) / FG_RES_WAVE;
    // Few tiles (C = 64: one) leave the card empty unless the draws are split: as many runs of draws per tile as it takes to reach
    // the aimed-at number of waves, never more than n.  Many tiles: one run, every wave streams all n draws of its tile.
    const long long want = (long long)n_cu * (P.global_tile ? FG_RES_WAVES_PER_CU_GLOBAL : FG_RES_WAVES_PER_CU);
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
