// fg_abc_plan.h -- the host side of the ABC kernels (fg_abc.hip) ahead of a launch: the grid of k_abc_mixture (tiles of 64 accepted
// particles times the splits of the range of centers), the sizes of its partial buffers, and the grid of the ordered compaction of a
// round of attempts.  Plain C++ (no HIP, no engine): tests/test_abc_cpu.py walks the plans over a grid of shapes through a
// stand-alone build of tests/cpp/abc_plan_driver.cpp, and the kernels take a wave's work from the same fg_abc_mix_item, so what the
// driver proves about the ownership of (particle, center) pairs holds for the launch.
//
// k_abc_mixture computes log sum_j w_j K(x_i | theta_j) of weighted ABC-SMC (abc.rs:612-616, :776-799) for the m accepted particles
// of a stage against the n centers of the previous population: one lane per accepted particle, the centers wave-uniform.  A wave
// owns one 64-particle tile and one range of consecutive centers and leaves a partial (max, sum); a finish kernel combines the
// partials of a particle in split order.  A split is a range of centers; a range without work (beyond n) is legal and leaves the
// empty partial (-inf, 0).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/fugue_amd.h"

#if defined(__HIPCC__)
#define FG_ABC_HD __host__ __device__
#else
#define FG_ABC_HD
#endif

#define FG_ABC_WAVE 64                     /* = FG_WAVE (fg_interp.h) */
#define FG_ABC_MIX_W 4                     /* waves per workgroup of k_abc_mixture (they share nothing) */
#define FG_ABC_WAVES_PER_CU 16             /* waves the mixture grid aims at per CU (4 per SIMD) */
#define FG_ABC_MAX_SPLITS 65535            /* of the range of centers (forced or planned) */
#define FG_ABC_DREG 8                      /* coordinates a lane keeps in registers; beyond it (and d = 0) the loop over memory */
#define FG_ABC_SCAN_THREADS 1024           /* one workgroup scans the wave counts of a round in chunks of this many */

struct FgAbcMixPlan {
    long long tiles;                      // 64-particle tiles of the m accepted particles
    long long splits;                     // ranges of centers
    long long centers_per_split;          // consecutive centers of a range (the last ranges may be short or empty)
    long long items;                      // tiles x splits = waves with a partial to write
    unsigned grid;                        // workgroups (x) of FG_ABC_MIX_W waves; 0: m == 0, nothing to launch
    unsigned finish_grid;                 // workgroups of 256 lanes of the finish kernel
    int d_reg;                            // the register form's coordinate count (1 .. FG_ABC_DREG), or 0: the loop over memory
    size_t partial_elems;                 // doubles of EACH of the two partial buffers [splits][m]
    size_t table_elems;                   // doubles of the center table [n][d + 1]: the hoisted constant, then the pre-scaled coordinates
};

// Work item g (= workgroup x FG_ABC_MIX_W + wave): its tile and its centers [j0, j1) (j0 >= j1: no work, the empty partial).
FG_ABC_HD inline void fg_abc_mix_item(long long g, long long tiles, long long centers_per_split, long long n, long long *tile, long long *split, long long *j0,
                                      long long *j1) {
    *split = g / tiles;
    *tile = g - *split * tiles;
    const long long a = *split * centers_per_split, b = a + centers_per_split;
    *j0 = a < n ? a : n;
    *j1 = b < n ? b : n;
}
// cells: a partial [splits][m], the center table [n][d + 1], coordinates [d][m] / [d][n] -- 64-bit throughout
FG_ABC_HD inline long long fg_abc_partial_index(long long split, long long m, long long i) { return split * m + i; }
FG_ABC_HD inline long long fg_abc_table_index(long long j, long long d, long long c) { return j * (d + 1) + c; }
FG_ABC_HD inline long long fg_abc_coord_index(long long c, long long n, long long j) { return c * n + j; }

// FG_E_BAD_ARG: m < 0, n < 1, d < 0, force_splits < 0; FG_E_LIMIT: more workgroups than a grid's x dimension holds.
// force_splits > 0 fixes the number of ranges (more ranges than centers leave ranges without work).
inline int fg_abc_mix_plan(long long m, long long n, long long d, int n_cu, long long force_splits, FgAbcMixPlan *out) {
    if (m < 0 || n < 1 || d < 0 || force_splits < 0 || !out) return FG_E_BAD_ARG;
    if (n_cu < 1) n_cu = 1;
    FgAbcMixPlan P;
    P.tiles = (m + FG_ABC_WAVE - 1) / FG_ABC_WAVE;
    P.d_reg = (d >= 1 && d <= FG_ABC_DREG) ? (int)d : 0;
    if (n > (long long)(0x7fffffffffffffffLL / 8) / (d + 1)) return FG_E_LIMIT;
    P.table_elems = (size_t)n * (size_t)(d + 1);
    if (m == 0) { P.splits = 0; P.centers_per_split = 0; P.items = 0; P.grid = 0; P.finish_grid = 0; P.partial_elems = 0; *out = P; return FG_OK; }
    long long splits;
    if (force_splits > 0) splits = force_splits;
    else {                                                 // a small m still fills the machine: split the centers until the aimed-at waves are reached
        const long long want = (long long)n_cu * FG_ABC_WAVES_PER_CU;
        splits = (want + P.tiles - 1) / P.tiles;
        if (splits > n) splits = n;
    }
    if (splits < 1) splits = 1;
    if (splits > FG_ABC_MAX_SPLITS) splits = FG_ABC_MAX_SPLITS;
    P.centers_per_split = (n + splits - 1) / splits;
    P.splits = force_splits > 0 ? splits : (n + P.centers_per_split - 1) / P.centers_per_split;
    if (P.tiles > 0x7fffffffLL * FG_ABC_MIX_W / P.splits) return FG_E_LIMIT;
    P.items = P.tiles * P.splits;
    const long long groups = (P.items + FG_ABC_MIX_W - 1) / FG_ABC_MIX_W;
    if (groups > 0x7fffffffLL) return FG_E_LIMIT;
    P.grid = (unsigned)groups;
    P.finish_grid = (unsigned)((m + 255) / 256);
    P.partial_elems = (size_t)P.splits * (size_t)m;
    *out = P;
    return FG_OK;
}

// The ordered compaction of a round of B attempts (first n accepted attempts in attempt order, never an atomic slot counter):
// pass 1, one wave per 64 attempts: ballot of the accept flags, the wave's count to counts[wave];
// pass 2, ONE workgroup: the exclusive scan of counts[waves] in chunks of FG_ABC_SCAN_THREADS, in wave order;
// pass 3, one wave per 64 attempts: slot = base + offset[wave] + popcount(ballot below the lane), stored while slot < capacity.
struct FgAbcCompactPlan {
    long long waves;                      // 64-attempt waves of a round = entries of the count / offset buffers
    unsigned grid;                        // workgroups of 256 lanes (4 waves) of passes 1 and 3
    long long scan_chunks;                // chunks the scanning workgroup walks
};
inline int fg_abc_compact_plan(long long B, FgAbcCompactPlan *out) {
    if (B < 1 || !out) return FG_E_BAD_ARG;
    FgAbcCompactPlan P;
    P.waves = (B + FG_ABC_WAVE - 1) / FG_ABC_WAVE;
    const long long groups = (P.waves + 3) / 4;
    if (groups > 0x7fffffffLL) return FG_E_LIMIT;
    P.grid = (unsigned)groups;
    P.scan_chunks = (P.waves + FG_ABC_SCAN_THREADS - 1) / FG_ABC_SCAN_THREADS;
    *out = P;
    return FG_OK;
}
// rounds a host loop over a budget of attempts takes at most: ceil(budget / B)
inline long long fg_abc_max_rounds(long long budget, long long B) { return (B < 1 || budget < 1) ? 0 : (budget + B - 1) / B; }
