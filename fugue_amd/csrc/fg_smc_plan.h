// fg_smc_plan.h -- the host side of adaptive_smc (fg_smc.hip) ahead of its launches: the grids of the population-wide passes, the
// layout of the engine's SMC arena, and which rejuvenation kernel runs on which grid.  Plain C++ (no HIP, no engine):
// tests/test_smc_plan_cpu.py pins every field against tests/golden/smc_plans.json through a g++ build of tests/cpp/smc_plan_driver.cpp.
#pragma once
#include <algorithm>
#include <cstddef>
#include <string>

#include "../../include/fugue_amd.h"

// ---- the sizes of the streaming passes
#define RED_BLOCKS 512
#define RED_THREADS 256
#define SCAN_THREADS 256
#define SCAN_ITEMS 8
#define SCAN_CHUNK (SCAN_THREADS * SCAN_ITEMS)
// few, large blocks: a pass is dominated by what follows the sums -- one ticket atomic per block, the last block's sweep over the
// blocks' partials -- not by the two exps per particle (512 x 256: 1.13 ms per run, 128 x 512: 1.00 ms, 2048 x 256: 2.3 ms)
#ifndef ESS_BLOCKS
#define ESS_BLOCKS 128
#endif
#ifndef ESS_THREADS
#define ESS_THREADS 512
#endif
#define ESS_MAXC 8
#ifndef ESS2_BLOCKS
#define ESS2_BLOCKS 256
#endif
#ifndef ESS2_THREADS
#define ESS2_THREADS 512
#endif
#define FG_SMC_WPB(SCORE) ((SCORE) < 0 ? 1 : ((SCORE) == 2 ? 4 : 16))   /* tiles (waves) per block of k_smc_rejuv<SCORE> */
#define FG_SMC_LDS_MAX (150 * 1024)       /* what the tiles of a rejuvenation block may take of a CU's LDS (the rest: counts, block maxima) */
#define FG_SMC_LDS_PLAIN (64 * 1024)      /* what a block gets without raising the function's limit (fg_launch raises it above this) */
#define FG_SMC_PLAN_WAVE 64               /* = FG_WAVE (fg_interp.h) */
#define FG_SMC_PLAN_HIST 320              /* = FG_SMC_HIST (fg_dev_types.h): sites the block histogram of a sweep holds */
#define FG_SMC_SCALARS_BYTES 256          /* room for FgSmcScalars (fg_dev_types.h; fg_smc.hip asserts that it fits) */

// ---- the arena: every region in carving order, X(name, bytes).  N particles, Sn = max(1, S) sites, n_chunks scan chunks, max_blk
// rejuvenation blocks at one tile per block.  Every region starts on a 256-byte boundary.
// (ess_part: k_smc_ess_pass's [ESS_BLOCKS][ESS_MAXC][3]; the 8 doubles behind it have no reader any more -- they stay in the layout, so
// that a grown arena keeps its size)
#define FG_SMC_REGIONS(X)                                                                                                              \
    X(ll, N * 8) X(lprior, N * 8) X(scale, Sn * 8) X(log_scale, Sn * 8) X(acc, Sn * 8) X(tot, Sn * 8) X(st, FG_SMC_SCALARS_BYTES)       \
    X(lw, N * 8) X(w, N * 8) X(ll2, N * 8) X(lp2, N * 8) X(vals2, Sn * N * 8) X(idx, N * 8)                                            \
    X(part_max, std::max<size_t>(RED_BLOCKS, max_blk) * 8) X(part_sum, 2 * RED_BLOCKS * 8) X(ess_part, ((size_t)ESS_BLOCKS * ESS_MAXC * 3 + 8) * 8) \
    X(ess2, ess2_doubles * 8) X(chunk, n_chunks * 8) X(chunk2, n_chunks * 8) X(cum, N * 8) X(blk, max_blk * 2 * Sn * 4) X(red, 64)
enum FgSmcRegion {
#define FG_SMC_REGION_ID(name, bytes) FG_SMC_R_##name,
    FG_SMC_REGIONS(FG_SMC_REGION_ID)
#undef FG_SMC_REGION_ID
    FG_SMC_N_REGIONS
};
struct FgSmcArena {
    size_t off[FG_SMC_N_REGIONS], len[FG_SMC_N_REGIONS];   // where a region starts, the bytes it was asked for
    size_t bytes;                                          // the whole arena
    size_t adapt_reset_off, adapt_reset_bytes;             // log_scale, acc, tot: what a fresh DiminishingAdaptation zeroes (fg_smc_rejuvenate)
};
// ess2_doubles: Reducer::ess2_doubles() (fg_smc.hip) -- it depends on a device-side struct
inline FgSmcArena fg_smc_arena_layout(long long n_particles, int S, size_t ess2_doubles) {
    const size_t N = (size_t)n_particles, Sn = (size_t)std::max(1, S);
    const size_t n_chunks = (N + SCAN_CHUNK - 1) / SCAN_CHUNK, max_blk = (N + FG_SMC_PLAN_WAVE - 1) / FG_SMC_PLAN_WAVE;
    FgSmcArena A;
    size_t at = 0;
#define FG_SMC_CARVE(name, bytes) A.off[FG_SMC_R_##name] = at; A.len[FG_SMC_R_##name] = (size_t)(bytes); at += ((size_t)(bytes) + 255) & ~(size_t)255;
    FG_SMC_REGIONS(FG_SMC_CARVE)
#undef FG_SMC_CARVE
    A.bytes = at;
    A.adapt_reset_off = A.off[FG_SMC_R_log_scale];
    A.adapt_reset_bytes = A.off[FG_SMC_R_tot] + A.len[FG_SMC_R_tot] - A.adapt_reset_off;
    return A;
}

// ---- the rejuvenation sweep: X(SCORE, GT), the template arguments of k_smc_rejuv and k_smc_rejuv_seq
#define FG_SMC_REJUV_VARIANTS(X) X(0, false) X(0, true) X(2, false) X(2, true) X(3, false) X(3, true) X(-1, false) X(-1, true)

struct FgSmcRejuvIn {
    long long N; int S, d; size_t lds_score; int tw;         // particles, sites, coordinates, bytes of one tile (512 n_slots), lanes per tile
    bool has_sstream; int sstream_kinds; bool sstream_gen;   // the program's score stream (FgProgramDev)
    int jit_state;                                           // the unit compiled at run time: 0 not tried, 1 loaded, -1 unavailable
    bool sequential;                                         // fg_smc_config.sequential_adaptation: k_smc_rejuv_seq, one wave
    bool from_run;                                           // fg_smc_run asks (false: fg_smc_rejuvenate)
};
struct FgSmcRejuvKey { int score; bool gt, seq; };
struct FgSmcRejuvPlan {
    int score;                 // 0 = score stream of fast Normals, 3 = + linear predictors / option selects / Categorical tables, 2 = + general records, -1 = the interpreter
    bool global_tile;          // the tile lives in the engine's global scratch, one wave per block
    int wpb; size_t lds; unsigned nblk, threads;   // tiles (waves) per block, dynamic LDS bytes, the grid, the block
    bool try_compiled;         // k_smc_jit_rejuv first (fg_smc_jit_rejuv_launch); the library kernel when it refuses
    FgSmcRejuvKey key;         // the library instantiation (FG_SMC_REJUV_VARIANTS)
    std::string name;          // ... as diagnostics print it
};
// FG_E_UNSUPPORTED: a program without coordinates has no site to move.
inline int fg_smc_rejuv_plan(const FgSmcRejuvIn &in, FgSmcRejuvPlan *out) {
    if (in.d < 1 || in.N < 1 || in.tw < 1) return FG_E_UNSUPPORTED;
    FgSmcRejuvPlan p;
    p.score = !in.has_sstream ? -1 : (in.sstream_kinds == 0 ? 0 : (in.sstream_gen ? 2 : 3));
    // tiles (waves) per block: as many as the kernel is built for and 150 KB of LDS hold; a tile beyond one CU's LDS (or more sites
    // than the block histogram has) lives in the engine's global scratch, one wave per block
    p.global_tile = in.lds_score > FG_SMC_LDS_MAX || in.S > FG_SMC_PLAN_HIST;
    if (in.sequential) {                                     // the reference's order: one wave walks the population, particle by particle
        p.wpb = 1; p.lds = p.global_tile ? 0 : in.lds_score; p.nblk = 1; p.threads = FG_SMC_PLAN_WAVE;
        p.try_compiled = false;
    } else {
        p.wpb = p.global_tile ? 1 : (int)std::max<size_t>(1, std::min<size_t>((size_t)FG_SMC_WPB(p.score), FG_SMC_LDS_MAX / std::max<size_t>(1, in.lds_score)));
        p.lds = p.global_tile ? 0 : in.lds_score * p.wpb;
        p.nblk = (unsigned)((in.N + (long long)in.tw * p.wpb - 1) / ((long long)in.tw * p.wpb));
        p.threads = p.global_tile ? FG_SMC_PLAN_WAVE : (unsigned)(in.tw * p.wpb);
        // The compiled model where there is one: programs without a score stream, and stream programs with general / option-select /
        // Categorical records (hier_scale 3.2 -> 2.3 ms per 262 144-particle run, mixture 3.4 -> 2.4).  Fast-Normal streams keep
        // k_smc_rejuv<0> -- except in a run of a large population, which had the unit built for its prior draw (28.6 -> 24.7 us per
        // sweep of 1 048 576 particles).  That exception is fg_smc_run's alone: fg_smc_rejuvenate never took it, and from_run keeps the
        // two as they were.
        p.try_compiled = !p.global_tile && (p.score != 0 || (in.from_run && in.jit_state == 1 && in.N >= (1LL << 18)));
    }
    p.key = { p.score, p.global_tile, in.sequential };
    p.name = std::string(in.sequential ? "k_smc_rejuv_seq<" : "k_smc_rejuv<") + std::to_string(p.score) + (p.global_tile ? ", GT>" : ">") +
             (in.sequential ? "" : " wpb=" + std::to_string(p.wpb)) + (p.try_compiled ? " behind k_smc_jit_rejuv" : "");
    *out = p;
    return FG_OK;
}

// ---- the sweep through the model compiled at run time (k_smc_jit_rejuv, fg_hmc_jit_body.h): S site rows per tile, C particles
struct FgSmcJitShape { int wpb; size_t lds; unsigned nblk; };
// FG_E_UNSUPPORTED: more sites than the block histogram has, or a tile beyond 150 KB.
inline int fg_smc_jit_rejuv_shape(int S, long long C, FgSmcJitShape *out) {
    if (S > FG_SMC_PLAN_HIST) return FG_E_UNSUPPORTED;
    const size_t tile = (size_t)S * FG_SMC_PLAN_WAVE * sizeof(double);
    if (tile > FG_SMC_LDS_MAX) return FG_E_UNSUPPORTED;
    // tiles (waves) per block: four; sixteen for a program of a few sites (fewer blocks, fewer rows of counts and block maxima: 0.39 -> 0.375 ms
    // per 1 048 576-particle run of the one-site model)
    out->wpb = (int)std::max<size_t>(1, std::min<size_t>(16 * tile <= 16 * 1024 ? 16 : 4, FG_SMC_LDS_MAX / tile));
    out->lds = tile * out->wpb;
    out->nblk = (unsigned)((C + (long long)FG_SMC_PLAN_WAVE * out->wpb - 1) / ((long long)FG_SMC_PLAN_WAVE * out->wpb));
    return FG_OK;
}
