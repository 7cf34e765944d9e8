// fg_hmc_sep_plan.h -- the host side of k_hmc_sep_steps (fg_hmc_sep.hip) ahead of the launch: which instantiation runs, on which
// grid, and how the coordinates go to the waves.  Plain C++ (no HIP, no engine): tests/test_hmc_sep_plan_cpu.py pins every field
// of the plan against tests/golden/hmc_sep_plans.json through a g++ build of tests/cpp/sep_plan_driver.cpp.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "fg_ir.h"
#include "fg_switch.h"
#include "../../include/fugue_amd.h"

#define FG_SEP_WMAX 16
#define FG_SEP_WAVE 64            /* = FG_WAVE (fg_interp.h) */

struct FgSegSep { int c[FG_SEP_WMAX + 1]; int sum4;       // sum4: the four in-order sums of a transition's end on four waves (tiles that are alone on their CU)
                  int predraw;                           // resident form: waves 1.. draw their next transition's momenta while wave 0 decides
                  int own[FG_SEP_WMAX][4], n_own[FG_SEP_WMAX]; };   // MODE 3 (dense, coordinates in registers): each wave's <= 4 coordinates (whole Box-Muller pairs), ascending

// The instantiations of k_hmc_sep_steps, each named once: X(MASS, MODE, HALF, NC, NOBS_R, U0_R, FOLD), the kernel's template arguments.
// Per MASS: sparse / dense / analytic / half / quarter tiles / dense with the coordinates in registers, the folded sparse forms, and the
// resident form (NC = 2, 4) of the five record shapes (0 .. 3 observations; U0 prior + one observation), plain and folded.
#define FG_SEP_VARIANTS_RES(X, M, NC, FO) X(M, 0, 0, NC, 0, false, FO) X(M, 0, 0, NC, 1, false, FO) X(M, 0, 0, NC, 2, false, FO) X(M, 0, 0, NC, 3, false, FO) X(M, 0, 0, NC, 1, true, FO)
#define FG_SEP_VARIANTS_M(X, M)                                                                                                                   \
    X(M, 0, 0, 0, 0, false, false) X(M, 1, 0, 0, 0, false, false) X(M, 2, 0, 0, 0, false, false) X(M, 0, 1, 0, 0, false, false) X(M, 0, 2, 0, 0, false, false) \
    X(M, 3, 0, 0, 0, false, false) X(M, 0, 0, 0, 0, false, true) X(M, 0, 1, 0, 0, false, true) X(M, 0, 2, 0, 0, false, true)                       \
    FG_SEP_VARIANTS_RES(X, M, 2, false) FG_SEP_VARIANTS_RES(X, M, 2, true) FG_SEP_VARIANTS_RES(X, M, 4, false) FG_SEP_VARIANTS_RES(X, M, 4, true)
#define FG_SEP_VARIANTS(X) FG_SEP_VARIANTS_M(X, false) FG_SEP_VARIANTS_M(X, true)

struct FgSepKey { bool mass; int mode, half, nc, nobs; bool u0, fold; };
inline bool operator==(const FgSepKey &a, const FgSepKey &b) {
    return a.mass == b.mass && a.mode == b.mode && a.half == b.half && a.nc == b.nc && a.nobs == b.nobs && a.u0 == b.u0 && a.fold == b.fold;
}

struct FgSepPlanIn {
    long long C; int d, n_simd, n_slots, n_sep_free, n_sstream;
    int grad_mode; bool use_mass; int mw_override;         // (FG_HMC_WAVES)
    bool gt, sep_disabled, res_disabled, fold_disabled, sep_fold;   // (fg_engine: FG_HMC_SEP, FG_HMC_SEP_RESIDENT, FG_HMC_SEP_FOLD; sep_fold: fg_program's, and 2h passed fg_div2_prove)
    const std::vector<FgSepCoord> *coord; const std::vector<FgSepRec> *rec;   // fg_program's sep_coord / sep
    FgSwitch sep_half, dense_fast, sum4, prio, stagger, predraw;   // FG_HMC_SEP_HALF, FG_HMC_DENSE_FAST, FG_HMC_SUM4, FG_HMC_PRIO, FG_HMC_STAGGER, FG_HMC_PREDRAW
};
struct FgSepPlan {
    int half, tw;                                            // 1: half tiles, 2: quarter tiles; chains per tile
    unsigned tiles; int W; size_t lds;                       // grid, waves per tile, bytes of the LDS tile
    FgSepKey key;                                            // the instantiation (FG_SEP_VARIANTS)
    FgSegSep seg;
    std::string name;                                        // fg_hmc_last_kernel
};

// the static part of that: fg_hmc_sep_launch's first early-out, and what fg_hmc_jit_first (fg_hmc_split_plan.h) asks
inline bool fg_hmc_sep_gate(bool gt, bool has_sep, bool sep_disabled, int d) { return !gt && has_sep && !sep_disabled && d >= 1; }

// FG_E_UNSUPPORTED when the program / configuration is not an independent-sites run this kernel takes.
inline int fg_hmc_sep_plan(const FgSepPlanIn &in, FgSepPlan *out) {
    const int d = in.d;
    const bool dense = in.grad_mode == FG_GRAD_FD_DENSE, analytic = in.grad_mode == FG_GRAD_ANALYTIC;
    if (in.gt) return FG_E_UNSUPPORTED;                       // tiles in global memory: the one-wave-per-tile kernels (fg_engine.hip)
    const std::vector<FgSepCoord> &cd = *in.coord;
    if (cd.empty() || (in.grad_mode != FG_GRAD_FD_SPARSE && !dense && !analytic) || d < 1 || in.sep_disabled) return FG_E_UNSUPPORTED;
    const long long n_cu = std::max(1, in.n_simd / 4);
    const long long tiles64 = (in.C + FG_SEP_WAVE - 1) / FG_SEP_WAVE;
    // half tiles (32 chains per workgroup, the two coordinates of a Box-Muller pair in the two lane halves): when 64-chain tiles
    // would leave half of the CUs without one, for programs whose coordinates all have one record shape with power-of-two sigmas
    int half = 0;                                            // 1: half tiles, 2: quarter tiles (16 chains, four coordinates per wave)
    bool uniform = true;
    for (const FgSepCoord &q : cd) uniform = uniform && q.n == cd[0].n && (q.n & 256);
    if (!dense && !analytic && d >= 2) {
        // half tiles up to two of them per CU (16 384 chains: 1.57e10 with 64-chain tiles, 1.67e10, 1.75e10 with the late start below);
        // quarter tiles where even half tiles leave CUs without one (4 096 chains: 6.7e9 -> 9.2e9; at 8 192 the two are level)
        if (uniform && tiles64 <= n_cu) half = (4 * tiles64 < 2 * n_cu && d >= 8) ? 2 : 1;
        if (in.sep_half.set) half = uniform ? std::max(0, std::min(2, in.sep_half.v)) : 0;
        if (half == 2 && d < 4) half = 1;
    }
    const int tw = FG_SEP_WAVE >> half;
    const unsigned tiles = (unsigned)((in.C + tw - 1) / tw);
    // dense with the coordinates in registers (fg_dense_trajectory): every coordinate one Normal prior with or without ONE observation,
    // all sigmas powers of two, no statement that reads no coordinate
    bool dfast = dense && in.n_sep_free == 0;
    if (dfast) {
        for (const FgSepCoord &q : cd) dfast = dfast && (q.n & 256) && (q.n & 7) == (cd[0].n & 7) && ((q.n & 7) == 1 || (q.n & 7) == 2);
        if (in.dense_fast.set) dfast = dfast && in.dense_fast.v != 0;
    }
    const size_t rows = (size_t)(in.n_sep_free > 0 ? in.n_slots : 0) + 2 * (size_t)d + (size_t)in.n_sstream + 3 +
                        (dense ? 8 : 4 + 8);     // (dense: the kinetic terms end the tile -- the in-order sums read whole chunks of eight rows; sparse: 4 exchange rows + the chunk a sum may read past them)
    // (the register-resident dense form has two sets of n_s term rows, the second of which also takes the 2 d kinetic terms: with n_s = d
    // or 2 d that is the 2 d + n_s rows of the row-resident form)
    const size_t lds = rows * tw * sizeof(double);
    if (lds > 160 * 1024) return FG_E_UNSUPPORTED;
    // waves per tile: aim at 4 waves per SIMD (16 per CU); the LDS tile caps the tiles resident on a CU, few tiles (small
    // chain counts) leave CUs with one tile -- the waves then come from sharing the tile.  Every wave owns >= 2 coordinates
    // (a half tile: >= 1 pair, both coordinates at once).
    const int unit = half == 2 ? 4 : 2;                      // coordinates a wave takes at a time
    const int pairs = (d + unit - 1) / unit;
    int W = in.mw_override > 0 ? in.mw_override : 1;
    if (in.mw_override <= 0) {
        const long long resident = std::max(1LL, std::min<long long>((160 * 1024) / (long long)lds, ((long long)tiles + n_cu - 1) / n_cu));
        while (W < FG_SEP_WMAX && resident * W < 16 && (half ? pairs >= 2 * W : d >= 4 * W)) W *= 2;     // (a half tile with a pair per wave beats two pairs per wave sharing their random numbers: 1.31e10 against 1.25e10 at 8 192 chains)
    }
    while (W > 1 && unit * (W - 1) >= d + 1) W /= 2;             // no empty waves
    FgSegSep seg;
    std::memset(&seg, 0, sizeof(seg));
    if (dfast) {
        // Whole Box-Muller pairs, at most two per wave.  A coordinate whose own row is r adds 2 (rows - r) terms behind it: the pairs go
        // out by row, to the waves and back (0 .. W-1, W-1 .. 0), so every wave adds about the same number; within a wave by row.
        const int np = (d + 1) / 2, W_plain = W;
        W = std::min(std::max(W, (np + 1) / 2), np);
        if (W > FG_SEP_WMAX) dfast = false;
        else {
            auto row_of = [&](int i, int k) { return (int)(*in.rec)[(size_t)cd[i].off + k].trow; };
            std::vector<int> pr(np);
            for (int q = 0; q < np; ++q) pr[q] = q;
            std::stable_sort(pr.begin(), pr.end(), [&](int a, int b) { return row_of(2 * a, 0) < row_of(2 * b, 0); });
            for (int q = 0; q < np; ++q) {
                const int w = q < W ? q : 2 * W - 1 - q;
                for (int i = 2 * pr[q]; i < std::min(d, 2 * pr[q] + 2); ++i) seg.own[w][seg.n_own[w]++] = i;
            }
            const bool obs = (cd[0].n & 7) == 2;
            for (int w = 0; w < W && dfast; ++w) {
                std::sort(seg.own[w], seg.own[w] + seg.n_own[w], [&](int a, int b) { return row_of(a, 0) < row_of(b, 0); });
                for (int j = 0; j + 1 < seg.n_own[w]; ++j)
                    if (row_of(seg.own[w][j], 0) >= row_of(seg.own[w][j + 1], 0) || (obs && row_of(seg.own[w][j], 1) >= row_of(seg.own[w][j + 1], 1))) dfast = false;
                if (seg.n_own[w] < 1) dfast = false;
            }
        }
        if (!dfast) { std::memset(&seg, 0, sizeof(seg)); W = W_plain; }       // (rows out of order within a wave, or more than 32 pairs: the row-resident form)
    }
    seg.sum4 = (!dense && half != 0) ? 1 : 0;                    // a tile alone on its CU: the transition's four end sums on four waves
    if (in.sum4.set) seg.sum4 = in.sum4.v != 0 ? 1 : 0;
    for (int w = 0; w <= FG_SEP_WMAX; ++w) seg.c[w] = d;
    for (int w = 0; w < W; ++w) seg.c[w] = std::min(d, unit * (int)((long long)pairs * w / W));
    // host flags in the last boundary (otherwise d): -1 priority turns, -2 / -3 the late start of the grid's second half / of the odd tiles
    if (W == 8 && !half && !(in.prio.set && in.prio.v == 0)) seg.c[FG_SEP_WMAX] = -1;                     // priority turns: two waves of a tile per SIMD
    if (half == 1 && (long long)tiles > n_cu && (long long)tiles <= 2 * n_cu) seg.c[FG_SEP_WMAX] = -3;   // two half tiles on a CU: the odd ones start late (+5 %; 64-chain tiles lose 5 % to it)
    if (in.stagger.set) seg.c[FG_SEP_WMAX] = (in.stagger.v == 1 || in.stagger.v == 2) ? -1 - in.stagger.v : (seg.c[FG_SEP_WMAX] <= -2 ? d : seg.c[FG_SEP_WMAX]);   // experiments
    // the resident form: 64-chain sparse tiles of one record shape with power-of-two sigmas, <= 4 coordinates per wave
    int res_nc = 0;
    if (!dense && !analytic && !half && uniform && in.n_sep_free == 0 && !in.res_disabled && (cd[0].n & 7) >= 1 && (cd[0].n & 7) <= 4) {
        int most = 0;
        for (int w = 0; w < W; ++w) most = std::max(most, (w + 1 < W ? seg.c[w + 1] : d) - seg.c[w]);
        res_nc = most <= 2 ? 2 : (most <= 4 ? 4 : 0);
    }
    seg.predraw = 1;
    if (in.predraw.set) seg.predraw = in.predraw.v != 0 ? 1 : 0;   // experiments
    FgSepKey key = { in.use_mass, dfast ? 3 : (dense ? 1 : (analytic ? 2 : 0)), half, res_nc, 0, false,
                     // the folded trajectory loop (fg_sep_trajectory's FOLD): sparse finite differences, the host's range of 1 / sigma
                     !dense && !analytic && in.sep_fold && !in.fold_disabled };
    if (res_nc) { key.nobs = (cd[0].n & 7) - 1; key.u0 = (cd[0].n & 512) && key.nobs == 1; }
    out->half = half; out->tw = tw; out->tiles = tiles; out->W = W; out->lds = lds; out->key = key; out->seg = seg;
    out->name = std::string("k_hmc_sep_steps") + (res_nc ? " (resident)" : key.mode == 3 ? " (dense, coordinates in registers)" : dense ? " (dense)" : analytic ? " (analytic)"
                                                  : half == 2 ? " (quarter tiles)" : half ? " (half tiles)" : "") + (key.fold ? " (folded)" : "") + " W=" + std::to_string(W);
    return FG_OK;
}
