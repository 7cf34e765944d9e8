// fg_loglik_stream_plan.h -- the log-likelihood stream (fg_loglik_stream.hip): WAIC and importance-sampling LOO from the table
// d_loglik [n][n_sel][C] that fg_predict_eval writes, handed over one chunk at a time and never stored.  The reference has neither
// figure; the definitions are the textbook ones (BDA3 7.2), DESIGN 3.16.  Plain C++ (no HIP, no engine): the device
// code and tests/cpp/loglik_stream_driver.cpp both run the functions below, the latter with host loops in place of the kernels.
//
// Per column (selected observe statement k, chain c) the stream keeps FG_LL_WORDS 8-byte words, stored [word][n_sel][C]:
//   0 mx     the largest finite cell              1 sp    sum exp(x - mx)
//   2 mn     the smallest finite cell             3 sn    sum exp(mn - x)            4 sn2   sum exp(mn - x)^2
//   5 pivot  the first finite cell                6 s1    sum (x - pivot)            7 s2    sum (x - pivot)^2
//   8 n_fin | n_neg_inf << 32                     9 n_pos_inf | n_nan << 32          (u32 counters: n_total < 2^31)
// all zero at creation (n_fin = 0: nothing seen).  A column is updated in draw order, so its words do not depend on where the chunk
// boundaries fall.  No division anywhere; the pivoted sums are k_diag_stream_update's (DESIGN 3.5 for their conditioning).
//
// State size: FG_LL_WORDS x n_sel x C x 8 bytes -- 80 bytes per (statement, chain), 5.4 GB at n_sel = 1 024, C = 65 536: a model
// with many observe statements selects the ones it compares (`sel` of fg_predict_eval, `pointwise=[addresses]` of the drivers).
//
// Read-out: the chains of a statement are pooled by fg_chain_pool.h's fixed tree on the chain index, FgLlPool its elements.
#pragma once
#include <math.h>
#include <stdint.h>

#include <cmath>

#include "fg_chain_pool.h"

#define FG_LL_WORDS 10               // state words per column
// FG_LL_POOLED (fugue_amd.h) = 8 pooled finite words per statement: mx sp mn sn sn2 n_fin mean ssd
#define FG_LL_ELEM 11                // a tree element in memory: the pooled words, then n_neg_inf, n_pos_inf, n_nan as int64 bits
#define FG_LL_UPDATE_THREADS 256

struct FgLlState {                   // a column while a chunk is walked
    double mx, sp, mn, sn, sn2, pivot, s1, s2;
    uint32_t n_fin, n_neg_inf, n_pos_inf, n_nan;
};

struct FgLlElem {                    // a tree element: a chain, or chains pooled
    double mx = 0.0, sp = 0.0, mn = 0.0, sn = 0.0, sn2 = 0.0;
    FgMoments m;                     // of the finite cells
    int64_t n_neg_inf = 0, n_pos_inf = 0, n_nan = 0;
};

FG_HD void fg_ll_state_load(FgLlState &s, const double *w, long long stride) {
    s.mx = w[0]; s.sp = w[stride]; s.mn = w[2 * stride]; s.sn = w[3 * stride]; s.sn2 = w[4 * stride];
    s.pivot = w[5 * stride]; s.s1 = w[6 * stride]; s.s2 = w[7 * stride];
    uint64_t a, b;                                             // the counter words hold integer bits
    __builtin_memcpy(&a, w + 8 * stride, 8); __builtin_memcpy(&b, w + 9 * stride, 8);
    s.n_fin = (uint32_t)a; s.n_neg_inf = (uint32_t)(a >> 32); s.n_pos_inf = (uint32_t)b; s.n_nan = (uint32_t)(b >> 32);
}
FG_HD void fg_ll_state_store(const FgLlState &s, double *w, long long stride) {
    w[0] = s.mx; w[stride] = s.sp; w[2 * stride] = s.mn; w[3 * stride] = s.sn; w[4 * stride] = s.sn2;
    w[5 * stride] = s.pivot; w[6 * stride] = s.s1; w[7 * stride] = s.s2;
    const uint64_t a = (uint64_t)s.n_fin | ((uint64_t)s.n_neg_inf << 32), b = (uint64_t)s.n_pos_inf | ((uint64_t)s.n_nan << 32);
    __builtin_memcpy(w + 8 * stride, &a, 8); __builtin_memcpy(w + 9 * stride, &b, 8);
}

// one cell.  Two exp in the common branch (the squared ratio is a product); a cell that is not finite only bumps its counter.
FG_HD void fg_ll_update(FgLlState &s, double x) {
    if (x != x) { ++s.n_nan; return; }
    if (x == INFINITY) { ++s.n_pos_inf; return; }
    if (x == -INFINITY) { ++s.n_neg_inf; return; }
    if (s.n_fin == 0) {
        s.mx = s.mn = s.pivot = x;
        s.sp = s.sn = s.sn2 = 1.0;
        s.s1 = s.s2 = 0.0;
        s.n_fin = 1;
        return;
    }
    const bool below = x <= s.mx, above = x >= s.mn;           // the common branch of each side; one exp per side either way
    const double eu = exp(below ? x - s.mx : s.mx - x);
    if (below) s.sp += eu;
    else { s.sp = s.sp * eu + 1.0; s.mx = x; }
    const double el = exp(above ? s.mn - x : x - s.mn), el2 = el * el;
    if (above) { s.sn += el; s.sn2 += el2; }
    else { s.sn = s.sn * el + 1.0; s.sn2 = s.sn2 * el2 + 1.0; s.mn = x; }
    const double d = x - s.pivot;
    s.s1 += d; s.s2 += d * d; s.n_fin += 1;
}

struct FgLlPool {
    typedef FgLlElem Elem;
    typedef FgLlState State;
    enum { WORDS = FG_LL_ELEM };
    static FG_HD Elem empty() { return Elem(); }
    static FG_HD void state_load(State &s, const double *w, long long stride) { fg_ll_state_load(s, w, stride); }
    // a chain as a tree leaf
    static FG_HD Elem leaf(const State &s) {
        Elem e;
        e.n_neg_inf = (int64_t)s.n_neg_inf; e.n_pos_inf = (int64_t)s.n_pos_inf; e.n_nan = (int64_t)s.n_nan;
        if (s.n_fin == 0) return e;
        e.mx = s.mx; e.sp = s.sp; e.mn = s.mn; e.sn = s.sn; e.sn2 = s.sn2;
        e.m = fg_moments_leaf((double)s.n_fin, s.pivot, s.s1, s.s2);
        return e;
    }
    // element i takes in element i + s.  Counters add; a side without finite cells passes the other side's finite words through
    // untouched; else the larger maximum (the smaller minimum) stays the reference point, and the moments merge as FgMoments do.
    static FG_HD Elem merge(const Elem &a, const Elem &b) {
        Elem r = a;
        if (a.m.n == 0.0) r = b;
        else if (b.m.n != 0.0) {
            if (a.mx >= b.mx) { r.sp = a.sp + b.sp * exp(b.mx - a.mx); r.mx = a.mx; }
            else { r.sp = b.sp + a.sp * exp(a.mx - b.mx); r.mx = b.mx; }
            if (a.mn <= b.mn) { const double f = exp(a.mn - b.mn); r.sn = a.sn + b.sn * f; r.sn2 = a.sn2 + b.sn2 * (f * f); r.mn = a.mn; }
            else { const double f = exp(b.mn - a.mn); r.sn = b.sn + a.sn * f; r.sn2 = b.sn2 + a.sn2 * (f * f); r.mn = b.mn; }
            r.m = fg_moments_merge(a.m, b.m);
        }
        r.n_neg_inf = a.n_neg_inf + b.n_neg_inf; r.n_pos_inf = a.n_pos_inf + b.n_pos_inf; r.n_nan = a.n_nan + b.n_nan;
        return r;
    }
    static FG_HD void elem_store(const Elem &e, double *w) {
        w[0] = e.mx; w[1] = e.sp; w[2] = e.mn; w[3] = e.sn; w[4] = e.sn2; w[5] = e.m.n; w[6] = e.m.mean; w[7] = e.m.ssd;
        __builtin_memcpy(w + 8, &e.n_neg_inf, 8); __builtin_memcpy(w + 9, &e.n_pos_inf, 8); __builtin_memcpy(w + 10, &e.n_nan, 8);
    }
    static FG_HD Elem elem_load(const double *w) {
        Elem e;
        e.mx = w[0]; e.sp = w[1]; e.mn = w[2]; e.sn = w[3]; e.sn2 = w[4]; e.m.n = w[5]; e.m.mean = w[6]; e.m.ssd = w[7];
        __builtin_memcpy(&e.n_neg_inf, w + 8, 8); __builtin_memcpy(&e.n_pos_inf, w + 9, 8); __builtin_memcpy(&e.n_nan, w + 10, 8);
        return e;
    }
};

// ------------------------------------------------------------------ host side

struct FgLlPlan {
    FgDraws draws;
    int n_sel = 0;
    long long C = 0;
    std::vector<FgPoolLaunch> launches;                       // of every update: columns of the n_sel x C
    std::vector<FgPoolLevel> levels;                          // of the pooling tree
    std::vector<FgPoolSlice> slices;                          // statements of every level
};

inline size_t fg_ll_state_words(const FgLlPlan &P) { return (size_t)FG_LL_WORDS * (size_t)P.n_sel * (size_t)P.C; }
// the two buffers the tree alternates between, in elements per statement
inline long long fg_ll_scratch_elems(const FgLlPlan &P) { return P.levels.empty() ? 1 : P.levels[0].m_out; }

// max_grid_x / max_grid_y: the tests pass small ones to see the cuts
inline int fg_ll_init(FgLlPlan &P, int n_total, long long C, int n_sel, std::string *err, long long max_grid_x = FG_POOL_MAX_GRID_X,
                      long long max_grid_y = FG_POOL_MAX_GRID_Y) {
    std::string bad;
    if (n_total < 1) bad = "n_total < 1";
    else if (n_sel < 1) bad = "n_sel < 1";
    else if (C < 1) bad = "no chains";
    else if (max_grid_x < 1 || max_grid_y < 1) bad = "a grid limit below 1";
    if (!bad.empty()) { if (err) *err = "fg_loglik_stream_new: " + bad; return FG_E_BAD_ARG; }
    P = FgLlPlan();
    P.draws.n_total = n_total; P.n_sel = n_sel; P.C = C;
    P.launches = fg_pool_launches((long long)n_sel * C, FG_LL_UPDATE_THREADS, max_grid_x);
    P.levels = fg_pool_levels(C);
    P.slices = fg_pool_slices(n_sel, max_grid_y);
    return FG_OK;
}

enum { FG_LL_LPPD = 0, FG_LL_MEAN_LL = 1, FG_LL_P_WAIC = 2, FG_LL_ELPD_WAIC = 3, FG_LL_ELPD_LOO = 4, FG_LL_P_LOO = 5, FG_LL_IS_ESS = 6, FG_LL_MAX_WEIGHT = 7 };

// The figures of one statement from its pooled element, N = n_total x C draws: what the two-pass formulas give in IEEE arithmetic.
// -inf cells are zero mass in lppd but count in N (the reference's log_sum_exp, numerical.rs:15-38); +inf cells add nothing to
// the sum of ratios but count in N.  p_waic divides by N - 1 (BDA3 eq. 7.12).
inline void fg_ll_finish(const FgLlElem &e, double N, double *fig /*[FG_LL_FIGURES]*/) {
    const double nan = std::nan(""), inf = INFINITY;
    const int64_t a = e.n_neg_inf, b = e.n_pos_inf, z = e.n_nan;
    const bool none = e.m.n == 0.0;
    if (z > 0) { for (int i = 0; i < FG_LL_FIGURES; ++i) fig[i] = nan; return; }
    const double lnN = std::log(N);
    fig[FG_LL_LPPD] = b > 0 ? inf : (none ? -inf : e.mx + std::log(e.sp) - lnN);
    fig[FG_LL_ELPD_LOO] = a > 0 ? -inf : (none ? inf : lnN + e.mn - std::log(e.sn));
    fig[FG_LL_MEAN_LL] = a > 0 && b > 0 ? nan : (a > 0 ? -inf : (b > 0 ? inf : e.m.mean));
    fig[FG_LL_P_WAIC] = a == 0 && b == 0 && N > 1.0 ? e.m.ssd / (N - 1.0) : nan;
    fig[FG_LL_ELPD_WAIC] = fig[FG_LL_LPPD] - fig[FG_LL_P_WAIC];
    fig[FG_LL_P_LOO] = fig[FG_LL_LPPD] - fig[FG_LL_ELPD_LOO];
    const bool ratios = a == 0 && !none;
    fig[FG_LL_IS_ESS] = ratios ? e.sn * e.sn / e.sn2 : nan;
    fig[FG_LL_MAX_WEIGHT] = ratios ? 1.0 / e.sn : nan;
}
