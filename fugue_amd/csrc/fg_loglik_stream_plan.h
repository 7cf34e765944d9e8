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
// Read-out: the chains of a statement are pooled by a FIXED binary tree on the chain index -- for stride s = 1, 2, 4, ... element
// i (a multiple of 2 s) takes in element i + s when i + s < C and passes through unchanged otherwise -- so the pooled words are a
// function of the table and of C alone.  A missing partner is the empty element, and merging with it is the identity, bit for bit;
// so a block of FG_LL_POOL_THREADS consecutive elements is a subtree whatever C is, and the tree is run level by level:
// level 0 turns C columns into ceil(C / 256) elements, level 1 those into ceil(. / 256), ... down to one.
#pragma once
#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/fugue_amd.h"

#ifndef FG_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FG_HD __host__ __device__ __forceinline__
#else
#define FG_HD inline
#endif
#endif

#define FG_LL_WORDS 10               // state words per column
// FG_LL_POOLED (fugue_amd.h) = 8 pooled finite words per statement: mx sp mn sn sn2 n_fin mean ssd
#define FG_LL_ELEM 11                // a tree element in memory: the pooled words, then n_neg_inf, n_pos_inf, n_nan as int64 bits
#define FG_LL_UPDATE_THREADS 256
#define FG_LL_POOL_THREADS 256       // elements per block of a tree level; a power of two (the block is a subtree)
#define FG_LL_MAX_GRID_X 0x7fffff    // blocks of an update launch: threads stay below 2^31
#define FG_LL_MAX_GRID_Y 65535

struct FgLlState {                   // a column while a chunk is walked
    double mx, sp, mn, sn, sn2, pivot, s1, s2;
    uint32_t n_fin, n_neg_inf, n_pos_inf, n_nan;
};

struct FgLlElem {                    // a tree element: a chain, or chains pooled
    double mx, sp, mn, sn, sn2, n, mean, ssd;      // n: the finite cells (below 2^47, exact)
    int64_t n_neg_inf, n_pos_inf, n_nan;
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

FG_HD FgLlElem fg_ll_empty() {
    FgLlElem e;
    e.mx = e.sp = e.mn = e.sn = e.sn2 = e.n = e.mean = e.ssd = 0.0;
    e.n_neg_inf = e.n_pos_inf = e.n_nan = 0;
    return e;
}

// a chain as a tree leaf: (n, mean, ssd) by fg_diag_stream's identities, mu = s1 / n, mean = pivot + mu, ssd = s2 - s1 mu
FG_HD FgLlElem fg_ll_leaf(const FgLlState &s) {
    FgLlElem e = fg_ll_empty();
    e.n_neg_inf = (int64_t)s.n_neg_inf; e.n_pos_inf = (int64_t)s.n_pos_inf; e.n_nan = (int64_t)s.n_nan;
    if (s.n_fin == 0) return e;
    e.mx = s.mx; e.sp = s.sp; e.mn = s.mn; e.sn = s.sn; e.sn2 = s.sn2;
    e.n = (double)s.n_fin;
    const double mu = s.s1 / e.n;
    e.mean = s.pivot + mu;
    e.ssd = s.s2 - s.s1 * mu;
    return e;
}

// element i takes in element i + s.  Counters add; a side without finite cells passes the other side's finite words through
// untouched; else the larger maximum (the smaller minimum) stays the reference point, and the moments merge by Chan's formulas.
FG_HD FgLlElem fg_ll_merge(const FgLlElem &a, const FgLlElem &b) {
    FgLlElem r = a;
    if (a.n == 0.0) r = b;
    else if (b.n != 0.0) {
        if (a.mx >= b.mx) { r.sp = a.sp + b.sp * exp(b.mx - a.mx); r.mx = a.mx; }
        else { r.sp = b.sp + a.sp * exp(a.mx - b.mx); r.mx = b.mx; }
        if (a.mn <= b.mn) { const double f = exp(a.mn - b.mn); r.sn = a.sn + b.sn * f; r.sn2 = a.sn2 + b.sn2 * (f * f); r.mn = a.mn; }
        else { const double f = exp(b.mn - a.mn); r.sn = b.sn + a.sn * f; r.sn2 = b.sn2 + a.sn2 * (f * f); r.mn = b.mn; }
        const double n = a.n + b.n, delta = b.mean - a.mean;
        r.n = n;
        r.mean = a.mean + delta * (b.n / n);
        r.ssd = a.ssd + b.ssd + delta * delta * (a.n * b.n / n);
    }
    r.n_neg_inf = a.n_neg_inf + b.n_neg_inf; r.n_pos_inf = a.n_pos_inf + b.n_pos_inf; r.n_nan = a.n_nan + b.n_nan;
    return r;
}

FG_HD void fg_ll_elem_store(const FgLlElem &e, double *w) {
    w[0] = e.mx; w[1] = e.sp; w[2] = e.mn; w[3] = e.sn; w[4] = e.sn2; w[5] = e.n; w[6] = e.mean; w[7] = e.ssd;
    __builtin_memcpy(w + 8, &e.n_neg_inf, 8); __builtin_memcpy(w + 9, &e.n_pos_inf, 8); __builtin_memcpy(w + 10, &e.n_nan, 8);
}
FG_HD FgLlElem fg_ll_elem_load(const double *w) {
    FgLlElem e;
    e.mx = w[0]; e.sp = w[1]; e.mn = w[2]; e.sn = w[3]; e.sn2 = w[4]; e.n = w[5]; e.mean = w[6]; e.ssd = w[7];
    __builtin_memcpy(&e.n_neg_inf, w + 8, 8); __builtin_memcpy(&e.n_pos_inf, w + 9, 8); __builtin_memcpy(&e.n_nan, w + 10, 8);
    return e;
}

// ------------------------------------------------------------------ host side

struct FgLlLaunch { long long col0 = 0, cols = 0; };          // columns [col0, col0 + cols) of the n_sel x C columns
struct FgLlLevel { long long m_in = 0, m_out = 0; };          // a tree level: m_in elements per statement -> m_out = ceil(m_in / 256)
struct FgLlSlice { int k0 = 0, nk = 0; };                     // statements [k0, k0 + nk) of a pool launch (grid y)

struct FgLlPlan {
    int n_total = 0, n_sel = 0, count = 0;
    long long C = 0;
    std::vector<FgLlLaunch> launches;                         // of every update
    std::vector<FgLlLevel> levels;                            // of the pooling tree
    std::vector<FgLlSlice> slices;                            // of every level
};

inline size_t fg_ll_state_words(const FgLlPlan &P) { return (size_t)FG_LL_WORDS * (size_t)P.n_sel * (size_t)P.C; }
// the two buffers the tree alternates between, in elements per statement
inline long long fg_ll_scratch_elems(const FgLlPlan &P) { return P.levels.empty() ? 1 : P.levels[0].m_out; }

// max_grid_x / max_grid_y: FG_LL_MAX_GRID_X / _Y; the tests pass small ones to see the cuts
inline int fg_ll_init(FgLlPlan &P, int n_total, long long C, int n_sel, std::string *err, long long max_grid_x = FG_LL_MAX_GRID_X,
                      int max_grid_y = FG_LL_MAX_GRID_Y) {
    std::string bad;
    if (n_total < 1) bad = "n_total < 1";
    else if (n_sel < 1) bad = "n_sel < 1";
    else if (C < 1) bad = "no chains";
    else if (max_grid_x < 1 || max_grid_y < 1) bad = "a grid limit below 1";
    if (!bad.empty()) { if (err) *err = "fg_loglik_stream_new: " + bad; return FG_E_BAD_ARG; }
    P = FgLlPlan();
    P.n_total = n_total; P.n_sel = n_sel; P.C = C;
    const long long cols = (long long)n_sel * C, per = max_grid_x * FG_LL_UPDATE_THREADS;
    for (long long c0 = 0; c0 < cols; c0 += per) {
        FgLlLaunch L;
        L.col0 = c0; L.cols = std::min(per, cols - c0);
        P.launches.push_back(L);
    }
    long long m = C;
    do {
        FgLlLevel L;
        L.m_in = m; L.m_out = (m + FG_LL_POOL_THREADS - 1) / FG_LL_POOL_THREADS;
        P.levels.push_back(L);
        m = L.m_out;
    } while (m > 1);
    for (int k0 = 0; k0 < n_sel; k0 += max_grid_y) {
        FgLlSlice S;
        S.k0 = k0; S.nk = std::min(max_grid_y, n_sel - k0);
        P.slices.push_back(S);
    }
    return FG_OK;
}

// n_chunk more draws: FG_E_STATE past n_total.  n_chunk == 0 is FG_OK (the caller launches nothing).
inline int fg_ll_take(FgLlPlan &P, int n_chunk, std::string *err) {
    if (n_chunk < 0) { if (err) *err = "fg_loglik_stream_update: n_chunk < 0"; return FG_E_BAD_ARG; }
    if (n_chunk > P.n_total - P.count) {
        if (err) *err = "fg_loglik_stream_update: " + std::to_string(P.count) + " + " + std::to_string(n_chunk) + " draws pass n_total = " + std::to_string(P.n_total);
        return FG_E_STATE;
    }
    P.count += n_chunk;
    return FG_OK;
}
inline void fg_ll_untake(FgLlPlan &P, int n_chunk) { P.count -= n_chunk; }       // a launch that never ran gives its draws back

inline int fg_ll_complete(const FgLlPlan &P, const char *who, std::string *err) {
    if (P.count == P.n_total) return FG_OK;
    if (err) *err = std::string(who) + ": " + std::to_string(P.count) + " of " + std::to_string(P.n_total) + " draws have arrived";
    return FG_E_STATE;
}

// One block of a tree level on the host: elements e[0 .. n) (n <= 256) by the stride rule; the result is e[0].  The device block
// runs the same pairs with the missing partners as empty elements.
inline FgLlElem fg_ll_block_tree(FgLlElem *e, int n) {
    for (int s = 1; s < n; s *= 2)
        for (int i = 0; i + s < n; i += 2 * s) e[i] = fg_ll_merge(e[i], e[i + s]);
    return e[0];
}

enum { FG_LL_LPPD = 0, FG_LL_MEAN_LL = 1, FG_LL_P_WAIC = 2, FG_LL_ELPD_WAIC = 3, FG_LL_ELPD_LOO = 4, FG_LL_P_LOO = 5, FG_LL_IS_ESS = 6, FG_LL_MAX_WEIGHT = 7 };

// The figures of one statement from its pooled element, N = n_total x C draws: what the two-pass formulas give in IEEE arithmetic.
// -inf cells are zero mass in lppd but count in N (the reference's log_sum_exp, numerical.rs:15-38); +inf cells add nothing to
// the sum of ratios but count in N.  p_waic divides by N - 1 (BDA3 eq. 7.12).
inline void fg_ll_finish(const FgLlElem &e, double N, double *fig /*[FG_LL_FIGURES]*/) {
    const double nan = std::nan(""), inf = INFINITY;
    const int64_t a = e.n_neg_inf, b = e.n_pos_inf, z = e.n_nan;
    const bool none = e.n == 0.0;
    if (z > 0) { for (int i = 0; i < FG_LL_FIGURES; ++i) fig[i] = nan; return; }
    const double lnN = std::log(N);
    fig[FG_LL_LPPD] = b > 0 ? inf : (none ? -inf : e.mx + std::log(e.sp) - lnN);
    fig[FG_LL_ELPD_LOO] = a > 0 ? -inf : (none ? inf : lnN + e.mn - std::log(e.sn));
    fig[FG_LL_MEAN_LL] = a > 0 && b > 0 ? nan : (a > 0 ? -inf : (b > 0 ? inf : e.mean));
    fig[FG_LL_P_WAIC] = a == 0 && b == 0 && N > 1.0 ? e.ssd / (N - 1.0) : nan;
    fig[FG_LL_ELPD_WAIC] = fig[FG_LL_LPPD] - fig[FG_LL_P_WAIC];
    fig[FG_LL_P_LOO] = fig[FG_LL_LPPD] - fig[FG_LL_ELPD_LOO];
    const bool ratios = a == 0 && !none;
    fig[FG_LL_IS_ESS] = ratios ? e.sn * e.sn / e.sn2 : nan;
    fig[FG_LL_MAX_WEIGHT] = ratios ? 1.0 / e.sn : nan;
}
