// fg_diag_mcse_plan.h -- the rule of the Monte Carlo standard errors and effective sample sizes of a mean, a standard deviation and
// quantiles (fg_diag_mcse.hip; the figures of the R `posterior` package's summarise_draws: mcse_mean, mcse_sd, mcse_quantile, ess_mean,
// ess_sd, ess_quantile, mad; the reference has none of it).  Plain C++ (no HIP, no engine): the device code and tests/cpp/mcse_driver.cpp
// both call it; tests/mcse_restatement.py restates it in numpy.  DESIGN 3.24.
//
// One coordinate of d_draws [n][d][C] is S = n C pooled cells; cell i = draw i / C, chain i % C.  Key, median, k_p and the sort are
// fg_diag_rank_plan.h's.  Per coordinate, in IEEE double, a product and a sum never contracted:
//   1  mean, sd, rhat, ess_mean   fg_diag_rhat_ess's h_mean, h_std, h_rhat, h_ess of the raw draws; mcse_mean = sd / sqrt(ess_mean)
//   2  c = x - mean; row A = |c|, row B = c c.  ess_sd = ESS(A) (`posterior`'s current definition), ess_sq = ESS(B), Evar = pooled mean
//      of B, V = std_B^2 (S - 1) / S (the population variance of B: mean(c^4) - Evar^2), all from ONE fg_diag_rhat_ess call on the rows;
//      mcse_sd = sqrt(V / ess_sq / Evar / 4) (Kenney and Keeping, as posterior::mcse_sd)
//   3  per probability p: k_p = floor((S - 1) p), q_p = sorted[k_p], I_p(x) = key(x) <= key(sorted[k_p]) ? 1 : 0, ess_quantile_p = ESS(I_p);
//      the type-7 quantile: h = (S - 1) p, g = h - k_p, a = sorted[k_p], b = sorted[min(k_p + 1, S - 1)], q7 = a if a == b or g == 0,
//      else (1 - g) a + g b
//   4  alpha = ess_quantile_p p + 1, beta = ess_quantile_p (1 - p) + 1, a1 = betaincinv(alpha, beta, 0.15865525393145707),
//      a2 = betaincinv(alpha, beta, 0.8413447460685429); i_lo = max(floor(a1 S), 1) - 1, i_hi = min(ceil(a2 S), S) - 1 (each product
//      rounded once); th_lo = sorted[i_lo], th_hi = sorted[i_hi], mcse_quantile_p = 0.5 (th_hi - th_lo).  ess_quantile_p not finite or
//      not positive: no positions (-1), th_lo, th_hi and mcse_quantile_p NaN
//   5  median = fg_rank_median of the first sort; mad = 1.4826 fg_rank_median of the sorted |x - median| (R's constant); NaN if a folded
//      cell is NaN
//   6  a NaN cell makes every word of its coordinate NaN (its count is reported); +-inf cells are ordinary values of the sort, and what
//      passes through the mean is NaN or +-inf by plain IEEE evaluation of the formulas above
//   7  the ESS is the reference's estimator (fg_diag_rhat_ess: whole chains, Geyer's sequence as the reference truncates it) applied to
//      the same rows as `posterior`, which applies Stan's split-chain FFT estimator; transforms, Beta rule and formulas are `posterior`'s
#pragma once
#include "fg_diag_rank_plan.h"

#define FG_MCSE_Y_LO 0.15865525393145707          /* pnorm(-1) */
#define FG_MCSE_Y_HI 0.8413447460685429           /* pnorm(+1) */
#define FG_MCSE_MAD_CONSTANT 1.4826               /* R's mad() */
#define FG_MCSE_THREADS 256                       /* k_mcse_rows, k_mcse_gather */

FG_RANK_HD int fg_mcse_rows(int n_probs) { return 2 + n_probs; }
FG_RANK_HD int fg_mcse_words(int n_probs) { return FG_MCSE_FIXED_WORDS + FG_MCSE_PROB_WORDS * n_probs; }
FG_RANK_HD int fg_mcse_counts(int n_probs) { return FG_MCSE_FIXED_COUNTS + FG_MCSE_PROB_COUNTS * n_probs; }
// keys a block gathers per coordinate: the two median positions, then per probability k_p, min(k_p + 1, S - 1); later i_lo, i_hi
FG_RANK_HD int fg_mcse_pairs(int n_probs) { return 2 + 2 * n_probs; }

// the rows of one cell: c = x - mean is one subtraction, c c one multiplication
FG_RANK_HD double fg_mcse_centre(double x, double mean) { return x - mean; }
FG_RANK_HD double fg_mcse_row_abs(double c) { return fabs(c); }
FG_RANK_HD double fg_mcse_row_sq(double c) { return c * c; }
FG_RANK_HD double fg_mcse_indicator(uint64_t key, uint64_t key_at_kp) { return key <= key_at_kp ? 1.0 : 0.0; }

// the interpolated type-7 quantile from the two neighbouring order statistics
inline double fg_mcse_q7(int64_t S, double p, int64_t k_p, double a, double b) {
    const double h = (double)(S - 1) * p;
    const double g = h - (double)k_p;
    if (a == b || g == 0.0) return a;
    const double ta = (1.0 - g) * a, tb = g * b;
    return ta + tb;
}
inline double fg_mcse_mean_error(double sd, double ess_mean) { return sd / sqrt(ess_mean); }
inline double fg_mcse_sd_error(double std_b, double evar, double ess_sq, int64_t S) {
    const double V = std_b * std_b * (double)(S - 1) / (double)S;
    return sqrt(V / ess_sq / evar / 4.0);
}
inline double fg_mcse_mad(double a, double b, int64_t n_nan_folded) {
    if (n_nan_folded > 0) return std::nan("");
    return FG_MCSE_MAD_CONSTANT * fg_rank_median(a, b);
}

// ---- the regularised incomplete beta function and its inverse, host only, for a, b >= 1 ---------------------------------------------
// lgamma(x) - ((x - 1/2) log x - x + log(2 pi) / 2): Stirling's series from x = 10 on, the difference itself below
inline double fg_mcse_stirling_corr(double x) {
    if (x < 10.0) return lgamma(x) - ((x - 0.5) * log(x) - x + 0.91893853320467274178);
    const double r = 1.0 / x, r2 = r * r;
    // B_2k / (2k (2k - 1)): 1/12, -1/360, 1/1260, -1/1680, 1/1188, -691/360360, 1/156
    return r * (1.0 / 12.0 + r2 * (-1.0 / 360.0 + r2 * (1.0 / 1260.0 + r2 * (-1.0 / 1680.0 + r2 * (1.0 / 1188.0 + r2 * (-691.0 / 360360.0 + r2 * (1.0 / 156.0)))))));
}
// log(1 + u) - u without the cancellation near 0
inline double fg_mcse_log1pmx(double u) {
    if (fabs(u) >= 0.1) return log1p(u) - u;
    double term = -u, sum = 0.0;                   // - sum_{k >= 2} (-u)^k / k
    for (int k = 2; k < 64; ++k) {
        term *= -u;
        const double add = -term / (double)k;
        sum += add;
        if (fabs(add) <= 1e-18 * fabs(sum)) break;
    }
    return sum;
}
// x^a (1 - x)^b / B(a, b), 0 < x < 1: with x0 = a / (a + b), a log(x / x0) + b log((1 - x) / (1 - x0)) = a log1pmx(u1) + b log1pmx(u2)
// (the linear terms a u1 + b u2 vanish), so nothing of size a or b is ever subtracted; the rest is Stirling's form of 1 / B(a, b)
inline double fg_mcse_beta_front(double a, double b, double x) {
    const double s = a + b;
    const double u1 = (x * s - a) / a, u2 = ((1.0 - x) * s - b) / b;
    const double e = a * fg_mcse_log1pmx(u1) + b * fg_mcse_log1pmx(u2) - (fg_mcse_stirling_corr(a) + fg_mcse_stirling_corr(b) - fg_mcse_stirling_corr(s));
    return sqrt(a * b / (s * 6.283185307179586476925)) * exp(e);
}
// the continued fraction of I_x(a, b) by the modified Lentz method (Numerical Recipes 6.4; Lentz 1976, Thompson and Barnett 1986)
inline double fg_mcse_beta_cf(double a, double b, double x) {
    const double tiny = 1e-300, eps = 2.3e-16;     // a factor within one place of 1 ends the fraction
    const double qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * x / qap;
    if (fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 4000000; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * x / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d; if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d; if (fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (fabs(del - 1.0) <= eps) break;
    }
    return h;
}
// I_x(a, b); `upper`, if given, receives 1 - I_x(a, b) computed without the subtraction on its own side of the symmetry switch
inline double fg_mcse_betainc(double a, double b, double x, double *upper = nullptr) {
    double lo, hi;
    if (!(x > 0.0)) { lo = 0.0; hi = 1.0; }
    else if (!(x < 1.0)) { lo = 1.0; hi = 0.0; }
    else if (x < (a + 1.0) / (a + b + 2.0)) { lo = fg_mcse_beta_front(a, b, x) * fg_mcse_beta_cf(a, b, x) / a; hi = 1.0 - lo; }
    else { hi = fg_mcse_beta_front(a, b, x) * fg_mcse_beta_cf(b, a, 1.0 - x) / b; lo = 1.0 - hi; }
    if (upper) *upper = hi;
    return lo;
}
// x in [0, 1] with I_x(a, b) = y: Newton steps from the normal approximation, kept inside a bracket that only shrinks; a step that
// would leave the bracket is a bisection.  The residual is taken on the side of the symmetry switch that is computed directly.
inline double fg_mcse_betaincinv(double a, double b, double y) {
    if (!(y > 0.0)) return 0.0;
    if (!(y < 1.0)) return 1.0;
    double lo = 0.0, hi = 1.0;
    const double s = a + b, x0 = a / s, sd = sqrt(a * b / (s * s * (s + 1.0)));
    double x = x0 + (y < 0.5 ? -sd : sd);
    if (!(x > 0.0 && x < 1.0)) x = 0.5;
    for (int it = 0; it < 400; ++it) {
        double up;
        const double low = fg_mcse_betainc(a, b, x, &up);
        const double f = low <= 0.5 ? low - y : (1.0 - y) - up;
        if (f == 0.0) return x;
        if (f < 0.0) lo = x; else hi = x;
        const double pdf = fg_mcse_beta_front(a, b, x) / (x * (1.0 - x));
        double nx = x - f / pdf;
        if (!(nx > lo && nx < hi)) nx = 0.5 * lo + 0.5 * hi;
        if (!(nx > lo && nx < hi)) return x;       // the bracket has no double inside
        const double step = fabs(nx - x);
        x = nx;
        if (step <= 4.5e-16 * x) break;
    }
    return x;
}

// FG_E_BAD_ARG: S < 1, p outside [0, 1] (or NaN), ess not finite or not positive, a null pointer
inline int fg_mcse_ranks(int64_t S, double p, double ess, int64_t *i_lo, int64_t *i_hi) {
    if (!i_lo || !i_hi || S < 1 || !(p >= 0.0 && p <= 1.0) || !(ess > 0.0) || std::isinf(ess)) return FG_E_BAD_ARG;
    const double alpha = ess * p + 1.0, beta = ess * (1.0 - p) + 1.0;
    const double a1 = fg_mcse_betaincinv(alpha, beta, FG_MCSE_Y_LO), a2 = fg_mcse_betaincinv(alpha, beta, FG_MCSE_Y_HI);
    const double f1 = floor(a1 * (double)S), f2 = ceil(a2 * (double)S);
    const int64_t l = (int64_t)f1, h = (int64_t)f2;
    *i_lo = (l > 1 ? l : 1) - 1;
    *i_hi = (h < S ? h : S) - 1;                   // a2 > 0, so ceil(a2 S) >= 1
    return FG_OK;
}

struct FgMcsePlan {
    FgRankPlan rank;                               // the sort's blocks and buffers; its k_lo / k_hi are not used
    int n_probs, rows;
    long long k_p[FG_MCSE_MAX_PROBS];
    size_t b_coord_out;                            // bytes of d_out per coordinate: n x rows x C doubles
    size_t b_coord_keys;                           // the sorted keys kept per coordinate of a block: 8 S
};

// FG_E_BAD_ARG: fg_rank_plan's (n, C, d, the block), n_probs outside [1, 8], a null h_probs, a probability outside [0, 1] (or NaN).
// FG_E_LIMIT: S = n C >= 2^31.
inline int fg_mcse_plan(long long n, long long C, long long d, long long j0, long long n_j, const double *h_probs, int n_probs, FgMcsePlan *out) {
    if (!h_probs || n_probs < 1 || n_probs > FG_MCSE_MAX_PROBS) return FG_E_BAD_ARG;
    for (int i = 0; i < n_probs; ++i) if (!(h_probs[i] >= 0.0 && h_probs[i] <= 1.0)) return FG_E_BAD_ARG;
    FgMcsePlan p;
    if (int rc = fg_rank_plan(n, C, d, j0, n_j, 0.0, 1.0, &p.rank)) return rc;
    p.n_probs = n_probs;
    p.rows = fg_mcse_rows(n_probs);
    for (int i = 0; i < FG_MCSE_MAX_PROBS; ++i) p.k_p[i] = i < n_probs ? fg_rank_kp(p.rank.S, h_probs[i]) : 0;
    p.b_coord_out = (size_t)n * (size_t)p.rows * (size_t)C * 8;
    p.b_coord_keys = (size_t)p.rank.S * 8;
    *out = p;
    return FG_OK;
}
// coordinates of one block of fg_diag_mcse: as many as keep the rows and the kept sorted keys under max_out_bytes (0: the default), at
// least one; fg_diag_rhat_ess takes at most 65535 rows
inline long long fg_mcse_block(const FgMcsePlan &p, long long d, long long max_out_bytes) {
    const long long budget = max_out_bytes > 0 ? max_out_bytes : FG_RANK_DEFAULT_OUT_BYTES;
    long long per = budget / (long long)(p.b_coord_out + p.b_coord_keys);
    if (per < 1) per = 1;
    const long long cap = 65535 / p.rows;
    if (per > cap) per = cap;
    return per > d ? d : per;
}

// the words of one coordinate.  raw4: mean, sd, rhat, ess_mean of the raw draws; ess_rows / mean_rows / std_rows [rows]: the
// combination's figures of the coordinate's rows; sorted_at [fg_mcse_pairs]: the values at the two median positions, then per
// probability at k_p and min(k_p + 1, S - 1); th [2 n_probs]: the values at i_lo, i_hi (read only where the positions exist).
inline void fg_mcse_figures(const FgMcsePlan &P, const double *h_probs, const double raw4[4], const double *ess_rows, const double *mean_rows, const double *std_rows,
                            const double *sorted_at, double mad, const double *th, const int64_t *counts, double *w) {
    const double nan = std::nan("");
    w[0] = raw4[0]; w[1] = raw4[1]; w[2] = raw4[2]; w[3] = raw4[3];
    w[4] = fg_mcse_mean_error(w[1], w[3]);
    w[5] = ess_rows[0]; w[6] = ess_rows[1];
    w[7] = fg_mcse_sd_error(std_rows[1], mean_rows[1], ess_rows[1], P.rank.S);
    w[8] = fg_rank_median(sorted_at[0], sorted_at[1]);
    w[9] = mad;
    for (int i = 0; i < P.n_probs; ++i) {
        double *q = w + FG_MCSE_FIXED_WORDS + FG_MCSE_PROB_WORDS * i;
        const int64_t *c = counts + FG_MCSE_FIXED_COUNTS + FG_MCSE_PROB_COUNTS * i;
        q[0] = sorted_at[2 + 2 * i];
        q[1] = fg_mcse_q7(P.rank.S, h_probs[i], P.k_p[i], sorted_at[2 + 2 * i], sorted_at[3 + 2 * i]);
        q[2] = ess_rows[2 + i];
        const bool have = c[1] >= 0 && c[2] >= 0;
        q[4] = have ? th[2 * i] : nan;
        q[5] = have ? th[2 * i + 1] : nan;
        q[3] = have ? 0.5 * (q[5] - q[4]) : nan;
    }
    if (counts[1] > 0) for (int i = 0; i < fg_mcse_words(P.n_probs); ++i) w[i] = nan;
}
