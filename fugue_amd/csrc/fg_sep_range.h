// fg_sep_range.h -- host only: the proof that the numerator n = lp(q + h) - lp(q - h) of k_hmc_sep_steps's folded trajectory loop
// (fg_hmc_sep.hip, FOLD) never leaves the window 2^-823 <= |n| < 2^953 of the two-instruction quotient by 2h unless it is +0 or not
// finite -- for ONE program and ONE h.  With it the loop issues no range test at all.  Plain C++ without a HIP call: the engine runs
// it once per configuration (fg_internal_hmc_set_cfg, next to fg_div2_prove) and tests/cpp/sep_range_driver.cpp builds it with g++.
//
// The argument ("The range test leaves the step"), K = 0.5 ln 2 pi in [0.5, 1):
//   * lower side, every program: a term of the folded loop is RN(r - K) for some double r, or the U0 form fma(-0.5, m, -K) <= -K.
//     Both are multiples of 2^-54 (|r| < 0.5: the difference lies in (-1.5, -0.41); |r| >= 0.5: both operands are multiples of
//     2^-53) and never -0.  Rounded sums and differences of such numbers are such numbers: n = tp - tm is +0 or |n| >= 2^-54.
//     For n = +0 the quotient fma(+0, Ch, +0 Cl) is +0 = +0 / 2h: no test needed.
//   * not finite: g = fma(n, Ch, n Cl) is inf or NaN, so is the kick hk g (0 inf = NaN), and a momentum that once was not finite stays
//     so: the caller's test of the endpoint momentum re-runs the coordinate through the checked instance, as before.
//   * upper side, this program and h: q + h != q - h needs |q| < 2^55 h (else both round to q, the two sides are the same bits
//     and n = +0).  Then |d| = |q +- h - c_k| <= D_k = 2^55 h + h + |c_k| and a term is at most M_k = 0.5 s_k^2 D_k^2 + |ln sigma_k| + K
//     in magnitude (s_k = RN(1 / sigma_k): the record's own factor, or within an ulp of the quotient by sigma_k), so
//     |n| <= 2 sum_k M_k up to the roundings of the chain -- fewer than 32 of them, each 2^-53 relative.  fg_sep_range_bound forms
//     2 sum_k M_k in doubles (its own roundings: fewer than 32 again) and scales by 1 + 2^-40, which covers both with room.
//   * verdict: every coordinate's bound is below 2^953 (a NaN or infinite bound, a non-positive or non-finite h: refused).
#pragma once
#include <cmath>
#include <cstddef>

#define FG_SEP_RANGE_HALF_LN_2PI 0.91893853320467274178       /* K, = 0.5 * FG_LN_2PI of fg_math.h */

// an upper bound of |n| for one coordinate with nrec records (constant operand c, factor s = 1 / sigma, ln sigma), finite n != 0
inline double fg_sep_range_bound(double h, int nrec, const double *c, const double *s, const double *lns) {
    const double Q = 0x1p55 * h + h;
    double sum = 0.0;
    for (int k = 0; k < nrec; ++k) {
        const double D = Q + std::fabs(c[k]);
        sum += 0.5 * (s[k] * s[k]) * (D * D) + std::fabs(lns[k]) + FG_SEP_RANGE_HALF_LN_2PI;
    }
    return 2.0 * sum * (1.0 + 0x1p-40);
}

inline bool fg_sep_range_ok(double h, double bound) { return h > 0.0 && std::isfinite(h) && bound < 0x1p953; }   // (NaN: false)

// the whole program: coordinate j's records are entries [off[j], off[j] + n[j]) of c / s / lns.  *worst: the largest bound (NaN: kept)
inline bool fg_sep_range_prove(double h, size_t ncoord, const int *off, const int *n, const double *c, const double *s, const double *lns, double *worst) {
    bool ok = ncoord > 0;
    double w = 0.0;
    for (size_t j = 0; j < ncoord; ++j) {
        const double b = fg_sep_range_bound(h, n[j], c + off[j], s + off[j], lns + off[j]);
        if (!fg_sep_range_ok(h, b)) ok = false;
        if (w == w && !(b <= w)) w = b;
    }
    if (worst) *worst = w;
    return ok;
}
