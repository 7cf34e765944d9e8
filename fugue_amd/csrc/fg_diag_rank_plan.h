// fg_diag_rank_plan.h -- the rule of the rank-normalised diagnostics (fg_diag_rank.hip; Vehtari, Gelman, Simpson, Carpenter, Buerkner
// 2021, "Rank-normalization, folding, and localization: an improved R-hat"; the reference has none of it).  Plain C++ (no HIP, no
// engine): the device code and tests/cpp/rank_driver.cpp both call it; tests/rank_restatement.py restates it in numpy.  DESIGN 3.23.
//
// One coordinate of d_draws [n][d][C] is S = n C pooled cells; cell i = draw i / C, chain i % C.
//   key     fg_rank_key: fg_qs_key's order with -0.0 keyed as +0.0 and every NaN on ONE key above +inf: ties are ties of values
//   ranks   lo(x) = cells with a smaller key, hi(x) = cells with a smaller or equal key, r2 = lo + hi + 1 in [2, 2 S]: the doubled
//           average rank
//   z       fg_rank_z(r2, S) = ndtri((r - 3/8) / (S + 1/4)), r = r2 / 2, through integer numerators (each quotient rounded once) and
//           Wichura's AS241 PPND16 in the published Horner order; z(r2) = -z(2 S + 2 - r2) exactly
//   median  fg_rank_median(sorted[(S - 1) / 2], sorted[S / 2])
//   fold    fg_rank_fold(x, med) = |x - med| in double (NaN for a NaN cell and for inf - inf); sorted a second time under the same key
//   tails   k_p = fg_rank_kp(S, p) = floor((S - 1) p); I_p(x) = lo(x) <= k_p ? 1 : 0, that is x <= sorted[k_p]
// NaN cells are one tie run at the top and take that run's ranks; the figures of such a coordinate are NaN (fg_rank_figures).
//
// THE SORT: a stable least-significant-digit radix sort of (key, cell index), FG_RANK_DIGIT_BITS bits a pass, FG_RANK_PASSES passes.
// A pass whose digit is the same in every cell (one bin of its histogram holds all S) is skipped.  A block of a pass owns the
// FG_RANK_TILE consecutive positions [b TILE, (b + 1) TILE) of the pass's input; inside it wave w owns FG_RANK_WAVE_TILE consecutive
// positions and lane l of round k the position w WAVE_TILE + 64 k + l.  The output position of an element is
//     (cells of smaller digits) + (cells of its digit in earlier blocks) + (cells of its digit earlier in its block):
// integers only, so the permutation -- the stable one -- and every output bit are independent of the grid and of scheduling.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/fugue_amd.h"

#ifdef __HIPCC__
#define FG_RANK_HD __host__ __device__ inline
#else
#define FG_RANK_HD inline
#endif

#define FG_RANK_S_MAX 0x7fffffffLL                /* S < 2^31: a cell index and r2 = lo + hi + 1 <= 2 S fit 32 bits */
#define FG_RANK_DIGIT_BITS 8
#define FG_RANK_BINS 256
#define FG_RANK_PASSES 8
#define FG_RANK_THREADS 256                       /* sort kernels */
#define FG_RANK_WAVES (FG_RANK_THREADS / 64)
#define FG_RANK_ITEMS 16                          /* rounds of a wave */
#define FG_RANK_WAVE_TILE (64 * FG_RANK_ITEMS)
#define FG_RANK_TILE (FG_RANK_THREADS * FG_RANK_ITEMS)
#define FG_RANK_RUN_THREADS 256                   /* run pass: a thread owns FG_RANK_RUN_ITEMS consecutive sorted positions */
#define FG_RANK_RUN_ITEMS 4
#define FG_RANK_RUN_TILE (FG_RANK_RUN_THREADS * FG_RANK_RUN_ITEMS)
#define FG_RANK_KEY_BLOCKS 1024                   /* the key pass's grid cap (grid-stride; its histograms are integer counts) */
#define FG_RANK_STAT_WORDS 8                      /* u32 per sort: -inf, +inf, NaN cells, tie runs, longest run, spare x 3 */
#define FG_RANK_DEFAULT_OUT_BYTES (1ll << 30)
#define FG_RANK_NAN_KEY 0xfff8000000000000ull     /* above fg_rank_key(+inf) = 0xfff0000000000000 */

FG_RANK_HD uint64_t fg_rank_bits(double v) { uint64_t u; memcpy(&u, &v, 8); return u; }
FG_RANK_HD double fg_rank_from_bits(uint64_t u) { double v; memcpy(&v, &u, 8); return v; }
FG_RANK_HD uint64_t fg_rank_key(double v) {
    if (v != v) return FG_RANK_NAN_KEY;
    const uint64_t u = v == 0.0 ? 0ull : fg_rank_bits(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
FG_RANK_HD double fg_rank_unkey(uint64_t k) {
    if (k == FG_RANK_NAN_KEY) return fg_rank_from_bits(0x7ff8000000000000ull);
    return fg_rank_from_bits((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k);
}

// AS241 PPND16: the polynomials, highest power first (eight coefficients each)
FG_RANK_HD double fg_rank_horner(const double *c, double r) {
    double v = c[0];
    for (int i = 1; i < 8; ++i) v = v * r + c[i];
    return v;
}
FG_RANK_HD double fg_rank_z(int64_t r2, int64_t S) {
    const double A[8] = { 2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
                          1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0 };
    const double B[8] = { 5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
                          5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0 };
    const double Cc[8] = { 7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
                           3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0 };
    const double D[8] = { 1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
                          6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0 };
    const double E[8] = { 2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
                          2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0 };
    const double F[8] = { 2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
                          1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0 };
    const double q = (double)(2 * r2 - 2 * S - 2) / (double)(4 * S + 1);
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        return fg_rank_horner(A, r) * q / fg_rank_horner(B, r);
    }
    const int64_t a = 4 * r2 - 3, b = 8 * S + 2 - a;
    const double pt = (double)(a < b ? a : b) / (double)(8 * S + 2);
    double r = sqrt(-log(pt)), x;
    if (r <= 5.0) { r = r - 1.6; x = fg_rank_horner(Cc, r) / fg_rank_horner(D, r); }
    else { r = r - 5.0; x = fg_rank_horner(E, r) / fg_rank_horner(F, r); }
    return q < 0.0 ? -x : x;
}
FG_RANK_HD double fg_rank_median(double a, double b) { return a == b ? a : 0.5 * a + 0.5 * b; }
FG_RANK_HD double fg_rank_fold(double x, double med) { return fabs(x - med); }
FG_RANK_HD int64_t fg_rank_kp(int64_t S, double p) { return (int64_t)floor((double)(S - 1) * p); }

struct FgRankPlan {
    long long S;
    long long k_lo, k_hi;                          // the tail indicators' order statistics
    unsigned nb, nb_run, nb_key;                   // blocks of a radix pass, of the run pass, of the key pass
    size_t b_keys, b_idx, b_table, b_hist, b_stat, b_carry;      // one of the two key / index buffers, the scan table, ...
    size_t b_coord_out;                            // bytes of d_out per coordinate: n x FG_RANK_ROWS x C doubles
};

// FG_E_BAD_ARG: n < 1, C < 1, d outside [1, 65535], the block [j0, j0 + n_j) outside [0, d) or empty, a probability outside [0, 1] (or
// NaN), p_lo > p_hi.  FG_E_LIMIT: S = n C >= 2^31.
inline int fg_rank_plan(long long n, long long C, long long d, long long j0, long long n_j, double p_lo, double p_hi, FgRankPlan *out) {
    if (n < 1 || C < 1 || d < 1 || d > 65535 || j0 < 0 || n_j < 1 || j0 >= d || n_j > d - j0) return FG_E_BAD_ARG;
    if (!(p_lo >= 0.0 && p_lo <= 1.0 && p_hi >= 0.0 && p_hi <= 1.0 && p_lo <= p_hi)) return FG_E_BAD_ARG;
    if (n > FG_RANK_S_MAX || C > FG_RANK_S_MAX || n * C > FG_RANK_S_MAX) return FG_E_LIMIT;
    FgRankPlan p;
    p.S = n * C;
    p.k_lo = fg_rank_kp(p.S, p_lo);
    p.k_hi = fg_rank_kp(p.S, p_hi);
    p.nb = (unsigned)((p.S + FG_RANK_TILE - 1) / FG_RANK_TILE);
    p.nb_run = (unsigned)((p.S + FG_RANK_RUN_TILE - 1) / FG_RANK_RUN_TILE);
    const long long nk = (p.S + FG_RANK_THREADS - 1) / FG_RANK_THREADS;
    p.nb_key = (unsigned)(nk > FG_RANK_KEY_BLOCKS ? FG_RANK_KEY_BLOCKS : nk);
    p.b_keys = (size_t)p.S * 8;
    p.b_idx = (size_t)p.S * 4;
    p.b_table = (size_t)FG_RANK_BINS * p.nb * 4;
    p.b_hist = (size_t)FG_RANK_PASSES * FG_RANK_BINS * 4;
    p.b_stat = (size_t)FG_RANK_STAT_WORDS * 4;
    p.b_carry = (size_t)p.nb_run * 2 * 4;
    p.b_coord_out = (size_t)n * FG_RANK_ROWS * (size_t)C * 8;
    *out = p;
    return FG_OK;
}
// coordinates of one block of fg_diag_rank_rhat_ess: as many as keep d_out under max_out_bytes (0: the default), at least one
inline long long fg_rank_block(const FgRankPlan &p, long long d, long long max_out_bytes) {
    const long long budget = max_out_bytes > 0 ? max_out_bytes : FG_RANK_DEFAULT_OUT_BYTES;
    long long per = budget / (long long)p.b_coord_out;
    if (per < 1) per = 1;
    const long long cap = 65535 / FG_RANK_ROWS;    // fg_diag_rhat_ess takes at most 65535 rows
    if (per > cap) per = cap;
    return per > d ? d : per;
}
// whether a pass is skipped: one bin of its histogram holds every cell
FG_RANK_HD bool fg_rank_pass_skipped(const unsigned int *hist256, long long S) {
    for (int b = 0; b < FG_RANK_BINS; ++b) if ((long long)hist256[b] == S) return true;
    return false;
}
// the ten figures from the library's own split R-hat / multi-chain ESS of the four transformed rows
inline void fg_rank_figures(const double rhat4[4], const double ess4[4], double median, double x_lo, double x_hi, long long n_nan, long long n_nan_folded,
                            double *w) {
    const double nan = std::nan("");
    const double rb = rhat4[0], rf = n_nan_folded > 0 ? nan : rhat4[1];
    w[0] = (rb != rb || rf != rf) ? nan : (rb > rf ? rb : rf);
    w[1] = rb; w[2] = rf;
    w[3] = ess4[0];
    w[5] = ess4[2]; w[6] = ess4[3];
    w[4] = (w[5] != w[5] || w[6] != w[6]) ? nan : (w[5] < w[6] ? w[5] : w[6]);
    w[7] = median; w[8] = x_lo; w[9] = x_hi;
    if (n_nan > 0) for (int i = 0; i < FG_RANK_WORDS; ++i) w[i] = nan;
}
