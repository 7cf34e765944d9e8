// fg_psis_plan.h -- the host side of Pareto-smoothed importance-sampling LOO on a stored pointwise log-likelihood table
// d_ll [n][n_sel][C] (fg_psis.hip; Vehtari, Simpson, Gelman, Yao, Gabry; the generalised Pareto fit of Zhang and Stephens 2009 with
// the weakly informative prior, as the R `loo` package's psis / gpdfit state it; r_eff = 1; the reference has none of it).  Plain
// C++ (no HIP, no engine): the device code and tests/cpp/psis_plan_driver.cpp both call it.  DESIGN 3.22.
//
// Integers of a statement of S = n C pooled cells:
//   M   the tail length: min(ceil(S / 5), b), b the smallest integer with b b >= 9 S; no fit below FG_PSIS_MIN_TAIL
//   G   the profile points of the fit: 30 + floor(sqrt M);  the quartile t* = t_(floor((M + 2) / 4)), 1-based
//   P   the padded sort length: the smallest power of two >= max(M, 2)
//
// Select.  The CUTOFF is the cell of rank r = min(M + 1, S) in fg_qs_key's order, found by radix select over FG_PSIS_DIGIT_BITS-bit
// digits from the top, fg_psis_passes() passes over the table; each pass leaves per statement the prefix decided so far, the rank
// inside the bucket and the count of cells below the bucket.  After the last pass: the cutoff key kc, L cells strictly below it and
// E cells equal to it.  The TAIL is the L cells below kc and M - L copies of kc (L <= M <= L + E whenever S > M); the M-th
// smallest key is kc when L < M and the largest collected key otherwise.  The BODY holds the cells above kc and E - (M - L) copies of kc.
//
// THE SUMMATION ORDERS, functions of (S, M) alone -- never of n_sel, the slicing of the statements or the grid:
//   a sum over the pooled cells (the body's sum exp(x_min - x), lppd's sum exp(x - x_max)); cell i = draw i / C, chain i % C:
//     1. NB = fg_psis_blocks(S) blocks of FG_PSIS_THREADS threads; thread t of block b adds the cells b T + t, + NB T, + 2 NB T, ...
//        (< S) in that sequence, starting from +0.0 (a cell that does not take part adds +0.0);
//     2. each wave of 64 folds its partials by halves: lane l takes v[l] + v[l ^ 32], then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1;
//     3. the wave totals of a block are added in wave order, starting from +0.0;
//     4. the NB block partials, padded with +0.0 to the next power of two NBP, are folded by halves: a[i] += a[i + h] for
//        h = NBP / 2, ..., 1; a[0] is the sum.
//   a sum over the M tail values (every profile sum, k_raw, the two sums of the smoothed tail), j = 0 ... M - 1 in ascending ratio:
//     1. lane l of ONE wave adds the terms l, l + 64, l + 128, ... (< M) in that sequence, starting from +0.0;
//     2. the 64 partials are folded by halves as above.
//   the G terms of the softmax and of theta-hat are added in index order, starting from +0.0.
// The sums over the cells run in double on the device.  The sums over the tail and the G terms run in double-double there (fg_psis_dd.h;
// a partial is a pair hi, lo and an addition fg_dd_add) and a word is rounded once at the end; the restatement runs every order in
// double and, to size the tolerances, in long double.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/fugue_amd.h"

#define FG_PSIS_MIN_TAIL 5
#define FG_PSIS_S_MAX 0x7fffffffLL               /* S < 2^31: a cell index and every count fit 32 bits */
#define FG_PSIS_DIGIT_BITS 11                     /* 2 048 bins of u32 in LDS: 8 KiB */
#define FG_PSIS_THREADS 256                       /* select and collect */
#define FG_PSIS_CELLS_PER_BLOCK 4096              /* cells a block takes before NB grows */
#define FG_PSIS_MAX_BLOCKS 256                    /* NB's cap: the fit folds the partials in LDS */
#define FG_PSIS_FIT_THREADS 1024                  /* one workgroup per statement */
#define FG_PSIS_SORT_CHUNK 4096                   /* keys of a bitonic stage that runs in LDS: 32 KiB */
#define FG_PSIS_G_MAX 512                         /* G <= 30 + floor(sqrt(M(2^31 - 1))) = 402 */
#define FG_PSIS_MAX_GRID_Y 65535
#define FG_PSIS_WORK_BYTES (1ll << 30)            /* the work buffers of one slice of statements */
#define FG_PSIS_STATE_WORDS 8                     /* u64 per statement: prefix, rank, below, equal, min key, max key (no NaN), cursor, spare */
enum { FG_PSIS_ST_PREFIX = 0, FG_PSIS_ST_RANK, FG_PSIS_ST_BELOW, FG_PSIS_ST_EQUAL, FG_PSIS_ST_MIN, FG_PSIS_ST_MAX, FG_PSIS_ST_CURSOR, FG_PSIS_ST_SPARE };
#define FG_PSIS_CLASS_WORDS 4                     /* u32 per statement: -inf, +inf, NaN, spare */

// the smallest b with b b >= v
inline long long fg_psis_isqrt_ceil(long long v) {
    long long lo = 0, hi = 3037000499ll;          // floor(sqrt(2^63 - 1))
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (mid * mid >= v) hi = mid; else lo = mid + 1;
    }
    return lo;
}
inline long long fg_psis_isqrt_floor(long long v) {
    const long long c = fg_psis_isqrt_ceil(v);
    return c * c == v ? c : c - 1;
}
// M, or FG_E_BAD_ARG (S < 1) / FG_E_LIMIT (S >= 2^31)
inline long long fg_psis_tail(long long S) {
    if (S < 1) return FG_E_BAD_ARG;
    if (S > FG_PSIS_S_MAX) return FG_E_LIMIT;
    const long long a = (S + 4) / 5, b = fg_psis_isqrt_ceil(9 * S);
    return a < b ? a : b;
}
inline int fg_psis_profile_points(long long M) { return 30 + (int)fg_psis_isqrt_floor(M); }
inline long long fg_psis_quartile_index(long long M) { return (M + 2) / 4; }      // 1-based
inline int fg_psis_passes() { return (64 + FG_PSIS_DIGIT_BITS - 1) / FG_PSIS_DIGIT_BITS; }
// pass p decides bits [64 - b - w, 64 - b) of the key, b = p FG_PSIS_DIGIT_BITS
inline int fg_psis_pass_width(int p) { const int b = p * FG_PSIS_DIGIT_BITS; return 64 - b < FG_PSIS_DIGIT_BITS ? 64 - b : FG_PSIS_DIGIT_BITS; }
inline long long fg_psis_pow2(long long v) { long long p = 1; while (p < v) p *= 2; return p; }
inline long long fg_psis_sort_len(long long M) { return fg_psis_pow2(M < 2 ? 2 : M); }
inline unsigned fg_psis_blocks(long long S) {
    const long long nb = (S + FG_PSIS_CELLS_PER_BLOCK - 1) / FG_PSIS_CELLS_PER_BLOCK;
    return (unsigned)(nb < 1 ? 1 : (nb > FG_PSIS_MAX_BLOCKS ? FG_PSIS_MAX_BLOCKS : nb));
}

struct FgPsisPlan {
    long long S, M, P; int G; long long tstar;     // per statement
    long long rank;                                // of the cutoff, 1-based: min(M + 1, S)
    unsigned nb, nbp;                              // blocks per statement of a pass, and padded to a power of two
    int passes;
    long long rows_per;                            // statements of one slice: the work budget and the grid's y
    // bytes of the work buffers of a slice of `rows_per` statements
    size_t b_state, b_class, b_hist, b_part, b_tail, b_sort, b_t, b_fig, b_cnt, b_row;
};

// FG_E_BAD_ARG: n < 1, C < 1, n_sel < 1; FG_E_LIMIT: S = n C >= 2^31, or one statement's work buffers above FG_PSIS_WORK_BYTES
inline int fg_psis_plan(long long n, long long C, long long n_sel, FgPsisPlan *out) {
    if (n < 1 || C < 1 || n_sel < 1 || n_sel > 0x7fffffffLL) return FG_E_BAD_ARG;
    if (n > FG_PSIS_S_MAX || C > FG_PSIS_S_MAX || n * C > FG_PSIS_S_MAX) return FG_E_LIMIT;
    FgPsisPlan p;
    p.S = n * C;
    p.M = fg_psis_tail(p.S);
    p.P = fg_psis_sort_len(p.M);
    p.G = fg_psis_profile_points(p.M);
    p.tstar = fg_psis_quartile_index(p.M);
    p.rank = p.M + 1 < p.S ? p.M + 1 : p.S;
    p.nb = fg_psis_blocks(p.S);
    p.nbp = (unsigned)fg_psis_pow2(p.nb);
    p.passes = fg_psis_passes();
    if (p.G > FG_PSIS_G_MAX) return FG_E_LIMIT;
    p.b_row = (size_t)FG_PSIS_STATE_WORDS * 8 + (size_t)FG_PSIS_CLASS_WORDS * 4 + ((size_t)4 << FG_PSIS_DIGIT_BITS) + (size_t)p.nb * 2 * 8 + (size_t)p.M * 8 + (size_t)p.P * 8 +
              (size_t)p.M * 16 + (size_t)FG_PSIS_WORDS * 8 + (size_t)FG_PSIS_COUNTS * 8;
    if (p.b_row > (size_t)FG_PSIS_WORK_BYTES) return FG_E_LIMIT;
    long long per = FG_PSIS_WORK_BYTES / (long long)p.b_row;
    if (per > FG_PSIS_MAX_GRID_Y) per = FG_PSIS_MAX_GRID_Y;
    if (per > n_sel) per = n_sel;
    p.rows_per = per;
    const size_t r = (size_t)per;
    p.b_state = r * FG_PSIS_STATE_WORDS * 8;
    p.b_class = r * FG_PSIS_CLASS_WORDS * 4;
    p.b_hist = r * ((size_t)4 << FG_PSIS_DIGIT_BITS);
    p.b_part = r * p.nb * 2 * 8;
    p.b_tail = r * (size_t)p.M * 8;
    p.b_sort = r * (size_t)p.P * 8;
    p.b_t = r * (size_t)p.M * 16;
    p.b_fig = r * FG_PSIS_WORDS * 8;
    p.b_cnt = r * FG_PSIS_COUNTS * 8;
    *out = p;
    return FG_OK;
}
// the cell of (block, thread, slot) in a pass over the S pooled cells, or -1
inline long long fg_psis_cell(const FgPsisPlan &p, unsigned block, int thread, long long slot) {
    const long long i = ((long long)slot * p.nb + block) * FG_PSIS_THREADS + thread;
    return i < p.S ? i : -1;
}
// the tail term of (lane, slot) of the wave that sums it, or -1
inline long long fg_psis_tail_term(const FgPsisPlan &p, int lane, long long slot) {
    const long long j = slot * 64 + lane;
    return j < p.M ? j : -1;
}
#ifdef __HIPCC__
#define FG_PSIS_HD __host__ __device__ inline
#else
#define FG_PSIS_HD inline
#endif
// The selection step on `nbins` counts whose total is at least rank >= 1: the first bin d with h[0] + ... + h[d] >= rank (the last bin
// if none); *before = h[0] + ... + h[d - 1].  A pass applies it twice: to the sums of FG_PSIS_PICK_GROUP consecutive digits, then inside
// the group it names.
#define FG_PSIS_PICK_GROUP ((1 << FG_PSIS_DIGIT_BITS) / FG_PSIS_THREADS)
FG_PSIS_HD int fg_psis_pick_bin(const unsigned int *h, int nbins, unsigned long long rank, unsigned long long *before) {
    unsigned long long cum = 0;
    int d = 0;
    for (; d < nbins - 1; ++d) { if (cum + h[d] >= rank) break; cum += h[d]; }
    *before = cum;
    return d;
}
// the state of a statement after a pass of width w at b decided bits, from the digit and the cells before it
FG_PSIS_HD void fg_psis_advance(unsigned long long *st, int b, int w, int digit, unsigned long long before, unsigned long long in_digit) {
    st[FG_PSIS_ST_PREFIX] |= (unsigned long long)digit << (64 - b - w);
    st[FG_PSIS_ST_RANK] -= before;
    st[FG_PSIS_ST_BELOW] += before;
    st[FG_PSIS_ST_EQUAL] = in_digit;
}

// khat's threshold: min(1 - 1 / log10 S, 0.7)
inline double fg_psis_threshold(long long S) {
    const double t = 1.0 - 1.0 / std::log10((double)S);
    return t < 0.7 ? t : 0.7;
}

#ifdef __HIPCC__
// fg_qs_key / fg_sort_key: ascending in the double's order, -0.0 just below +0.0, positive-sign NaN above +inf
__device__ __forceinline__ unsigned long long fg_psis_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double fg_psis_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}
#endif
