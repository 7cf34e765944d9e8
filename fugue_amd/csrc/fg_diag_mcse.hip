// fg_diag_mcse.hip -- Monte Carlo standard errors and effective sample sizes of the mean, the standard deviation and quantiles, and the
// median absolute deviation (the figures of the R `posterior` package's summarise_draws; the reference has none of it) of stored draws
// d_draws [n][d][C] on the device.  The rule, the Beta inverse and every limit are fg_diag_mcse_plan.h's; the sort is fg_diag_rank.hip's
// (fg_diag_rank_internal.h); here are the row kernel, the gather and the C ABI.  Nothing is replayed and no engine state changes: the
// calls read the engine's chain count, device and stream.  This engine's chains only.
//
//   k_mcse_rows     one read of the S = n C cells of a coordinate (chains fastest, as k_rank_keys reads them) -> the R = 2 + n_probs
//                   rows |x - mean|, (x - mean)^2 and I_p = key(x) <= key(sorted[k_p]) (the thresholds are kernel arguments) in the
//                   caller's [n][R n_j][C] layout, coalesced, and in the same read the folded key pass of the second sort: key and
//                   index of |x - median|, the eight digit histograms (LDS, integer atomics) and the folded cells' -inf / +inf / NaN counts
//   k_mcse_gather   the keys at a list of flat positions (coordinate S + position) of the kept sorted keys -> a small buffer
//   k_mcse_unkey    sorted keys -> the doubles they stand for
// Integer atomics only, and only where order cannot matter (counts).  No floating-point atomics.
#include "fg_diag_rank_internal.h"
#include "fg_diag_mcse_plan.h"

struct FgMcseRowArgs {
    const double *draws; u32 S, C; long long d, j; double mean, med;
    u64 *keys; u32 *idx; u32 *hist /*[8][256]*/, *stat;
    double *out; long long rows, row0; int n_probs;
    u64 thr[FG_MCSE_MAX_PROBS];                    // key(sorted[k_p])
};

__global__ __launch_bounds__(FG_RANK_THREADS) void k_mcse_rows(FgMcseRowArgs A) {
    __shared__ u32 sh[FG_RANK_PASSES * FG_RANK_BINS];
    for (int k = threadIdx.x; k < FG_RANK_PASSES * FG_RANK_BINS; k += FG_RANK_THREADS) sh[k] = 0u;
    __syncthreads();
    u32 c0 = 0u, c1 = 0u, c2 = 0u;
    const u64 stride = (u64)gridDim.x * FG_RANK_THREADS;
    const long long C = (long long)A.C;
    for (u64 i = (u64)blockIdx.x * FG_RANK_THREADS + threadIdx.x; i < A.S; i += stride) {
        const u32 t = (u32)i / A.C, c = (u32)i - t * A.C;
        const double x = A.draws[((long long)t * A.d + A.j) * C + (long long)c];
        const double cen = fg_mcse_centre(x, A.mean);
        const u64 k0 = fg_rank_key(x);
        double *o = A.out + ((long long)t * A.rows + A.row0) * C + (long long)c;
        o[0] = fg_mcse_row_abs(cen);
        o[C] = fg_mcse_row_sq(cen);
#pragma unroll
        for (int p = 0; p < FG_MCSE_MAX_PROBS; ++p)
            if (p < A.n_probs) o[(long long)(2 + p) * C] = fg_mcse_indicator(k0, A.thr[p]);
        const double f = fg_rank_fold(x, A.med);
        const u64 key = fg_rank_key(f);
        A.keys[i] = key;
        A.idx[i] = (u32)i;
#pragma unroll
        for (int p = 0; p < FG_RANK_PASSES; ++p) atomicAdd(&sh[p * FG_RANK_BINS + ((u32)(key >> (8 * p)) & 255u)], 1u);
        c0 += f == -INFINITY ? 1u : 0u; c1 += f == INFINITY ? 1u : 0u; c2 += f != f ? 1u : 0u;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < FG_RANK_PASSES * FG_RANK_BINS; k += FG_RANK_THREADS)
        if (sh[k]) atomicAdd(&A.hist[k], sh[k]);
    for (int o = 32; o > 0; o >>= 1) { c0 += __shfl_down(c0, o, 64); c1 += __shfl_down(c1, o, 64); c2 += __shfl_down(c2, o, 64); }
    if ((threadIdx.x & 63) == 0) {
        if (c0) atomicAdd(&A.stat[0], c0);
        if (c1) atomicAdd(&A.stat[1], c1);
        if (c2) atomicAdd(&A.stat[2], c2);
    }
}

// out[i] = keys[at[i]] for at[i] < n_keys; a position past the keys is never a read (its word is the NaN key)
__global__ __launch_bounds__(FG_MCSE_THREADS) void k_mcse_gather(const u64 *keys, u64 n_keys, const u64 *at, u32 n_at, u64 *out) {
    const u32 i = blockIdx.x * FG_MCSE_THREADS + threadIdx.x;
    if (i >= n_at) return;
    const u64 a = at[i];
    out[i] = a < n_keys ? keys[a] : FG_RANK_NAN_KEY;
}

__global__ __launch_bounds__(FG_MCSE_THREADS) void k_mcse_unkey(const u64 *keys, u64 n_keys, double *out) {
    const u64 stride = (u64)gridDim.x * FG_MCSE_THREADS;
    for (u64 i = (u64)blockIdx.x * FG_MCSE_THREADS + threadIdx.x; i < n_keys; i += stride) out[i] = fg_rank_unkey(keys[i]);
}

namespace {

struct McseWork {                              // what a call keeps beside the sort's workspace
    u64 *skeys = nullptr;                      // [per][S]: the sorted keys of every coordinate of the current block
    u64 *at = nullptr, *got = nullptr;         // [per x pairs]: a gather's positions and its keys
    u64 *at_fold = nullptr, *got_fold = nullptr;   // the two median positions of a folded sort; [per][2] the keys found there
    long long per = 0;
    int init(RankWork &W, const FgMcsePlan &P, long long per_) {
        per = per_;
        const size_t pairs = (size_t)per * fg_mcse_pairs(P.n_probs);
        if (W.alloc(&skeys, (size_t)per * P.b_coord_keys, "the sorted keys") || W.alloc(&at, pairs * 8, "the gather's positions") || W.alloc(&got, pairs * 8, "the gathered keys") ||
            W.alloc(&at_fold, 16, "the gather's positions") || W.alloc(&got_fold, (size_t)per * 16, "the gathered keys"))
            return FG_E_HIP;
        return FG_OK;
    }
};

int mcse_gather(fg_engine *e, const u64 *d_keys, u64 n_keys, const u64 *d_at, u32 n_at, u64 *d_got) {
    hipLaunchKernelGGL(k_mcse_gather, dim3((n_at + FG_MCSE_THREADS - 1) / FG_MCSE_THREADS), dim3(FG_MCSE_THREADS), 0, e->stream, d_keys, n_keys, d_at, n_at, d_got);
    HIPCHK(hipGetLastError());
    return FG_OK;
}

// coordinates [j0, j0 + n_j) (n_j <= M.per), centred at h_mean [n_j] -> d_out [n][R n_j][C]; M.skeys [n_j][S] the sorted keys;
// h_at [n_j][fg_mcse_pairs]: the values at the two median positions, then per probability at k_p and min(k_p + 1, S - 1);
// h_fold [n_j][2]: the values at the two median positions of the folded sort; h_counts [n_j][fg_mcse_counts] (i_lo, i_hi = -1)
int mcse_transform(fg_engine *e, const FgMcsePlan &P, RankWork &W, McseWork &M, const double *d_draws, int n, int d, int j0, int n_j, const double *h_mean, double *d_out,
                   double *h_at, double *h_fold, int64_t *h_counts) {
    const FgRankPlan &R = P.rank;
    const u64 S = (u64)R.S;
    const int pairs = fg_mcse_pairs(P.n_probs), nc = fg_mcse_counts(P.n_probs);
    std::vector<u32> st((size_t)n_j * 2 * FG_RANK_STAT_WORDS);
    std::vector<long long> passes((size_t)n_j, 0);
    // the first sort of every coordinate of the block; its keys are kept
    for (int k = 0; k < n_j; ++k) {
        HIPCHK(hipMemsetAsync(W.hist, 0, R.b_hist, e->stream));
        HIPCHK(hipMemsetAsync(W.stat, 0, 2 * R.b_stat, e->stream));
        if (int rc = rank_keys(e, R, W, d_draws, d, (long long)j0 + k)) return rc;
        HIPCHK(hipMemcpyAsync(&st[(size_t)k * 2 * FG_RANK_STAT_WORDS], W.stat, R.b_stat, hipMemcpyDeviceToHost, e->stream));
        int cur = 0;
        if (int rc = rank_sort(e, R, W, &cur, &passes[k])) return rc;
        HIPCHK(hipMemcpyAsync(M.skeys + (size_t)k * S, W.key[cur], R.b_keys, hipMemcpyDeviceToDevice, e->stream));
    }
    // one gather for the block: the median positions, k_p and its upper neighbour of every coordinate
    std::vector<u64> at((size_t)n_j * pairs), got((size_t)n_j * pairs);
    for (int k = 0; k < n_j; ++k) {
        u64 *a = &at[(size_t)k * pairs];
        a[0] = (u64)k * S + (u64)((R.S - 1) / 2); a[1] = (u64)k * S + (u64)(R.S / 2);
        for (int i = 0; i < P.n_probs; ++i) {
            const long long up = P.k_p[i] + 1 < R.S ? P.k_p[i] + 1 : R.S - 1;
            a[2 + 2 * i] = (u64)k * S + (u64)P.k_p[i]; a[3 + 2 * i] = (u64)k * S + (u64)up;
        }
    }
    const u64 fold_at[2] = { (u64)((R.S - 1) / 2), (u64)(R.S / 2) };
    HIPCHK(hipMemcpyAsync(M.at, at.data(), at.size() * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(M.at_fold, fold_at, 16, hipMemcpyHostToDevice, e->stream));
    if (int rc = mcse_gather(e, M.skeys, (u64)n_j * S, M.at, (u32)at.size(), M.got)) return rc;
    HIPCHK(hipMemcpyAsync(got.data(), M.got, got.size() * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (size_t i = 0; i < got.size(); ++i) h_at[i] = fg_rank_unkey(got[i]);
    // the rows and, in the same read, the folded keys; the second sort; its two median keys
    for (int k = 0; k < n_j; ++k) {
        FgMcseRowArgs A;
        A.draws = d_draws; A.S = (u32)S; A.C = (u32)e->C; A.d = d; A.j = (long long)j0 + k; A.mean = h_mean[k];
        A.med = fg_rank_median(h_at[(size_t)k * pairs], h_at[(size_t)k * pairs + 1]);
        A.keys = W.key[0]; A.idx = W.idx[0]; A.hist = W.hist; A.stat = W.stat + FG_RANK_STAT_WORDS;
        A.out = d_out; A.rows = (long long)P.rows * n_j; A.row0 = (long long)P.rows * k; A.n_probs = P.n_probs;
        for (int i = 0; i < FG_MCSE_MAX_PROBS; ++i) A.thr[i] = i < P.n_probs ? got[(size_t)k * pairs + 2 + 2 * i] : 0ull;
        HIPCHK(hipMemsetAsync(W.hist, 0, R.b_hist, e->stream));
        HIPCHK(hipMemsetAsync(W.stat, 0, 2 * R.b_stat, e->stream));
        hipLaunchKernelGGL(k_mcse_rows, dim3(R.nb_key), dim3(FG_RANK_THREADS), 0, e->stream, A);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&st[(size_t)(2 * k + 1) * FG_RANK_STAT_WORDS], W.stat + FG_RANK_STAT_WORDS, R.b_stat, hipMemcpyDeviceToHost, e->stream));
        int cur = 0;
        if (int rc = rank_sort(e, R, W, &cur, &passes[k])) return rc;
        if (int rc = mcse_gather(e, W.key[cur], S, M.at_fold, 2u, M.got_fold + 2 * (size_t)k)) return rc;
    }
    std::vector<u64> gf((size_t)2 * n_j);
    HIPCHK(hipMemcpyAsync(gf.data(), M.got_fold, gf.size() * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (int k = 0; k < n_j; ++k) {
        h_fold[2 * k] = fg_rank_unkey(gf[2 * (size_t)k]); h_fold[2 * k + 1] = fg_rank_unkey(gf[2 * (size_t)k + 1]);
        const u32 *s1 = &st[(size_t)k * 2 * FG_RANK_STAT_WORDS], *s2 = s1 + FG_RANK_STAT_WORDS;
        int64_t *c = h_counts + (size_t)k * nc;
        c[0] = R.S; c[1] = s1[2]; c[2] = s1[0]; c[3] = s1[1]; c[4] = s2[2]; c[5] = passes[k];
        for (int i = 0; i < P.n_probs; ++i) { c[FG_MCSE_FIXED_COUNTS + 3 * i] = P.k_p[i]; c[FG_MCSE_FIXED_COUNTS + 3 * i + 1] = -1; c[FG_MCSE_FIXED_COUNTS + 3 * i + 2] = -1; }
    }
    return FG_OK;
}

int mcse_check(const char *who, bool pointers, int n, int d, int j0, int n_j, const double *h_probs, int n_probs) {
    if (!pointers) { fg_set_error(std::string(who) + ": null d_draws, h_probs or output pointer"); return FG_E_BAD_ARG; }
    if (n < 1) { fg_set_error(std::string(who) + ": n must be at least 1"); return FG_E_BAD_ARG; }
    if (d < 1 || d > 65535) { fg_set_error(std::string(who) + ": d outside [1, 65535]"); return FG_E_BAD_ARG; }
    if (j0 < 0 || n_j < 1 || j0 >= d || n_j > d - j0) { fg_set_error(std::string(who) + ": the block of coordinates lies outside [0, d)"); return FG_E_BAD_ARG; }
    if (n_probs < 1 || n_probs > FG_MCSE_MAX_PROBS) { fg_set_error(std::string(who) + ": n_probs outside [1, 8]"); return FG_E_BAD_ARG; }
    for (int i = 0; i < n_probs; ++i)
        if (!(h_probs[i] >= 0.0 && h_probs[i] <= 1.0)) { fg_set_error(std::string(who) + ": probabilities outside [0, 1]"); return FG_E_BAD_ARG; }
    return FG_OK;
}

int mcse_plan_for(const char *who, fg_engine *e, int n, int d, int j0, int n_j, const double *h_probs, int n_probs, FgMcsePlan *P) {
    if (!e) { fg_set_error(std::string(who) + ": null engine"); return FG_E_BAD_ARG; }
    const int rc = fg_mcse_plan(n, e->C, d, j0, n_j, h_probs, n_probs, P);
    if (rc == FG_E_LIMIT) fg_set_error(std::string(who) + ": n x chains = " + std::to_string((long long)n * e->C) + " pooled draws: the limit is 2^31 - 1");
    else if (rc) fg_set_error(std::string(who) + ": bad argument");
    return rc;
}

}  // namespace

extern "C" {

int fg_diag_mcse_words(int n_probs) {
    if (n_probs < 1 || n_probs > FG_MCSE_MAX_PROBS) { fg_set_error("fg_diag_mcse_words: n_probs outside [1, 8]"); return FG_E_BAD_ARG; }
    return fg_mcse_words(n_probs);
}

int fg_mcse_quantile_ranks(int64_t S, double p, double ess, int64_t *i_lo, int64_t *i_hi) {
    const int rc = fg_mcse_ranks(S, p, ess, i_lo, i_hi);
    if (rc) fg_set_error("fg_mcse_quantile_ranks: a null pointer, S < 1, p outside [0, 1], or ess not finite or not positive");
    return rc;
}

int fg_diag_mcse_transform(fg_engine *e, const double *d_draws, int n, int d, int j0, int n_j, const double *h_mean, const double *h_probs, int n_probs, double *d_out,
                           double *d_sorted_or_null, double *h_median, double *h_mad, int64_t *h_counts) {
    if (int rc = mcse_check("fg_diag_mcse_transform", d_draws && h_mean && h_probs && d_out && h_median && h_mad && h_counts, n, d, j0, n_j, h_probs, n_probs)) return rc;
    FgMcsePlan P;
    if (int rc = mcse_plan_for("fg_diag_mcse_transform", e, n, d, j0, n_j, h_probs, n_probs, &P)) return rc;
    if (hipSetDevice(e->device) != hipSuccess) { fg_set_error("hipSetDevice failed"); return FG_E_HIP; }
    RankWork W;
    McseWork M;
    if (int rc = W.init(P.rank)) return rc;
    if (int rc = M.init(W, P, n_j)) return rc;
    const int pairs = fg_mcse_pairs(n_probs), nc = fg_mcse_counts(n_probs);
    std::vector<double> at((size_t)n_j * pairs), fold((size_t)2 * n_j);
    if (int rc = mcse_transform(e, P, W, M, d_draws, n, d, j0, n_j, h_mean, d_out, at.data(), fold.data(), h_counts)) return rc;
    for (int k = 0; k < n_j; ++k) {
        h_median[k] = fg_rank_median(at[(size_t)k * pairs], at[(size_t)k * pairs + 1]);
        h_mad[k] = fg_mcse_mad(fold[2 * k], fold[2 * k + 1], h_counts[(size_t)k * nc + 4]);
    }
    if (d_sorted_or_null) {
        const u64 cells = (u64)n_j * (u64)P.rank.S;
        const u64 nb = (cells + FG_MCSE_THREADS - 1) / FG_MCSE_THREADS;
        hipLaunchKernelGGL(k_mcse_unkey, dim3((unsigned)(nb > 2048 ? 2048 : nb)), dim3(FG_MCSE_THREADS), 0, e->stream, (const u64 *)M.skeys, cells, d_sorted_or_null);
        HIPCHK(hipGetLastError());
        HIPCHK(hipStreamSynchronize(e->stream));
    }
    return FG_OK;
}

int fg_diag_mcse(fg_engine *e, const double *d_draws, int n, int d, const double *h_probs, int n_probs, int64_t max_out_bytes, double *h_figures, int64_t *h_counts) {
    if (int rc = mcse_check("fg_diag_mcse", d_draws && h_probs && h_figures && h_counts, n, d, 0, d < 1 ? 1 : d, h_probs, n_probs)) return rc;
    if (max_out_bytes < 0) { fg_set_error("fg_diag_mcse: max_out_bytes must not be negative"); return FG_E_BAD_ARG; }
    FgMcsePlan P;
    if (int rc = mcse_plan_for("fg_diag_mcse", e, n, d, 0, d, h_probs, n_probs, &P)) return rc;
    if (hipSetDevice(e->device) != hipSuccess) { fg_set_error("hipSetDevice failed"); return FG_E_HIP; }
    RankWork W;
    McseWork M;
    if (int rc = W.init(P.rank)) return rc;
    const long long per = fg_mcse_block(P, d, max_out_bytes);
    if (int rc = M.init(W, P, per)) return rc;
    double *d_out = nullptr;
    if (int rc = W.alloc(&d_out, (size_t)per * P.b_coord_out, "the rows")) return rc;
    const int R = P.rows, pairs = fg_mcse_pairs(n_probs), nw = fg_mcse_words(n_probs), nc = fg_mcse_counts(n_probs);
    const long long exchanged = e->diag_bytes;                     // fg_diag_rhat_ess's own read-out: this call leaves it as it was
    // 1. the plain figures of the raw draws: one call, so that its words are the ones fg_diag_rhat_ess reports for this buffer
    std::vector<double> raw((size_t)4 * d);
    double *r_mean = raw.data(), *r_std = r_mean + d, *r_rhat = r_std + d, *r_ess = r_rhat + d;
    const int rc_raw = fg_diag_rhat_ess(e, d_draws, n, d, nullptr, r_rhat, r_ess, r_mean, r_std, nullptr);
    e->diag_bytes = exchanged;
    if (rc_raw) return rc_raw;
    std::vector<double> at((size_t)per * pairs), fold((size_t)2 * per), ess((size_t)R * per), mean((size_t)R * per), sd((size_t)R * per), th((size_t)2 * n_probs * per);
    std::vector<u64> th_at((size_t)2 * n_probs * per), th_got((size_t)2 * n_probs * per);
    const u64 S = (u64)P.rank.S;
    for (long long j0 = 0; j0 < d; j0 += per) {
        const int nj = (int)std::min<long long>(per, d - j0);
        int64_t *counts = h_counts + (size_t)j0 * nc;
        // 2. sort and rows
        if (int rc = mcse_transform(e, P, W, M, d_draws, n, d, (int)j0, nj, r_mean + j0, d_out, at.data(), fold.data(), counts)) return rc;
        // 3. the combination on the rows
        const int rc_comb = fg_diag_rhat_ess(e, d_out, n, R * nj, nullptr, nullptr, ess.data(), mean.data(), sd.data(), nullptr);
        e->diag_bytes = exchanged;
        if (rc_comb) return rc_comb;
        // 4. the Beta rule on the host
        const size_t n_th = (size_t)2 * n_probs * nj;
        for (int k = 0; k < nj; ++k)
            for (int i = 0; i < n_probs; ++i) {
                int64_t *c = counts + (size_t)k * nc + FG_MCSE_FIXED_COUNTS + FG_MCSE_PROB_COUNTS * i;
                int64_t lo = -1, hi = -1;
                if (fg_mcse_ranks(P.rank.S, h_probs[i], ess[(size_t)R * k + 2 + i], &lo, &hi)) lo = hi = -1;
                c[1] = lo; c[2] = hi;
                const size_t s = ((size_t)k * n_probs + i) * 2;
                th_at[s] = (u64)k * S + (u64)(lo < 0 ? 0 : lo); th_at[s + 1] = (u64)k * S + (u64)(hi < 0 ? 0 : hi);
            }
        // 5. the gather
        HIPCHK(hipMemcpyAsync(M.at, th_at.data(), n_th * 8, hipMemcpyHostToDevice, e->stream));
        if (int rc = mcse_gather(e, M.skeys, (u64)nj * S, M.at, (u32)n_th, M.got)) return rc;
        HIPCHK(hipMemcpyAsync(th_got.data(), M.got, n_th * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        for (size_t i = 0; i < n_th; ++i) th[i] = fg_rank_unkey(th_got[i]);
        for (int k = 0; k < nj; ++k) {
            const int64_t *c = counts + (size_t)k * nc;
            const double raw4[4] = { r_mean[j0 + k], r_std[j0 + k], r_rhat[j0 + k], r_ess[j0 + k] };
            fg_mcse_figures(P, h_probs, raw4, &ess[(size_t)R * k], &mean[(size_t)R * k], &sd[(size_t)R * k], &at[(size_t)k * pairs], fg_mcse_mad(fold[2 * k], fold[2 * k + 1], c[4]),
                            &th[(size_t)2 * n_probs * k], c, h_figures + (size_t)(j0 + k) * nw);
        }
    }
    return FG_OK;
}

}  // extern "C"
