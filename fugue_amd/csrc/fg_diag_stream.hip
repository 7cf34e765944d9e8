// fg_diag_stream.hip -- the diagnostics of fg_diag.hip without stored draws: split R-hat (src/inference/diagnostics.rs:240-304),
// multi-chain ESS (src/inference/mcmc_utils.rs:231-339) and the pooled mean / std (diagnostics.rs:331-352) of a run that is handed
// over one chunk [n_chunk][d][C] at a time.  A second producer of the per-chain moments [d][6][C] and of the pooled lag sums
// [d][lags]; the combination, the exchange between ranks and the cross term of the pooled std are fg_diag.hip's, unchanged.
//
// State per column (coordinate i, chain c), rows of [d][C] (chain fastest), every entry a plain in-order sum over y_t = x_t - pivot,
// so the state does not depend on where the chunk boundaries fall:
//   row 0        pivot = x_0
//   rows 1-6     S1 = sum y, S2 = sum y^2 of the full chain, of [0, n/2) and of [n/2, 2 (n/2))   (split_f64_chains :240-253)
//   P    [K]     P_t = sum_{i = 0}^{n - 1 - t} y_i y_{i + t}, added in ascending i               (autocovariances, mcmc_utils.rs:231-244)
//   head [K]     y_0 ... y_{K - 1}
//   ring [K]     the last K values of y: slot u mod K holds y_u
// (3 K + 7) doubles per column, whatever the run length.
#include "fg_engine_internal.h"
#include "fg_diag_internal.h"

#define FG_STREAM_LAGS 32
#define FG_STREAM_ROWS 7
#define FG_STREAM_MAX_LAG 2048       // the reference's cap (mcmc_utils.rs:266)

struct fg_diag_stream {
    fg_engine *e = nullptr;
    int n_total = 0, d = 0, K = 0, count = 0;
    double *state = nullptr;         // [FG_STREAM_ROWS + 3 K][d][C]
};

// One thread per column.  K / 32 sweeps over the chunk, each with the last 32 values of the lagged stream y_{u - l0 - k} in registers
// (k_diag_autocov's window); values from before the chunk come from the ring, which is rewritten only after the last sweep.  Then
// one more pass for the six sums, head and ring.  Products are RN(y_i y_{i + t}) added in ascending i (-ffp-contract=off); a window
// slot from before the chain starts holds 0 and adds +-0.
__global__ __launch_bounds__(256) void k_diag_stream_update(const double *chunk, int n_c, int t0, int n_total, int d, long long C, int K, double *state) {
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (c >= C) return;
    const long long st = (long long)d * C;
    const double *x = chunk + (long long)i * C + c;
    double *s = state + (long long)i * C + c;
    double *P = s + FG_STREAM_ROWS * st, *head = P + K * st, *ring = head + K * st;
    const double pivot = t0 == 0 ? x[0] : s[0];
    for (int l0 = 0; l0 < K && l0 < t0 + n_c; l0 += FG_STREAM_LAGS) {          // lags beyond the last index seen pair nothing yet
        double acc[FG_STREAM_LAGS], win[FG_STREAM_LAGS];
#pragma unroll
        for (int k = 0; k < FG_STREAM_LAGS; ++k) {
            acc[k] = P[(l0 + k) * st];
            const int v = t0 - 1 - l0 - k;                                     // win[k] before the first shift
            win[k] = v >= 0 ? ring[(v % K) * st] : 0.0;
        }
        for (int j = 0; j < n_c; ++j) {
            const double cur = x[j * st] - pivot;
            const int v = t0 + j - l0;                                         // index of the value that enters the window
            double in = cur;
            if (l0 > 0) in = v < 0 ? 0.0 : (v < t0 ? ring[(v % K) * st] : x[(v - t0) * st] - pivot);
#pragma unroll
            for (int k = FG_STREAM_LAGS - 1; k > 0; --k) win[k] = win[k - 1];
            win[0] = in;
#pragma unroll
            for (int k = 0; k < FG_STREAM_LAGS; ++k) acc[k] += win[k] * cur;  // win[k] = y_{t0 + j - l0 - k}
        }
#pragma unroll
        for (int k = 0; k < FG_STREAM_LAGS; ++k) P[(l0 + k) * st] = acc[k];
    }
    const int half = n_total / 2;
    double s1f = s[st], s2f = s[2 * st], s1a = s[3 * st], s2a = s[4 * st], s1b = s[5 * st], s2b = s[6 * st];
    for (int j = 0; j < n_c; ++j) {
        const int u = t0 + j;
        const double y = x[j * st] - pivot, yy = y * y;
        s1f += y; s2f += yy;
        if (u < half) { s1a += y; s2a += yy; }
        else if (u < 2 * half) { s1b += y; s2b += yy; }
        if (u < K) head[u * st] = y;
        if (j >= n_c - K) ring[(u % K) * st] = y;
    }
    if (t0 == 0) s[0] = pivot;
    s[st] = s1f; s[2 * st] = s2f; s[3 * st] = s1a; s[4 * st] = s2a; s[5 * st] = s1b; s[6 * st] = s2b;
}

// moments [d][6][C] of k_diag_moments from the sums: mu = S1 / n_seg, mean = pivot + mu, ssd = S2 - S1 mu.  `resid` (may be NULL)
// [d][C]: n (pivot + S1 / n - mean), what the rounding of pivot + mu (two-sum) and of the division leave over -- the row
// k_diag_std_cross wants (the ssd here is about the unrounded mean, so the residual is all of the cross term).
__global__ void k_diag_stream_moments(const double *state, int n, int d, long long C, double *out, double *resid) {
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (c >= C) return;
    const long long st = (long long)d * C;
    const double *s = state + (long long)i * C + c;
    const double pivot = s[0];
    const int half = n / 2;
    double *o = out + (long long)i * 6 * C + c;
    for (int k = 0; k < 3; ++k) {
        const int nseg = k == 0 ? n : half;
        const double s1 = s[(1 + 2 * k) * st], s2 = s[(2 + 2 * k) * st];
        double mean = NAN, ssd = 0.0;
        if (nseg > 0) {
            const double mu = s1 / (double)nseg;
            mean = pivot + mu;
            ssd = s2 - s1 * mu;
            if (k == 0 && resid) {
                const double bb = mean - pivot, err = (pivot - (mean - bb)) + (mu - bb);
                resid[(long long)i * C + c] = (double)n * err + fma(-(double)n, mu, s1);
            }
        }
        o[2 * k * C] = mean; o[(2 * k + 1) * C] = ssd;
    }
}

// Per column the biased autocovariance of the 32 lags [lag0, lag0 + 32) about the full-chain mean mu of y,
//   (P_t - mu (2 S1 - head_sum_t - tail_sum_t) + (n - t) mu^2) / n,   head_sum_t / tail_sum_t = the sums of the first / last t values of y
// (added from the ends inwards); lags >= min(n, K) give 0.  Then k_diag_autocov's block tree; k_diag_acov_finish adds the partials.
__global__ __launch_bounds__(256) void k_diag_stream_acov(const double *state, int n, int d, long long C, int K, int lag0,
                                                           double *partial /*[d][FG_STREAM_LAGS][gridDim.x]*/) {
    __shared__ double sh[4][FG_STREAM_LAGS];
    const long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    double acc[FG_STREAM_LAGS];
#pragma unroll
    for (int k = 0; k < FG_STREAM_LAGS; ++k) acc[k] = 0.0;
    if (c < C) {
        const long long st = (long long)d * C;
        const double *s = state + (long long)i * C + c;
        const double *P = s + FG_STREAM_ROWS * st, *head = P + K * st, *ring = head + K * st;
        const int lim = n < K ? n : K;
        const double s1 = s[st], nf = (double)n, mu = s1 / nf;
        double hs = 0.0, ts = 0.0;
        for (int t = 1; t < lag0 && t < lim; ++t) { hs += head[(t - 1) * st]; ts += ring[((n - t) % K) * st]; }
#pragma unroll
        for (int k = 0; k < FG_STREAM_LAGS; ++k) {
            const int t = lag0 + k;
            if (t < lim) {
                if (t > 0) { hs += head[(t - 1) * st]; ts += ring[((n - t) % K) * st]; }
                const double cross = mu * ((2.0 * s1 - hs) - ts);
                acc[k] = ((P[t * st] - cross) + ((double)(n - t) * mu) * mu) / nf;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < FG_STREAM_LAGS; ++k) {
        double v = acc[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < FG_STREAM_LAGS) {
        const int k = threadIdx.x;
        partial[((long long)i * FG_STREAM_LAGS + k) * gridDim.x + blockIdx.x] = sh[0][k] + sh[1][k] + sh[2][k] + sh[3][k];
    }
}

// this engine's pooled lag sums d_sums [d][n_lags] (n_lags <= 32) on the device; a lag the stream did not keep is an error
static int stream_sums_device(fg_diag_stream *s, int lag0, int n_lags, double *d_sums) {
    fg_engine *e = s->e;
    const int need = std::min(lag0 + n_lags, s->n_total);           // lags >= n_total are 0 by definition
    if (need > s->K) {
        fg_set_error("fg_diag_stream: lag " + std::to_string(std::max(lag0, s->K)) + " is needed, the stream keeps K = " + std::to_string(s->K) +
                     " lags (fg_diag_stream_new's max_lag)");
        return FG_E_LIMIT;
    }
    const unsigned nb = (unsigned)((e->C + 255) / 256);
    double *d_part = nullptr;
    int rc = dev_alloc(&d_part, (size_t)s->d * FG_STREAM_LAGS * nb);
    if (rc) return rc;
    hipLaunchKernelGGL(k_diag_stream_acov, dim3(nb, (unsigned)s->d), dim3(256), 0, e->stream, (const double *)s->state, s->n_total, s->d, e->C, s->K, lag0, d_part);
    rc = fg_diag_finish_lag_sums(e, d_part, (int)nb, n_lags, s->d, d_sums);
    (void)hipFree(d_part);
    return rc;
}
static int stream_sums_cb(AcovCtx *A, int lag0, int n_lags, double *d_sums) { return stream_sums_device(A->src, lag0, n_lags, d_sums); }

static int need_complete(const fg_diag_stream *s, const char *what) {
    if (!s || !s->e) { fg_set_error("null stream"); return FG_E_BAD_ARG; }
    if (hipSetDevice(s->e->device) != hipSuccess) { fg_set_error("hipSetDevice failed"); return FG_E_HIP; }
    if (s->count != s->n_total) {
        fg_set_error(std::string(what) + ": " + std::to_string(s->count) + " of " + std::to_string(s->n_total) + " draws have arrived");
        return FG_E_STATE;
    }
    return FG_OK;
}

extern "C" {

int fg_diag_stream_new(fg_engine *e, int n_total, int d, int max_lag, fg_diag_stream **out) {
    NEED_ENGINE(e);
    if (!out) return FG_E_BAD_ARG;
    *out = nullptr;
    if (n_total < 1) { fg_set_error("fg_diag_stream_new: n_total < 1"); return FG_E_BAD_ARG; }
    if (d < 1 || d > 65535) { fg_set_error("fg_diag_stream_new: d must lie in [1, 65535]"); return FG_E_BAD_ARG; }
    if (max_lag < 1 || max_lag > FG_STREAM_MAX_LAG) { fg_set_error("fg_diag_stream_new: max_lag must lie in [1, 2048]"); return FG_E_BAD_ARG; }
    fg_diag_stream *s = new fg_diag_stream;
    s->e = e; s->n_total = n_total; s->d = d;
    s->K = (max_lag + FG_STREAM_LAGS - 1) / FG_STREAM_LAGS * FG_STREAM_LAGS;
    const int rc = dev_alloc(&s->state, (size_t)(FG_STREAM_ROWS + 3 * s->K) * d * e->C);      // zeroed: every sum starts at +0
    if (rc) { delete s; return rc; }
    *out = s;
    return FG_OK;
}

int fg_diag_stream_update(fg_diag_stream *s, const double *d_draws, int n_chunk) {
    if (!s) { fg_set_error("null stream"); return FG_E_BAD_ARG; }
    NEED_ENGINE(s->e);
    if (!d_draws || n_chunk < 1) return FG_E_BAD_ARG;
    if (n_chunk > s->n_total - s->count) {
        fg_set_error("fg_diag_stream_update: " + std::to_string(s->count) + " + " + std::to_string(n_chunk) + " draws pass n_total = " + std::to_string(s->n_total));
        return FG_E_STATE;
    }
    fg_engine *e = s->e;
    hipLaunchKernelGGL(k_diag_stream_update, dim3((unsigned)((e->C + 255) / 256), (unsigned)s->d), dim3(256), 0, e->stream, d_draws, n_chunk, s->count, s->n_total,
                       s->d, e->C, s->K, s->state);
    HIPCHK(hipGetLastError());
    s->count += n_chunk;
    return FG_OK;
}

int fg_diag_stream_count(const fg_diag_stream *s) { return s ? s->count : 0; }

int fg_diag_stream_moments(fg_diag_stream *s, double *d_moments) {
    const int rc = need_complete(s, "fg_diag_stream_moments");
    if (rc) return rc;
    if (!d_moments) return FG_E_BAD_ARG;
    fg_engine *e = s->e;
    hipLaunchKernelGGL(k_diag_stream_moments, dim3((unsigned)((e->C + 255) / 256), (unsigned)s->d), dim3(256), 0, e->stream, (const double *)s->state, s->n_total, s->d,
                       e->C, d_moments, (double *)nullptr);
    HIPCHK(hipGetLastError());
    return FG_OK;
}

int fg_diag_stream_autocov_sums(fg_diag_stream *s, int lag0, int n_lags, double *h_sums) {
    int rc = need_complete(s, "fg_diag_stream_autocov_sums");
    if (rc) return rc;
    if (!h_sums || lag0 < 0 || n_lags <= 0) return FG_E_BAD_ARG;
    std::vector<double> out((size_t)s->d * n_lags, 0.0);
    double *d_sums = nullptr;
    rc = dev_alloc(&d_sums, (size_t)s->d * FG_STREAM_LAGS);
    if (rc) return rc;
    for (int l0 = 0; l0 < n_lags && lag0 + l0 < s->n_total && !rc; l0 += FG_STREAM_LAGS) {       // chunks of 32 lags
        const int nl = std::min(FG_STREAM_LAGS, n_lags - l0);
        rc = stream_sums_device(s, lag0 + l0, nl, d_sums);
        std::vector<double> tmp((size_t)s->d * nl);
        if (!rc && hipMemcpy(tmp.data(), d_sums, tmp.size() * 8, hipMemcpyDeviceToHost) != hipSuccess) { fg_set_error("fg_diag_stream_autocov_sums: copy failed"); rc = FG_E_HIP; }
        for (int i = 0; i < s->d && !rc; ++i) for (int k = 0; k < nl; ++k) out[(size_t)i * n_lags + l0 + k] = tmp[(size_t)i * nl + k];
    }
    (void)hipFree(d_sums);
    if (rc) return rc;
    std::memcpy(h_sums, out.data(), out.size() * 8);
    return FG_OK;
}

int fg_diag_stream_rhat_ess(fg_diag_stream *s, void *comm, double *h_rhat, double *h_ess, double *h_mean, double *h_std, int64_t *out_total_chains) {
    int rc = need_complete(s, "fg_diag_stream_rhat_ess");
    if (rc) return rc;
    fg_engine *e = s->e;
    const int n = s->n_total, d = s->d;
    double *d_mom = nullptr, *d_res = nullptr;
    rc = dev_alloc(&d_mom, (size_t)d * 6 * e->C);
    if (rc) return rc;
    if (h_std) rc = dev_alloc(&d_res, (size_t)d * e->C);
    if (rc) { (void)hipFree(d_mom); return rc; }
    hipLaunchKernelGGL(k_diag_stream_moments, dim3((unsigned)((e->C + 255) / 256), (unsigned)d), dim3(256), 0, e->stream, (const double *)s->state, n, d, e->C, d_mom, d_res);
    if (hipGetLastError() != hipSuccess) { fg_set_error("fg_diag_stream_rhat_ess: the moments kernel did not launch"); rc = FG_E_HIP; }
    if (!rc) {
        AcovCtx proto{ e, nullptr, n, d, d_mom, comm, nullptr, nullptr, 0 };
        proto.sums = stream_sums_cb; proto.src = s;
        rc = fg_diag_rhat_ess_from_moments(e, n, d, comm, d_mom, d_res, proto, h_rhat, h_ess, h_mean, h_std, out_total_chains);
    }
    (void)hipFree(d_mom);
    if (d_res) (void)hipFree(d_res);
    return rc;
}

void fg_diag_stream_free(fg_diag_stream *s) {
    if (!s) return;
    if (s->state && s->e && hipSetDevice(s->e->device) == hipSuccess) (void)hipFree(s->state);
    delete s;
}

}  // extern "C"
