// fg_abc.hip -- the device pieces of approximate Bayesian computation (reference: src/inference/abc.rs).
//
//   k_abc_distance   the reference's three DistanceFunction<Vec<f64>> (abc.rs:132-145 Euclidean, :168-180 Manhattan, :183-226
//                    SummaryStats) of a table of simulated data [K][B] against one observed vector: one lane per attempt, rows read
//                    coalesced (attempt-fastest).  IEEE operations only, in the reference's order (-ffp-contract=off): bit-identical
//                    to a sequential restatement (tests/abc_restatement.py).  The median of SummaryStats is an exact selection without
//                    a per-lane array: the lane bisects on the order-preserving integer image of the doubles, one counting pass over
//                    its column per bit (64 K loads), and for an even K finds the upper middle element in two more passes.
//                    Divergence from the reference, on purpose: a NaN among the simulated values gives a NaN distance (never
//                    accepted); the reference panics in `partial_cmp().unwrap()` (abc.rs:202).  -0.0 sorts below +0.0 here, any order
//                    in the reference's stable sort: the sign of a zero median does not reach the distance ((o - s)^2).
//   k_abc_mixture    log sum_j w_j K(x_i | theta_j), the denominator of the importance weight of weighted ABC-SMC (abc.rs:612-616,
//                    :776-799), for m accepted particles against n centers: the one part of the method that is quadratic in the
//                    population.  One lane per accepted particle with its pre-scaled coordinates in registers; the centers are
//                    wave-uniform and come through scalar loads from a table [n][d + 1] = {ln w_j - sum ln s_c - d ln(2 pi)/2,
//                    theta_jc / s_c}: a pair costs d subtractions, d multiply-adds and one exp.  NOT the reference's rounding (it
//                    divides per pair and sums log-densities term by term): agreement is to ~1e-12, tests hold 1e-9.  The range of
//                    centers is split over waves (fg_abc_plan.h); every (tile, split) leaves a partial (max, sum) of a running
//                    log-sum-exp and k_abc_mix_finish combines a particle's partials in split order.
//                    Expected bound, stated before any measurement: with wave-uniform centers nothing per pair comes from memory
//                    per lane, so the kernel should sit at the f64 ALU and the exp, not at bandwidth.
#include "fg_engine_internal.h"
#include "fg_abc_plan.h"

// ---- distance ------------------------------------------------------------------------------------------------------------------
// order-preserving image of a double that is no NaN: -inf < ... < -0.0 < +0.0 < ... < +inf as unsigned integers
__host__ __device__ static inline unsigned long long fg_abc_key(double x) {
    unsigned long long b;
    memcpy(&b, &x, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__host__ __device__ static inline double fg_abc_unkey(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double x;
    memcpy(&x, &b, 8);
    return x;
}

// compute_stats (abc.rs:192-210) of the K values col[0], col[stride], ...: mean, population std, median.  *has_nan: a NaN was met
// (the statistics are then not used).  The host calls it with stride 1 on the observed vector: the same arithmetic.
__host__ __device__ static inline void fg_abc_stats(const double *col, long long K, long long stride, double *st, bool *has_nan) {
    *has_nan = false;
    if (K <= 0) { st[0] = 0.0; st[1] = 0.0; st[2] = 0.0; return; }
    double sum = 0.0;
    bool nan = false;
    for (long long k = 0; k < K; ++k) { const double x = col[k * stride]; nan = nan || (x != x); sum = sum + x; }
    if (nan) { *has_nan = true; st[0] = st[1] = st[2] = NAN; return; }
    const double mean = sum / (double)K;
    double ss = 0.0;
    for (long long k = 0; k < K; ++k) { const double dv = col[k * stride] - mean; ss = ss + dv * dv; }
    const double var = ss / (double)K;
    // the element of rank r (0-based) of the sorted column: the largest v with #{key < v} <= r
    const long long r = (K & 1) ? K / 2 : K / 2 - 1;
    unsigned long long v = 0ull;
    for (int bit = 63; bit >= 0; --bit) {
        const unsigned long long cand = v | (1ull << bit);
        long long below = 0;
        for (long long k = 0; k < K; ++k) below += fg_abc_key(col[k * stride]) < cand ? 1 : 0;
        if (below <= r) v = cand;
    }
    double med = fg_abc_unkey(v);
    if (!(K & 1)) {                                        // the element of rank r + 1: v again while it has enough copies, else the least key above it
        long long le = 0;
        unsigned long long up = ~0ull;
        for (long long k = 0; k < K; ++k) {
            const unsigned long long q = fg_abc_key(col[k * stride]);
            le += q <= v ? 1 : 0;
            if (q > v && q < up) up = q;
        }
        const double hi = le >= r + 2 ? med : fg_abc_unkey(up);
        med = (med + hi) / 2.0;
    }
    st[0] = mean; st[1] = sqrt(var); st[2] = med;
}

struct FgAbcDistArgs {
    int kind, mismatch, n_w;              // FG_ABC_*; K != n_observed (Euclidean / Manhattan: +inf); weights used = min(3, n_weights)
    double ostat[3], w[3];                // SummaryStats: the observed vector's statistics (host, same arithmetic) and the weights
};

__global__ __launch_bounds__(256) void k_abc_distance(FgAbcDistArgs A, const double *sim, long long K, long long B, const double *obs, double *dist) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    double out;
    if (A.kind == FG_ABC_SUMMARY_STATS) {
        double st[3];
        bool nan;
        fg_abc_stats(sim + b, K, B, st, &nan);
        double s = 0.0;
        for (int i = 0; i < A.n_w; ++i) { const double dv = A.ostat[i] - st[i]; s = s + A.w[i] * (dv * dv); }
        out = nan ? NAN : sqrt(s);
    } else if (A.mismatch) out = INFINITY;
    else if (A.kind == FG_ABC_EUCLIDEAN) {
        double s = 0.0;
        for (long long k = 0; k < K; ++k) { const double dv = obs[k] - sim[k * B + b]; s = s + dv * dv; }
        out = sqrt(s);
    } else {
        double s = 0.0;
        for (long long k = 0; k < K; ++k) s = s + fabs(obs[k] - sim[k * B + b]);
        out = s;
    }
    dist[b] = out;
}

// the launch alone: obs is a device copy of the observed vector (Euclidean / Manhattan), ostat the host statistics (SummaryStats)
static int abc_distance_launch(fg_engine *e, const double *d_sim, long long K, long long B, const double *d_obs, long long n_obs, int kind, const double *ostat,
                               const double *h_w, int n_w, double *d_dist) {
    FgAbcDistArgs A = {};
    A.kind = kind;
    A.mismatch = (K != n_obs) ? 1 : 0;
    A.n_w = n_w < 3 ? n_w : 3;
    for (int i = 0; i < 3; ++i) { A.ostat[i] = ostat ? ostat[i] : 0.0; A.w[i] = (h_w && i < A.n_w) ? h_w[i] : 0.0; }
    const long long groups = (B + 255) / 256;
    if (groups > 0x7fffffffLL) { fg_set_error("fg_abc_distance: more attempts than a grid holds"); return FG_E_LIMIT; }
    hipLaunchKernelGGL(k_abc_distance, dim3((unsigned)groups), dim3(256), 0, e->stream, A, d_sim, K, B, d_obs, d_dist);
    HIPCHK(hipGetLastError());
    return FG_OK;
}

extern "C" int fg_abc_distance(fg_engine *e, const double *d_sim, int K, int64_t B, const double *h_observed, int n_observed, int kind, const double *h_weights,
                               int n_weights, double *d_dist) {
    NEED_ENGINE(e);
    if (K < 0 || B < 0 || n_observed < 0 || n_weights < 0) { fg_set_error("fg_abc_distance: a negative size"); return FG_E_BAD_ARG; }
    if (kind != FG_ABC_EUCLIDEAN && kind != FG_ABC_MANHATTAN && kind != FG_ABC_SUMMARY_STATS) { fg_set_error("fg_abc_distance: unknown distance kind " + std::to_string(kind)); return FG_E_BAD_ARG; }
    if (!d_dist || (!d_sim && K > 0 && B > 0) || (!h_observed && n_observed > 0) || (!h_weights && n_weights > 0)) { fg_set_error("fg_abc_distance: a null argument"); return FG_E_BAD_ARG; }
    double ostat[3] = {0.0, 0.0, 0.0};
    if (kind == FG_ABC_SUMMARY_STATS) {
        bool nan;
        fg_abc_stats(h_observed, n_observed, 1, ostat, &nan);
        if (nan) { fg_set_error("fg_abc_distance: a NaN in the observed vector (the reference panics in compute_stats, abc.rs:202)"); return FG_E_BAD_ARG; }
    }
    if (B == 0) return FG_OK;
    double *d_obs = nullptr;
    if (kind != FG_ABC_SUMMARY_STATS && n_observed > 0 && K == n_observed) {
        HIPCHK(hipMalloc((void **)&d_obs, (size_t)n_observed * sizeof(double)));
        const hipError_t he = hipMemcpyAsync(d_obs, h_observed, (size_t)n_observed * sizeof(double), hipMemcpyHostToDevice, e->stream);
        if (he != hipSuccess) { (void)hipFree(d_obs); fg_set_error(std::string("fg_abc_distance: ") + hipGetErrorString(he)); return FG_E_HIP; }
    }
    int rc = abc_distance_launch(e, d_sim, K, B, d_obs, n_observed, kind, ostat, h_weights, n_weights, d_dist);
    if (d_obs) {                                           // the copy is this call's own: the kernel is done with it before it goes
        const hipError_t he = hipStreamSynchronize(e->stream);
        (void)hipFree(d_obs);
        if (!rc && he != hipSuccess) { fg_set_error(std::string("fg_abc_distance: ") + hipGetErrorString(he)); rc = FG_E_HIP; }
    }
    return rc;
}

// ---- the kernel mixture --------------------------------------------------------------------------------------------------------
// table[j] = { konst[j], centers[c][j] * inv_s[c] ... }
__global__ __launch_bounds__(256) void k_abc_mix_table(const double *centers, const double *konst, const double *inv_s, long long n, long long d, double *table) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    table[fg_abc_table_index(j, d, 0)] = konst[j];
    for (long long c = 0; c < d; ++c) table[fg_abc_table_index(j, d, 1 + c)] = centers[fg_abc_coord_index(c, n, j)] * inv_s[c];
}

// one step of a running log-sum-exp (max M, sum S of exp(term - M)) with one exp: a term of -inf adds nothing, a NaN term stays
__device__ __forceinline__ void fg_abc_lse_step(double t, double &M, double &S) {
    if (t == FG_NEG_INF) return;
    const double dl = t - M;                               // M = -inf before the first finite term: dl = +inf, e = 0, S = 1
    const double ex = exp(-fabs(dl));
    const bool up = dl > 0.0;
    S = up ? S * ex + 1.0 : S + ex;
    M = up ? t : M;
}

// DR >= 1: the lane's DR pre-scaled coordinates in registers; DR == 0: any d (0 included), coordinates re-read from memory per pair
template <int DR>
__global__ __launch_bounds__(FG_WAVE * FG_ABC_MIX_W) void k_abc_mixture(const double *x, long long m, const double *table, const double *inv_s, long long n, long long d,
                                                                       long long tiles, long long centers_per_split, long long items, double *pmax, double *psum) {
    const int lane = (int)(threadIdx.x & (FG_WAVE - 1));
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / FG_WAVE));   // wave-uniform by construction: said so, and the centers' addresses are scalar
    const long long g = (long long)blockIdx.x * FG_ABC_MIX_W + wave;
    if (g >= items) return;                                // (no barrier anywhere: the waves of a workgroup share nothing)
    long long tile, split, j0, j1;
    fg_abc_mix_item(g, tiles, centers_per_split, n, &tile, &split, &j0, &j1);
    const long long i_own = tile * FG_WAVE + lane;
    const bool live = i_own < m;
    const long long i = live ? i_own : m - 1;              // a lane beyond m repeats the last particle's work and stores nothing
    const FG_AS4 double *tab = (const FG_AS4 double *)(uintptr_t)table;   // wave-uniform addresses: scalar loads
    const FG_AS4 double *is4 = (const FG_AS4 double *)(uintptr_t)inv_s;
    double M = FG_NEG_INF, S = 0.0;
    if constexpr (DR > 0) {
        double xr[DR > 0 ? DR : 1];
#pragma unroll
        for (int c = 0; c < DR; ++c) xr[c] = x[fg_abc_coord_index(c, m, i)] * is4[c];
        for (long long j = j0; j < j1; ++j) {
            const FG_AS4 double *row = tab + j * (DR + 1);
            double q = 0.0;
#pragma unroll
            for (int c = 0; c < DR; ++c) { const double z = xr[c] - row[1 + c]; q = fma(z, z, q); }
            fg_abc_lse_step(row[0] - 0.5 * q, M, S);
        }
    } else {
        for (long long j = j0; j < j1; ++j) {
            const FG_AS4 double *row = tab + fg_abc_table_index(j, d, 0);
            double q = 0.0;
            for (long long c = 0; c < d; ++c) { const double z = x[fg_abc_coord_index(c, m, i)] * is4[c] - row[1 + c]; q = fma(z, z, q); }
            fg_abc_lse_step(row[0] - 0.5 * q, M, S);
        }
    }
    if (live) {
        const long long o = fg_abc_partial_index(split, m, i);
        pmax[o] = (S != S) ? NAN : M; psum[o] = S;   // a NaN coordinate: the particle's log-density is NaN, whatever the other splits hold
    }
}

// log_denom_i = LSE over the splits' partials, in split order; every partial empty: -inf
__global__ __launch_bounds__(256) void k_abc_mix_finish(const double *pmax, const double *psum, long long m, long long splits, double *out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    double M = FG_NEG_INF;
    bool nan = false;
    for (long long s = 0; s < splits; ++s) { const double pm = pmax[fg_abc_partial_index(s, m, i)]; nan = nan || (pm != pm); M = pm > M ? pm : M; }
    double S = 0.0;
    for (long long s = 0; s < splits; ++s) {
        const long long o = fg_abc_partial_index(s, m, i);
        const double pm = pmax[o];
        if (pm == FG_NEG_INF) continue;
        S = S + psum[o] * exp(pm - M);
    }
    out[i] = nan ? NAN : (M == FG_NEG_INF ? FG_NEG_INF : M + log(S));
}

typedef void (*FgAbcMixFn)(const double *, long long, const double *, const double *, long long, long long, long long, long long, long long, double *, double *);
static FgAbcMixFn g_abc_mix_variants[FG_ABC_DREG + 1] = { k_abc_mixture<0>, k_abc_mixture<1>, k_abc_mixture<2>, k_abc_mixture<3>, k_abc_mixture<4>,
                                                          k_abc_mixture<5>, k_abc_mixture<6>, k_abc_mixture<7>, k_abc_mixture<8> };

// The launches alone, on device buffers the caller owns: d_konst [n], d_inv_s [max(d, 1)], d_table [plan.table_elems], d_pmax / d_psum
// [plan.partial_elems].
static int abc_mixture_launch(fg_engine *e, const FgAbcMixPlan &pl, const double *d_x, long long m, const double *d_centers, long long n, long long d, const double *d_konst,
                              const double *d_inv_s, double *d_table, double *d_pmax, double *d_psum, double *d_out) {
    hipLaunchKernelGGL(k_abc_mix_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, d_centers, d_konst, d_inv_s, n, d, d_table);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(g_abc_mix_variants[pl.d_reg], dim3(pl.grid), dim3(FG_WAVE * FG_ABC_MIX_W), 0, e->stream, d_x, m, (const double *)d_table, d_inv_s, n, d, pl.tiles,
                       pl.centers_per_split, pl.items, d_pmax, d_psum);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_abc_mix_finish, dim3(pl.finish_grid), dim3(256), 0, e->stream, (const double *)d_pmax, (const double *)d_psum, m, pl.splits, d_out);
    HIPCHK(hipGetLastError());
    return FG_OK;
}

// the hoisted per-center constants and the reciprocal bandwidths, on the host (O(n + d) once per stage)
static void abc_mixture_consts(const double *h_weights, long long n, const double *h_std, long long d, std::vector<double> &konst, std::vector<double> &inv_s) {
    double sum_ln_s = 0.0;
    inv_s.assign((size_t)std::max<long long>(d, 1), 1.0);
    for (long long c = 0; c < d; ++c) {
        const double s = std::fmax(h_std[c], 1e-12);       // abc.rs:794
        inv_s[(size_t)c] = 1.0 / s;
        sum_ln_s += std::log(s);
    }
    const double base = -sum_ln_s - (double)d * (0.5 * FG_LN_2PI);
    konst.resize((size_t)n);
    for (long long j = 0; j < n; ++j) konst[(size_t)j] = std::log(h_weights[j]) + base;   // w_j = 0: -inf, the center contributes nothing
}

extern "C" int fg_abc_mixture(fg_engine *e, const double *d_x, int64_t m, const double *d_centers, int64_t n, int d, const double *h_weights, const double *h_std,
                              double *d_out) {
    NEED_ENGINE(e);
    if (m < 0 || n < 1 || d < 0) { fg_set_error("fg_abc_mixture: m < 0, n < 1 or d < 0"); return FG_E_BAD_ARG; }
    if (!h_weights || (d > 0 && (!h_std || !d_centers || (m > 0 && !d_x))) || (m > 0 && !d_out)) { fg_set_error("fg_abc_mixture: a null argument"); return FG_E_BAD_ARG; }
    const char *fs = std::getenv("FG_ABC_MIX_SPLITS");
    const long long force = fs ? std::atoll(fs) : 0;
    FgAbcMixPlan pl;
    int rc = fg_abc_mix_plan(m, n, d, std::max(1, e->n_simd / 4), force < 0 ? 0 : force, &pl);
    if (rc) { fg_set_error("fg_abc_mixture: no launch plan for this shape"); return rc; }
    if (m == 0) return FG_OK;
    std::vector<double> konst, inv_s;
    abc_mixture_consts(h_weights, n, h_std, d, konst, inv_s);
    // one allocation for this call's scratch: konst [n] | inv_s [max(d,1)] | table | pmax | psum
    const size_t n_k = (size_t)n, n_s = inv_s.size(), total = n_k + n_s + pl.table_elems + 2 * pl.partial_elems;
    double *buf = nullptr;
    HIPCHK(hipMalloc((void **)&buf, total * sizeof(double)));
    double *d_konst = buf, *d_inv_s = d_konst + n_k, *d_table = d_inv_s + n_s, *d_pmax = d_table + pl.table_elems, *d_psum = d_pmax + pl.partial_elems;
    hipError_t he = hipMemcpyAsync(d_konst, konst.data(), n_k * sizeof(double), hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(d_inv_s, inv_s.data(), n_s * sizeof(double), hipMemcpyHostToDevice, e->stream);
    if (he != hipSuccess) { (void)hipFree(buf); fg_set_error(std::string("fg_abc_mixture: ") + hipGetErrorString(he)); return FG_E_HIP; }
    rc = abc_mixture_launch(e, pl, d_x, m, d_centers, n, d, d_konst, d_inv_s, d_table, d_pmax, d_psum, d_out);
    he = hipStreamSynchronize(e->stream);                  // the scratch (and the host vectors the copies read) are this call's own
    (void)hipFree(buf);
    if (!rc && he != hipSuccess) { fg_set_error(std::string("fg_abc_mixture: ") + hipGetErrorString(he)); rc = FG_E_HIP; }
    return rc;
}

// ---- rounds of attempts --------------------------------------------------------------------------------------------------------
// Ordered compaction of a round (fg_abc_plan.h): ballot, popcount prefix, scan of the wave counts -- never an atomic slot counter, so
// the accepted set is the first n accepted attempts in attempt order whatever the batch size.
__global__ __launch_bounds__(256) void k_abc_accept(const double *dist, const double *log_prior, long long B, long long live, double tol, int need_prior, int *flag,
                                                    int *counts) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    bool ok = false;
    if (b < live) {                                        // attempts beyond the budget are masked (live <= B)
        const double dv = dist[b];
        ok = dv <= tol;                                    // a NaN distance is never accepted
        if (need_prior) { const double lp = log_prior[b]; ok = ok && fg_finite(lp); }
    }
    const unsigned long long ballot = __ballot(ok);
    if (b < B) flag[b] = ok ? 1 : 0;
    if ((threadIdx.x & (FG_WAVE - 1)) == 0 && b < B) counts[b / FG_WAVE] = __popcll(ballot);
}

// one workgroup: offs[w] = counts[0] + ... + counts[w - 1], *total = the sum, walked in chunks of FG_ABC_SCAN_THREADS in wave order
__global__ __launch_bounds__(FG_ABC_SCAN_THREADS) void k_abc_scan(const int *counts, long long waves, long long *offs, long long *total) {
    __shared__ long long s[FG_ABC_SCAN_THREADS];
    __shared__ long long carry;
    const int tid = (int)threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (long long base = 0; base < waves; base += FG_ABC_SCAN_THREADS) {
        const long long idx = base + tid;
        const long long v = idx < waves ? (long long)counts[idx] : 0;
        s[tid] = v;
        __syncthreads();
        for (int off = 1; off < FG_ABC_SCAN_THREADS; off <<= 1) {
            const long long t = tid >= off ? s[tid - off] : 0;
            __syncthreads();
            s[tid] += t;
            __syncthreads();
        }
        const long long incl = s[tid];
        if (idx < waves) offs[idx] = carry + incl - v;
        __syncthreads();
        if (tid == FG_ABC_SCAN_THREADS - 1) carry += incl;
        __syncthreads();
    }
    if (tid == 0) *total = carry;
}

struct FgAbcPop { long long *cells; double *w, *dist, *lp, *ld; long long *att; long long n; };   // cells [S][cap], the others [cap]

__global__ __launch_bounds__(256) void k_abc_append(const int *flag, const long long *offs, long long B, long long a0, long long filled, long long cap, const long long *values,
                                                    int S, const double *dist, const double *log_prior, FgAbcPop pop) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = b < B && flag[b] != 0;
    const unsigned long long ballot = __ballot(ok);
    if (!ok) return;
    const int lane = (int)(threadIdx.x & (FG_WAVE - 1));
    const long long slot = filled + offs[b / FG_WAVE] + __popcll(ballot & ((1ull << lane) - 1ull));
    if (slot >= cap) return;                               // the n-th accept ended the stage: later accepts are not part of it
    for (int j = 0; j < S; ++j) pop.cells[(long long)j * cap + slot] = values[(long long)j * B + b];
    pop.dist[slot] = dist[b]; pop.att[slot] = a0 + b; pop.lp[slot] = log_prior[b]; pop.ld[slot] = 0.0; pop.w[slot] = 0.0;
}

// abc.rs:586-598 for attempt a0 + b: sample_index over the in-order cumulative weights (binary search: the first i with u total <=
// cum[i] is what the reference's walk returns, the last index when none qualifies), the base particle's cells into the engine's values,
// every f64 site moved by bw[c] z with z ~ Normal(0, 1) drawn as FG_MODE_PRIOR draws a Normal site (p0 + p1 z, p0 = 0, p1 = 1)
__global__ __launch_bounds__(256) void k_abc_propose(unsigned long long seed, uint32_t chain_base, uint32_t stage, long long B, const double *cum, long long n, double total,
                                                     const long long *pcells, long long cap, long long *values, int S, const int *f64_site, int d, const double *bw,
                                                     long long *base_out) {
    const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    FgStream rng = fg_stream(seed, chain_base + (uint32_t)b, stage, FG_RNG_ABC);
    const double ut = fg_rng_u01(rng) * total;
    long long lo = 0, hi = n;
    while (lo < hi) { const long long mid = lo + (hi - lo) / 2; if (ut <= cum[mid]) hi = mid; else lo = mid + 1; }
    const long long idx = lo < n ? lo : n - 1;
    for (int j = 0; j < S; ++j) values[(long long)j * B + b] = pcells[(long long)j * cap + idx];
    for (int c = 0; c < d; ++c) {
        const long long g = (long long)f64_site[c] * B + b;
        const double z = 0.0 + 1.0 * fg_rng_normal(rng);
        values[g] = fg_as_i64(fg_as_double(values[g]) + bw[c] * z);
    }
    base_out[b] = idx;
}

// coordinates [d][m] (contiguous) of the first m particles of a population's cells [S][cap]
__global__ __launch_bounds__(256) void k_abc_coords(const long long *cells, long long cap, long long m, const int *f64_site, int d, double *out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    for (int c = 0; c < d; ++c) out[fg_abc_coord_index(c, m, i)] = fg_as_double(cells[(long long)f64_site[c] * cap + i]);
}

struct fg_abc {
    fg_engine *e = nullptr;
    long long B = 0, cap = 0;
    int S = 0, d = 0, sim_kind = 0, K = 0, n_src = 0, kind = 0;   // n_src: rows of the simulator's raw table (selected observes, or all R results)
    std::vector<int32_t> sel, rows, vtypes;               // the simulator selection; the row gather / conversion of fg_diag_cells_f64
    std::vector<double> obs, wts;
    double ostat[3] = {0.0, 0.0, 0.0};
    std::vector<void *> allocs;
    double *d_obs = nullptr, *d_sim = nullptr, *d_dist = nullptr, *d_cum = nullptr, *d_bw = nullptr, *d_xc = nullptr, *d_cc = nullptr, *d_out = nullptr;
    long long *d_raw = nullptr, *d_offs = nullptr, *d_total = nullptr, *d_base = nullptr, *d_save = nullptr;
    int *d_flag = nullptr, *d_counts = nullptr;
    FgAbcPop pop[2];
    int cur = 0;
    bool stage_open = false, have_round = false, round_prior = false;
    long long stage_n = 0;                                 // particles of the population the stage was opened on
    double total = 0.0;
    std::vector<double> bw, prev_w;
};

template <typename T>
static int abc_alloc(fg_abc *a, T **p, size_t n) {
    int rc = dev_alloc(p, n);
    if (!rc) a->allocs.push_back((void *)*p);
    return rc;
}

extern "C" void fg_abc_free(fg_abc *a) {
    if (!a) return;
    if (a->e && hipSetDevice(a->e->device) == hipSuccess) {
        (void)hipStreamSynchronize(a->e->stream);
        for (void *q : a->allocs) (void)hipFree(q);
    }
    delete a;
}

extern "C" int fg_abc_new(fg_engine *e, int sim_kind, const int32_t *h_sel, int n_sel, const double *h_observed, int n_observed, int kind, const double *h_weights,
                          int n_weights, int64_t capacity, fg_abc **out) {
    NEED_ENGINE(e);
    if (!out) { fg_set_error("fg_abc_new: null out"); return FG_E_BAD_ARG; }
    *out = nullptr;
    if (sim_kind != FG_ABC_SIM_OBSERVE && sim_kind != FG_ABC_SIM_RESULT) { fg_set_error("fg_abc_new: the simulator is FG_ABC_SIM_OBSERVE or FG_ABC_SIM_RESULT"); return FG_E_BAD_ARG; }
    if (kind != FG_ABC_EUCLIDEAN && kind != FG_ABC_MANHATTAN && kind != FG_ABC_SUMMARY_STATS) { fg_set_error("fg_abc_new: unknown distance kind " + std::to_string(kind)); return FG_E_BAD_ARG; }
    if (capacity < 1 || n_observed < 0 || n_weights < 0 || (!h_observed && n_observed > 0) || (!h_weights && n_weights > 0)) { fg_set_error("fg_abc_new: capacity < 1, a negative size or a null vector"); return FG_E_BAD_ARG; }
    const fg_program *p = e->prog;
    const int n_all = sim_kind == FG_ABC_SIM_OBSERVE ? p->n_observes : fg_program_n_results(p);
    if (n_all < 1) { fg_set_error(sim_kind == FG_ABC_SIM_OBSERVE ? "fg_abc_new: the program has no observe statement" : "fg_abc_new: the program has no result"); return FG_E_STATE; }
    fg_abc *a = new fg_abc();
    a->e = e; a->B = e->C; a->cap = capacity; a->S = e->S; a->d = e->d; a->sim_kind = sim_kind; a->kind = kind;
    if (!h_sel) { for (int k = 0; k < n_all; ++k) a->sel.push_back(k); }
    else {
        if (n_sel < 1) { delete a; fg_set_error("fg_abc_new: an empty selection"); return FG_E_BAD_ARG; }
        for (int r = 0; r < n_sel; ++r) {
            const int k = h_sel[r];
            if (k < 0 || k >= n_all || (sim_kind == FG_ABC_SIM_OBSERVE && r > 0 && k <= h_sel[r - 1])) {
                delete a; fg_set_error("fg_abc_new: selection " + std::to_string(r) + " is outside the program's list, or the observe statements are not in program order"); return FG_E_BAD_ARG;
            }
            a->sel.push_back(k);
        }
    }
    a->K = (int)a->sel.size();
    if (sim_kind == FG_ABC_SIM_OBSERVE) {                  // fg_predict_eval stores the K selected rows; each converted by its own tag
        a->n_src = a->K;
        for (int r = 0; r < a->K; ++r) { a->rows.push_back(r); a->vtypes.push_back(fg_program_observe_vtype(p, a->sel[r])); }
    } else {                                               // fg_result_eval stores all R rows of doubles; the selection gathers
        a->n_src = n_all;
        for (int r = 0; r < a->K; ++r) { a->rows.push_back(a->sel[r]); a->vtypes.push_back(FG_F64); }
    }
    a->obs.assign(h_observed, h_observed + n_observed);
    a->wts.assign(h_weights, h_weights + n_weights);
    if (kind == FG_ABC_SUMMARY_STATS) {
        bool nan;
        fg_abc_stats(a->obs.data(), n_observed, 1, a->ostat, &nan);
        if (nan) { delete a; fg_set_error("fg_abc_new: a NaN in the observed vector (the reference panics in compute_stats, abc.rs:202)"); return FG_E_BAD_ARG; }
    }
    FgAbcCompactPlan cp;
    int rc = fg_abc_compact_plan(a->B, &cp);
    const size_t B = (size_t)a->B, cap = (size_t)a->cap, S1 = (size_t)std::max(1, a->S), d1 = (size_t)std::max(1, a->d);
    if (!rc) rc = abc_alloc(a, &a->d_obs, a->obs.size());
    if (!rc && !a->obs.empty()) { const hipError_t he = hipMemcpy(a->d_obs, a->obs.data(), a->obs.size() * sizeof(double), hipMemcpyHostToDevice); if (he != hipSuccess) { fg_set_error(std::string("fg_abc_new: ") + hipGetErrorString(he)); rc = FG_E_HIP; } }
    if (!rc) rc = abc_alloc(a, &a->d_raw, (size_t)a->n_src * B);
    if (!rc) rc = abc_alloc(a, &a->d_sim, (size_t)a->K * B);
    if (!rc) rc = abc_alloc(a, &a->d_dist, B);
    if (!rc) rc = abc_alloc(a, &a->d_flag, B);
    if (!rc) rc = abc_alloc(a, &a->d_base, B);
    if (!rc) rc = abc_alloc(a, &a->d_counts, (size_t)cp.waves);
    if (!rc) rc = abc_alloc(a, &a->d_offs, (size_t)cp.waves);
    if (!rc) rc = abc_alloc(a, &a->d_total, 1);
    if (!rc) rc = abc_alloc(a, &a->d_save, S1 * B);
    if (!rc) rc = abc_alloc(a, &a->d_cum, cap);
    if (!rc) rc = abc_alloc(a, &a->d_bw, d1);
    if (!rc) rc = abc_alloc(a, &a->d_xc, d1 * cap);
    if (!rc) rc = abc_alloc(a, &a->d_cc, d1 * cap);
    if (!rc) rc = abc_alloc(a, &a->d_out, cap);
    for (int q = 0; q < 2 && !rc; ++q) {
        FgAbcPop &P = a->pop[q];
        P.n = 0;
        rc = abc_alloc(a, &P.cells, S1 * cap);
        if (!rc) rc = abc_alloc(a, &P.w, cap);
        if (!rc) rc = abc_alloc(a, &P.dist, cap);
        if (!rc) rc = abc_alloc(a, &P.lp, cap);
        if (!rc) rc = abc_alloc(a, &P.ld, cap);
        if (!rc) rc = abc_alloc(a, &P.att, cap);
    }
    if (rc) { fg_abc_free(a); return rc; }
    *out = a;
    return FG_OK;
}

#define NEED_ABC(a) do { if (!(a) || !(a)->e) { fg_set_error("null ABC handle"); return FG_E_BAD_ARG; } NEED_ENGINE((a)->e); } while (0)

// the simulator's table [K][B] at the engine's current values, then the distances [B]
static int abc_simulate_and_measure(fg_abc *a, uint32_t stage) {
    fg_engine *e = a->e;
    int rc;
    if (a->sim_kind == FG_ABC_SIM_OBSERVE) rc = fg_predict_eval(e, nullptr, 1, nullptr, 0, stage, a->sel.data(), a->K, a->d_raw, nullptr);
    else rc = fg_result_eval(e, nullptr, 1, nullptr, 0, (double *)a->d_raw);
    if (rc) return rc;
    rc = fg_diag_cells_f64(e, a->d_raw, 1, a->n_src, a->rows.data(), a->vtypes.data(), a->K, a->d_sim);
    if (rc) return rc;
    return abc_distance_launch(e, a->d_sim, a->K, a->B, a->d_obs, (long long)a->obs.size(), a->kind, a->ostat, a->wts.data(), (int)a->wts.size(), a->d_dist);
}

// The rounds of one stage: stage 0 draws from the prior, stage t >= 1 proposes from the population the stage was opened on.  The
// engine's chain base is moved to chain_offset + a0 for a round's launches and put back (on every path) before the call returns.
static int abc_rounds(fg_abc *a, uint32_t stage, bool prior, double tol, long long budget, FgAbcPop &dst, int64_t *accepted, int64_t *attempts) {
    fg_engine *e = a->e;
    if (budget < 0 || budget > (1LL << 32) - (long long)e->chain0) { fg_set_error("ABC: the attempt budget must lie in [0, 2^32 - chain_offset]"); return FG_E_BAD_ARG; }
    if (tol != tol) { fg_set_error("ABC: the tolerance is NaN"); return FG_E_BAD_ARG; }
    const uint32_t chain0 = e->chain0;
    const bool live_session = e->hmc_ready || e->mh_ready || e->smc_pop_ready;
    const size_t vbytes = (size_t)e->S * (size_t)e->C * 8;
    if (live_session && vbytes) HIPCHK(hipMemcpyAsync(a->d_save, e->d_values, vbytes, hipMemcpyDeviceToDevice, e->stream));
    FgAbcCompactPlan cp;
    int rc = fg_abc_compact_plan(a->B, &cp);
    dst.n = 0;
    a->have_round = false;
    const long long max_rounds = fg_abc_max_rounds(budget, a->B);
    const unsigned g256 = (unsigned)((a->B + 255) / 256);
    for (long long r = 0; r < max_rounds && !rc && dst.n < a->cap; ++r) {
        const long long a0 = r * a->B, live = std::min<long long>(a->B, budget - a0);
        e->chain0 = chain0 + (uint32_t)a0; e->X.chain0 = e->chain0;
        if (prior) rc = fg_launch_prior(e, stage, FG_RNG_PRIOR, e->d_acc, nullptr);
        else {
            hipLaunchKernelGGL(k_abc_propose, dim3(g256), dim3(256), 0, e->stream, e->seed, e->chain0, stage, a->B, (const double *)a->d_cum, a->stage_n, a->total,
                               (const long long *)a->pop[a->cur].cells, a->cap, e->d_values, a->S, (const int *)e->d_f64_slot, a->d, (const double *)a->d_bw, a->d_base);
            if (hipGetLastError() != hipSuccess) { fg_set_error("ABC: the proposal kernel did not launch"); rc = FG_E_HIP; }
            if (!rc) rc = fg_log_joint(e, nullptr, nullptr);   // the scoring pass at the proposal: log_prior = row 0 of the accumulators, on the device
        }
        if (!rc) rc = abc_simulate_and_measure(a, stage);
        if (rc) break;
        hipLaunchKernelGGL(k_abc_accept, dim3(cp.grid), dim3(256), 0, e->stream, (const double *)a->d_dist, (const double *)e->d_acc, a->B, live, tol, prior ? 0 : 1, a->d_flag,
                           a->d_counts);
        hipLaunchKernelGGL(k_abc_scan, dim3(1), dim3(FG_ABC_SCAN_THREADS), 0, e->stream, (const int *)a->d_counts, cp.waves, a->d_offs, a->d_total);
        hipLaunchKernelGGL(k_abc_append, dim3(cp.grid), dim3(256), 0, e->stream, (const int *)a->d_flag, (const long long *)a->d_offs, a->B, a0, dst.n, a->cap,
                           (const long long *)e->d_values, a->S, (const double *)a->d_dist, (const double *)e->d_acc, dst);
        long long got = 0;                                 // the one small count that comes back per round
        hipError_t he = hipGetLastError();
        if (he == hipSuccess) he = hipMemcpyAsync(&got, a->d_total, sizeof(long long), hipMemcpyDeviceToHost, e->stream);
        if (he == hipSuccess) he = hipStreamSynchronize(e->stream);
        if (he != hipSuccess) { fg_set_error(std::string("ABC round: ") + hipGetErrorString(he)); rc = FG_E_HIP; break; }
        dst.n = std::min<long long>(a->cap, dst.n + got);
        a->have_round = true; a->round_prior = prior;
    }
    e->chain0 = chain0; e->X.chain0 = chain0;
    if (live_session && vbytes) {
        const hipError_t he = hipMemcpyAsync(e->d_values, a->d_save, vbytes, hipMemcpyDeviceToDevice, e->stream);
        if (he != hipSuccess && !rc) { fg_set_error(std::string("ABC: ") + hipGetErrorString(he)); rc = FG_E_HIP; }
    }
    if (rc) return rc;
    long long att = budget;
    if (dst.n == a->cap) {                                 // the sequential loop stops right after the n-th accept
        HIPCHK(hipMemcpyAsync(&att, dst.att + (a->cap - 1), sizeof(long long), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        att += 1;
    } else HIPCHK(hipStreamSynchronize(e->stream));
    if (accepted) *accepted = dst.n;
    if (attempts) *attempts = att;
    return FG_OK;
}

static int abc_fill(fg_abc *a, double *d_p, long long n, double v) {
    if (n < 1) return FG_OK;
    hipLaunchKernelGGL(k_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, a->e->stream, d_p, n, v);
    HIPCHK(hipGetLastError());
    return FG_OK;
}

extern "C" int fg_abc_round_prior(fg_abc *a, double tol, int64_t budget, int64_t *accepted, int64_t *attempts) {
    NEED_ABC(a);
    a->stage_open = false;
    FgAbcPop &dst = a->pop[a->cur];
    int rc = abc_rounds(a, 0u, true, tol, budget, dst, accepted, attempts);
    if (rc) { dst.n = 0; return rc; }
    if (dst.n > 0) rc = abc_fill(a, dst.w, dst.n, 1.0 / (double)dst.n);   // abc.rs:555-558
    if (!rc) HIPCHK(hipStreamSynchronize(a->e->stream));
    return rc;
}

extern "C" int fg_abc_stage_begin(fg_abc *a) {
    NEED_ABC(a);
    fg_engine *e = a->e;
    const FgAbcPop &P = a->pop[a->cur];
    a->stage_open = false;
    if (P.n < 1) { fg_set_error("fg_abc_stage_begin: no population (abc.rs:548-553)"); return FG_E_STATE; }
    const long long n = P.n;
    const int d = a->d;
    std::vector<double> coords((size_t)std::max(1, d) * (size_t)n);
    a->prev_w.resize((size_t)n);
    for (int c = 0; c < d; ++c)
        HIPCHK(hipMemcpyAsync(coords.data() + (size_t)c * n, P.cells + (long long)e->prog->f64_slot[c] * a->cap, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipMemcpyAsync(a->prev_w.data(), P.w, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    // kernel_bandwidths (abc.rs:751-773) and sample_index's total and cumulative sums (abc.rs:817-824), in the reference's order
    double total = 0.0;
    std::vector<double> cum((size_t)n);
    for (long long j = 0; j < n; ++j) { total = total + a->prev_w[(size_t)j]; cum[(size_t)j] = total; }
    if (!(total > 0.0)) { fg_set_error("fg_abc_stage_begin: the population's weights have no mass (abc.rs:818: the reference draws an index uniformly)"); return FG_E_STATE; }
    a->bw.assign((size_t)std::max(1, d), 1e-3);
    for (int c = 0; c < d; ++c) {
        const double *x = coords.data() + (size_t)c * n;
        double mean = 0.0;
        for (long long j = 0; j < n; ++j) mean = mean + a->prev_w[(size_t)j] * x[j];
        mean = mean / total;
        double var = 0.0;
        for (long long j = 0; j < n; ++j) { const double dv = x[j] - mean; var = var + a->prev_w[(size_t)j] * dv * dv; }
        var = var / total;
        const double b = std::sqrt(2.0 * var);
        a->bw[(size_t)c] = b > 1e-12 ? b : 1e-3;
    }
    HIPCHK(hipMemcpyAsync(a->d_cum, cum.data(), (size_t)n * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(a->d_bw, a->bw.data(), a->bw.size() * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));               // (the host vectors of the copies are locals)
    a->total = total; a->stage_n = n; a->pop[1 - a->cur].n = 0; a->stage_open = true;
    return FG_OK;
}

extern "C" int fg_abc_round_stage(fg_abc *a, uint32_t stage, double tol, int64_t budget, int64_t *accepted, int64_t *attempts) {
    NEED_ABC(a);
    if (!a->stage_open) { fg_set_error("fg_abc_round_stage: no open stage (fg_abc_stage_begin)"); return FG_E_STATE; }
    if (stage < 1u) { fg_set_error("fg_abc_round_stage: stage 0 is the prior stage (fg_abc_round_prior)"); return FG_E_BAD_ARG; }
    return abc_rounds(a, stage, false, tol, budget, a->pop[1 - a->cur], accepted, attempts);
}

extern "C" int fg_abc_stage_end(fg_abc *a) {
    NEED_ABC(a);
    fg_engine *e = a->e;
    FgAbcPop &nx = a->pop[1 - a->cur];
    const FgAbcPop &pv = a->pop[a->cur];
    if (!a->stage_open || nx.n < 1) { fg_set_error("fg_abc_stage_end: no open stage, or nothing accepted (abc.rs:623-630)"); return FG_E_STATE; }
    const long long m = nx.n, n = a->stage_n;
    const int d = a->d;
    const char *fs = std::getenv("FG_ABC_MIX_SPLITS");
    const long long force = fs ? std::atoll(fs) : 0;
    FgAbcMixPlan pl;
    int rc = fg_abc_mix_plan(m, n, d, std::max(1, e->n_simd / 4), force < 0 ? 0 : force, &pl);
    if (rc) { fg_set_error("fg_abc_stage_end: no launch plan for this shape"); return rc; }
    if (d > 0) {
        hipLaunchKernelGGL(k_abc_coords, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, e->stream, (const long long *)nx.cells, a->cap, m, (const int *)e->d_f64_slot, d, a->d_xc);
        hipLaunchKernelGGL(k_abc_coords, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, e->stream, (const long long *)pv.cells, a->cap, n, (const int *)e->d_f64_slot, d, a->d_cc);
        HIPCHK(hipGetLastError());
    }
    std::vector<double> konst, inv_s;
    abc_mixture_consts(a->prev_w.data(), n, a->bw.data(), d, konst, inv_s);
    const size_t n_k = (size_t)n, n_s = inv_s.size(), total = n_k + n_s + pl.table_elems + 2 * pl.partial_elems;
    double *buf = nullptr;
    HIPCHK(hipMalloc((void **)&buf, total * sizeof(double)));
    double *d_konst = buf, *d_inv_s = d_konst + n_k, *d_table = d_inv_s + n_s, *d_pmax = d_table + pl.table_elems, *d_psum = d_pmax + pl.partial_elems;
    std::vector<double> lp((size_t)m), ld((size_t)m);
    hipError_t he = hipMemcpyAsync(d_konst, konst.data(), n_k * sizeof(double), hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(d_inv_s, inv_s.data(), n_s * sizeof(double), hipMemcpyHostToDevice, e->stream);
    if (he == hipSuccess) { rc = abc_mixture_launch(e, pl, a->d_xc, m, a->d_cc, n, d, d_konst, d_inv_s, d_table, d_pmax, d_psum, nx.ld); if (rc) he = hipErrorUnknown; }
    if (he == hipSuccess) he = hipMemcpyAsync(ld.data(), nx.ld, (size_t)m * 8, hipMemcpyDeviceToHost, e->stream);
    if (he == hipSuccess) he = hipMemcpyAsync(lp.data(), nx.lp, (size_t)m * 8, hipMemcpyDeviceToHost, e->stream);
    const hipError_t hs = hipStreamSynchronize(e->stream);
    (void)hipFree(buf);
    if (rc) return rc;
    if (he != hipSuccess || hs != hipSuccess) { fg_set_error(std::string("fg_abc_stage_end: ") + hipGetErrorString(he != hipSuccess ? he : hs)); return FG_E_HIP; }
    // log w = log pi(theta) - log_denom, normalised by log_sum_exp (numerical.rs:15-38); 1 / n each when the normaliser is not finite (abc.rs:632-640)
    std::vector<double> w((size_t)m);
    double mx = FG_NEG_INF;
    for (long long i = 0; i < m; ++i) { w[(size_t)i] = lp[(size_t)i] - ld[(size_t)i]; mx = std::fmax(mx, w[(size_t)i]); }
    double log_norm = FG_NEG_INF;
    if (!(std::isinf(mx) && mx < 0.0)) {
        double se = 0.0;
        for (long long i = 0; i < m; ++i) se = se + std::exp(w[(size_t)i] - mx);
        log_norm = se == 0.0 ? FG_NEG_INF : mx + std::log(se);
    }
    for (long long i = 0; i < m; ++i) w[(size_t)i] = std::isfinite(log_norm) ? std::exp(w[(size_t)i] - log_norm) : 1.0 / (double)m;
    HIPCHK(hipMemcpyAsync(nx.w, w.data(), (size_t)m * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    a->cur = 1 - a->cur;
    a->stage_open = false;
    return FG_OK;
}

extern "C" int fg_abc_last_round(fg_abc *a, int64_t *h_index, double *h_dist, double *h_log_prior, int32_t *h_accept) {
    NEED_ABC(a);
    fg_engine *e = a->e;
    if (!a->have_round) { fg_set_error("fg_abc_last_round: no round has run"); return FG_E_STATE; }
    const size_t B = (size_t)a->B;
    if (h_index) {
        if (a->round_prior) for (size_t b = 0; b < B; ++b) h_index[b] = -1;
        else HIPCHK(hipMemcpyAsync(h_index, a->d_base, B * 8, hipMemcpyDeviceToHost, e->stream));
    }
    if (h_dist) HIPCHK(hipMemcpyAsync(h_dist, a->d_dist, B * 8, hipMemcpyDeviceToHost, e->stream));
    if (h_log_prior) HIPCHK(hipMemcpyAsync(h_log_prior, e->d_acc, B * 8, hipMemcpyDeviceToHost, e->stream));
    if (h_accept) HIPCHK(hipMemcpyAsync(h_accept, a->d_flag, B * 4, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return FG_OK;
}

extern "C" int fg_abc_get_population(fg_abc *a, int which, int64_t *out_n, void *h_cells, double *h_weights, double *h_dist, int64_t *h_attempt, double *h_log_prior,
                                     double *h_log_denom) {
    NEED_ABC(a);
    fg_engine *e = a->e;
    if (which != 0 && which != 1) { fg_set_error("fg_abc_get_population: which is 0 (current) or 1 (the open stage's accepted set)"); return FG_E_BAD_ARG; }
    if (which == 1 && !a->stage_open) { fg_set_error("fg_abc_get_population: no open stage"); return FG_E_STATE; }
    const FgAbcPop &P = a->pop[which == 0 ? a->cur : 1 - a->cur];
    const size_t n = (size_t)P.n;
    if (out_n) *out_n = P.n;
    if (n == 0) return FG_OK;
    if (h_cells) for (int j = 0; j < a->S; ++j) HIPCHK(hipMemcpyAsync((long long *)h_cells + (size_t)j * n, P.cells + (long long)j * a->cap, n * 8, hipMemcpyDeviceToHost, e->stream));
    if (h_weights) HIPCHK(hipMemcpyAsync(h_weights, P.w, n * 8, hipMemcpyDeviceToHost, e->stream));
    if (h_dist) HIPCHK(hipMemcpyAsync(h_dist, P.dist, n * 8, hipMemcpyDeviceToHost, e->stream));
    if (h_attempt) HIPCHK(hipMemcpyAsync(h_attempt, P.att, n * 8, hipMemcpyDeviceToHost, e->stream));
    if (h_log_prior) HIPCHK(hipMemcpyAsync(h_log_prior, P.lp, n * 8, hipMemcpyDeviceToHost, e->stream));
    if (h_log_denom) HIPCHK(hipMemcpyAsync(h_log_denom, P.ld, n * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return FG_OK;
}

extern "C" int fg_abc_set_population(fg_abc *a, int64_t n, const void *h_cells, const double *h_weights, const double *h_dist, const int64_t *h_attempt,
                                     const double *h_log_prior, const double *h_log_denom) {
    NEED_ABC(a);
    fg_engine *e = a->e;
    if (n < 1 || n > a->cap || !h_weights || (a->S > 0 && !h_cells)) { fg_set_error("fg_abc_set_population: n outside [1, capacity], or null cells / weights"); return FG_E_BAD_ARG; }
    FgAbcPop &P = a->pop[a->cur];
    a->stage_open = false;
    const size_t nn = (size_t)n;
    for (int j = 0; j < a->S; ++j) HIPCHK(hipMemcpyAsync(P.cells + (long long)j * a->cap, (const long long *)h_cells + (size_t)j * nn, nn * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(P.w, h_weights, nn * 8, hipMemcpyHostToDevice, e->stream));
    struct { double *dst; const void *src; } opt[] = { { P.dist, h_dist }, { (double *)P.att, h_attempt }, { P.lp, h_log_prior }, { P.ld, h_log_denom } };
    for (auto &o : opt) {
        if (o.src) HIPCHK(hipMemcpyAsync(o.dst, o.src, nn * 8, hipMemcpyHostToDevice, e->stream));
        else HIPCHK(hipMemsetAsync(o.dst, 0, nn * 8, e->stream));
    }
    HIPCHK(hipStreamSynchronize(e->stream));
    P.n = n;
    return FG_OK;
}
