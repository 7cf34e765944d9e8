// fg_vi.hip -- mean-field variational inference (src/inference/vi.rs:104-923) over many Monte Carlo samples.
//
// One lane = one sample of one ELBO evaluation.  An evaluation is a guide: a row of factors {family, site, a, b} in
// address-sorted order.  The optimizer's 1 + 4P evaluations of an iteration (the monitor, and +eps / -eps for each of the
// 2P guide coordinates: vi.rs:784-864) are independent, so they are ONE grid (ceil(N / 64), n_eval).
//
//   k_vi_elbo    lane n of block (b, e): opens fg_stream(seed, sample0 + n, stream_id[e], FG_RNG_VI), draws every factor of
//                guide e in table order (MeanFieldGuide::sample_trace, vi.rs:609-630), scores the draw under the factor,
//                writes it into the site's slot (a factor whose address is no model site is drawn, so the stream advances
//                as in the reference, and adds nothing to log q: vi.rs:659-664), scores the program once (ScoreGivenTrace)
//                and forms term = (prior + lik + fac) - log_q.  Common random numbers are nothing but equal stream ids:
//                the +eps and -eps evaluations of a coordinate share one (elbo_gradient_fd, vi.rs:687-725).
//   k_vi_reduce  one block per evaluation adds the per-wave sums and divides by N.
//
// THE ENGINE'S ELBO SUM (no atomics; the two orders below define it, tests/vi_restatement.py restates them in numpy):
//   wave order   v = the wave's 64 terms (dead lanes: +0.0);  for s in 32, 16, 8, 4, 2, 1:  v[i] = v[i] + v[i + s], i < s;
//                partial[e][b] = v[0]
//   block order  thread t < 256 adds partial[e][t], partial[e][t + 256], ... onto +0.0 in that order;  then
//                for s in 128, 64, .., 1:  a[t] = a[t] + a[t + s], t < s;   elbo[e] = a[0] / N
// IEEE does the rest: one -inf term makes the ELBO -inf, and a (-inf) - (-inf) gradient is NaN, which the optimizer skips
// like the reference (vi.rs:846-853).
#include "fg_engine_internal.h"

// One factor as the kernel reads it: 64 bytes = one s_load_dwordx16 (the table is wave-uniform).  The host resolves what
// is the same for every sample: the distribution kind, the LDS slot of the site, exp() of the log-scale coordinates and
// the hoisted constants of fg_hoist (host libm: the arithmetic the oracle's log-density uses).
struct FgViFactorDev { uint32_t kind; int32_t slot; uint32_t hoisted, pad0; double p0, p1, h0, h1; double pad1[2]; };
static_assert(sizeof(FgViFactorDev) == 64, "FgViFactorDev must be 64 bytes");

struct FgViDev {
    const FgViFactorDev *tab;      // [n_eval][n_factors]
    const uint32_t *stream_id;     // [n_eval]
    int n_factors;
    double *terms;                 // [n_eval][N] or null (with them, evaluation 0 leaves its draws in the engine's values)
    double *partial;               // [n_eval][n_blocks]
    double *gtile;                 // GT: [n_eval * n_blocks][n_slots][64]
};

#define FG_VI_RED 256             /* threads of k_vi_reduce */

// the wave order (see the head of this file); every lane returns a value, lane 0 the wave's sum
__device__ __forceinline__ double fg_vi_wave_sum(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_down(v, s, FG_WAVE);
    return v;
}

template <bool GT>
__global__ __launch_bounds__(FG_WAVE, FG_MIN_WAVES) void k_vi_elbo(FgProgramDev P, FgChainCtx X, FgViDev V) {
    extern __shared__ double lds_[];
    const int e = blockIdx.y;
    double *lds = GT ? V.gtile + ((size_t)e * gridDim.x + blockIdx.x) * P.n_slots * FG_WAVE : lds_;
    constexpr int tw = FG_WAVE;                        // one lane = one sample
    const long long n = (long long)blockIdx.x * tw + threadIdx.x;
    const bool live = n < X.C;
    const long long c = live ? n : X.C - 1;
    double *slots = lds + threadIdx.x;
    for (int j = 0; j < P.n_slots; ++j) slots[j * tw] = 0.0;
    FgStream rng = fg_stream(X.seed, X.chain0 + (uint32_t)c, V.stream_id[e], FG_RNG_VI);
    const FG_AS4 char *tb = (const FG_AS4 char *)(uintptr_t)(V.tab + (size_t)e * V.n_factors);
    double log_q = 0.0;
    for (int f = 0; f < V.n_factors; ++f) {
        const fg_u32x16 q = *(const FG_AS4 fg_u32x16 *)(tb + 64 * (size_t)f);
        const uint32_t kind = q[0];
        const int slot = (int)q[1];
        const bool hoisted = q[2] != 0u;
        const double p0 = fg_dbl(q[4], q[5]), p1 = fg_dbl(q[6], q[7]);
        const double x = fg_as_double(fg_sample_cold(kind, false, p0, p1, 0.0, &rng));          // param.sample, vi.rs:294-323
        const double lq = fg_logpdf_cold(kind, hoisted, false, x, 0, p0, p1, 0.0, fg_dbl(q[8], q[9]), fg_dbl(q[10], q[11]), 0.0, 0.0, 0.0, false);
        if (slot >= 0) { log_q += lq; slots[slot * tw] = x; }                                    // vi.rs:659-664
    }
    if (live && V.terms && e == 0) fg_store_values(P, X, c, slots, tw);                          // the guide trace of evaluation 0, for inspection
    FgAcc3 A = {0.0, 0.0, 0.0};
    fg_exec<FG_MODE_SCORE, true>(P.ins_fast, P.n_ins, P.pool, slots, tw, A, nullptr, nullptr, X.C, live);
    const double term = fg_total(A) - log_q;                                                     // vi.rs:657-665
    if (live && V.terms) V.terms[(long long)e * X.C + n] = term;
    const double s = fg_vi_wave_sum(live ? term : 0.0);
    if (threadIdx.x == 0) V.partial[(size_t)e * gridDim.x + blockIdx.x] = s;
}

// estimate_elbo (vi.rs:905-923): the per-sample term is log_likelihood + log_factors of a prior run; same wave order
__global__ __launch_bounds__(FG_WAVE) void k_vi_prior_terms(const double *acc /*[3][N]*/, long long N, double *partial) {
    const long long n = (long long)blockIdx.x * FG_WAVE + threadIdx.x;
    const bool live = n < N;
    const long long c = live ? n : N - 1;
    const double term = acc[N + c] + acc[2 * N + c];
    const double s = fg_vi_wave_sum(live ? term : 0.0);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

// the block order (see the head of this file)
__global__ __launch_bounds__(FG_VI_RED) void k_vi_reduce(const double *partial /*[n_eval][nb]*/, int nb, long long N, double *elbo /*[n_eval]*/) {
    __shared__ double a[FG_VI_RED];
    const int t = threadIdx.x;
    const double *row = partial + (size_t)blockIdx.x * nb;
    double v = 0.0;
    for (int b = t; b < nb; b += FG_VI_RED) v = v + row[b];
    a[t] = v;
    __syncthreads();
    for (int s = FG_VI_RED / 2; s >= 1; s >>= 1) {
        if (t < s) a[t] = a[t] + a[t + s];
        __syncthreads();
    }
    if (t == 0) elbo[blockIdx.x] = a[0] / (double)N;
}

namespace {

int vi_alloc(fg_engine *e, void **p, size_t bytes) {
    HIPCHK(hipMalloc(p, bytes ? bytes : 1));
    e->vi_allocs.push_back(*p);
    return FG_OK;
}

// device scratch of the VI calls, grown on demand and kept for the engine's life (freed by fg_engine_free)
int vi_reserve(fg_engine *e, int n_eval, int n_factors, bool want_terms) {
    const size_t nb = (size_t)((e->C + FG_WAVE - 1) / FG_WAVE);
    const size_t n_tab = (size_t)n_eval * std::max(1, n_factors);
    if (n_tab > e->vi_cap_tab) { if (int rc = vi_alloc(e, &e->d_vi_tab, n_tab * sizeof(FgViFactorDev))) return rc; e->vi_cap_tab = n_tab; }
    if ((size_t)n_eval > e->vi_cap_eval) {
        if (int rc = vi_alloc(e, (void **)&e->d_vi_sid, (size_t)n_eval * 4)) return rc;
        if (int rc = vi_alloc(e, (void **)&e->d_vi_partial, (size_t)n_eval * nb * 8)) return rc;
        if (int rc = vi_alloc(e, (void **)&e->d_vi_elbo, (size_t)n_eval * 8)) return rc;
        if (e->gt) { if (int rc = vi_alloc(e, (void **)&e->d_vi_gtile, (size_t)n_eval * nb * e->n_slots * FG_WAVE * 8)) return rc; }
        e->vi_cap_eval = (size_t)n_eval;
    }
    if (want_terms && (size_t)n_eval > e->vi_cap_terms) {
        if (int rc = vi_alloc(e, (void **)&e->d_vi_terms, (size_t)n_eval * e->C * 8)) return rc;
        e->vi_cap_terms = (size_t)n_eval;
    }
    return FG_OK;
}

const uint32_t VI_KIND[3] = { FG_NORMAL, FG_LOGNORMAL, FG_BETA };

// ScoreGivenTrace over a guide trace needs every sample site in the trace as an f64 (interpreters.rs:138-163 panics
// otherwise; GuideError::UnsupportedDiscreteLatent, vi.rs:136-144), and a factor needs finite parameters.
int vi_validate(const fg_engine *e, const fg_vi_factor *row, int n_factors) {
    for (int j = 0; j < e->S; ++j) if (e->prog->site_vtype[j] != FG_F64) {
        fg_set_error("mean-field VI does not support the discrete latent at " + e->prog->stmts[e->prog->sorted_stmt[j]].addr + ": only continuous latents (Normal/LogNormal/Beta factors) can be approximated");
        return FG_ERR_ADDRESS_NOT_FOUND; }
    std::vector<char> seen((size_t)std::max(1, e->S), 0);
    int last = -1;                                             // site of the last factor that has one
    for (int f = 0; f < n_factors; ++f) {
        const fg_vi_factor &q = row[f];
        if (q.family < 0 || q.family > 2) { fg_set_error("fg_vi: factor family must be 0 (Normal), 1 (LogNormal) or 2 (Beta)"); return FG_E_BAD_ARG; }
        if (q.site < -1 || q.site >= e->S) { fg_set_error("fg_vi: factor site out of range"); return FG_E_BAD_ARG; }
        if (!std::isfinite(q.a)) { fg_set_error("fg_vi: non-finite factor parameter (location)"); return q.family == 2 ? FG_ERR_INVALID_SHAPE : FG_ERR_INVALID_MEAN; }
        if (!std::isfinite(q.b)) { fg_set_error("fg_vi: non-finite factor parameter (scale)"); return q.family == 2 ? FG_ERR_INVALID_SHAPE : FG_ERR_INVALID_VARIANCE; }
        if (q.site >= 0) {
            if (q.site <= last) { fg_set_error("fg_vi: factors must be in address-sorted order, one per site"); return FG_E_BAD_ARG; }
            last = q.site; seen[q.site] = 1;
        }
    }
    for (int j = 0; j < e->S; ++j) if (!seen[j]) {
        fg_set_error("address not found in the guide trace: " + e->prog->stmts[e->prog->sorted_stmt[j]].addr);
        return FG_ERR_ADDRESS_NOT_FOUND; }
    return FG_OK;
}

FgViFactorDev vi_lower(const fg_engine *e, const fg_vi_factor &q) {
    FgViFactorDev r; std::memset(&r, 0, sizeof(r));
    r.kind = VI_KIND[q.family];
    r.slot = q.site >= 0 ? e->prog->site_slot[q.site] : -1;
    r.p0 = q.family == 2 ? std::exp(q.a) : q.a;            // Beta: alpha = exp(log_alpha), vi.rs:314
    r.p1 = std::exp(q.b);                                  // sigma = exp(log_sigma) / beta = exp(log_beta), vi.rs:297,304,315
    double h[5];
    r.hoisted = fg_hoist(r.kind, r.p0, r.p1, 0.0, h) ? 1u : 0u;      // invalid (exp under- or overflowed): the device guards give -inf
    r.h0 = h[0]; r.h1 = h[1];
    return r;
}

unsigned long long vi_raised[2] = {0ull, 0ull};

// table + stream ids up, one k_vi_elbo launch over all evaluations, one k_vi_reduce launch; results stay on the device
int vi_launch(fg_engine *e, const std::vector<FgViFactorDev> &tab, const std::vector<uint32_t> &sid, int n_eval, int n_factors, bool want_terms) {
    if (n_eval < 1 || n_eval > 65535) { fg_set_error("fg_vi: n_eval must be in [1, 65535]"); return FG_E_LIMIT; }
    if (int rc = vi_reserve(e, n_eval, n_factors, want_terms)) return rc;
    if (!tab.empty()) HIPCHK(hipMemcpyAsync(e->d_vi_tab, tab.data(), tab.size() * sizeof(FgViFactorDev), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->d_vi_sid, sid.data(), (size_t)n_eval * 4, hipMemcpyHostToDevice, e->stream));
    const unsigned nb = (unsigned)((e->C + FG_WAVE - 1) / FG_WAVE);
    FgViDev V; V.tab = (const FgViFactorDev *)e->d_vi_tab; V.stream_id = e->d_vi_sid; V.n_factors = n_factors;
    V.terms = want_terms ? e->d_vi_terms : nullptr; V.partial = e->d_vi_partial; V.gtile = e->d_vi_gtile;
    int rc;
    if (e->gt) rc = fg_launch(e, k_vi_elbo<true>, vi_raised[1], dim3(nb, (unsigned)n_eval), dim3(FG_WAVE), 0, e->P, e->X, V);
    else rc = fg_launch(e, k_vi_elbo<false>, vi_raised[0], dim3(nb, (unsigned)n_eval), dim3(FG_WAVE), e->lds_score, e->P, e->X, V);
    if (rc) return rc;
    hipLaunchKernelGGL(k_vi_reduce, dim3((unsigned)n_eval), dim3(FG_VI_RED), 0, e->stream, (const double *)e->d_vi_partial, (int)nb, e->C, e->d_vi_elbo);
    HIPCHK(hipGetLastError());
    return FG_OK;
}

// apply_update's clamps (vi.rs:104-109, 457-483): locations of Normal / LogNormal to +-1e6, every log-scale to [-20, 20]
double vi_clamped(int family, int coord, double v) {
    const double lo = (family != 2 && coord == 0) ? -1.0e6 : -20.0, hi = (family != 2 && coord == 0) ? 1.0e6 : 20.0;
    return v < lo ? lo : (v > hi ? hi : v);
}

}  // namespace

extern "C" {

void fg_vi_config_default(fg_vi_config *c) {      // VIConfig::default, vi.rs:747-759 (n_samples_per_iter is the engine's n_chains)
    if (!c) return;
    c->n_iterations = 1000; c->convergence_window = 20; c->base_learning_rate = 0.1; c->fd_eps = 0.01; c->convergence_tol = 1e-4;
    c->step_decay_exponent = 0.6;
}

int fg_vi_elbo_batch(fg_engine *e, const fg_vi_factor *h_factors, int n_eval, int n_factors, const uint32_t *h_stream_ids, double *h_elbo,
                     double *h_terms) {
    NEED_ENGINE(e);
    if (n_eval < 1 || n_factors < 0 || !h_stream_ids || !h_elbo || (n_factors > 0 && !h_factors)) { fg_set_error("fg_vi_elbo_batch: bad argument"); return FG_E_BAD_ARG; }
    std::vector<FgViFactorDev> tab((size_t)n_eval * n_factors);
    for (int k = 0; k < n_eval; ++k) {
        if (int rc = vi_validate(e, h_factors + (size_t)k * n_factors, n_factors)) return rc;
        for (int f = 0; f < n_factors; ++f) tab[(size_t)k * n_factors + f] = vi_lower(e, h_factors[(size_t)k * n_factors + f]);
    }
    const std::vector<uint32_t> sid(h_stream_ids, h_stream_ids + n_eval);
    if (int rc = vi_launch(e, tab, sid, n_eval, n_factors, h_terms != nullptr)) return rc;
    HIPCHK(hipMemcpyAsync(h_elbo, e->d_vi_elbo, (size_t)n_eval * 8, hipMemcpyDeviceToHost, e->stream));
    if (h_terms) HIPCHK(hipMemcpyAsync(h_terms, e->d_vi_terms, (size_t)n_eval * e->C * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return FG_OK;
}

// optimize_meanfield_vi_with_config (vi.rs:784-864) with the loop on the host: per iteration one k_vi_elbo launch over the
// monitor and the 4P perturbed guides, one k_vi_reduce launch and one copy of 1 + 4P doubles.  Stream ids: iteration t uses
// t (2P + 1) for the monitor and t (2P + 1) + 1 + j for both signs of coordinate j = 2 factor + (0 location | 1 scale) --
// the reference's one fresh seed per monitor and per coordinate (vi.rs:800, 836).
int fg_vi_optimize(fg_engine *e, fg_vi_factor *h_factors, int n_factors, const fg_vi_config *cfg, double *h_elbo_history, fg_vi_result *res) {
    NEED_ENGINE(e);
    if (!cfg || !res || n_factors < 0 || (n_factors > 0 && !h_factors) || cfg->n_iterations < 0 || cfg->convergence_window < 0 ||
        (cfg->n_iterations > 0 && !h_elbo_history)) { fg_set_error("fg_vi_optimize: bad argument"); return FG_E_BAD_ARG; }
    const int P = n_factors, n_eval = 1 + 4 * P;
    if ((unsigned long long)cfg->n_iterations * (2ull * P + 1ull) >= (1ull << 32)) {
        fg_set_error("fg_vi_optimize: n_iterations (2 n_factors + 1) must stay below 2^32 (one random stream per monitor and per coordinate)"); return FG_E_LIMIT; }
    if (int rc = vi_validate(e, h_factors, P)) return rc;
    res->converged = 0; res->iterations = 0;
    std::vector<FgViFactorDev> tab((size_t)n_eval * P);
    std::vector<uint32_t> sid((size_t)n_eval);
    std::vector<double> elbo((size_t)n_eval);
    const double eps = cfg->fd_eps;
    const size_t w = (size_t)cfg->convergence_window;
    for (int t = 0; t < cfg->n_iterations; ++t) {
        res->iterations = t + 1;
        const uint32_t s0 = (uint32_t)t * (uint32_t)(2 * P + 1);
        std::vector<FgViFactorDev> base((size_t)P);
        for (int f = 0; f < P; ++f) base[f] = vi_lower(e, h_factors[f]);
        for (int k = 0; k < n_eval; ++k) std::copy(base.begin(), base.end(), tab.begin() + (size_t)k * P);
        sid[0] = s0;
        for (int j = 0; j < 2 * P; ++j)
            for (int sg = 0; sg < 2; ++sg) {                                       // shifted(), vi.rs:418-454
                const int k = 1 + 2 * j + sg;
                fg_vi_factor q = h_factors[j / 2];
                ((j & 1) ? q.b : q.a) += sg ? -eps : eps;
                tab[(size_t)k * P + j / 2] = vi_lower(e, q);
                sid[k] = s0 + 1u + (uint32_t)j;
            }
        if (int rc = vi_launch(e, tab, sid, n_eval, P, false)) return rc;
        HIPCHK(hipMemcpyAsync(elbo.data(), e->d_vi_elbo, (size_t)n_eval * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        h_elbo_history[t] = elbo[0];
        const size_t n = (size_t)t + 1;
        if (w > 0 && n >= 2 * w) {                                                 // ELBO plateau, vi.rs:809-821
            double recent = 0.0, previous = 0.0;
            for (size_t i = n - w; i < n; ++i) recent += h_elbo_history[i];
            for (size_t i = n - 2 * w; i < n - w; ++i) previous += h_elbo_history[i];
            recent /= (double)w; previous /= (double)w;
            const double denom = std::fmax(std::fabs(previous), 1e-8);
            if (std::fabs(recent - previous) / denom < cfg->convergence_tol) { res->converged = 1; break; }
        }
        const double step = cfg->base_learning_rate * std::pow((double)(t + 1), -cfg->step_decay_exponent);   // Robbins-Monro, vi.rs:824-825
        for (int j = 0; j < 2 * P; ++j) {                                          // Jacobi update from the snapshot, vi.rs:827-855
            const double grad = (elbo[1 + 2 * j] - elbo[2 + 2 * j]) / (2.0 * eps);
            if (!std::isfinite(grad)) continue;
            const double update = step * grad;
            if (!std::isfinite(update)) continue;
            fg_vi_factor &q = h_factors[j / 2];
            double &x = (j & 1) ? q.b : q.a;
            x = vi_clamped(q.family, j & 1, x + update);
        }
    }
    return FG_OK;
}

int fg_vi_estimate_elbo(fg_engine *e, uint32_t iteration, double *h_elbo) {
    NEED_ENGINE(e);
    if (!h_elbo) return FG_E_BAD_ARG;
    if (int rc = vi_reserve(e, 1, 0, false)) return rc;
    if (int rc = fg_launch_prior(e, iteration, FG_RNG_PRIOR, e->d_acc, nullptr)) return rc;
    const unsigned nb = (unsigned)((e->C + FG_WAVE - 1) / FG_WAVE);
    hipLaunchKernelGGL(k_vi_prior_terms, dim3(nb), dim3(FG_WAVE), 0, e->stream, (const double *)e->d_acc, e->C, e->d_vi_partial);
    hipLaunchKernelGGL(k_vi_reduce, dim3(1), dim3(FG_VI_RED), 0, e->stream, (const double *)e->d_vi_partial, (int)nb, e->C, e->d_vi_elbo);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_elbo, e->d_vi_elbo, 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return FG_OK;
}

}  // extern "C"
