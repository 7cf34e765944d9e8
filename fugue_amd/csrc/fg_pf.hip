// fg_pf.hip -- a bank of bootstrap particle filters on the device: WasmParticleFilter (crates/fugue-wasm/src/pf.rs), the reference's one
// sequential-in-time inference, B independent filters at once.  One workgroup = one filter; the filter's population stays in LDS for
// the whole launch and the kernel loops over the launch's observations (fg_pf_plan.h: the workgroup, who owns which particle, the
// fixed summation order, the cap on N, the cut of T into launches).  HBM is touched for the state at the launch's two ends and for
// five summary words per step and filter; the record form (fg_pf_step with array outputs) is the same kernel with non-null record
// pointers and changes no bit of any result.
//
// A step, pf.rs:107-172 line by line:
//   x_i += Normal(0, sig_step)               one Normal of the stream (seed, i, t, FG_RNG_PF), drawn as fg_sample draws a Normal site
//   lw_i += Normal(obs, sig_obs).log_prob(x) fg_logpdf's Normal (distribution.rs:189-208), ln sig_obs from the host
//   log_z_inc = log_sum_exp(lw) - ln n       numerical.rs:15-38 (max, sum of exp(lw - max), max + ln sum; -inf when all are -inf)
//   normalize_particles                      smc.rs:719-753: uniform on an all -inf population, else exp(lw - lse) and / sum when sum > 0
//   ess_frac = 1 / sum w^2 / n; resampled = ess_frac < threshold
//   resampled:  cumulative weights, systematic indices with thr_j = U / n + j / n and the index rule of k_resample_search
//               (fg_smc.hip), x = propagated[parents], lw = 0
//   otherwise:  lw_i = ln(max(w_i n, 1e-300))
#include "fg_engine_internal.h"
#include "fg_cold.h"
#include "fg_pf_plan.h"

namespace {

struct FgPfParam { double sig_step, sig_obs, ln_sig_obs, threshold; unsigned long long seed; };   // clamped; ln by the host's log
struct FgPfDev {
    double *x, *lw, *log_z;              // [B][n], [B][n], [B]: the state between launches
    const FgPfParam *par;                // [B]
    const double *obs;                   // the launch's observations: obs[b * obs_stride + s]
    long long obs_stride;                // 0: shared by the filters
    uint32_t t0;                         // steps taken before the launch: step s draws with iteration word t0 + s + 1
    int steps, n, n_pad, per_thread;
    double ln_n;                         // ln n by the host's log
    double *ess_frac, *log_z_inc, *mean, *var; int *resampled;   // [steps][B]
    double *r_prev, *r_prop, *r_w, *r_post; long long *r_parents;   // [B][n] or null (one step)
};

__device__ __forceinline__ double pf_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, FG_PF_WAVE);
    return v;
}
// the plan's sum of one value per thread (fg_pf_plan.h, steps 2 and 3); `slot` = this call's row of wave totals.  Every sum of a step has
// a row of its own, and a barrier that every step passes (the one of sum w^2) lies between two writes of a row: one barrier per call
__device__ __forceinline__ double pf_block_sum(double v, double *red, int slot, int lane, int wave, int n_waves) {
    v = pf_wave_sum(v);
    if (lane == 0) red[slot * 16 + wave] = v;
    __syncthreads();
    double tot = 0.0;
    for (int w = 0; w < n_waves; ++w) tot += red[slot * 16 + w];
    return tot;
}
__device__ __forceinline__ double pf_block_max(double v, double *red, int slot, int lane, int wave, int n_waves) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, FG_PF_WAVE));
    if (lane == 0) red[slot * 16 + wave] = v;
    __syncthreads();
    double m = FG_NEG_INF;
    for (int w = 0; w < n_waves; ++w) m = fmax(m, red[slot * 16 + w]);
    return m;
}

__global__ void k_pf_init(double *x, double *lw, const fg_pf_params *par, long long n, long long total) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= total) return;
    const long long b = g / n, i = g - b * n;
    FgStream s = fg_stream(par[b].seed, (uint32_t)i, 0u, FG_RNG_PF);
    x[g] = 0.0 + par[b].prior_sig * fg_rng_normal(s);      // pf.rs:86-88
    lw[g] = 0.0;
}

__global__ __launch_bounds__(FG_PF_MAX_THREADS) void k_pf_steps(FgPfDev Q) {
    extern __shared__ __attribute__((aligned(16))) double lds_pf[];
    const int n = Q.n, tid = (int)threadIdx.x, T = (int)blockDim.x, lane = tid & (FG_PF_WAVE - 1), wave = tid / FG_PF_WAVE, n_waves = T / FG_PF_WAVE;
    const long long b = blockIdx.x;
    double *xa = lds_pf, *xb = xa + Q.n_pad, *a = xb + Q.n_pad, *red = a + Q.n_pad;   // red: [6][16] rows of wave totals, one row per sum of a step; the scan's [16] behind them
    double *scn = red + 96;
    const FgPfParam P = Q.par[b];
    const size_t base = (size_t)b * (size_t)n;
    const double dn = (double)n;
    for (int i = tid; i < n; i += T) { xa[i] = Q.x[base + i]; a[i] = Q.lw[base + i]; }
    double log_z = Q.log_z[b];
    // (every elementwise phase below touches a thread's own particles i = tid, tid + T, ...: no barrier between them)
    for (int s = 0; s < Q.steps; ++s) {
        const double obs = Q.obs[b * Q.obs_stride + s];
        const uint32_t t = Q.t0 + (uint32_t)s + 1u;
        double m = FG_NEG_INF;
        for (int i = tid; i < n; i += T) {
            const double x0 = xa[i];
            const double z0 = fg_cold_normal_pair((uint32_t)P.seed, (uint32_t)(P.seed >> 32), (uint32_t)i, 0u, t, FG_RNG_PF).a;   // = fg_rng_normal on the fresh stream
            const double x1 = x0 + (0.0 + P.sig_step * z0);                    // pf.rs:112-117
            xa[i] = x1;
            double lp = FG_NEG_INF;                                            // distribution.rs:189-208
            if (fg_finite(x1)) { const double z = (x1 - obs) / P.sig_obs; lp = -0.5 * z * z - P.ln_sig_obs - 0.5 * FG_LN_2PI; }
            const double lw = a[i] + lp;                                       // pf.rs:124
            a[i] = lw;
            m = fmax(m, lw);
            if (Q.r_prev) Q.r_prev[base + i] = x0;
            if (Q.r_prop) Q.r_prop[base + i] = x1;
        }
        m = pf_block_max(m, red, 0, lane, wave, n_waves);
        const bool dead = m == FG_NEG_INF;                                     // numerical.rs:26: every log-weight is -inf
        double lse = FG_NEG_INF;
        if (!dead) {
            double se = 0.0;
            for (int i = tid; i < n; i += T) se += fg_cold_exp(a[i] - m);
            se = pf_block_sum(se, red, 1, lane, wave, n_waves);
            lse = se == 0.0 ? FG_NEG_INF : m + fg_cold_log(se);                        // numerical.rs:31-37
        }
        const double log_z_inc = lse - Q.ln_n;                                 // pf.rs:130
        log_z += log_z_inc;
        if (lse == FG_NEG_INF) {                                               // smc.rs:733-739
            for (int i = tid; i < n; i += T) a[i] = 1.0 / dn;
        } else {
            double sw = 0.0;
            for (int i = tid; i < n; i += T) { const double w = fg_cold_exp(a[i] - lse); a[i] = w; sw += w; }
            sw = pf_block_sum(sw, red, 2, lane, wave, n_waves);
            if (sw > 0.0) for (int i = tid; i < n; i += T) a[i] = a[i] / sw;   // smc.rs:747-752
        }
        double s2 = 0.0, sx = 0.0;
        for (int i = tid; i < n; i += T) { const double w = a[i]; s2 += w * w; sx += w * xa[i]; if (Q.r_w) Q.r_w[base + i] = w; }
        s2 = pf_wave_sum(s2); sx = pf_wave_sum(sx);
        if (lane == 0) { red[3 * 16 + wave] = s2; red[4 * 16 + wave] = sx; }
        __syncthreads();
        s2 = 0.0; sx = 0.0;
        for (int w = 0; w < n_waves; ++w) { s2 += red[3 * 16 + w]; sx += red[4 * 16 + w]; }
        const double mean = sx;
        double sv = 0.0;
        for (int i = tid; i < n; i += T) { const double d = xa[i] - mean; sv += a[i] * (d * d); }
        sv = pf_block_sum(sv, red, 5, lane, wave, n_waves);
        const double ess_frac = (1.0 / s2) / dn;                               // smc.rs:230-233, pf.rs:136
        const bool resampled = ess_frac < P.threshold;                         // the same bits in every thread: a uniform branch
        if (tid == 0) {
            const size_t o = (size_t)s * gridDim.x + (size_t)b;
            Q.ess_frac[o] = ess_frac; Q.log_z_inc[o] = log_z_inc; Q.resampled[o] = resampled ? 1 : 0; Q.mean[o] = mean; Q.var[o] = sv;
        }
        if (resampled) {
            FgStream su = fg_stream(P.seed, 0u, t, FG_RNG_PF_RESAMPLE);
            const double U = fg_rng_u01(su);
            __syncthreads();                                                   // the weights of every owner are in `a`; ownership changes to runs
            const int c0 = tid * Q.per_thread, c1 = c0 + Q.per_thread < n ? c0 + Q.per_thread : n;
            double run = 0.0;
            for (int i = c0; i < c1; ++i) { run += a[i]; a[i] = run; }
            double incl = run;
#pragma unroll
            for (int o = 1; o < FG_PF_WAVE; o <<= 1) { const double v = __shfl_up(incl, o, FG_PF_WAVE); if (lane >= o) incl += v; }
            double excl = __shfl_up(incl, 1, FG_PF_WAVE);
            if (lane == 0) excl = 0.0;
            if (lane == FG_PF_WAVE - 1) scn[wave] = incl;
            __syncthreads();
            double woff = 0.0;
            for (int w = 0; w < wave; ++w) woff += scn[w];
            const double off = woff + excl;
            for (int i = c0; i < c1; ++i) a[i] = off + a[i];
            __syncthreads();                                                   // cum complete
            for (int j = tid; j < n; j += T) {
                const double thr = U / dn + (double)j / dn;                    // smc.rs:258,264
                int lo = 0, hi = n;                                            // first k in [0, n) with cum[k] >= thr (k_resample_search)
                while (lo < hi) { const int mid = (lo + hi) >> 1; if (a[mid] >= thr) hi = mid; else lo = mid + 1; }
                const int p = lo < n ? lo : n - 1;
                const double xp = xa[p];
                xb[j] = xp;
                if (Q.r_parents) Q.r_parents[base + j] = p;
                if (Q.r_post) Q.r_post[base + j] = xp;
            }
            __syncthreads();                                                   // every search is done with cum and with xa
            for (int i = tid; i < n; i += T) a[i] = 0.0;                       // pf.rs:145
            double *sw_ = xa; xa = xb; xb = sw_;
        } else {
            for (int i = tid; i < n; i += T) {
                a[i] = fg_cold_log(fmax(a[i] * dn, 1e-300));                   // pf.rs:155
                if (Q.r_parents) Q.r_parents[base + i] = i;
                if (Q.r_post) Q.r_post[base + i] = xa[i];
            }
        }
    }
    for (int i = tid; i < n; i += T) { Q.x[base + i] = xa[i]; Q.lw[base + i] = a[i]; }
    if (tid == 0) Q.log_z[b] = log_z;
}

int pf_device_or_fail(int device) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { fg_set_error("no HIP device available: no CPU fallback (FG_E_NO_DEVICE)"); return FG_E_NO_DEVICE; }
    if (device < 0 || device >= ndev) { fg_set_error("bad device ordinal"); return FG_E_BAD_ARG; }
    HIPCHK(hipSetDevice(device));
    return FG_OK;
}

}  // namespace

struct fg_pf {
    int device = 0; long long n = 0, B = 0; uint64_t t = 0;
    FgPfPlan plan{};
    std::vector<fg_pf_params> par;                         // clamped
    hipStream_t stream = nullptr;
    double *d_x = nullptr, *d_lw = nullptr, *d_log_z = nullptr; FgPfParam *d_par = nullptr;
    double *d_obs = nullptr; size_t obs_cap = 0;           // grown as a run asks
    double *d_sum = nullptr; size_t sum_cap = 0;           // five summary tables [T][B] back to back (resampled as int)
    double *d_rec = nullptr;                               // five record arrays [B][n], at the first recorded step
    bool lds_raised = false;                               // k_pf_steps may declare FG_PF_LDS_BUDGET on this device
};

static int pf_upload_params(fg_pf *h) {
    std::vector<FgPfParam> dp((size_t)h->B);
    for (long long b = 0; b < h->B; ++b) {
        const fg_pf_params &p = h->par[(size_t)b];
        dp[(size_t)b] = { p.sig_step, p.sig_obs, std::log(p.sig_obs), p.ess_threshold, p.seed };
    }
    HIPCHK(hipMemcpyAsync(h->d_par, dp.data(), dp.size() * sizeof(FgPfParam), hipMemcpyHostToDevice, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));               // (dp is a local)
    return FG_OK;
}
static int pf_need(const fg_pf *h, const char *who) {
    if (!h) { fg_set_error(std::string(who) + ": null particle filter"); return FG_E_BAD_ARG; }
    return FG_OK;
}
template <class T> static int pf_grow(T **p, size_t *cap, size_t want) {
    if (want <= *cap) return FG_OK;
    if (*p) { HIPCHK(hipFree(*p)); *p = nullptr; *cap = 0; }
    HIPCHK(hipMalloc((void **)p, want * sizeof(T)));
    *cap = want;
    return FG_OK;
}

extern "C" {

int fg_pf_new(int device, int64_t n_particles, int64_t n_filters, const fg_pf_params *params, fg_pf **out) {
    if (!out) { fg_set_error("fg_pf_new: null out"); return FG_E_BAD_ARG; }
    *out = nullptr;
    if (!params) { fg_set_error("fg_pf_new: null params"); return FG_E_BAD_ARG; }
    if (n_filters < 1) { fg_set_error("fg_pf_new: n_filters must be at least 1"); return FG_E_BAD_ARG; }
    FgPfPlan pl;
    if (int rc = fg_pf_plan(n_particles, n_filters, &pl)) {
        fg_set_error(rc == FG_E_LIMIT ? "fg_pf_new: n_particles = " + std::to_string(n_particles) + " is above the " + std::to_string(FG_PF_N_CAP) + " one workgroup's LDS holds"
                                      : std::string("fg_pf_new: n_particles must be at least 2 (and n_filters below 2^31)"));
        return rc;
    }
    std::vector<fg_pf_params> par((size_t)n_filters);
    for (int64_t b = 0; b < n_filters; ++b) {
        fg_pf_params p = params[b];
        if (!std::isfinite(p.prior_sig) || !std::isfinite(p.sig_step) || !std::isfinite(p.sig_obs) || !std::isfinite(p.ess_threshold)) {
            fg_set_error("fg_pf_new: a non-finite parameter of filter " + std::to_string(b)); return FG_E_BAD_ARG; }
        p.prior_sig = std::max(p.prior_sig, 1e-6); p.sig_step = std::max(p.sig_step, 1e-6); p.sig_obs = std::max(p.sig_obs, 1e-6);   // pf.rs:85-94
        p.ess_threshold = std::min(std::max(p.ess_threshold, 0.0), 1.0);
        par[(size_t)b] = p;
    }
    if (int rc = pf_device_or_fail(device)) return rc;
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (std::string(prop.gcnArchName).rfind("gfx950", 0) != 0) { fg_set_error(std::string("device arch ") + prop.gcnArchName + " is not gfx950; kernels are built for MI355X only"); return FG_E_NO_DEVICE; }
    fg_pf *h = new fg_pf();
    h->device = device; h->n = n_particles; h->B = n_filters; h->plan = pl; h->par = par;
    const size_t BN = (size_t)n_filters * (size_t)n_particles;
    fg_pf_params *d_raw = nullptr;
    auto fail = [&](const char *what) { fg_set_error(std::string("fg_pf_new: ") + what); if (d_raw) (void)hipFree(d_raw); fg_pf_free(h); return FG_E_HIP; };
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess) return fail("no stream");
    if (hipMalloc((void **)&h->d_x, BN * 8) != hipSuccess || hipMalloc((void **)&h->d_lw, BN * 8) != hipSuccess || hipMalloc((void **)&h->d_log_z, (size_t)n_filters * 8) != hipSuccess ||
        hipMalloc((void **)&h->d_par, (size_t)n_filters * sizeof(FgPfParam)) != hipSuccess || hipMalloc((void **)&d_raw, (size_t)n_filters * sizeof(fg_pf_params)) != hipSuccess)
        return fail("no device memory for the bank");
    if (hipMemcpyAsync(d_raw, par.data(), par.size() * sizeof(fg_pf_params), hipMemcpyHostToDevice, h->stream) != hipSuccess ||
        hipMemsetAsync(h->d_log_z, 0, (size_t)n_filters * 8, h->stream) != hipSuccess) return fail("upload failed");
    hipLaunchKernelGGL(k_pf_init, dim3((unsigned)((BN + 255) / 256)), dim3(256), 0, h->stream, h->d_x, h->d_lw, (const fg_pf_params *)d_raw, (long long)n_particles, (long long)BN);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(h->stream) != hipSuccess) return fail("the initial draw failed");
    (void)hipFree(d_raw); d_raw = nullptr;
    if (int rc = pf_upload_params(h)) { fg_pf_free(h); return rc; }
    *out = h;
    return FG_OK;
}

int fg_pf_set_sig_obs(fg_pf *h, int64_t filter, double sig_obs) {
    if (int rc = pf_need(h, "fg_pf_set_sig_obs")) return rc;
    if (filter < -1 || filter >= h->B) { fg_set_error("fg_pf_set_sig_obs: filter outside [-1, n_filters)"); return FG_E_BAD_ARG; }
    if (!std::isfinite(sig_obs)) { fg_set_error("fg_pf_set_sig_obs: a non-finite sig_obs"); return FG_E_BAD_ARG; }
    HIPCHK(hipSetDevice(h->device));
    const double v = std::max(sig_obs, 1e-6);                                  // pf.rs:101-103
    for (long long b = 0; b < h->B; ++b) if (filter < 0 || b == filter) h->par[(size_t)b].sig_obs = v;
    return pf_upload_params(h);
}

// steps [0, T) of the run on obs (device copy in h->d_obs), the record pointers for a single step
static int pf_launches(fg_pf *h, long long T, long long obs_stride, double *const rec[5]) {
    const long long B = h->B;
    const FgPfPlan &pl = h->plan;
    if (pl.lds > 64 * 1024 && !h->lds_raised) {
        HIPCHK(hipFuncSetAttribute((const void *)k_pf_steps, hipFuncAttributeMaxDynamicSharedMemorySize, (int)FG_PF_LDS_BUDGET));
        h->lds_raised = true;
    }
    double *sum = h->d_sum;
    const size_t TB = (size_t)T * (size_t)B;
    for (long long k = 0; k < fg_pf_n_launches(pl, T); ++k) {
        long long first, count;
        fg_pf_launch_steps(pl, T, k, &first, &count);
        const size_t o = (size_t)first * (size_t)B;
        FgPfDev Q = { h->d_x, h->d_lw, h->d_log_z, h->d_par, h->d_obs + first, obs_stride, (uint32_t)h->t, (int)count, pl.n, pl.n_pad, pl.per_thread,
                      std::log((double)pl.n), sum + o, sum + TB + o, sum + 2 * TB + o, sum + 3 * TB + o, (int *)(sum + 4 * TB) + o,
                      rec ? rec[0] : nullptr, rec ? rec[1] : nullptr, rec ? rec[2] : nullptr, rec ? rec[4] : nullptr, rec ? (long long *)rec[3] : nullptr };
        hipLaunchKernelGGL(k_pf_steps, dim3(pl.grid), dim3((unsigned)pl.threads), pl.lds, h->stream, Q);
        HIPCHK(hipGetLastError());
        h->t += (uint64_t)count;                           // with the launch: a later launch that is refused leaves t where the state on the device is
    }
    HIPCHK(hipStreamSynchronize(h->stream));
    return FG_OK;
}
static int pf_check_obs(const char *who, const double *h_obs, long long count, int per_filter) {
    if (per_filter != 0 && per_filter != 1) { fg_set_error(std::string(who) + ": per_filter must be 0 or 1"); return FG_E_BAD_ARG; }
    if (count > 0 && !h_obs) { fg_set_error(std::string(who) + ": null observations"); return FG_E_BAD_ARG; }
    for (long long i = 0; i < count; ++i)
        if (!std::isfinite(h_obs[i])) { fg_set_error(std::string(who) + ": observation " + std::to_string(i) + " is not finite (Normal::new(obs, .).unwrap() panics: pf.rs:121)"); return FG_E_BAD_ARG; }
    return FG_OK;
}
static int pf_run_impl(fg_pf *h, const char *who, const double *h_obs, long long T, int per_filter, double *h_ess_frac, double *h_log_z_inc, int32_t *h_resampled,
                       double *h_mean, double *h_var, double *const h_rec[5]) {
    const long long B = h->B, n_obs = per_filter ? B * T : T;
    if (h->t + (uint64_t)T > 0xffffffffull) { fg_set_error(std::string(who) + ": more than 2^32 - 1 steps (the stream's iteration word)"); return FG_E_LIMIT; }
    if (T == 0) return FG_OK;
    HIPCHK(hipSetDevice(h->device));
    const size_t TB = (size_t)T * (size_t)B, BN = (size_t)B * (size_t)h->n;
    if (int rc = pf_grow(&h->d_obs, &h->obs_cap, (size_t)n_obs)) return rc;
    if (int rc = pf_grow(&h->d_sum, &h->sum_cap, 5 * TB)) return rc;
    bool want_rec = false;
    for (int k = 0; h_rec && k < 5; ++k) want_rec = want_rec || h_rec[k];
    double *rec[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    if (want_rec) {
        if (!h->d_rec) HIPCHK(hipMalloc((void **)&h->d_rec, 5 * BN * 8));
        for (int k = 0; k < 5; ++k) rec[k] = h->d_rec + (size_t)k * BN;      // (all five are written: which ones the caller reads changes no launch)
    }
    HIPCHK(hipMemcpyAsync(h->d_obs, h_obs, (size_t)n_obs * 8, hipMemcpyHostToDevice, h->stream));
    if (int rc = pf_launches(h, T, per_filter ? T : 0, want_rec ? rec : nullptr)) return rc;
    double *const outs[4] = { h_ess_frac, h_log_z_inc, h_mean, h_var };
    for (int k = 0; k < 4; ++k) if (outs[k]) HIPCHK(hipMemcpyAsync(outs[k], h->d_sum + (size_t)k * TB, TB * 8, hipMemcpyDeviceToHost, h->stream));
    if (h_resampled) HIPCHK(hipMemcpyAsync(h_resampled, h->d_sum + 4 * TB, TB * 4, hipMemcpyDeviceToHost, h->stream));
    for (int k = 0; want_rec && k < 5; ++k) if (h_rec[k]) HIPCHK(hipMemcpyAsync(h_rec[k], rec[k], BN * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return FG_OK;
}

int fg_pf_run(fg_pf *h, const double *h_obs, int64_t T, int per_filter, double *h_ess_frac, double *h_log_z_inc, int32_t *h_resampled, double *h_mean, double *h_var) {
    if (int rc = pf_need(h, "fg_pf_run")) return rc;
    if (T < 0) { fg_set_error("fg_pf_run: negative T"); return FG_E_BAD_ARG; }
    if (T > (1LL << 32)) { fg_set_error("fg_pf_run: more than 2^32 steps"); return FG_E_LIMIT; }
    if (int rc = pf_check_obs("fg_pf_run", h_obs, per_filter == 1 ? h->B * T : T, per_filter)) return rc;
    return pf_run_impl(h, "fg_pf_run", h_obs, T, per_filter, h_ess_frac, h_log_z_inc, h_resampled, h_mean, h_var, nullptr);
}

int fg_pf_step(fg_pf *h, const double *h_obs, int per_filter, double *h_ess_frac, double *h_log_z_inc, int32_t *h_resampled, double *h_mean, double *h_var,
               double *h_prev, double *h_propagated, double *h_weights, int64_t *h_parents, double *h_posterior) {
    if (int rc = pf_need(h, "fg_pf_step")) return rc;
    if (!h_obs) { fg_set_error("fg_pf_step: null observations"); return FG_E_BAD_ARG; }
    if (int rc = pf_check_obs("fg_pf_step", h_obs, per_filter == 1 ? h->B : 1, per_filter)) return rc;
    double *const rec[5] = { h_prev, h_propagated, h_weights, (double *)h_parents, h_posterior };
    return pf_run_impl(h, "fg_pf_step", h_obs, 1, per_filter, h_ess_frac, h_log_z_inc, h_resampled, h_mean, h_var, rec);
}

int fg_pf_log_evidence(fg_pf *h, double *h_out) {
    if (int rc = pf_need(h, "fg_pf_log_evidence")) return rc;
    if (!h_out) { fg_set_error("fg_pf_log_evidence: null h_out"); return FG_E_BAD_ARG; }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(h_out, h->d_log_z, (size_t)h->B * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return FG_OK;
}

int64_t fg_pf_t(const fg_pf *h) { return h ? (int64_t)h->t : -1; }

int fg_pf_positions(fg_pf *h, double *h_x) {
    if (int rc = pf_need(h, "fg_pf_positions")) return rc;
    if (!h_x) { fg_set_error("fg_pf_positions: null h_x"); return FG_E_BAD_ARG; }
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemcpyAsync(h_x, h->d_x, (size_t)h->B * (size_t)h->n * 8, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(hipStreamSynchronize(h->stream));
    return FG_OK;
}

void fg_pf_free(fg_pf *h) {
    if (!h) return;
    if (hipSetDevice(h->device) == hipSuccess) {
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        for (void *p : { (void *)h->d_x, (void *)h->d_lw, (void *)h->d_log_z, (void *)h->d_par, (void *)h->d_obs, (void *)h->d_sum, (void *)h->d_rec })
            if (p) (void)hipFree(p);
        if (h->stream) (void)hipStreamDestroy(h->stream);
    }
    delete h;
}

}  // extern "C"
