// fg_psis.hip -- Pareto-smoothed importance-sampling LOO and k-hat per observe statement from a stored pointwise log-likelihood
// table d_ll [n][n_sel][C] on the device (the reference has neither; the rule is the R `loo` package's psis / gpdfit, restated in
// tests/psis_restatement.py).  Integers, work buffers and every summation order are fg_psis_plan.h's; here are the kernels and the C
// ABI.  Nothing is replayed and no engine state changes: the call reads the engine's chain count, device and stream.
//
//   k_psis_hist     one radix pass of the select: the cells of a statement (grid y) whose key matches the prefix decided so far are
//                   counted per digit in LDS (u32, integer atomics) and flushed to the statement's global histogram; the first
//                   pass also leaves the smallest key, the largest key that is no NaN and the counts of -inf / +inf / NaN cells
//   k_psis_pick     the selection step of a pass, one workgroup per statement: the digit that holds the rank; zeroes the histogram
//   k_psis_collect  one pass: cells below the cutoff key go into the statement's tail through an integer cursor (arrival order is
//                   arbitrary: the sort removes it), cells above it add exp(x_min - x) to the body's sum, every cell exp(x - x_max)
//                   to lppd's; block partials in the plan's order, no floating-point atomics
//                   (plain double: closed bounds hold for these two sums)
//   k_psis_fit      one workgroup per statement: fills the cutoff's copies in by count, sorts the tail (bitonic, in the work buffer;
//                   the stages that fit a chunk run in LDS), t_j, the G profile sums, theta-hat, k-hat, sigma-hat, the smoothed tail and
//                   its two sums, and the statement's row of words and counts; everything after the rule's doubles lw = x_min - x
//                   in double-double (fg_psis_dd.h), every word rounded once
#include "fg_engine_internal.h"
#include "fg_psis_plan.h"
#include "fg_psis_dd.h"

#define FG_PSIS_BINS (1 << FG_PSIS_DIGIT_BITS)
#define FG_PSIS_WAVES (FG_PSIS_THREADS / 64)
#define FG_PSIS_FIT_WAVES (FG_PSIS_FIT_THREADS / 64)


__device__ __forceinline__ double psis_cell(const double *ll, unsigned i, unsigned C, long long n_sel, long long k) {
    const unsigned draw = i / C, chain = i - draw * C;
    return ll[((long long)draw * n_sel + k) * (long long)C + (long long)chain];
}

__global__ __launch_bounds__(FG_PSIS_THREADS) void k_psis_hist(const double *ll, unsigned S, unsigned C, long long n_sel, long long k0, int b, int w, int first,
                                                                unsigned long long *state, unsigned int *cls, unsigned int *hist) {
    __shared__ unsigned int sh[FG_PSIS_BINS];
    __shared__ unsigned long long mm[FG_PSIS_WAVES][2];
    __shared__ unsigned int cc[FG_PSIS_WAVES][3];
    const long long k = blockIdx.y;
    for (int j = threadIdx.x; j < FG_PSIS_BINS; j += FG_PSIS_THREADS) sh[j] = 0u;
    const unsigned long long pf = state[k * FG_PSIS_STATE_WORDS + FG_PSIS_ST_PREFIX];
    const int lo = 64 - b - w;
    const unsigned int mask = (1u << w) - 1u;
    unsigned long long a = ~0ull, z = 0ull;
    unsigned int c0 = 0u, c1 = 0u, c2 = 0u;
    __syncthreads();
    const unsigned long long stride = (unsigned long long)gridDim.x * FG_PSIS_THREADS;
    for (unsigned long long i = (unsigned long long)blockIdx.x * FG_PSIS_THREADS + threadIdx.x; i < S; i += stride) {
        const double x = psis_cell(ll, (unsigned)i, C, n_sel, k0 + k);
        const unsigned long long key = fg_psis_key(x);
        if (first) {
            const bool nan = x != x;
            a = key < a ? key : a;
            if (!nan) z = key > z ? key : z;
            c0 += x == -INFINITY ? 1u : 0u; c1 += x == INFINITY ? 1u : 0u; c2 += nan ? 1u : 0u;
        }
        if (b == 0 || ((key ^ pf) >> (64 - b)) == 0ull) atomicAdd(&sh[(unsigned int)(key >> lo) & mask], 1u);
    }
    __syncthreads();
    unsigned int *h = hist + k * FG_PSIS_BINS;
    for (int j = threadIdx.x; j < FG_PSIS_BINS; j += FG_PSIS_THREADS)
        if (sh[j]) atomicAdd(&h[j], sh[j]);
    if (!first) return;
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long a2 = __shfl_down(a, o, 64), z2 = __shfl_down(z, o, 64);
        a = a2 < a ? a2 : a; z = z2 > z ? z2 : z;
        c0 += __shfl_down(c0, o, 64); c1 += __shfl_down(c1, o, 64); c2 += __shfl_down(c2, o, 64);
    }
    if ((threadIdx.x & 63) == 0) { mm[threadIdx.x >> 6][0] = a; mm[threadIdx.x >> 6][1] = z; cc[threadIdx.x >> 6][0] = c0; cc[threadIdx.x >> 6][1] = c1; cc[threadIdx.x >> 6][2] = c2; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int v = 1; v < FG_PSIS_WAVES; ++v) {
            a = mm[v][0] < a ? mm[v][0] : a; z = mm[v][1] > z ? mm[v][1] : z;
            c0 += cc[v][0]; c1 += cc[v][1]; c2 += cc[v][2];
        }
        atomicMin(&state[k * FG_PSIS_STATE_WORDS + FG_PSIS_ST_MIN], a);
        atomicMax(&state[k * FG_PSIS_STATE_WORDS + FG_PSIS_ST_MAX], z);
        if (c0) atomicAdd(&cls[k * FG_PSIS_CLASS_WORDS + 0], c0);
        if (c1) atomicAdd(&cls[k * FG_PSIS_CLASS_WORDS + 1], c1);
        if (c2) atomicAdd(&cls[k * FG_PSIS_CLASS_WORDS + 2], c2);
    }
}

// The bins of a pass hold the cells of the bucket; the digit d with (cells of the digits before d) < rank <= (... through d) is the
// next digit of the cutoff key.
__global__ __launch_bounds__(FG_PSIS_THREADS) void k_psis_pick(unsigned long long *state, unsigned int *hist, int b, int w) {
    __shared__ unsigned int part[FG_PSIS_THREADS];
    const long long k = blockIdx.x;
    unsigned int *h = hist + k * FG_PSIS_BINS;
    const int per = FG_PSIS_PICK_GROUP;                    // the bins past 2^w of a narrow last pass stay zero
    unsigned int s = 0u;
    for (int j = 0; j < per; ++j) s += h[threadIdx.x * per + j];
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long *st = state + k * FG_PSIS_STATE_WORDS;
        const unsigned long long rank = st[FG_PSIS_ST_RANK];
        unsigned long long c1, c2;
        const int g = fg_psis_pick_bin(part, FG_PSIS_THREADS, rank, &c1);
        const int d = fg_psis_pick_bin(h + g * per, per, rank - c1, &c2);
        fg_psis_advance(st, b, w, g * per + d, c1 + c2, h[g * per + d]);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < FG_PSIS_BINS; j += FG_PSIS_THREADS) h[j] = 0u;
}

__device__ __forceinline__ FgDD psis_dd_shfl_xor(FgDD v, int o) { FgDD r; r.hi = __shfl_xor(v.hi, o, 64); r.lo = __shfl_xor(v.lo, o, 64); return r; }
// the plan's fold of a wave's 64 partials: v[l] + v[l ^ 32], then ^ 16, ... ^ 1 (every lane ends with the total), on pairs
__device__ __forceinline__ FgDD psis_dd_wave_fold(FgDD v) {
    for (int o = 32; o > 0; o >>= 1) v = fg_dd_add(v, psis_dd_shfl_xor(v, o));
    return v;
}
static __device__ __noinline__ FgDD psis_dd_exp(FgDD a) { return fg_dd_exp(a); }
static __device__ __noinline__ FgDD psis_dd_log(FgDD a) { return fg_dd_log(a); }
static __device__ __noinline__ FgDD psis_dd_expm1(FgDD a) { return fg_dd_expm1(a); }
// exp(a - b) of two cells: the difference is the rule's IEEE double (lw = x_min - x is data of every later formula), the rest is not rounded
__device__ __forceinline__ FgDD psis_dd_exp_diff(double a, double b) { return psis_dd_exp(fg_dd(a - b)); }

// the plan's fold of a wave's 64 double partials
__device__ __forceinline__ double psis_wave_fold(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The body's and lppd's sums have closed bounds (one exp per term, a sum of non-negative terms in a fixed order) and run in plain
// double: this pass is bound by the table's bytes.
__global__ __launch_bounds__(FG_PSIS_THREADS) void k_psis_collect(const double *ll, unsigned S, unsigned C, long long n_sel, long long k0, long long M,
                                                                   unsigned long long *state, double *tail, double *part) {
    __shared__ double red[FG_PSIS_WAVES][2];
    const long long k = blockIdx.y;
    unsigned long long *st = state + k * FG_PSIS_STATE_WORDS;
    const unsigned long long kc = st[FG_PSIS_ST_PREFIX];
    const double xmin = fg_psis_unkey(st[FG_PSIS_ST_MIN]), xmax = fg_psis_unkey(st[FG_PSIS_ST_MAX]);
    double *tl = tail + k * M;
    double sd = 0.0, sl = 0.0;
    const unsigned long long stride = (unsigned long long)gridDim.x * FG_PSIS_THREADS;
    for (unsigned long long i = (unsigned long long)blockIdx.x * FG_PSIS_THREADS + threadIdx.x; i < S; i += stride) {
        const double x = psis_cell(ll, (unsigned)i, C, n_sel, k0 + k);
        const unsigned long long key = fg_psis_key(x);
        if (key < kc) {
            const unsigned long long pos = atomicAdd(&st[FG_PSIS_ST_CURSOR], 1ull);
            if (pos < (unsigned long long)M) tl[pos] = x;               // a cursor past M is the host's integrity error, never a write
        }
        sd += key > kc ? exp(xmin - x) : 0.0;
        sl += exp(x - xmax);
    }
    sd = psis_wave_fold(sd); sl = psis_wave_fold(sl);
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = sd; red[threadIdx.x >> 6][1] = sl; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double td = 0.0, tll = 0.0;
        for (int v = 0; v < FG_PSIS_WAVES; ++v) { td += red[v][0]; tll += red[v][1]; }
        part[(k * gridDim.x + blockIdx.x) * 2 + 0] = td;
        part[(k * gridDim.x + blockIdx.x) * 2 + 1] = tll;
    }
}

__device__ __forceinline__ void psis_ce(unsigned long long &a, unsigned long long &b, bool up) {
    if ((a > b) == up) { const unsigned long long t = a; a = b; b = t; }
}
// the steps j = j0, j0 / 2, ..., 1 of stage k on the chunk [c0, c0 + CH) of g, in LDS (j0 < CH)
__device__ void psis_sort_chunk(unsigned long long *g, unsigned long long *sk, long long c0, int CH, long long k_first, long long k_last, bool whole) {
    for (int i = threadIdx.x; i < CH; i += FG_PSIS_FIT_THREADS) sk[i] = g[c0 + i];
    __syncthreads();
    for (long long k = k_first; k <= k_last; k <<= 1)
        for (int j = whole ? (int)(k >> 1) : CH >> 1; j > 0; j >>= 1) {
            for (int p = threadIdx.x; p < CH / 2; p += FG_PSIS_FIT_THREADS) {
                const int i = 2 * p - (p & (j - 1)), l = i + j;
                const bool up = ((c0 + i) & k) == 0;
                unsigned long long a = sk[i], b = sk[l];
                psis_ce(a, b, up);
                sk[i] = a; sk[l] = b;
            }
            __syncthreads();
        }
    for (int i = threadIdx.x; i < CH; i += FG_PSIS_FIT_THREADS) g[c0 + i] = sk[i];
    __threadfence_block();
    __syncthreads();
}
// ascending bitonic sort of g [P], P a power of two >= 2, by one workgroup
__device__ void psis_sort(unsigned long long *g, unsigned long long *sk, long long P) {
    const int CH = P < FG_PSIS_SORT_CHUNK ? (int)P : FG_PSIS_SORT_CHUNK;
    for (long long c0 = 0; c0 < P; c0 += CH) psis_sort_chunk(g, sk, c0, CH, 2, CH, true);
    for (long long k = 2ll * CH; k <= P; k <<= 1) {
        for (long long j = k >> 1; j >= CH; j >>= 1) {
            for (long long p = threadIdx.x; p < P / 2; p += FG_PSIS_FIT_THREADS) {
                const long long i = 2 * p - (p & (j - 1)), l = i + j;
                unsigned long long a = g[i], b = g[l];
                psis_ce(a, b, (i & k) == 0);
                g[i] = a; g[l] = b;
            }
            __threadfence_block();
            __syncthreads();
        }
        for (long long c0 = 0; c0 < P; c0 += CH) psis_sort_chunk(g, sk, c0, CH, k, k, false);
    }
}

// the plan's sum of one term per tail value by the calling wave: f(j) for j = lane, lane + 64, ...
template <typename F>
__device__ __forceinline__ FgDD psis_tail_sum(long long M, F f) {
    FgDD s = fg_dd(0.0);
    for (long long j = threadIdx.x & 63; j < M; j += 64) s = fg_dd_add(s, f(j));
    return psis_dd_wave_fold(s);
}
__device__ __forceinline__ FgDD psis_dd_load(const double *hi, const double *lo, long long j) { FgDD r; r.hi = hi[j]; r.lo = lo[j]; return r; }
// log1p(-theta t)
__device__ __forceinline__ FgDD psis_profile_term(FgDD theta, FgDD t) { return psis_dd_log(fg_dd_add_d(fg_dd_neg(fg_dd_mul(theta, t)), 1.0)); }

struct FgPsisFitArgs {
    long long S, M, P, tstar; int G; unsigned nb, nbp; double threshold;
    unsigned long long *state; unsigned int *cls; double *part, *tail, *t; unsigned long long *sort; double *fig; long long *cnt;
};

__global__ __launch_bounds__(FG_PSIS_FIT_THREADS) void k_psis_fit(FgPsisFitArgs A) {
    __shared__ unsigned long long sk[FG_PSIS_SORT_CHUNK];
    __shared__ double th_hi[FG_PSIS_G_MAX], th_lo[FG_PSIS_G_MAX], lj_hi[FG_PSIS_G_MAX], lj_lo[FG_PSIS_G_MAX];
    __shared__ double pd[FG_PSIS_MAX_BLOCKS], pl[FG_PSIS_MAX_BLOCKS];
    __shared__ double sc[8];
    const long long k = blockIdx.x, M = A.M, S = A.S;
    const int tid = threadIdx.x, wave = tid >> 6;
    const unsigned long long *st = A.state + k * FG_PSIS_STATE_WORDS;
    const unsigned long long kc = st[FG_PSIS_ST_PREFIX];
    const long long below = (long long)st[FG_PSIS_ST_BELOW], equal = (long long)st[FG_PSIS_ST_EQUAL], cursor = (long long)st[FG_PSIS_ST_CURSOR];
    const long long n_ninf = A.cls[k * FG_PSIS_CLASS_WORDS + 0], n_pinf = A.cls[k * FG_PSIS_CLASS_WORDS + 1], n_nan = A.cls[k * FG_PSIS_CLASS_WORDS + 2];
    const double xmin = fg_psis_unkey(st[FG_PSIS_ST_MIN]), xmax = fg_psis_unkey(st[FG_PSIS_ST_MAX]), xc = fg_psis_unkey(kc);
    const long long L = below < M ? below : M;
    unsigned long long *g = A.sort + k * A.P;
    double *tl = A.tail + k * M, *t_hi = A.t + k * 2 * M, *t_lo = t_hi + M;

    // the block partials of the two sums over the cells, through the plan's tree (plain double, as the collect pass)
    for (int i = tid; i < (int)A.nbp; i += FG_PSIS_FIT_THREADS) {
        pd[i] = i < (int)A.nb ? A.part[(k * A.nb + i) * 2 + 0] : 0.0;
        pl[i] = i < (int)A.nb ? A.part[(k * A.nb + i) * 2 + 1] : 0.0;
    }
    __syncthreads();
    for (int h = (int)A.nbp >> 1; h > 0; h >>= 1) {
        if (tid < h) { pd[tid] += pd[tid + h]; pl[tid] += pl[tid + h]; }
        __syncthreads();
    }

    // the tail's keys: the collected cells, the cutoff's copies by count, the padding above every key
    for (long long j = tid; j < A.P; j += FG_PSIS_FIT_THREADS) g[j] = j < L ? fg_psis_key(tl[j]) : (j < M ? kc : ~0ull);
    __threadfence_block();
    __syncthreads();
    psis_sort(g, sk, A.P);
    const FgDD ecut = psis_dd_exp_diff(xmin, xc);
    for (long long j = tid; j < M; j += FG_PSIS_FIT_THREADS) {
        tl[j] = fg_psis_unkey(g[j]);                                           // the sorted raw tail, ascending
        const FgDD tj = fg_dd_sub(psis_dd_exp_diff(xmin, fg_psis_unkey(g[M - 1 - j])), ecut);     // ascending ratio
        t_hi[j] = tj.hi; t_lo[j] = tj.lo;
    }
    __threadfence_block();
    __syncthreads();

    int status = FG_PSIS_FITTED;
    if (n_nan > 0 || n_ninf > 0 || xc == INFINITY) status = FG_PSIS_NONFINITE;
    else if (M < FG_PSIS_MIN_TAIL) status = FG_PSIS_TOO_FEW;
    const FgDD tstar = psis_dd_load(t_hi, t_lo, A.tstar > 0 ? A.tstar - 1 : 0);
    if (status == FG_PSIS_FITTED && !fg_dd_gt(tstar, fg_dd(0.0))) status = FG_PSIS_DEGENERATE;

    FgDD khat = fg_dd(INFINITY), sigma = fg_dd(NAN), theta = fg_dd(NAN);
    const FgDD dM = fg_dd((double)M);
    if (status == FG_PSIS_FITTED) {
        const int G = A.G;
        const FgDD inv_tM = fg_dd_div(fg_dd(1.0), psis_dd_load(t_hi, t_lo, M - 1)), ts3 = fg_dd_mul_d(tstar, 3.0);
        for (int j = tid; j < G; j += FG_PSIS_FIT_THREADS) {
            const FgDD r = fg_dd_sqrt(fg_dd_div(fg_dd((double)G), fg_dd((double)(j + 1) - 0.5)));
            const FgDD v = fg_dd_add(inv_tM, fg_dd_div(fg_dd_add_d(fg_dd_neg(r), 1.0), ts3));
            th_hi[j] = v.hi; th_lo[j] = v.lo;
        }
        __syncthreads();
        for (int j = wave; j < G; j += FG_PSIS_FIT_WAVES) {
            const FgDD thj = psis_dd_load(th_hi, th_lo, j);
            const FgDD kj = fg_dd_div(psis_tail_sum(M, [&](long long i) { return psis_profile_term(thj, psis_dd_load(t_hi, t_lo, i)); }), dM);
            if ((tid & 63) == 0) {
                const FgDD l = fg_dd_mul(dM, fg_dd_add_d(fg_dd_sub(psis_dd_log(fg_dd_div(fg_dd_neg(thj), kj)), kj), -1.0));
                lj_hi[j] = l.hi; lj_lo[j] = l.lo;
            }
        }
        __syncthreads();
        if (tid == 0) {
            FgDD lmax = psis_dd_load(lj_hi, lj_lo, 0);
            for (int j = 1; j < G; ++j) { const FgDD l = psis_dd_load(lj_hi, lj_lo, j); if (fg_dd_gt(l, lmax)) lmax = l; }
            FgDD Z = fg_dd(0.0), num = fg_dd(0.0);
            for (int j = 0; j < G; ++j) {
                const FgDD ej = psis_dd_exp(fg_dd_sub(psis_dd_load(lj_hi, lj_lo, j), lmax));
                Z = fg_dd_add(Z, ej);
                num = fg_dd_add(num, fg_dd_mul(psis_dd_load(th_hi, th_lo, j), ej));
            }
            const FgDD v = fg_dd_div(num, Z);
            sc[0] = v.hi; sc[1] = v.lo;
        }
        __syncthreads();
        theta.hi = sc[0]; theta.lo = sc[1];
        if (wave == 0) {
            const FgDD thh = theta;
            const FgDD kraw = fg_dd_div(psis_tail_sum(M, [&](long long i) { return psis_profile_term(thh, psis_dd_load(t_hi, t_lo, i)); }), dM);
            if (tid == 0) {
                const FgDD sg = fg_dd_div(fg_dd_neg(kraw), thh), kh = fg_dd_div(fg_dd_add_d(fg_dd_mul(kraw, dM), 5.0), fg_dd_add_d(dM, 10.0));
                sc[2] = sg.hi; sc[3] = sg.lo; sc[4] = kh.hi; sc[5] = kh.lo;
            }
        }
        __syncthreads();
        sigma.hi = sc[2]; sigma.lo = sc[3]; khat.hi = sc[4]; khat.lo = sc[5];
    }
    __syncthreads();
    // the tail's two sums: smoothed when khat is finite, raw otherwise
    const bool smooth = status == FG_PSIS_FITTED && fg_dd_finite(khat.hi);
    if (wave == 0) {
        int capped = 0;
        FgDD sa = fg_dd(0.0), sb = fg_dd(0.0);
        for (long long j = tid; j < M; j += 64) {
            const FgDD lw = fg_dd(xmin - fg_psis_unkey(g[M - 1 - j]));
            FgDD lwt = lw;
            if (smooth) {
                const FgDD p = fg_dd_div(fg_dd((double)(j + 1) - 0.5), dM);
                const FgDD l1 = psis_dd_log(fg_dd_add_d(fg_dd_neg(p), 1.0));
                const FgDD q = fg_dd_div(fg_dd_mul(sigma, psis_dd_expm1(fg_dd_neg(fg_dd_mul(khat, l1)))), khat);
                const FgDD v = psis_dd_log(fg_dd_add(q, ecut));
                const bool cap = fg_dd_gt(v, fg_dd(0.0));
                capped += cap ? 1 : 0;
                lwt = cap ? fg_dd(0.0) : v;
            }
            sa = fg_dd_add(sa, psis_dd_exp(fg_dd_sub(lwt, lw)));
            sb = fg_dd_add(sb, psis_dd_exp(lwt));
        }
        sa = psis_dd_wave_fold(sa); sb = psis_dd_wave_fold(sb);
        for (int o = 32; o > 0; o >>= 1) capped += __shfl_xor(capped, o, 64);
        if (tid == 0) {
            const long long ties = equal - (M - L);                            // the cutoff's copies that stay in the body
            FgDD body = fg_dd(pd[0]);
            if (ties > 0) body = fg_dd_add(body, fg_dd_mul_d(ecut, (double)ties));
            const FgDD num = psis_dd_log(fg_dd_add_d(sa, (double)(S - M))), den = psis_dd_log(fg_dd_add(body, sb));
            FgDD elpd = fg_dd_add_d(fg_dd_sub(num, den), xmin);
            FgDD lppd = fg_dd_add_d(fg_dd_sub(psis_dd_log(fg_dd(pl[0])), psis_dd_log(fg_dd((double)S))), xmax);
            if (n_pinf > 0) lppd = fg_dd(INFINITY);
            else if (n_ninf == S) lppd = fg_dd(-INFINITY);
            if (n_ninf > 0) elpd = fg_dd(-INFINITY);
            else if (n_pinf == S) elpd = fg_dd(INFINITY);
            double *f = A.fig + k * FG_PSIS_WORDS;                             // every word rounded once
            f[0] = fg_dd_round(elpd); f[1] = fg_dd_round(fg_dd_sub(lppd, elpd)); f[2] = fg_dd_round(khat); f[3] = fg_dd_round(sigma); f[4] = A.threshold;
            f[5] = fg_dd_round(lppd); f[6] = xmin; f[7] = xc; f[8] = fg_dd_round(ecut); f[9] = fg_dd_round(tstar); f[10] = fg_dd_round(theta);
            f[11] = fg_dd_round(body); f[12] = fg_dd_round(sb); f[13] = fg_dd_round(sa);
            if (n_nan > 0)
                for (int i = 0; i < FG_PSIS_WORDS; ++i) if (i != 4) f[i] = NAN;
            long long *c = A.cnt + k * FG_PSIS_COUNTS;
            c[0] = M; c[1] = status; c[2] = capped; c[3] = S - n_ninf - n_pinf - n_nan; c[4] = n_ninf; c[5] = n_pinf; c[6] = n_nan;
            c[7] = below; c[8] = equal; c[9] = cursor;
        }
    }
}

namespace {

struct PsisScope {                             // device buffers of one call
    std::vector<void *> p;
    ~PsisScope() { for (void *q : p) (void)hipFree(q); }
    template <typename T>
    int alloc(T **out, size_t bytes, const char *what) {
        if (hipMalloc((void **)out, bytes ? bytes : 1) != hipSuccess) { fg_set_error(std::string("fg_psis_loo: no device memory for ") + what); return FG_E_HIP; }
        p.push_back(*out);
        return FG_OK;
    }
};

}  // namespace

extern "C" {

int fg_psis_words(void) { return FG_PSIS_WORDS; }

int64_t fg_psis_tail_len(int64_t S) { return (int64_t)fg_psis_tail(S); }

int fg_psis_loo(fg_engine *e, const double *d_ll, int n, int n_sel, double *h_figures, int64_t *h_counts, double *d_tail_or_null) {
    if (!e) { fg_set_error("fg_psis_loo: null engine"); return FG_E_BAD_ARG; }
    if (!d_ll || !h_figures || !h_counts) { fg_set_error("fg_psis_loo: null d_ll, h_figures or h_counts"); return FG_E_BAD_ARG; }
    if (n < 1 || n_sel < 1) { fg_set_error("fg_psis_loo: n and n_sel must be at least 1"); return FG_E_BAD_ARG; }
    FgPsisPlan P;
    if (int rc = fg_psis_plan(n, e->C, n_sel, &P)) {
        fg_set_error(rc == FG_E_LIMIT ? "fg_psis_loo: n x chains = " + std::to_string((long long)n * e->C) + " pooled draws: the limit is 2^31 - 1"
                                      : std::string("fg_psis_loo: n, n_sel and the engine's chains must be at least 1"));
        return rc;
    }
    if (hipSetDevice(e->device) != hipSuccess) { fg_set_error("hipSetDevice failed"); return FG_E_HIP; }
    PsisScope sc;
    unsigned long long *d_state = nullptr, *d_sort = nullptr;
    unsigned int *d_cls = nullptr, *d_hist = nullptr;
    double *d_part = nullptr, *d_tail = nullptr, *d_t = nullptr, *d_fig = nullptr;
    long long *d_cnt = nullptr;
    if (sc.alloc(&d_state, P.b_state, "the select's state") || sc.alloc(&d_cls, P.b_class, "the cell counters") || sc.alloc(&d_hist, P.b_hist, "the histograms") ||
        sc.alloc(&d_part, P.b_part, "the block partials") || sc.alloc(&d_tail, P.b_tail, "the tails") || sc.alloc(&d_sort, P.b_sort, "the sort buffer") ||
        sc.alloc(&d_t, P.b_t, "the tail's exceedances") || sc.alloc(&d_fig, P.b_fig, "the figures") || sc.alloc(&d_cnt, P.b_cnt, "the counts"))
        return FG_E_HIP;
    const unsigned S = (unsigned)P.S, C = (unsigned)e->C;
    std::vector<unsigned long long> init;
    std::vector<long long> cnt;
    for (long long k0 = 0; k0 < n_sel; k0 += P.rows_per) {
        const long long rows = std::min<long long>(P.rows_per, n_sel - k0);
        init.assign((size_t)rows * FG_PSIS_STATE_WORDS, 0ull);
        for (long long k = 0; k < rows; ++k) { init[(size_t)k * FG_PSIS_STATE_WORDS + FG_PSIS_ST_RANK] = (unsigned long long)P.rank; init[(size_t)k * FG_PSIS_STATE_WORDS + FG_PSIS_ST_MIN] = ~0ull; }
        HIPCHK(hipMemcpyAsync(d_state, init.data(), init.size() * 8, hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemsetAsync(d_cls, 0, (size_t)rows * FG_PSIS_CLASS_WORDS * 4, e->stream));
        HIPCHK(hipMemsetAsync(d_hist, 0, (size_t)rows * FG_PSIS_BINS * 4, e->stream));
        const dim3 grid(P.nb, (unsigned)rows), block(FG_PSIS_THREADS);
        for (int p = 0; p < P.passes; ++p) {
            const int b = p * FG_PSIS_DIGIT_BITS, w = fg_psis_pass_width(p);
            hipLaunchKernelGGL(k_psis_hist, grid, block, 0, e->stream, d_ll, S, C, (long long)n_sel, k0, b, w, p == 0 ? 1 : 0, d_state, d_cls, d_hist);
            HIPCHK(hipGetLastError());
            hipLaunchKernelGGL(k_psis_pick, dim3((unsigned)rows), block, 0, e->stream, d_state, d_hist, b, w);
            HIPCHK(hipGetLastError());
        }
        hipLaunchKernelGGL(k_psis_collect, grid, block, 0, e->stream, d_ll, S, C, (long long)n_sel, k0, (long long)P.M, d_state, d_tail, d_part);
        HIPCHK(hipGetLastError());
        FgPsisFitArgs A;
        A.S = P.S; A.M = P.M; A.P = P.P; A.tstar = P.tstar; A.G = P.G; A.nb = P.nb; A.nbp = P.nbp; A.threshold = fg_psis_threshold(P.S);
        A.state = d_state; A.cls = d_cls; A.part = d_part; A.tail = d_tail; A.t = d_t; A.sort = d_sort; A.fig = d_fig; A.cnt = d_cnt;
        hipLaunchKernelGGL(k_psis_fit, dim3((unsigned)rows), dim3(FG_PSIS_FIT_THREADS), 0, e->stream, A);
        HIPCHK(hipGetLastError());
        cnt.resize((size_t)rows * FG_PSIS_COUNTS);
        HIPCHK(hipMemcpyAsync(h_figures + (size_t)k0 * FG_PSIS_WORDS, d_fig, (size_t)rows * FG_PSIS_WORDS * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt, cnt.size() * 8, hipMemcpyDeviceToHost, e->stream));
        if (d_tail_or_null) HIPCHK(hipMemcpyAsync(d_tail_or_null + (size_t)k0 * (size_t)P.M, d_tail, (size_t)rows * (size_t)P.M * 8, hipMemcpyDeviceToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        for (long long k = 0; k < rows; ++k) {
            const long long *c = &cnt[(size_t)k * FG_PSIS_COUNTS];
            if (c[9] != c[7] || c[7] > P.M || (P.S > P.M && c[7] + c[8] < P.M)) {
                fg_set_error("fg_psis_loo: statement " + std::to_string(k0 + k) + " collected " + std::to_string(c[9]) + " cells where the select counted " + std::to_string(c[7]) +
                             " below the cutoff and " + std::to_string(c[8]) + " on it, for a tail of " + std::to_string(P.M));
                return FG_E_STATE;
            }
            for (int j = 0; j < FG_PSIS_COUNTS; ++j) h_counts[(size_t)(k0 + k) * FG_PSIS_COUNTS + j] = (int64_t)c[j];
        }
    }
    return FG_OK;
}

}  // extern "C"
