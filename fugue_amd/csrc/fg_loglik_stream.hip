// fg_loglik_stream.hip -- WAIC and importance-sampling LOO from the table fg_predict_eval writes, d_loglik [n][n_sel][C], handed
// over one chunk at a time and never stored (the reference has neither figure).  The words a column keeps, their
// update, the pair merge of the pooling tree and the final figures are fg_loglik_stream_plan.h's; this file launches them.
//
// k_loglik_stream_update: one thread per column (k, c), c fastest, so a draw's row is one coalesced 512 B load per wave; the ten
// state words live in registers for the launch and the chunk's draws are walked in order (k_diag_stream_update's shape).  No
// atomics: a column has one writer.  Two exp and about a dozen f64 operations per 8-byte cell: bound by the f64 VALU rate.
// k_loglik_stream_pool: one block row per statement, one level of the fixed tree on the chain index per launch.
#include "fg_engine_internal.h"
#include "fg_loglik_stream_plan.h"

struct fg_loglik_stream {
    fg_engine *e = nullptr;
    FgLlPlan P;
    double *state = nullptr;         // [FG_LL_WORDS][n_sel][C]
    double *tree[2] = { nullptr, nullptr };       // [n_sel][m][FG_LL_ELEM], the levels alternate
};

__global__ __launch_bounds__(FG_LL_UPDATE_THREADS) void k_loglik_stream_update(const double *chunk, int n_c, long long col0, long long cols, long long stride,
                                                                               double *state) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cols) return;
    const long long col = col0 + j;
    FgLlState s;
    fg_ll_state_load(s, state + col, stride);
    const double *x = chunk + col;
#pragma unroll 4
    for (int t = 0; t < n_c; ++t) fg_ll_update(s, x[(long long)t * stride]);
    fg_ll_state_store(s, state + col, stride);
}

__device__ __forceinline__ FgLlElem ll_shfl_down(const FgLlElem &e, int s) {
    FgLlElem r;
    r.mx = __shfl_down(e.mx, s, 64); r.sp = __shfl_down(e.sp, s, 64); r.mn = __shfl_down(e.mn, s, 64); r.sn = __shfl_down(e.sn, s, 64);
    r.sn2 = __shfl_down(e.sn2, s, 64); r.n = __shfl_down(e.n, s, 64); r.mean = __shfl_down(e.mean, s, 64); r.ssd = __shfl_down(e.ssd, s, 64);
    r.n_neg_inf = __shfl_down((long long)e.n_neg_inf, s, 64); r.n_pos_inf = __shfl_down((long long)e.n_pos_inf, s, 64);
    r.n_nan = __shfl_down((long long)e.n_nan, s, 64);
    return r;
}

// One level: element i of statement k0 + blockIdx.y is the state column (LEAF) or in[k][i]; a block pools 256 consecutive elements
// (an index past m_in: the empty element, whose merge is the identity) by strides 1 .. 32 inside each wave, 64 and 128 through LDS,
// and writes out[k][blockIdx.x].  The pairs are those of the stride rule on the chain index, whatever the grid.
template <bool LEAF>
__global__ __launch_bounds__(FG_LL_POOL_THREADS) void k_loglik_stream_pool(const double *in, long long m_in, long long stride, int k0, double *out, long long m_out) {
    __shared__ double sh[FG_LL_POOL_THREADS / 64][FG_LL_ELEM];
    const long long i = (long long)blockIdx.x * FG_LL_POOL_THREADS + threadIdx.x;
    const long long k = (long long)k0 + blockIdx.y;
    FgLlElem e = fg_ll_empty();
    if (i < m_in) {
        if (LEAF) {
            FgLlState s;
            fg_ll_state_load(s, in + k * m_in + i, stride);
            e = fg_ll_leaf(s);
        } else e = fg_ll_elem_load(in + (k * m_in + i) * FG_LL_ELEM);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int s = 1; s < 64; s *= 2) {
        const FgLlElem o = ll_shfl_down(e, s);
        if ((lane & (2 * s - 1)) == 0) e = fg_ll_merge(e, o);
    }
    if (lane == 0) fg_ll_elem_store(e, sh[wave]);
    __syncthreads();
    if (threadIdx.x == 0) {
        const FgLlElem lo = fg_ll_merge(fg_ll_elem_load(sh[0]), fg_ll_elem_load(sh[1]));
        const FgLlElem hi = fg_ll_merge(fg_ll_elem_load(sh[2]), fg_ll_elem_load(sh[3]));
        fg_ll_elem_store(fg_ll_merge(lo, hi), out + (k * m_out + blockIdx.x) * FG_LL_ELEM);
    }
}

static int need_stream(const fg_loglik_stream *s) {
    if (!s || !s->e) { fg_set_error("null stream"); return FG_E_BAD_ARG; }
    if (hipSetDevice(s->e->device) != hipSuccess) { fg_set_error("hipSetDevice failed"); return FG_E_HIP; }
    return FG_OK;
}

// the tree of the plan, level by level; the pooled elements [n_sel][FG_LL_ELEM] on the host
static int pooled_elems(fg_loglik_stream *s, const char *who, std::vector<double> &h) {
    int rc = need_stream(s);
    if (rc) return rc;
    std::string err;
    rc = fg_ll_complete(s->P, who, &err);
    if (rc) { fg_set_error(err); return rc; }
    const FgLlPlan &P = s->P;
    fg_engine *e = s->e;
    const double *in = s->state;
    int side = 0;
    for (size_t l = 0; l < P.levels.size(); ++l) {
        const FgLlLevel &L = P.levels[l];
        for (const FgLlSlice &S : P.slices) {
            const dim3 grid((unsigned)L.m_out, (unsigned)S.nk), block(FG_LL_POOL_THREADS);
            if (l == 0) hipLaunchKernelGGL(k_loglik_stream_pool<true>, grid, block, 0, e->stream, in, L.m_in, (long long)P.n_sel * P.C, S.k0, s->tree[side], L.m_out);
            else hipLaunchKernelGGL(k_loglik_stream_pool<false>, grid, block, 0, e->stream, in, L.m_in, 0ll, S.k0, s->tree[side], L.m_out);
            HIPCHK(hipGetLastError());
        }
        in = s->tree[side];
        side ^= 1;
    }
    h.resize((size_t)P.n_sel * FG_LL_ELEM);
    HIPCHK(hipMemcpyAsync(h.data(), in, h.size() * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    return FG_OK;
}

extern "C" {

int fg_loglik_stream_new(fg_engine *e, int n_total, int n_sel, fg_loglik_stream **out) {
    NEED_ENGINE(e);
    if (!out) return FG_E_BAD_ARG;
    *out = nullptr;
    fg_loglik_stream *s = new fg_loglik_stream;
    std::string err;
    int rc = fg_ll_init(s->P, n_total, e->C, n_sel, &err);
    if (rc) { fg_set_error(err); delete s; return rc; }
    s->e = e;
    const size_t tree_words = (size_t)n_sel * (size_t)fg_ll_scratch_elems(s->P) * FG_LL_ELEM;
    rc = dev_alloc(&s->state, fg_ll_state_words(s->P));                 // zeroed: n_fin = 0, nothing seen
    if (!rc) rc = dev_alloc(&s->tree[0], tree_words);
    if (!rc) rc = dev_alloc(&s->tree[1], tree_words);
    if (rc) { fg_loglik_stream_free(s); return rc; }
    *out = s;
    return FG_OK;
}

int fg_loglik_stream_update(fg_loglik_stream *s, const double *d_loglik, int n_chunk) {
    int rc = need_stream(s);
    if (rc) return rc;
    std::string err;
    rc = fg_ll_take(s->P, n_chunk, &err);
    if (rc) { fg_set_error(err); return rc; }
    if (n_chunk == 0) return FG_OK;
    if (!d_loglik) { fg_ll_untake(s->P, n_chunk); fg_set_error("fg_loglik_stream_update: null table"); return FG_E_BAD_ARG; }
    const FgLlPlan &P = s->P;
    for (const FgLlLaunch &L : P.launches) {
        const unsigned nb = (unsigned)((L.cols + FG_LL_UPDATE_THREADS - 1) / FG_LL_UPDATE_THREADS);
        hipLaunchKernelGGL(k_loglik_stream_update, dim3(nb), dim3(FG_LL_UPDATE_THREADS), 0, s->e->stream, d_loglik, n_chunk, L.col0, L.cols, (long long)P.n_sel * P.C,
                           s->state);
        if (hipGetLastError() != hipSuccess) {
            if (&L == &P.launches.front()) fg_ll_untake(s->P, n_chunk);
            fg_set_error("fg_loglik_stream_update: the kernel did not launch");
            return FG_E_HIP;
        }
    }
    return FG_OK;
}

int fg_loglik_stream_count(const fg_loglik_stream *s) { return s ? s->P.count : 0; }

int fg_loglik_stream_pooled(fg_loglik_stream *s, double *h_words, int64_t *h_counts) {
    if (!h_words || !h_counts) { fg_set_error("fg_loglik_stream_pooled: null output"); return FG_E_BAD_ARG; }
    std::vector<double> h;
    const int rc = pooled_elems(s, "fg_loglik_stream_pooled", h);
    if (rc) return rc;
    for (int k = 0; k < s->P.n_sel; ++k) {
        const FgLlElem el = fg_ll_elem_load(&h[(size_t)k * FG_LL_ELEM]);
        std::memcpy(h_words + (size_t)k * FG_LL_POOLED, &h[(size_t)k * FG_LL_ELEM], FG_LL_POOLED * 8);
        h_counts[3 * k] = el.n_neg_inf; h_counts[3 * k + 1] = el.n_pos_inf; h_counts[3 * k + 2] = el.n_nan;
    }
    return FG_OK;
}

int fg_loglik_stream_result(fg_loglik_stream *s, double *h_figures, int64_t *h_counts) {
    if (!h_figures || !h_counts) { fg_set_error("fg_loglik_stream_result: null output"); return FG_E_BAD_ARG; }
    std::vector<double> h;
    const int rc = pooled_elems(s, "fg_loglik_stream_result", h);
    if (rc) return rc;
    const int n_sel = s->P.n_sel;
    const double N = (double)s->P.n_total * (double)s->P.C;
    for (int k = 0; k < n_sel; ++k) {
        const FgLlElem el = fg_ll_elem_load(&h[(size_t)k * FG_LL_ELEM]);
        double fig[FG_LL_FIGURES];
        fg_ll_finish(el, N, fig);
        for (int f = 0; f < FG_LL_FIGURES; ++f) h_figures[(size_t)f * n_sel + k] = fig[f];
        h_counts[3 * k] = el.n_neg_inf; h_counts[3 * k + 1] = el.n_pos_inf; h_counts[3 * k + 2] = el.n_nan;
    }
    return FG_OK;
}

void fg_loglik_stream_free(fg_loglik_stream *s) {
    if (!s) return;
    if (s->e && hipSetDevice(s->e->device) == hipSuccess)
        for (double *p : { s->state, s->tree[0], s->tree[1] }) if (p) (void)hipFree(p);
    delete s;
}

}  // extern "C"
