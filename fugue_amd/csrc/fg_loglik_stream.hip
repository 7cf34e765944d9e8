// fg_loglik_stream.hip -- WAIC and importance-sampling LOO from the table fg_predict_eval writes, d_loglik [n][n_sel][C], handed
// over one chunk at a time and never stored (the reference has neither figure).  The words a column keeps, their
// update, the pair merge of the pooling tree and the final figures are fg_loglik_stream_plan.h's; this file launches them.
//
// k_loglik_stream_update: one thread per column (k, c), c fastest, so a draw's row is one coalesced 512 B load per wave; the ten
// state words live in registers for the launch and the chunk's draws are walked in order (k_diag_stream_update's shape).  No
// atomics: a column has one writer.  Two exp and about a dozen f64 operations per 8-byte cell: bound by the f64 VALU rate.
// k_chain_pool<FgLlPool, .> (fg_chain_pool.h): one block row per statement, one level of the fixed tree on the chain index per launch.
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

// the tree of the plan, level by level; the pooled elements [n_sel][FG_LL_ELEM] on the host
static int pooled_elems(fg_loglik_stream *s, const char *who, std::vector<double> &h) {
    const int rc = fg_stream_ready(s, who);
    return rc ? rc : fg_chain_pool_run<FgLlPool>(s->e->stream, s->P.levels, s->P.slices, s->state, (long long)s->P.n_sel * s->P.C, s->tree, h);
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
    int rc = fg_need_stream(s);
    if (rc) return rc;
    std::string err;
    rc = s->P.draws.take(n_chunk, "fg_loglik_stream_update", &err);
    if (rc) { fg_set_error(err); return rc; }
    if (n_chunk == 0) return FG_OK;
    if (!d_loglik) { s->P.draws.untake(n_chunk); fg_set_error("fg_loglik_stream_update: null table"); return FG_E_BAD_ARG; }
    const FgLlPlan &P = s->P;
    for (const FgPoolLaunch &L : P.launches) {
        const unsigned nb = (unsigned)((L.cols + FG_LL_UPDATE_THREADS - 1) / FG_LL_UPDATE_THREADS);
        hipLaunchKernelGGL(k_loglik_stream_update, dim3(nb), dim3(FG_LL_UPDATE_THREADS), 0, s->e->stream, d_loglik, n_chunk, L.col0, L.cols, (long long)P.n_sel * P.C,
                           s->state);
        if (hipGetLastError() != hipSuccess) {
            if (&L == &P.launches.front()) s->P.draws.untake(n_chunk);
            fg_set_error("fg_loglik_stream_update: the kernel did not launch");
            return FG_E_HIP;
        }
    }
    return FG_OK;
}

int fg_loglik_stream_count(const fg_loglik_stream *s) { return s ? s->P.draws.count : 0; }

int fg_loglik_stream_pooled(fg_loglik_stream *s, double *h_words, int64_t *h_counts) {
    if (!h_words || !h_counts) { fg_set_error("fg_loglik_stream_pooled: null output"); return FG_E_BAD_ARG; }
    std::vector<double> h;
    const int rc = pooled_elems(s, "fg_loglik_stream_pooled", h);
    if (rc) return rc;
    for (int k = 0; k < s->P.n_sel; ++k) {
        const FgLlElem el = FgLlPool::elem_load(&h[(size_t)k * FG_LL_ELEM]);
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
    const double N = (double)s->P.draws.n_total * (double)s->P.C;
    for (int k = 0; k < n_sel; ++k) {
        const FgLlElem el = FgLlPool::elem_load(&h[(size_t)k * FG_LL_ELEM]);
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
