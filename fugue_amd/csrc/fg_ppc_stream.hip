// fg_ppc_stream.hip -- posterior predictive checks from the replicate table fg_predict_eval writes, d_yrep [n][n_rows][C] raw cells,
// handed over one chunk at a time and never stored (the last step of the reference's workflows,
// tests/end_to_end_workflows.rs:650-745, examples/bayesian_coin_flip.rs:211-).  The statistics of a data set, the words a (slot,
// chain) column keeps, their update, the pair merge of the pooling tree and the launch cuts are fg_ppc_stream_plan.h's; this file
// launches them.
//
// Two passes per piece of at most FG_PPC_SCRATCH_DRAWS draws, in stream order:
// k_ppc_stream_stats: one thread per (draw, check, chain), c fastest, so a member row is one coalesced 512 B load per wave and the
//   draws of a piece are in flight together; the check's members come from the CSR list through wave-uniform (scalar) loads; the
//   variance pass reads the K cells again (from cache); the statistics asked for go to the scratch table [draw][slot][C].
// k_ppc_stream_update: one thread per (slot, chain); the six state words live in registers for the launch and the piece's draws
//   are walked in order (k_loglik_stream_update's shape).  No atomics: a column has one writer.  A lane beyond C stores nothing.
// k_chain_pool<FgPpcPool, .> (fg_chain_pool.h): one block row per slot, one level of the fixed tree on the chain index per launch.
#include "fg_engine_internal.h"
#include "fg_ppc_stream_plan.h"

struct fg_ppc_stream {
    fg_engine *e = nullptr;
    FgPpcPlan P;
    int32_t *csr = nullptr;          // offsets [n_checks + 1], mask [n_checks], slot0 [n_checks], members [offsets[n_checks]]
    double *t_obs = nullptr;         // [n_slots]
    double *scratch = nullptr;       // [scratch_draws][n_slots][C]
    double *state = nullptr;         // [FG_PPC_WORDS][n_slots][C]
    double *tree[2] = { nullptr, nullptr };       // [n_slots][m][FG_PPC_ELEM], the levels alternate
};

// Pair p0 + blockIdx.y = (draw t of the piece, check q); chain c0 + the thread's index along x.  cells: the piece's first draw.
__global__ __launch_bounds__(FG_PPC_THREADS) void k_ppc_stream_stats(const unsigned long long *__restrict__ cells, long long n_rows, long long C, long long c0,
                                                                     long long cols, long long p0, int n_checks, int n_slots,
                                                                     const int32_t *__restrict__ csr, double *__restrict__ scratch) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cols) return;
    const long long c = c0 + j, p = p0 + blockIdx.y, t = p / n_checks;
    const int q = (int)(p - t * n_checks);
    const int o0 = csr[q], K = csr[q + 1] - o0, mask = csr[n_checks + 1 + q], slot = csr[2 * n_checks + 1 + q];
    const int32_t *members = csr + 3 * n_checks + 1 + o0;
    const unsigned long long *base = cells + t * n_rows * C + c;
    double T[FG_PPC_N_STATS];
    fg_ppc_stats(K, [&](int i) { const int m = members[i]; return fg_ppc_cell(base[(long long)(m >> 2) * C], m & 3); }, (mask >> FG_PPC_VAR) & 1, T);
    double *out = scratch + (t * n_slots + slot) * C + c;
#pragma unroll
    for (int st = 0; st < FG_PPC_N_STATS; ++st)
        if ((mask >> st) & 1) { *out = T[st]; out += C; }
}

// Slot k0 + blockIdx.y, chain c0 + the thread's index along x; n_c draws of the scratch table in order.
__global__ __launch_bounds__(FG_PPC_THREADS) void k_ppc_stream_update(const double *__restrict__ scratch, int n_c, long long C, long long c0, long long cols,
                                                                      long long k0, long long n_slots, const double *__restrict__ t_obs, double *state) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= cols) return;
    const long long k = k0 + blockIdx.y, col = k * C + c0 + j, stride = n_slots * C;
    const double obs = t_obs[k];
    FgPpcState s;
    fg_ppc_state_load(s, state + col, stride);
    const double *x = scratch + col;
#pragma unroll 4
    for (int t = 0; t < n_c; ++t) fg_ppc_update(s, x[(long long)t * stride], obs);
    fg_ppc_state_store(s, state + col, stride);
}

extern "C" {

int fg_ppc_stream_new(fg_engine *e, int n_total, int n_rows, const int32_t *h_vtypes, int n_checks, const int32_t *h_offsets, const int32_t *h_members,
                      const int32_t *h_stat_mask, const double *h_observed, fg_ppc_stream **out) {
    NEED_ENGINE(e);
    if (!out) return FG_E_BAD_ARG;
    *out = nullptr;
    fg_ppc_stream *s = new fg_ppc_stream;
    std::string err;
    int rc = fg_ppc_init(s->P, n_total, e->C, n_rows, h_vtypes, n_checks, h_offsets, h_members, h_stat_mask, h_observed, &err);
    if (rc) { fg_set_error(err); delete s; return rc; }
    s->e = e;
    const FgPpcPlan &P = s->P;
    std::vector<int32_t> csr(P.offsets);
    csr.insert(csr.end(), P.mask.begin(), P.mask.end());
    csr.insert(csr.end(), P.slot0.begin(), P.slot0.end());
    csr.insert(csr.end(), P.members.begin(), P.members.end());
    const size_t tree_words = (size_t)P.n_slots * (size_t)fg_ppc_tree_elems(P) * FG_PPC_ELEM;
    rc = dev_alloc(&s->state, fg_ppc_state_words(P));                    // zeroed: nothing seen
    if (!rc) rc = dev_alloc(&s->scratch, fg_ppc_scratch_words(P));
    if (!rc) rc = dev_alloc(&s->tree[0], tree_words);
    if (!rc) rc = dev_alloc(&s->tree[1], tree_words);
    if (!rc) rc = dev_alloc(&s->csr, csr.size());
    if (!rc) rc = dev_alloc(&s->t_obs, P.t_obs.size());
    if (!rc && hipMemcpy(s->csr, csr.data(), csr.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) { fg_set_error("fg_ppc_stream_new: the check list did not upload"); rc = FG_E_HIP; }
    if (!rc && hipMemcpy(s->t_obs, P.t_obs.data(), P.t_obs.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) { fg_set_error("fg_ppc_stream_new: the observed statistics did not upload"); rc = FG_E_HIP; }
    if (rc) { fg_ppc_stream_free(s); return rc; }
    *out = s;
    return FG_OK;
}

int fg_ppc_stream_update(fg_ppc_stream *s, const void *d_yrep, int n_chunk) {
    int rc = fg_need_stream(s);
    if (rc) return rc;
    std::string err;
    rc = s->P.draws.take(n_chunk, "fg_ppc_stream_update", &err);
    if (rc) { fg_set_error(err); return rc; }
    if (n_chunk == 0) return FG_OK;
    if (!d_yrep) { s->P.draws.untake(n_chunk); fg_set_error("fg_ppc_stream_update: null table"); return FG_E_BAD_ARG; }
    const FgPpcPlan &P = s->P;
    bool launched = false;
    for (int t0 = 0; t0 < n_chunk; t0 += P.scratch_draws) {
        const int n_piece = std::min(P.scratch_draws, n_chunk - t0);
        const unsigned long long *cells = (const unsigned long long *)d_yrep + (size_t)t0 * (size_t)P.n_rows * (size_t)P.C;
        const std::vector<FgPoolSlice> pairs = fg_ppc_pair_slices(P, n_piece);
        for (int pass = 0; pass < 2; ++pass)
            for (const FgPoolLaunch &L : P.launches) {
                const unsigned nb = (unsigned)((L.cols + FG_PPC_THREADS - 1) / FG_PPC_THREADS);
                for (const FgPoolSlice &S : pass == 0 ? pairs : P.slices) {
                    const dim3 grid(nb, (unsigned)S.nk), block(FG_PPC_THREADS);
                    if (pass == 0) hipLaunchKernelGGL(k_ppc_stream_stats, grid, block, 0, s->e->stream, cells, (long long)P.n_rows, P.C, L.col0, L.cols, S.k0, P.n_checks, P.n_slots, s->csr, s->scratch);
                    else hipLaunchKernelGGL(k_ppc_stream_update, grid, block, 0, s->e->stream, s->scratch, n_piece, P.C, L.col0, L.cols, S.k0, (long long)P.n_slots, s->t_obs, s->state);
                    if (hipGetLastError() != hipSuccess) {
                        if (!launched) s->P.draws.untake(n_chunk);                  // nothing ran: the draws go back
                        fg_set_error("fg_ppc_stream_update: a kernel did not launch");
                        return FG_E_HIP;
                    }
                    launched = true;
                }
            }
    }
    return FG_OK;
}

int fg_ppc_stream_count(const fg_ppc_stream *s) { return s ? s->P.draws.count : 0; }
int fg_ppc_stream_n_slots(const fg_ppc_stream *s) { return s ? s->P.n_slots : 0; }

int fg_ppc_stream_observed(const fg_ppc_stream *s, double *h_t_obs) {
    if (!s || !h_t_obs) { fg_set_error("fg_ppc_stream_observed: null stream or output"); return FG_E_BAD_ARG; }
    std::memcpy(h_t_obs, s->P.t_obs.data(), s->P.t_obs.size() * sizeof(double));
    return FG_OK;
}

int fg_ppc_stream_pooled(fg_ppc_stream *s, int64_t *h_counts, double *h_moments) {
    if (!h_counts || !h_moments) { fg_set_error("fg_ppc_stream_pooled: null output"); return FG_E_BAD_ARG; }
    int rc = fg_stream_ready(s, "fg_ppc_stream_pooled");
    if (rc) return rc;
    const FgPpcPlan &P = s->P;
    std::vector<double> h;
    rc = fg_chain_pool_run<FgPpcPool>(s->e->stream, P.levels, P.slices, s->state, (long long)P.n_slots * P.C, s->tree, h);
    if (rc) return rc;
    for (int k = 0; k < P.n_slots; ++k) fg_ppc_finish(FgPpcPool::elem_load(&h[(size_t)k * FG_PPC_ELEM]), h_counts + 5 * (size_t)k, h_moments + 2 * (size_t)k);
    return FG_OK;
}

int fg_ppc_stream_chains(fg_ppc_stream *s, int slot, int64_t *h_counts) {
    if (!h_counts) { fg_set_error("fg_ppc_stream_chains: null output"); return FG_E_BAD_ARG; }
    const int rc = fg_stream_ready(s, "fg_ppc_stream_chains");
    if (rc) return rc;
    const FgPpcPlan &P = s->P;
    if (slot < 0 || slot >= P.n_slots) { fg_set_error("fg_ppc_stream_chains: slot " + std::to_string(slot) + " lies outside [0, " + std::to_string(P.n_slots) + ")"); return FG_E_BAD_ARG; }
    const size_t C = (size_t)P.C;
    std::vector<uint64_t> w(3 * C);
    for (int i = 0; i < 3; ++i)
        HIPCHK(hipMemcpyAsync(w.data() + (size_t)i * C, s->state + ((size_t)i * (size_t)P.n_slots + (size_t)slot) * C, C * 8, hipMemcpyDeviceToHost, s->e->stream));
    HIPCHK(hipStreamSynchronize(s->e->stream));
    for (size_t c = 0; c < C; ++c) {
        h_counts[c] = (int64_t)(uint32_t)w[c]; h_counts[C + c] = (int64_t)(w[c] >> 32);
        h_counts[2 * C + c] = (int64_t)(uint32_t)w[C + c]; h_counts[3 * C + c] = (int64_t)(w[C + c] >> 32);
        h_counts[4 * C + c] = (int64_t)w[2 * C + c];
    }
    return FG_OK;
}

void fg_ppc_stream_free(fg_ppc_stream *s) {
    if (!s) return;
    if (s->e && hipSetDevice(s->e->device) == hipSuccess) {
        for (double *p : { s->state, s->scratch, s->t_obs, s->tree[0], s->tree[1] }) if (p) (void)hipFree(p);
        if (s->csr) (void)hipFree(s->csr);
    }
    delete s;
}

}  // extern "C"
