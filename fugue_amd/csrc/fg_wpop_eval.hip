// fg_wpop_eval.hip -- predictive checks and WAIC / IS-LOO of a weighted population where it lies: what the reference's
// workflows do after every sampler they have, SMC included (tests/end_to_end_workflows.rs:330-400, :650-745), for the particles
// ABCSMCResult::weighted_mean (abc.rs:476) and the doc example (smc.rs:445-453) walk on the host.  The categories, the staged terms,
// the slices, the integrity rule and the finish step are fg_wpop_eval_plan.h's (plain C++); here are the kernels and the C ABI.
// Both entries read the handle's own copy of the weights and their units: no engine state is read, none is changed.
//
// k_wpe_checks: one thread per (check, particle), particle-fastest, so a member row is one coalesced 512 B load per wave; the members
//   come from the CSR list through wave-uniform loads (k_ppc_stream_stats' loop).  The statistics asked for go to the scratch table
//   [slot][N]; the particle's units go to one category per slot in registers, then wave reduction, LDS, one 64-bit atomic per
//   (slot, category, block) that is not zero.
// k_wpe_ll_stage: the leaves of a slice of rows, staged [3][rows][N] = leaf weight | cell | w^2, with the counters by kind and the
//   min / max keys of the finite participating cells (k_wpop_hist's one atomic per block).
// k_wpe_ll_terms: over the staged leaves, the three words become w exp(x - mx) | w exp(mn - x) | its square; the largest second term
//   by atomicMax on its bits (the terms are >= +0.0, so the bits order as the doubles do).
// Every sum of doubles is k_chain_pool over the fixed tree on the particle index (fg_chain_pool.h).
#include "fg_wpop_internal.h"
#include "fg_wpop_eval_plan.h"

static_assert(FG_WPE_THREADS == FG_WP_THREADS, "wp_block_minmax reduces FG_WP_WAVES waves");
#define FG_WPE_CTR 7                 // words per row of k_wpe_ll_*: fin, -inf, +inf, nan, ~min key, max key, the bits of tmax

// Check q0 + blockIdx.y, particle c0 + the thread's index along x.  A lane beyond the columns reads and writes nothing; it stays for
// the reductions with zero units.  ctr [n_slots][8]: unit sums lt eq gt nan, element counts lt eq gt nan.
__global__ __launch_bounds__(FG_WPE_THREADS) void k_wpe_checks(const unsigned long long *__restrict__ cells, long long N, long long c0, long long cols, int q0, int n_checks,
                                                              const int32_t *__restrict__ csr, const double *__restrict__ t_obs, const unsigned long long *__restrict__ units,
                                                              long long s0, long long ns, double *__restrict__ scratch, unsigned long long *ctr) {
    __shared__ unsigned long long red[FG_WP_WAVES][FG_PPC_N_STATS][FG_WPOP_CATS];
    __shared__ unsigned int cnt[FG_WP_WAVES][FG_PPC_N_STATS];
    const long long j = (long long)blockIdx.x * FG_WPE_THREADS + threadIdx.x;
    const bool live = j < cols;
    const long long c = c0 + j;
    const int q = q0 + (int)blockIdx.y;
    const int o0 = csr[q], K = csr[q + 1] - o0, mask = csr[n_checks + 1 + q], slot0 = csr[2 * n_checks + 1 + q];
    const int32_t *members = csr + 3 * n_checks + 1 + o0;
    double T[FG_PPC_N_STATS];
    unsigned long long qi = 0ull;
    if (live) {
        const unsigned long long *base = cells + c;
        fg_ppc_stats(K, [&](int i) { const int m = members[i]; return fg_ppc_cell(base[(long long)(m >> 2) * N], m & 3); }, (mask >> FG_PPC_VAR) & 1, T);
        qi = units[c];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int slot = slot0;
#pragma unroll
    for (int st = 0; st < FG_PPC_N_STATS; ++st) {
        const bool asked = (mask >> st) & 1;
        const long long k = (long long)slot - s0;              // the slot's row of the slice
        const bool mine = asked && k >= 0 && k < ns;           // uniform over the block
        unsigned long long u[FG_WPOP_CATS] = {0ull, 0ull, 0ull, 0ull};
        unsigned int n4 = 0u;                                  // four 8-bit element counts: a wave holds 64 at most
        if (mine) {
            if (live) {
                scratch[k * N + c] = T[st];
                const int cat = fg_wpe_category(T[st], t_obs[slot]);
#pragma unroll
                for (int g = 0; g < FG_WPOP_CATS; ++g) u[g] = cat == g ? qi : 0ull;
                n4 = qi ? 1u << (8 * cat) : 0u;
            }
#pragma unroll
            for (int g = 0; g < FG_WPOP_CATS; ++g)
                for (int o = 32; o > 0; o >>= 1) u[g] += __shfl_down(u[g], o, 64);
            for (int o = 32; o > 0; o >>= 1) n4 += __shfl_down(n4, o, 64);      // a field reaches 64 = 0x40 at most: no carry into its neighbour
        }
        if (lane == 0) {
#pragma unroll
            for (int g = 0; g < FG_WPOP_CATS; ++g) red[wave][st][g] = u[g];
            cnt[wave][st] = n4;
        }
        slot += asked ? 1 : 0;
    }
    __syncthreads();
    if (threadIdx.x < 2 * FG_PPC_N_STATS * FG_WPOP_CATS) {
        const int t = threadIdx.x % (FG_PPC_N_STATS * FG_WPOP_CATS), st = t / FG_WPOP_CATS, g = t % FG_WPOP_CATS;
        const bool elems = threadIdx.x >= FG_PPC_N_STATS * FG_WPOP_CATS;
        const bool asked = (mask >> st) & 1;
        const int sl = slot0 + __popc((unsigned)mask & ((1u << st) - 1u));
        const long long k = (long long)sl - s0;
        if (asked && k >= 0 && k < ns) {
            unsigned long long tot = 0ull;
            for (int v = 0; v < FG_WP_WAVES; ++v) tot += elems ? (unsigned long long)((cnt[v][st] >> (8 * g)) & 0xffu) : red[v][st][g];
            if (tot) atomicAdd(&ctr[(long long)sl * (2 * FG_WPOP_CATS) + (elems ? FG_WPOP_CATS : 0) + g], tot);
        }
    }
}

// the participating weights as leaves of a plain sum: out [n]
__global__ __launch_bounds__(FG_WPE_THREADS) void k_wpe_weights(const double *w, long long n, double *out) {
    for (long long i = (long long)blockIdx.x * FG_WPE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FG_WPE_THREADS) out[i] = fg_wpe_weight(w[i]);
}

// Rows [r0, r0 + rows) of x (blockIdx.y): st [3][rows][n] = the leaf weight, the cell, the leaf weight squared; ctr [rows][FG_WPE_CTR].
__global__ __launch_bounds__(FG_WPE_THREADS) void k_wpe_ll_stage(const double *x, const double *w, long long n, long long r0, long long rows, double *st, unsigned long long *ctr) {
    __shared__ unsigned long long red[FG_WP_WAVES][FG_WLL_COUNTS], mm[FG_WP_WAVES][2];
    const long long k = blockIdx.y;
    unsigned long long s[FG_WLL_COUNTS] = {0ull, 0ull, 0ull, 0ull}, a = ~0ull, z = 0ull;
    for (long long i = (long long)blockIdx.x * FG_WPE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FG_WPE_THREADS) {
        const double xi = x[(r0 + k) * n + i], wi = w[i];
        const double lw = fg_wp_leaf_weight(wi, xi);
        st[k * n + i] = lw;
        st[(rows + k) * n + i] = xi;
        st[(2 * rows + k) * n + i] = fg_wll_w2_term(lw);
        if (fg_wpe_weight(wi) > 0.0) {
            const int kind = fg_wll_kind(xi);
#pragma unroll
            for (int g = 0; g < FG_WLL_COUNTS; ++g) s[g] += kind == g ? 1ull : 0ull;
            if (kind == FG_WLL_FIN) {
                const unsigned long long key = fg_wp_key(xi);
                a = key < a ? key : a; z = key > z ? key : z;
            }
        }
    }
#pragma unroll
    for (int g = 0; g < FG_WLL_COUNTS; ++g) {
        for (int o = 32; o > 0; o >>= 1) s[g] += __shfl_down(s[g], o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][g] = s[g];
    }
    wp_block_minmax(a, z, mm);                                                 // its barrier covers `red`
    unsigned long long *cr = ctr + k * FG_WPE_CTR;
    if (threadIdx.x == 0 && a <= z) { atomicMax(&cr[4], ~a); atomicMax(&cr[5], z); }
    if (threadIdx.x < FG_WLL_COUNTS) {
        unsigned long long t = 0ull;
        for (int v = 0; v < FG_WP_WAVES; ++v) t += red[v][threadIdx.x];
        if (t) atomicAdd(&cr[threadIdx.x], t);
    }
}

// The terms over the same staged leaves: ref [rows][2] = mx, mn of the row.
__global__ __launch_bounds__(FG_WPE_THREADS) void k_wpe_ll_terms(long long n, long long rows, const double *ref, double *st, unsigned long long *ctr) {
    __shared__ unsigned long long mm[FG_WP_WAVES][2];
    const long long k = blockIdx.y;
    const double mx = ref[2 * k], mn = ref[2 * k + 1];
    unsigned long long a = ~0ull, z = 0ull;
    for (long long i = (long long)blockIdx.x * FG_WPE_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FG_WPE_THREADS) {
        const double lw = st[k * n + i], xi = st[(rows + k) * n + i];
        const double tn = fg_wll_sn_term(lw, xi, mn);
        st[k * n + i] = fg_wll_sp_term(lw, xi, mx);
        st[(rows + k) * n + i] = tn;
        st[(2 * rows + k) * n + i] = tn * tn;
        const unsigned long long b = (unsigned long long)__double_as_longlong(tn);
        z = b > z ? b : z;
    }
    wp_block_minmax(a, z, mm);
    if (threadIdx.x == 0 && z) atomicMax(&ctr[k * FG_WPE_CTR + 6], z);
}

extern "C" {

int fg_wpop_checks_n_slots(int n_checks, const int32_t *h_stat_mask) {
    std::string err;
    const int n = fg_wpe_n_slots(n_checks, h_stat_mask, &err);
    if (n < 0) fg_set_error(err);
    return n;
}

int fg_wpop_checks(fg_wpop *h, const void *d_yrep, int n_rows, const int32_t *h_vtypes, int n_checks, const int32_t *h_offsets, const int32_t *h_members,
                   const int32_t *h_stat_mask, const double *h_observed, double *h_t_obs, uint64_t *h_units, int64_t *h_counts, double *h_moments) {
    if (int rc = need_wpop(h)) return rc;
    FgPpcPlan P;
    std::string err;
    if (int rc = fg_wpe_checks_init(P, h->n, n_rows, h_vtypes, n_checks, h_offsets, h_members, h_stat_mask, h_observed, &err)) { fg_set_error(err); return rc; }
    if (!d_yrep || !h_t_obs || !h_units || !h_counts || !h_moments) { fg_set_error("fg_wpop_checks: null d_yrep or output"); return FG_E_BAD_ARG; }
    fg_engine *e = h->e;
    const long long N = h->n, n_slots = P.n_slots, per = fg_wpe_slot_rows(N, n_slots);
    const std::vector<int32_t> csr = fg_wpe_csr(P);
    WpScope sc;
    int32_t *d_csr = nullptr;
    double *d_obs = nullptr, *d_scratch = nullptr;
    unsigned long long *d_ctr = nullptr;
    const size_t n_ctr = (size_t)n_slots * 2 * FG_WPOP_CATS;
    if (sc.alloc(&d_csr, csr.size(), "the check list") || sc.alloc(&d_obs, (size_t)n_slots, "the observed statistics") ||
        sc.alloc(&d_scratch, (size_t)per * (size_t)N, "the statistics") || sc.alloc(&d_ctr, n_ctr, "the counters"))
        return FG_E_HIP;
    HIPCHK(hipMemcpyAsync(d_csr, csr.data(), csr.size() * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(d_obs, P.t_obs.data(), (size_t)n_slots * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(d_ctr, 0, n_ctr * 8, e->stream));
    for (long long s0 = 0; s0 < n_slots; s0 += per) {
        const long long ns = std::min(per, n_slots - s0);
        int q0 = 0, q1 = 0;
        fg_wpe_slice_checks(P, s0, ns, &q0, &q1);
        for (const FgPoolLaunch &L : P.launches) {
            const dim3 grid((unsigned)((L.cols + FG_WPE_THREADS - 1) / FG_WPE_THREADS), (unsigned)(q1 - q0)), block(FG_WPE_THREADS);
            hipLaunchKernelGGL(k_wpe_checks, grid, block, 0, e->stream, (const unsigned long long *)d_yrep, N, L.col0, L.cols, q0, P.n_checks, (const int32_t *)d_csr,
                               (const double *)d_obs, (const unsigned long long *)h->d_q, s0, ns, d_scratch, d_ctr);
            HIPCHK(hipGetLastError());
        }
        if (int rc = fg_wpop_moments(h, d_scratch, (int)ns, h_moments + s0 * FG_WPOP_MOMENTS)) return rc;      // the same stream: after the statistics
    }
    std::vector<unsigned long long> ctr(n_ctr);
    HIPCHK(hipMemcpyAsync(ctr.data(), d_ctr, n_ctr * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    for (long long k = 0; k < n_slots; ++k)
        for (int g = 0; g < FG_WPOP_CATS; ++g) {
            h_units[k * FG_WPOP_CATS + g] = ctr[(size_t)k * 2 * FG_WPOP_CATS + g];
            h_counts[k * FG_WPOP_CATS + g] = (int64_t)ctr[(size_t)k * 2 * FG_WPOP_CATS + FG_WPOP_CATS + g];
        }
    std::memcpy(h_t_obs, P.t_obs.data(), (size_t)n_slots * 8);
    const int rc = fg_wpe_checks_verify((int)n_slots, h_units, h->T, &err);
    if (rc) fg_set_error(err);
    return rc;
}

int fg_wpop_loglik(fg_wpop *h, const double *d_ll, int n_sel, double *h_figures, double *h_words, int64_t *h_counts) {
    if (int rc = need_wpop(h)) return rc;
    std::string err;
    if (int rc = fg_wll_check(n_sel, &err)) { fg_set_error(err); return rc; }
    if (!d_ll || !h_figures) { fg_set_error("fg_wpop_loglik: null d_ll or h_figures"); return FG_E_BAD_ARG; }
    fg_engine *e = h->e;
    const long long N = h->n, per = fg_wll_rows(N, n_sel);
    const std::vector<FgPoolLevel> levels = fg_pool_levels(N);
    WpScope sc;
    double *st = nullptr, *tree[2] = {nullptr, nullptr}, *d_ref = nullptr;
    unsigned long long *d_ctr = nullptr;
    const size_t tree_words = (size_t)per * (size_t)levels[0].m_out * FgWpPool::WORDS;
    if (sc.alloc(&st, FG_WLL_STAGE * (size_t)per * (size_t)N, "the staged leaves") || sc.alloc(&tree[0], tree_words, "the tree") || sc.alloc(&tree[1], tree_words, "the tree") ||
        sc.alloc(&d_ref, 2 * (size_t)per, "the reference points") || sc.alloc(&d_ctr, FG_WPE_CTR * (size_t)per, "the counters"))
        return FG_E_HIP;
    std::vector<double> hW, h1, hs[4], ref;
    std::vector<unsigned long long> ctr((size_t)per * FG_WPE_CTR);
    // W: the participating weights, one number per handle
    hipLaunchKernelGGL(k_wpe_weights, dim3(fg_wp_blocks(N, 1)), dim3(FG_WPE_THREADS), 0, e->stream, (const double *)h->d_w, N, st);
    HIPCHK(hipGetLastError());
    if (int rc = fg_chain_pool_run<FgWpSumPool>(e->stream, levels, fg_pool_slices(1, FG_POOL_MAX_GRID_Y), st, 0, tree, hW)) return rc;
    for (long long r0 = 0; r0 < n_sel; r0 += per) {
        const long long rows = std::min<long long>(per, n_sel - r0);
        const std::vector<FgPoolSlice> slices = fg_pool_slices(rows, FG_POOL_MAX_GRID_Y);
        const dim3 grid(fg_wp_blocks(N, rows), (unsigned)rows), block(FG_WPE_THREADS);
        const size_t n_ctr = (size_t)rows * FG_WPE_CTR;
        HIPCHK(hipMemsetAsync(d_ctr, 0, n_ctr * 8, e->stream));
        hipLaunchKernelGGL(k_wpe_ll_stage, grid, block, 0, e->stream, d_ll, (const double *)h->d_w, N, r0, rows, st, d_ctr);
        HIPCHK(hipGetLastError());
        if (int rc = fg_chain_pool_run<FgWpPool>(e->stream, levels, slices, st, rows * N, tree, h1)) return rc;
        if (int rc = fg_chain_pool_run<FgWpSumPool>(e->stream, levels, slices, st + 2 * rows * N, 0, tree, hs[3])) return rc;
        HIPCHK(hipMemcpyAsync(ctr.data(), d_ctr, n_ctr * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        ref.assign(2 * (size_t)rows, 0.0);
        for (long long k = 0; k < rows; ++k)
            if (ctr[(size_t)k * FG_WPE_CTR + FG_WLL_FIN]) { ref[2 * (size_t)k] = fg_qs_unkey(ctr[(size_t)k * FG_WPE_CTR + 5]); ref[2 * (size_t)k + 1] = fg_qs_unkey(~ctr[(size_t)k * FG_WPE_CTR + 4]); }
        HIPCHK(hipMemcpyAsync(d_ref, ref.data(), ref.size() * 8, hipMemcpyHostToDevice, e->stream));
        hipLaunchKernelGGL(k_wpe_ll_terms, grid, block, 0, e->stream, N, rows, (const double *)d_ref, st, d_ctr);
        HIPCHK(hipGetLastError());
        for (int j = 0; j < 3; ++j)
            if (int rc = fg_chain_pool_run<FgWpSumPool>(e->stream, levels, slices, st + j * rows * N, 0, tree, hs[j])) return rc;
        HIPCHK(hipMemcpyAsync(ctr.data(), d_ctr, n_ctr * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        for (long long k = 0; k < rows; ++k) {
            const unsigned long long *cr = &ctr[(size_t)k * FG_WPE_CTR];
            const int64_t c[FG_WLL_COUNTS] = {(int64_t)cr[0], (int64_t)cr[1], (int64_t)cr[2], (int64_t)cr[3]};
            double w[FG_WLL_WORDS];
            if (int rc = fg_wll_words(hW[0], FgWpPool::elem_load(&h1[(size_t)k * FgWpPool::WORDS]), hs[3][(size_t)k], cr[4], cr[5], hs[0][(size_t)k], hs[1][(size_t)k],
                                      hs[2][(size_t)k], cr[6], c, r0 + k, w, &err)) { fg_set_error(err); return rc; }
            double fig[FG_WLL_FIGURES];
            fg_wll_finish(w, c, fig);
            for (int f = 0; f < FG_WLL_FIGURES; ++f) h_figures[(size_t)f * (size_t)n_sel + (size_t)(r0 + k)] = fig[f];
            if (h_words) std::memcpy(h_words + (size_t)(r0 + k) * FG_WLL_WORDS, w, sizeof(w));
            if (h_counts) std::memcpy(h_counts + (size_t)(r0 + k) * FG_WLL_COUNTS, c, sizeof(c));
        }
    }
    return FG_OK;
}

}  // extern "C"
