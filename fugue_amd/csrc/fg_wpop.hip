// fg_wpop.hip -- the summary of a weighted population on the device (what the reference leaves to ABCSMCResult::weighted_mean,
// abc.rs:476, and to the doc example that walks the particles by hand, smc.rs:445-453): weighted mean / spread / Monte Carlo error,
// exact weighted quantiles and exact weighted frequency tables of rows [d][N] that stay in HBM.  Definitions, the selection step,
// the pools of the moments and every read-out are fg_wpop_plan.h's (plain C++); here are the kernels that see the population and
// the C ABI.  This engine's device only; the handle keeps its own copy of the weights and their units, so it reads engine state at
// fg_wpop_new and never afterwards, and changes none.
//
// Device state of a quantile pass, all 64-bit words, zeroed at its start (nb = 2^w, H hist groups, K collect groups):
//   tab  [H + K][4]   row | prefix | offset of the group's pairs | its element count m
//   ctr  units [H][nb] | elements [H][nb] | mn [H] (as ~key under atomicMax, so 0 is "none yet") | mx [H] | cursor [K]
//   pairs [sum of the collect groups' m][2]   key, units
#include "fg_wpop_internal.h"

// w -> q, and the four sums: bad weights, good weights of zero units, the units' high and low halves.  Wave reduction, LDS, then one
// 64-bit atomic per block and non-zero sum.
__global__ __launch_bounds__(FG_WP_THREADS) void k_wpop_units(const double *w, long long n, unsigned long long *q, unsigned long long *ctr) {
    __shared__ unsigned long long red[FG_WP_WAVES][4];
    unsigned long long s[4] = {0ull, 0ull, 0ull, 0ull};
    for (long long i = (long long)blockIdx.x * FG_WP_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FG_WP_THREADS) {
        const double wi = w[i];
        const bool good = fg_wp_good(wi);
        const unsigned long long u = fg_wp_units(wi);
        q[i] = u;
        s[0] += good ? 0ull : 1ull;
        s[1] += good && u == 0ull ? 1ull : 0ull;
        s[2] += u >> 32;
        s[3] += u & 0xffffffffull;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        for (int o = 32; o > 0; o >>= 1) s[j] += __shfl_down(s[j], o, 64);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = s[j];
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        unsigned long long t = 0ull;
        for (int v = 0; v < FG_WP_WAVES; ++v) t += red[v][threadIdx.x];
        if (t) atomicAdd(&ctr[threadIdx.x], t);
    }
}

// The leaves of the moments, rows [r0, r0 + rows) of x (blockIdx.y): out [2][rows][n] = the leaf weight, the cell.
__global__ __launch_bounds__(FG_WP_THREADS) void k_wpop_leaves(const double *x, const double *w, long long n, long long r0, long long rows, double *out) {
    const long long k = blockIdx.y;
    for (long long i = (long long)blockIdx.x * FG_WP_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FG_WP_THREADS) {
        const double xi = x[(r0 + k) * n + i];
        out[k * n + i] = fg_wp_leaf_weight(w[i], xi);
        out[(rows + k) * n + i] = xi;
    }
}
// The terms of the second pass over the same staged leaves: word 0 becomes (lw (x - mean_k))^2.
__global__ __launch_bounds__(FG_WP_THREADS) void k_wpop_terms(long long n, long long rows, const double *mean, double *st) {
    const long long k = blockIdx.y;
    const double mu = mean[k];
    for (long long i = (long long)blockIdx.x * FG_WP_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FG_WP_THREADS)
        st[k * n + i] = fg_wp_mcse_term(st[k * n + i], st[(rows + k) * n + i], mu);
}

// One group per grid row (blockIdx.y), grid-stride over the n elements of its row.  An element of non-zero units whose key matches
// the group's prefix adds its units (u64) and 1 (u32: a block sees fewer than 2^32 elements, fg_wp_blocks) to its digit's bins in
// LDS, 2^w x 12 bytes; the non-zero bins are flushed with 64-bit atomics, min and max with one atomic per block.
__global__ __launch_bounds__(FG_WP_THREADS) void k_wpop_hist(const double *x, const unsigned long long *q, long long n, const unsigned long long *tab, int n_hist, int b, int w,
                                                           unsigned long long *ctr) {
    extern __shared__ unsigned long long shu[];
    __shared__ unsigned long long mm[FG_WP_WAVES][2];
    const int nb = 1 << w, g = blockIdx.y;
    unsigned int *shc = (unsigned int *)(shu + nb);
    for (int k = threadIdx.x; k < nb; k += FG_WP_THREADS) { shu[k] = 0ull; shc[k] = 0u; }
    const long long row = (long long)tab[4ll * g];
    const unsigned long long pf = tab[4ll * g + 1];
    const double *xr = x + row * n;
    const int lo = 64 - b - w;
    const unsigned int mask = (1u << w) - 1u;
    unsigned long long a = ~0ull, z = 0ull;
    __syncthreads();
    for (long long i = (long long)blockIdx.x * FG_WP_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FG_WP_THREADS) {
        const unsigned long long qi = q[i];
        if (qi == 0ull) continue;
        const unsigned long long key = fg_wp_key(xr[i]);
        if (!fg_wp_match(key, pf, b)) continue;
        const unsigned int digit = (unsigned int)(key >> lo) & mask;
        atomicAdd(&shu[digit], qi);
        atomicAdd(&shc[digit], 1u);
        a = key < a ? key : a; z = key > z ? key : z;
    }
    __syncthreads();
    unsigned long long *units = ctr + (long long)g * nb, *elems = ctr + ((long long)n_hist + g) * nb;
    for (int k = threadIdx.x; k < nb; k += FG_WP_THREADS)
        if (shc[k]) { atomicAdd(&units[k], shu[k]); atomicAdd(&elems[k], (unsigned long long)shc[k]); }
    wp_block_minmax(a, z, mm);
    if (threadIdx.x == 0 && a <= z) {
        unsigned long long *mn = ctr + 2ll * n_hist * nb;
        atomicMax(&mn[g], ~a);
        atomicMax(&mn[n_hist + g], z);
    }
}

// The same walk for the collect groups (tab: theirs): a matching element reserves a position with atomicAdd on the group's cursor
// and stores (key, units) only when the position lies below the group's element count m -- the pair buffer holds exactly the m of
// every group, and a cursor past m is the host's integrity error, never a write.
__global__ __launch_bounds__(FG_WP_THREADS) void k_wpop_collect(const double *x, const unsigned long long *q, long long n, const unsigned long long *tab, int b,
                                                              unsigned long long *cursor, ulonglong2 *pairs) {
    const int g = blockIdx.y;
    const long long row = (long long)tab[4ll * g];
    const unsigned long long pf = tab[4ll * g + 1], off = tab[4ll * g + 2], m = tab[4ll * g + 3];
    const double *xr = x + row * n;
    for (long long i = (long long)blockIdx.x * FG_WP_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FG_WP_THREADS) {
        const unsigned long long qi = q[i];
        if (qi == 0ull) continue;
        const unsigned long long key = fg_wp_key(xr[i]);
        if (!fg_wp_match(key, pf, b)) continue;
        const unsigned long long pos = atomicAdd(&cursor[g], 1ull);
        if (pos < m) pairs[off + pos] = make_ulonglong2(key, qi);
    }
}

// One row of integer cells per grid row (blockIdx.y; tab: fg_cs_table's five words).  A cell of non-zero units adds them to its bin
// of a u64 histogram in LDS (`lds_bins` words, the widest row's) or to the thread's below / above; one flush per block.
__global__ __launch_bounds__(FG_WP_THREADS) void k_wpop_counts(const unsigned long long *cells, const unsigned long long *q, long long n, const unsigned long long *tab,
                                                             unsigned long long *ctr, long long n_bins, int n_rows) {
    extern __shared__ unsigned long long hist[];
    __shared__ unsigned long long mm[FG_WP_WAVES][2], ba[FG_WP_WAVES][2];
    const int k = blockIdx.y;
    const unsigned long long *t5 = tab + (long long)k * FG_CS_TAB_WORDS;
    const unsigned long long klo = t5[1], flip = t5[4];
    const int bins = (int)(t5[2] & 0xffffffffull);
    const long long off = (long long)t5[3];
    for (int j = threadIdx.x; j < bins; j += FG_WP_THREADS) hist[j] = 0ull;
    __syncthreads();
    const unsigned long long *cr = cells + (long long)k * n;
    unsigned long long a = ~0ull, z = 0ull, below = 0ull, above = 0ull;
    for (long long i = (long long)blockIdx.x * FG_WP_THREADS + threadIdx.x; i < n; i += (long long)gridDim.x * FG_WP_THREADS) {
        const unsigned long long qi = q[i];
        if (qi == 0ull) continue;
        const unsigned long long key = cr[i] ^ flip;
        const int bin = fg_cs_bin(key, klo, bins);
        if (bin < 0) below += qi;
        else if (bin == bins) above += qi;
        else atomicAdd(&hist[bin], qi);
        a = key < a ? key : a; z = key > z ? key : z;
    }
    for (int o = 32; o > 0; o >>= 1) { below += __shfl_down(below, o, 64); above += __shfl_down(above, o, 64); }
    if ((threadIdx.x & 63) == 0) { ba[threadIdx.x >> 6][0] = below; ba[threadIdx.x >> 6][1] = above; }
    wp_block_minmax(a, z, mm);                                                 // its barrier covers `ba` and the histogram
    unsigned long long *gb = ctr + n_bins, *ga = gb + n_rows, *mn = ga + n_rows, *mx = mn + n_rows;
    if (threadIdx.x == 0) {
        for (int v = 1; v < FG_WP_WAVES; ++v) { below += ba[v][0]; above += ba[v][1]; }
        if (below) atomicAdd(&gb[k], below);
        if (above) atomicAdd(&ga[k], above);
        if (a <= z) { atomicMax(&mn[k], ~a); atomicMax(&mx[k], z); }
    }
    for (int j = threadIdx.x; j < bins; j += FG_WP_THREADS)
        if (hist[j]) atomicAdd(&ctr[off + j], hist[j]);
}

extern "C" {

int fg_wpop_new(fg_engine *e, int64_t n, const double *d_w, fg_wpop **out) {
    NEED_ENGINE(e);
    if (!out) { fg_set_error("fg_wpop_new: null out"); return FG_E_BAD_ARG; }
    *out = nullptr;
    std::string bad;
    if (int rc = fg_wp_new_check(n, &bad)) { fg_set_error(bad); return rc; }
    if (!d_w) {                                                                // the engine's own population
        if (int rc = fg_internal_smc_weights(e, &d_w)) return rc;
        if (n != e->C) { fg_set_error("fg_wpop_new: the engine's population has " + std::to_string(e->C) + " particles, n = " + std::to_string(n)); return FG_E_BAD_ARG; }
    }
    fg_wpop *h = new fg_wpop;
    h->e = e; h->n = n;
    unsigned long long *d_ctr = nullptr;
    unsigned long long ctr[4] = {0, 0, 0, 0};
    int rc = FG_OK;
    if (hipMalloc((void **)&h->d_w, (size_t)n * 8) != hipSuccess || hipMalloc((void **)&h->d_q, (size_t)n * 8) != hipSuccess) { fg_set_error("fg_wpop_new: no device memory for n weights and units"); rc = FG_E_HIP; }
    if (!rc) rc = dev_alloc(&d_ctr, 4);
    if (!rc) {
        auto run = [&]() -> int {
            HIPCHK(hipMemcpyAsync(h->d_w, d_w, (size_t)n * 8, hipMemcpyDeviceToDevice, e->stream));
            hipLaunchKernelGGL(k_wpop_units, dim3(fg_wp_blocks(n, 1)), dim3(FG_WP_THREADS), 0, e->stream, (const double *)h->d_w, (long long)n, h->d_q, d_ctr);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(ctr, d_ctr, sizeof(ctr), hipMemcpyDeviceToHost, e->stream));
            HIPCHK(hipStreamSynchronize(e->stream));
            return FG_OK;
        };
        rc = run();
    }
    if (d_ctr) (void)hipFree(d_ctr);
    if (!rc) {
        std::string err;
        rc = fg_wp_total(ctr[2], ctr[3], &h->T, &err);
        if (rc) fg_set_error(err);
        h->n_bad = ctr[0]; h->n_zero = ctr[1];
    }
    if (rc) { fg_wpop_free(h); return rc; }
    *out = h;
    return FG_OK;
}

int fg_wpop_units(const fg_wpop *h, uint64_t *out_T, uint64_t *out_n_bad, uint64_t *out_n_zero) {
    if (!h) { fg_set_error("null weighted population"); return FG_E_BAD_ARG; }
    if (out_T) *out_T = h->T;
    if (out_n_bad) *out_n_bad = h->n_bad;
    if (out_n_zero) *out_n_zero = h->n_zero;
    return FG_OK;
}

int fg_wpop_moments(fg_wpop *h, const double *d_x, int d, double *h_out) {
    if (int rc = need_wpop(h)) return rc;
    std::string bad;
    if (int rc = fg_wp_m_check(d, &bad)) { fg_set_error(bad); return rc; }
    if (!d_x || !h_out) { fg_set_error("fg_wpop_moments: null d_x or h_out"); return FG_E_BAD_ARG; }
    fg_engine *e = h->e;
    const long long N = h->n, rows_per = fg_wp_moment_rows(N, d);
    const std::vector<FgPoolLevel> levels = fg_pool_levels(N);
    WpScope sc;
    double *st = nullptr, *tree[2] = {nullptr, nullptr}, *d_mean = nullptr;
    const size_t tree_words = (size_t)rows_per * (size_t)levels[0].m_out * FgWpPool::WORDS;
    if (sc.alloc(&st, 2 * (size_t)rows_per * (size_t)N, "the staged leaves") || sc.alloc(&tree[0], tree_words, "the tree") || sc.alloc(&tree[1], tree_words, "the tree") ||
        sc.alloc(&d_mean, (size_t)rows_per, "the means"))
        return FG_E_HIP;
    std::vector<double> h1, h2, mean;
    for (long long r0 = 0; r0 < d; r0 += rows_per) {
        const long long rows = std::min<long long>(rows_per, d - r0);
        const std::vector<FgPoolSlice> slices = fg_pool_slices(rows, FG_POOL_MAX_GRID_Y);
        const dim3 grid(fg_wp_blocks(N, rows), (unsigned)rows), block(FG_WP_THREADS);
        hipLaunchKernelGGL(k_wpop_leaves, grid, block, 0, e->stream, d_x, (const double *)h->d_w, N, r0, rows, st);
        HIPCHK(hipGetLastError());
        if (int rc = fg_chain_pool_run<FgWpPool>(e->stream, levels, slices, st, rows * N, tree, h1)) return rc;
        mean.resize((size_t)rows);
        for (long long k = 0; k < rows; ++k) { const FgWpElem el = FgWpPool::elem_load(&h1[(size_t)k * FgWpPool::WORDS]); mean[(size_t)k] = el.n ? el.mean : std::nan(""); }
        HIPCHK(hipMemcpyAsync(d_mean, mean.data(), (size_t)rows * 8, hipMemcpyHostToDevice, e->stream));
        hipLaunchKernelGGL(k_wpop_terms, grid, block, 0, e->stream, N, rows, (const double *)d_mean, st);
        HIPCHK(hipGetLastError());
        if (int rc = fg_chain_pool_run<FgWpSumPool>(e->stream, levels, slices, st, 0, tree, h2)) return rc;
        for (long long k = 0; k < rows; ++k) fg_wp_finish(FgWpPool::elem_load(&h1[(size_t)k * FgWpPool::WORDS]), h2[(size_t)k], h_out + (r0 + k) * FG_WPOP_MOMENTS);
    }
    return FG_OK;
}

int fg_wpop_quantiles(fg_wpop *h, const double *d_x, int d, const double *h_probs, int n_probs, int digit_bits, int64_t capacity, double *h_out, int32_t *h_passes) {
    if (int rc = need_wpop(h)) return rc;
    std::string err;
    if (int rc = fg_wp_q_check(d, h_probs, n_probs, digit_bits, capacity, &err)) { fg_set_error(err); return rc; }
    if (!d_x || !h_out) { fg_set_error("fg_wpop_quantiles: null d_x or h_out"); return FG_E_BAD_ARG; }
    fg_engine *e = h->e;
    const long long N = h->n;
    const uint64_t n_live = (uint64_t)N - h->n_bad - h->n_zero;
    const int rows_per = std::max(1, FG_WP_MAX_GROUPS / n_probs);
    const size_t G = (size_t)std::min(rows_per, d) * n_probs;                  // the most groups of a pass
    WpScope sc;
    unsigned long long *d_tab = nullptr, *d_ctr = nullptr;
    ulonglong2 *d_pairs = nullptr;
    size_t pairs_cap = 0;
    const size_t ctr_cap = ((2 * G) << digit_bits) + 3 * G;
    if (sc.alloc(&d_tab, 4 * G, "the group table") || sc.alloc(&d_ctr, ctr_cap, "the counters")) return FG_E_HIP;
    std::vector<unsigned long long> tab, ctr;
    std::vector<ulonglong2> flat;
    FgWpQPlan P;
    for (int r0 = 0; r0 < d; r0 += rows_per) {
        const int rows = std::min(rows_per, d - r0);
        const double *x0 = d_x + (long long)r0 * N;
        fg_wp_q_init(P, rows, h_probs, n_probs, digit_bits, capacity, h->T, n_live);
        while (!P.done) {
            const size_t H = P.hist.size(), K = P.col.size(), nb = (size_t)1 << P.w;
            tab.assign(4 * (H + K), 0ull);
            for (size_t g = 0; g < H + K; ++g) {
                const FgWpGroup &gr = g < H ? P.hist[g] : P.col[g - H];
                tab[4 * g] = (unsigned long long)gr.row; tab[4 * g + 1] = gr.prefix; tab[4 * g + 2] = gr.off; tab[4 * g + 3] = gr.m;
            }
            const size_t n_ctr = 2 * H * nb + 2 * H + K;
            if (P.col_pairs > pairs_cap) {                                     // never read before written: no memset
                if (sc.alloc(&d_pairs, (size_t)P.col_pairs, "the collected pairs")) return FG_E_HIP;
                pairs_cap = (size_t)P.col_pairs;
            }
            HIPCHK(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, e->stream));
            HIPCHK(hipMemsetAsync(d_ctr, 0, n_ctr * 8, e->stream));
            if (H) {
                hipLaunchKernelGGL(k_wpop_hist, dim3(fg_wp_blocks(N, (long long)H), (unsigned)H), dim3(FG_WP_THREADS), nb * 12, e->stream, x0, (const unsigned long long *)h->d_q, N,
                                   (const unsigned long long *)d_tab, (int)H, P.b, P.w, d_ctr);
                HIPCHK(hipGetLastError());
            }
            if (K) {
                hipLaunchKernelGGL(k_wpop_collect, dim3(fg_wp_blocks(N, (long long)K), (unsigned)K), dim3(FG_WP_THREADS), 0, e->stream, x0, (const unsigned long long *)h->d_q, N,
                                   (const unsigned long long *)(d_tab + 4 * H), P.b, d_ctr + 2 * H * nb + 2 * H, d_pairs);
                HIPCHK(hipGetLastError());
            }
            ctr.resize(n_ctr);
            HIPCHK(hipMemcpyAsync(ctr.data(), d_ctr, n_ctr * 8, hipMemcpyDeviceToHost, e->stream));
            HIPCHK(hipStreamSynchronize(e->stream));
            std::vector<uint64_t> units(ctr.begin(), ctr.begin() + H * nb), elems(ctr.begin() + H * nb, ctr.begin() + 2 * H * nb), mn(H), mx(H), cursor(K);
            for (size_t g = 0; g < H; ++g) { mn[g] = ~ctr[2 * H * nb + g]; mx[g] = ctr[2 * H * nb + H + g]; }
            std::vector<FgWpPairs> pairs(K);
            bool fits = true;
            for (size_t g = 0; g < K; ++g) { cursor[g] = ctr[2 * H * nb + 2 * H + g]; fits = fits && cursor[g] == P.col[g].m; }
            if (K && fits && P.col_pairs) {                                    // a cursor off its m: the plan reports it, nothing is read
                flat.resize((size_t)P.col_pairs);
                HIPCHK(hipMemcpy(flat.data(), d_pairs, flat.size() * sizeof(ulonglong2), hipMemcpyDeviceToHost));
                for (size_t g = 0; g < K; ++g) {
                    pairs[g].reserve((size_t)P.col[g].m);
                    for (uint64_t j = 0; j < P.col[g].m; ++j) pairs[g].emplace_back(flat[(size_t)(P.col[g].off + j)].x, flat[(size_t)(P.col[g].off + j)].y);
                }
            }
            FgWpPassData D;
            D.units = units.data(); D.elems = elems.data(); D.mn = mn.data(); D.mx = mx.data(); D.cursor = cursor.data(); D.pairs = &pairs;
            if (int rc = fg_wp_end_pass(P, D, &err)) { fg_set_error(err); return rc; }
        }
        fg_wp_q_result(P, h_out + (size_t)r0 * n_probs, h_passes ? h_passes + (size_t)r0 * n_probs : nullptr);
    }
    return FG_OK;
}

int fg_wpop_counts(fg_wpop *h, const void *d_cells, int n_rows, const int32_t *h_vtypes, const int64_t *h_lo, const int32_t *h_bins, uint64_t *h_units, uint64_t *h_below,
                   uint64_t *h_above, int64_t *h_min, int64_t *h_max) {
    if (int rc = need_wpop(h)) return rc;
    FgCsPlan P;
    std::string err;
    if (int rc = fg_wp_c_init(P, h->n, n_rows, h_vtypes, h_lo, h_bins, &err)) { fg_set_error(err); return rc; }
    if (!d_cells || !h_units || !h_below || !h_above || !h_min || !h_max) { fg_set_error("fg_wpop_counts: null d_cells or output"); return FG_E_BAD_ARG; }
    fg_engine *e = h->e;
    std::vector<uint64_t> tab;
    fg_cs_table(P, tab);
    std::vector<unsigned long long> tab_dev(tab.begin(), tab.end()), ctr(fg_cs_words(P));
    WpScope sc;
    unsigned long long *d_tab = nullptr, *d_ctr = nullptr;
    if (sc.alloc(&d_tab, tab_dev.size(), "the row table") || sc.alloc(&d_ctr, ctr.size(), "the counters")) return FG_E_HIP;
    HIPCHK(hipMemcpyAsync(d_tab, tab_dev.data(), tab_dev.size() * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(d_ctr, 0, ctr.size() * 8, e->stream));
    hipLaunchKernelGGL(k_wpop_counts, dim3(fg_wp_blocks(h->n, n_rows), (unsigned)n_rows), dim3(FG_WP_THREADS), (size_t)fg_cs_lds_bins(P) * 8, e->stream,
                       (const unsigned long long *)d_cells, (const unsigned long long *)h->d_q, (long long)h->n, (const unsigned long long *)d_tab, d_ctr, (long long)P.n_bins, n_rows);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ctr.data(), d_ctr, ctr.size() * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    std::vector<uint64_t> words(ctr.begin(), ctr.end());
    const int rc = fg_wp_c_result(P, words.data(), h->T, h_units, h_below, h_above, h_min, h_max, &err);
    if (rc) fg_set_error(err);
    return rc;
}

void fg_wpop_free(fg_wpop *h) {
    if (!h) return;
    if (h->e && hipSetDevice(h->e->device) == hipSuccess) {
        if (h->d_w) (void)hipFree(h->d_w);
        if (h->d_q) (void)hipFree(h->d_q);
    }
    delete h;
}

}  // extern "C"
