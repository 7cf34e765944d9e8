// fg_grid.hip -- log-joint surfaces on the device: log_joint_grid (crates/fugue-wasm/src/grid.rs), every cell of a grid over one or two
// f64 sample sites scored by the run that k_log_joint does, for a bank of bases, with the normaliser, the two marginals, the mode and
// the non-finite counts of every base, and the mixture over the bases of the normalised surfaces (fg_grid_plan.h: the launches, the
// summation orders, the refusals).
//
// grid.rs:48-67 line by line, per base c (an engine chain) and cell = j n_a + i:
//   t = base.clone()                          fg_load_values from chain c for every lane: the engine's state is read only
//   choices[addr_a].value = F64(a)            the slot of site_a := a_values[i]
//   choices[addr_b].value = F64(b)            then the slot of site_b := b_values[j] (the same site: b wins)
//   run(ScoreGivenTrace, model)               fg_exec<FG_MODE_SCORE> over P.ins_fast, k_log_joint's body
//   out.push(scored.total_log_weight())       prior + likelihood + factors in that order (fg_total)
// The reductions run on the chunk table [bases of the chunk][n_b][n_a] after it is scored; nothing of size cells x bases outlives a chunk
// unless the caller hands a table in.
#include "fg_engine_internal.h"
#include "fg_grid_plan.h"

struct FgGridDev {
    const double *a, *b;         // the axes on the device; b null: one axis
    int slot_a, slot_b;          // LDS slot rows of the two sites (slot_b < 0: one axis)
    unsigned n_a, cells;
    long long chain0;            // engine chain of the chunk's first base
    double *chunk;               // [gridDim.y][cells]
    double *acc;                 // null, or the caller's [3][acc_bases][cells] at this chunk's first base
    long long acc_stride;        // acc_bases * cells
};

// ---- run(ScoreGivenTrace, model) at every cell: one wave per 64 consecutive cells, one base per wave ----
__global__ __launch_bounds__(FG_WAVE, FG_MIN_WAVES) void k_grid_eval(FgProgramDev P, FgChainCtx X, FgGridDev G) {
    extern __shared__ double lds_[];
    constexpr int tw = FG_WAVE;
    const unsigned cell = blockIdx.x * (unsigned)tw + threadIdx.x;
    const bool live = cell < G.cells;
    const unsigned cl = live ? cell : G.cells - 1u;          // dead lanes of the tail wave score the last cell and store nothing
    const long long c = G.chain0 + (long long)blockIdx.y;
    double *slots = lds_ + threadIdx.x;
    fg_load_values(P, X, c, slots, tw);
    const unsigned j = cl / G.n_a, i = cl - j * G.n_a;
    slots[G.slot_a * tw] = G.a[i];                           // grid.rs:52-54
    if (G.slot_b >= 0) slots[G.slot_b * tw] = G.b[j];        // grid.rs:55-57
    FgAcc3 A = {0.0, 0.0, 0.0};
    fg_exec<FG_MODE_SCORE, false>(P.ins_fast, P.n_ins, P.pool, slots, tw, A, nullptr, nullptr, 0, live);
    if (live) {
        const size_t o = (size_t)blockIdx.y * G.cells + cell;
        G.chunk[o] = fg_total(A);
        if (G.acc) { G.acc[o] = A.prior; G.acc[G.acc_stride + o] = A.lik; G.acc[2 * G.acc_stride + o] = A.fac; }
    }
}

// ---- log_marg_a: one thread per column, log_sum_exp over j in index order (numerical.rs:15-38) ----
__global__ __launch_bounds__(FG_GRID_COL_THREADS) void k_grid_cols(const double *chunk, unsigned n_a, unsigned n_b, double *lma /*[bases][n_a]*/) {
    const unsigned i = blockIdx.x * (unsigned)FG_GRID_COL_THREADS + threadIdx.x;
    if (i >= n_a) return;
    const double *col = chunk + (size_t)blockIdx.y * n_a * n_b + i;
    double m = FG_NEG_INF;
    for (unsigned j = 0; j < n_b; ++j) m = fmax(m, col[(size_t)j * n_a]);
    double r = FG_NEG_INF;
    if (m != FG_NEG_INF) {
        double s = 0.0;
        for (unsigned j = 0; j < n_b; ++j) s += exp(col[(size_t)j * n_a] - m);
        r = s == 0.0 ? FG_NEG_INF : m + log(s);
    }
    lma[(size_t)blockIdx.y * n_a + i] = r;
}

// ---- log_marg_b, and the row's share of the mode and of the counts: one workgroup per (row, base) ----
__global__ __launch_bounds__(FG_GRID_ROW_MAX_THREADS) void k_grid_rows(const double *chunk, unsigned n_a, unsigned n_b, double *lmb /*[bases][n_b]*/,
                                                                       double *row_max, long long *row_arg /*[bases][n_b]*/, int *row_cnt /*[bases][n_b][3]*/) {
    __shared__ double red_m[4], red_v[4], red_s[4];
    __shared__ int red_i[4], red_c[4][3];
    const int tid = (int)threadIdx.x, T = (int)blockDim.x, lane = tid & (FG_GRID_WAVE - 1), wave = tid / FG_GRID_WAVE, n_waves = T / FG_GRID_WAVE;
    const unsigned j = blockIdx.x;
    const size_t ro = (size_t)blockIdx.y * n_b + j;
    const double *row = chunk + ro * n_a;
    double m = FG_NEG_INF, best = FG_NEG_INF;
    int bi = -1, c_nan = 0, c_ninf = 0, c_pinf = 0;
    for (unsigned i = (unsigned)tid; i < n_a; i += (unsigned)T) {
        const double x = row[i];
        m = fmax(m, x);
        if (x > best) { best = x; bi = (int)i; }             // wasm.rs:119: strict >, NaN never wins
        c_nan += x != x; c_ninf += x == FG_NEG_INF; c_pinf += x == INFINITY;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        m = fmax(m, __shfl_xor(m, o, FG_GRID_WAVE));
        const double ob = __shfl_xor(best, o, FG_GRID_WAVE);
        const int oi = __shfl_xor(bi, o, FG_GRID_WAVE);
        if (oi >= 0 && (bi < 0 || ob > best || (ob == best && oi < bi))) { best = ob; bi = oi; }
        c_nan += __shfl_xor(c_nan, o, FG_GRID_WAVE); c_ninf += __shfl_xor(c_ninf, o, FG_GRID_WAVE); c_pinf += __shfl_xor(c_pinf, o, FG_GRID_WAVE);
    }
    if (lane == 0) { red_m[wave] = m; red_v[wave] = best; red_i[wave] = bi; red_c[wave][0] = c_nan; red_c[wave][1] = c_ninf; red_c[wave][2] = c_pinf; }
    __syncthreads();
    m = FG_NEG_INF;
    for (int w = 0; w < n_waves; ++w) m = fmax(m, red_m[w]);
    double lse = FG_NEG_INF;
    if (m != FG_NEG_INF) {                                   // the same bits in every thread: a uniform branch
        double s = 0.0;
        for (unsigned i = (unsigned)tid; i < n_a; i += (unsigned)T) s += exp(row[i] - m);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, FG_GRID_WAVE);
        if (lane == 0) red_s[wave] = s;
        __syncthreads();
        double tot = 0.0;
        for (int w = 0; w < n_waves; ++w) tot += red_s[w];
        lse = tot == 0.0 ? FG_NEG_INF : m + log(tot);
    }
    if (tid == 0) {
        best = FG_NEG_INF; bi = -1; c_nan = c_ninf = c_pinf = 0;
        for (int w = 0; w < n_waves; ++w) {
            if (red_i[w] >= 0 && (bi < 0 || red_v[w] > best || (red_v[w] == best && red_i[w] < bi))) { best = red_v[w]; bi = red_i[w]; }
            c_nan += red_c[w][0]; c_ninf += red_c[w][1]; c_pinf += red_c[w][2];
        }
        lmb[ro] = lse;
        row_max[ro] = best;
        row_arg[ro] = bi < 0 ? -1LL : (long long)j * n_a + bi;
        row_cnt[3 * ro] = c_nan; row_cnt[3 * ro + 1] = c_ninf; row_cnt[3 * ro + 2] = c_pinf;
    }
}

// ---- log_norm, max, argmax and the counts of a base: one thread, rows in index order ----
__global__ void k_grid_final(int n_bases, unsigned n_b, const double *lmb, const double *row_max, const long long *row_arg, const int *row_cnt,
                             double *sum_f /*[bases][2]: log_norm, max*/, long long *sum_i /*[bases][4]: argmax, n_nan, n_neg_inf, n_pos_inf*/) {
    const int b = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= n_bases) return;
    const size_t ro = (size_t)b * n_b;
    double m = FG_NEG_INF, best = FG_NEG_INF;
    long long arg = -1, c_nan = 0, c_ninf = 0, c_pinf = 0;
    for (unsigned j = 0; j < n_b; ++j) {
        m = fmax(m, lmb[ro + j]);
        if (row_max[ro + j] > best) { best = row_max[ro + j]; arg = row_arg[ro + j]; }
        c_nan += row_cnt[3 * (ro + j)]; c_ninf += row_cnt[3 * (ro + j) + 1]; c_pinf += row_cnt[3 * (ro + j) + 2];
    }
    double ln = FG_NEG_INF;
    if (m != FG_NEG_INF) {
        double s = 0.0;
        for (unsigned j = 0; j < n_b; ++j) s += exp(lmb[ro + j] - m);
        ln = s == 0.0 ? FG_NEG_INF : m + log(s);
    }
    sum_f[2 * b] = ln; sum_f[2 * b + 1] = best;
    sum_i[4 * b] = arg; sum_i[4 * b + 1] = c_nan; sum_i[4 * b + 2] = c_ninf; sum_i[4 * b + 3] = c_pinf;
}

// ---- the mixture: one thread per cell, the chunk's bases of finite log_norm in arrival order ----
__global__ __launch_bounds__(FG_GRID_COL_THREADS) void k_grid_mix(const double *chunk, unsigned cells, int n_bases, const double *sum_f, double *mix) {
    const unsigned cell = blockIdx.x * (unsigned)FG_GRID_COL_THREADS + threadIdx.x;
    if (cell >= cells) return;
    double v = mix[cell];
    for (int b = 0; b < n_bases; ++b) {
        const double ln = sum_f[2 * b];
        if (fg_finite(ln)) v += exp(chunk[(size_t)b * cells + cell] - ln);
    }
    mix[cell] = v;
}

template <class T> static int grid_grow(T **p, size_t *cap, size_t want) {
    if (want <= *cap) return FG_OK;
    if (*p) { HIPCHK(hipFree(*p)); *p = nullptr; *cap = 0; }
    HIPCHK(hipMalloc((void **)p, want * sizeof(T)));
    *cap = want;
    return FG_OK;
}

struct fg_grid {
    fg_engine *e = nullptr;
    int site_a = -1, site_b = -1;
    FgGridPlan plan{};
    double *d_a = nullptr, *d_b = nullptr, *d_mix = nullptr;
    // scratch of one chunk, grown to the largest chunk met
    double *d_chunk = nullptr, *d_red = nullptr /* the per-base words of a chunk: n_a + n_b + 6 each */, *d_row_max = nullptr;
    long long *d_row_arg = nullptr; int *d_row_cnt = nullptr;
    size_t cap_chunk = 0, cap_red = 0, cap_row_max = 0, cap_row_arg = 0, cap_row_cnt = 0;
    // what is kept per base that has arrived: n_a + n_b + 6 words
    std::vector<double> log_norm, max, lma, lmb;
    std::vector<long long> argmax, counts;
    long long n_mixed = 0, n_skipped = 0;
    bool reduce = true;          // FG_GRID_REDUCE=0: score only, no base arrives (tools/bench_grid.py: the reductions' share of a call)
};

static int grid_need(const fg_grid *g, const char *who) {
    if (!g) { fg_set_error(std::string(who) + ": null grid"); return FG_E_BAD_ARG; }
    if (hipSetDevice(g->e->device) != hipSuccess) { fg_set_error("hipSetDevice failed"); return FG_E_HIP; }
    return FG_OK;
}
static int grid_need_bases(const fg_grid *g, const char *who) {
    if (g->log_norm.empty()) { fg_set_error(std::string(who) + ": no base has arrived (call fg_grid_eval first)"); return FG_E_STATE; }
    return FG_OK;
}

extern "C" {

int fg_grid_new(fg_engine *e, int site_a, int site_b, const double *h_a, int64_t n_a, const double *h_b, int64_t n_b, int64_t base_chunk, fg_grid **out) {
    if (!out) { fg_set_error("fg_grid_new: null out"); return FG_E_BAD_ARG; }
    *out = nullptr;
    NEED_ENGINE(e);
    const fg_program *p = e->prog;
    const bool two = site_b != -1;
    auto f64_site = [&](int s) { return s >= 0 && s < e->S && p->site_vtype[(size_t)s] == FG_F64; };
    if (!f64_site(site_a) || (two && !f64_site(site_b))) {                    // grid.rs:42-46
        auto name = [&](int s) { return s >= 0 && s < e->S ? p->stmts[(size_t)p->sorted_stmt[(size_t)s]].addr : "#" + std::to_string(s); };
        fg_set_error(two ? "sites `" + name(site_a) + "`/`" + name(site_b) + "` must be f64 sample sites of the model"
                         : "site `" + name(site_a) + "` must be an f64 sample site of the model");
        return FG_E_BAD_ARG;
    }
    if (!two) n_b = 1;
    FgGridPlan pl;
    if (int rc = fg_grid_plan(n_a, n_b, base_chunk, &pl)) {
        fg_set_error(rc == FG_E_LIMIT ? std::string("fg_grid_new: 2^31 cells or more") : std::string("fg_grid_new: n_a and n_b must be at least 1, base_chunk at least 0"));
        return rc;
    }
    if (!h_a || (two && !h_b)) { fg_set_error("fg_grid_new: null axis values"); return FG_E_BAD_ARG; }
    if (e->gt) { fg_set_error("fg_grid_new: the program's tile lives in global memory (beyond a CU's LDS): not supported by k_grid_eval"); return FG_E_LIMIT; }
    if (int rc = set_lds(k_grid_eval, e->lds_score)) return rc;
    fg_grid *g = new fg_grid();
    g->e = e; g->site_a = site_a; g->site_b = two ? site_b : -1; g->plan = pl;
    if (const char *rv = std::getenv("FG_GRID_REDUCE")) g->reduce = std::atoi(rv) != 0;
    auto fail = [&](const char *what) { fg_set_error(std::string("fg_grid_new: ") + what); fg_grid_free(g); return FG_E_HIP; };
    if (hipMalloc((void **)&g->d_a, (size_t)n_a * 8) != hipSuccess || hipMalloc((void **)&g->d_mix, (size_t)pl.cells * 8) != hipSuccess ||
        (two && hipMalloc((void **)&g->d_b, (size_t)n_b * 8) != hipSuccess)) return fail("no device memory for the axes and the mixture");
    if (hipMemcpyAsync(g->d_a, h_a, (size_t)n_a * 8, hipMemcpyHostToDevice, e->stream) != hipSuccess ||
        (two && hipMemcpyAsync(g->d_b, h_b, (size_t)n_b * 8, hipMemcpyHostToDevice, e->stream) != hipSuccess) ||
        hipMemsetAsync(g->d_mix, 0, (size_t)pl.cells * 8, e->stream) != hipSuccess || hipStreamSynchronize(e->stream) != hipSuccess) return fail("upload failed");
    *out = g;
    return FG_OK;
}

int fg_grid_eval(fg_grid *g, int64_t chain0, int64_t n_bases, double *d_out, double *d_acc) {
    if (int rc = grid_need(g, "fg_grid_eval")) return rc;
    fg_engine *e = g->e;
    if (fg_grid_check_bases(e->C, chain0, n_bases)) {
        fg_set_error("fg_grid_eval: bases [" + std::to_string(chain0) + ", " + std::to_string(chain0 + n_bases) + ") are not chains of the engine (" + std::to_string(e->C) + "), or none");
        return FG_E_BAD_ARG;
    }
    const FgGridPlan &pl = g->plan;
    const size_t cells = (size_t)pl.cells, n_a = (size_t)pl.n_a, n_b = (size_t)pl.n_b;
    const size_t most = (size_t)std::min<long long>(pl.base_chunk, n_bases);
    if (int rc = grid_grow(&g->d_chunk, &g->cap_chunk, most * cells)) return rc;
    if (int rc = grid_grow(&g->d_red, &g->cap_red, most * (n_a + n_b + 6))) return rc;
    if (int rc = grid_grow(&g->d_row_max, &g->cap_row_max, most * n_b)) return rc;
    if (int rc = grid_grow(&g->d_row_arg, &g->cap_row_arg, most * n_b)) return rc;
    if (int rc = grid_grow(&g->d_row_cnt, &g->cap_row_cnt, most * n_b * 3)) return rc;
    const int slot_a = e->prog->site_slot[(size_t)g->site_a], slot_b = g->site_b >= 0 ? e->prog->site_slot[(size_t)g->site_b] : -1;
    std::vector<double> red;                                   // one chunk's per-base words as they come back
    for (long long k = 0; k < fg_grid_n_chunks(pl, n_bases); ++k) {
        long long first, count;
        fg_grid_chunk(pl, n_bases, k, &first, &count);
        const size_t cnt = (size_t)count;
        // the chunk's per-base words, back to back so that one copy brings them: log_marg_a, log_marg_b, {log_norm, max}, {argmax, counts}
        double *d_lma = g->d_red, *d_lmb = d_lma + cnt * n_a, *d_sum_f = d_lmb + cnt * n_b;
        long long *d_sum_i = (long long *)(d_sum_f + cnt * 2);
        FgGridDev G = { g->d_a, g->d_b, slot_a, slot_b, (unsigned)pl.n_a, (unsigned)pl.cells, chain0 + first, g->d_chunk,
                        d_acc ? d_acc + (size_t)first * cells : nullptr, (long long)n_bases * pl.cells };
        hipLaunchKernelGGL(k_grid_eval, dim3(pl.waves, (unsigned)count), dim3(FG_WAVE), e->lds_score, e->stream, e->P, e->X, G);
        HIPCHK(hipGetLastError());
        if (d_out) HIPCHK(hipMemcpyAsync(d_out + (size_t)first * cells, g->d_chunk, cnt * cells * 8, hipMemcpyDeviceToDevice, e->stream));
        if (!g->reduce) { HIPCHK(hipStreamSynchronize(e->stream)); continue; }
        hipLaunchKernelGGL(k_grid_cols, dim3(pl.col_blocks, (unsigned)count), dim3(FG_GRID_COL_THREADS), 0, e->stream, (const double *)g->d_chunk, (unsigned)pl.n_a, (unsigned)pl.n_b, d_lma);
        hipLaunchKernelGGL(k_grid_rows, dim3((unsigned)pl.n_b, (unsigned)count), dim3((unsigned)pl.row_threads), 0, e->stream, (const double *)g->d_chunk, (unsigned)pl.n_a, (unsigned)pl.n_b,
                           d_lmb, g->d_row_max, g->d_row_arg, g->d_row_cnt);
        hipLaunchKernelGGL(k_grid_final, dim3((unsigned)((count + FG_WAVE - 1) / FG_WAVE)), dim3(FG_WAVE), 0, e->stream, (int)count, (unsigned)pl.n_b, (const double *)d_lmb,
                           (const double *)g->d_row_max, (const long long *)g->d_row_arg, (const int *)g->d_row_cnt, d_sum_f, d_sum_i);
        hipLaunchKernelGGL(k_grid_mix, dim3(pl.mix_blocks), dim3(FG_GRID_COL_THREADS), 0, e->stream, (const double *)g->d_chunk, (unsigned)pl.cells, (int)count, (const double *)d_sum_f, g->d_mix);
        HIPCHK(hipGetLastError());
        red.resize(cnt * (n_a + n_b + 6));
        HIPCHK(hipMemcpyAsync(red.data(), g->d_red, red.size() * 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));               // the next chunk overwrites the scratch; the bases count as arrived from here
        g->lma.insert(g->lma.end(), red.begin(), red.begin() + cnt * n_a);
        g->lmb.insert(g->lmb.end(), red.begin() + cnt * n_a, red.begin() + cnt * (n_a + n_b));
        const double *sf = red.data() + cnt * (n_a + n_b);
        long long si[4];
        for (size_t b = 0; b < cnt; ++b) {
            std::memcpy(si, sf + cnt * 2 + 4 * b, sizeof si);
            g->log_norm.push_back(sf[2 * b]); g->max.push_back(sf[2 * b + 1]);
            g->argmax.push_back(si[0]);
            for (int q = 1; q < 4; ++q) g->counts.push_back(si[q]);
            if (std::isfinite(sf[2 * b])) ++g->n_mixed; else ++g->n_skipped;
        }
    }
    return FG_OK;
}

int fg_grid_summary(fg_grid *g, double *h_log_norm, double *h_max, int64_t *h_argmax, int64_t *h_counts) {
    if (int rc = grid_need(g, "fg_grid_summary")) return rc;
    if (int rc = grid_need_bases(g, "fg_grid_summary")) return rc;
    const size_t n = g->log_norm.size();
    if (h_log_norm) std::memcpy(h_log_norm, g->log_norm.data(), n * 8);
    if (h_max) std::memcpy(h_max, g->max.data(), n * 8);
    if (h_argmax) for (size_t b = 0; b < n; ++b) h_argmax[b] = g->argmax[b];
    if (h_counts) for (size_t k = 0; k < 3 * n; ++k) h_counts[k] = g->counts[k];
    return FG_OK;
}

int fg_grid_marginals(fg_grid *g, double *h_log_marg_a, double *h_log_marg_b) {
    if (int rc = grid_need(g, "fg_grid_marginals")) return rc;
    if (int rc = grid_need_bases(g, "fg_grid_marginals")) return rc;
    const size_t n = g->log_norm.size();
    if (h_log_marg_a) std::memcpy(h_log_marg_a, g->lma.data(), n * (size_t)g->plan.n_a * 8);
    if (h_log_marg_b) std::memcpy(h_log_marg_b, g->lmb.data(), n * (size_t)g->plan.n_b * 8);
    return FG_OK;
}

int fg_grid_mixture(fg_grid *g, double *h_log_mix, int64_t *n_mixed, int64_t *n_skipped) {
    if (int rc = grid_need(g, "fg_grid_mixture")) return rc;
    if (int rc = grid_need_bases(g, "fg_grid_mixture")) return rc;
    if (h_log_mix) {
        const size_t cells = (size_t)g->plan.cells;
        HIPCHK(hipMemcpyAsync(h_log_mix, g->d_mix, cells * 8, hipMemcpyDeviceToHost, g->e->stream));
        HIPCHK(hipStreamSynchronize(g->e->stream));
        const double n = (double)g->n_mixed;
        for (size_t k = 0; k < cells; ++k) h_log_mix[k] = std::log(h_log_mix[k] / n);      // the read-out: ln(mix / n_mixed), NaN when no base was mixed
    }
    if (n_mixed) *n_mixed = g->n_mixed;
    if (n_skipped) *n_skipped = g->n_skipped;
    return FG_OK;
}

int64_t fg_grid_count(const fg_grid *g) { return g ? (int64_t)g->log_norm.size() : -1; }

void fg_grid_free(fg_grid *g) {
    if (!g) return;
    if (hipSetDevice(g->e->device) == hipSuccess) {
        if (g->e->stream) (void)hipStreamSynchronize(g->e->stream);
        for (void *p : { (void *)g->d_a, (void *)g->d_b, (void *)g->d_mix, (void *)g->d_chunk, (void *)g->d_red, (void *)g->d_row_max, (void *)g->d_row_arg,
                         (void *)g->d_row_cnt })
            if (p) (void)hipFree(p);
    }
    delete g;
}

}  // extern "C"
