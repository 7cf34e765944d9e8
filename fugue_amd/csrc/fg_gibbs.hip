// fg_gibbs.hip -- exact Gibbs moves of the discrete sites on the device.  hmc.rs:68-71 holds every discrete site at its prior draw and
// says "compose with `mh` to also move discrete sites"; k_gibbs_sweep is that move with the exact conditional in place of mh's blind
// proposal: for every chain and every listed site the trace is scored at each value of the site's finite support by the run that
// k_log_joint and k_grid_eval do, the scores are normalised, and the new value is drawn (fg_gibbs_plan.h: the rule, the orders, the
// refusals).  The conditional probabilities are summed per (cell, chain) and pooled over the chains by fg_chain_pool.h's
// fixed tree: the Rao-Blackwell estimate of P(site = value | data).
//
// One wave per 64 chains, lane = chain, the [n_slots][64] LDS tile of the scoring kernels; the whole sweep, all sites, is one launch and
// the tile stays in LDS between sites.  The program counter is wave-uniform: K and lo of a site come from the site table by uniform
// loads, every lane loops over the same candidates, and what differs per lane (a stuck site, the pick) is predicated.
#include "fg_engine_internal.h"
#include "fg_gibbs_plan.h"

struct FgGibbsSiteDev { int slot, K; long long lo, cell0; int site, pad; };

struct FgGibbsDev {
    const FgGibbsSiteDev *tab;   // [n_sites]
    int n_sites;
    uint32_t t;                  // the sweep index: the stream's iteration word
    double *work;                // [K_max][C]: the scores of the site in flight, then its weights
    double *prob_sum;            // [cells][C]
    double *scores, *cond;       // null, or the caller's [cells][C] (the call's last sweep)
    unsigned long long *counts;  // [n_sites][FG_GIBBS_COUNTS]
    const int *rec_slot;         // [n_rec] LDS slots of the recorded sites
    int n_rec;
    long long *rec;              // null, or this sweep's [n_rec][C]
};

__global__ __launch_bounds__(FG_WAVE, FG_MIN_WAVES) void k_gibbs_sweep(FgProgramDev P, FgChainCtx X, FgGibbsDev G) {
    extern __shared__ double lds_[];
    constexpr int tw = FG_WAVE;
    const long long chain = (long long)blockIdx.x * tw + threadIdx.x;
    const bool live = chain < X.C;
    const long long c = live ? chain : X.C - 1;              // dead lanes of the tail wave run the last chain and store nothing
    const size_t C = (size_t)X.C;
    double *slots = lds_ + threadIdx.x;
    fg_load_values(P, X, c, slots, tw);
    FgStream rng = fg_stream(X.seed, X.chain0 + (uint32_t)c, G.t, FG_RNG_GIBBS);
    for (int i = 0; i < G.n_sites; ++i) {
        const FgGibbsSiteDev s = G.tab[i];
        double *slot = slots + s.slot * tw;
        const long long old = fg_as_i64(*slot);
        double *work = G.work + (size_t)c;
        // 1. the scores: k_log_joint's run at every value of the support, the other sites as they are
        for (int k = 0; k < s.K; ++k) {
            *slot = fg_as_double(s.lo + k);
            FgAcc3 A = {0.0, 0.0, 0.0};
            fg_exec<FG_MODE_SCORE, false>(P.ins_fast, P.n_ins, P.pool, slots, tw, A, nullptr, nullptr, 0, live);
            if (live) work[(size_t)k * C] = fg_total(A);
        }
        const double u = fg_rng_u01(rng);                    // block i of the stream, whether the site is stuck or not
        if (live) {                                          // a dead lane's table column belongs to the last chain's own lane
            // 2. the maximum: NaN never wins
            double m = FG_NEG_INF;
            for (int k = 0; k < s.K; ++k) m = fmax(m, work[(size_t)k * C]);
            const bool stuck = m == FG_NEG_INF || m == INFINITY;
            // 3. the weights, their running sum, and the scores' read-out
            double T = 0.0;
            int n_nan = 0, n_ninf = 0, last = 0;
            for (int k = 0; k < s.K; ++k) {
                const double l = work[(size_t)k * C];
                const double w = l != l ? 0.0 : exp(l - m);
                n_nan += l != l; n_ninf += l == FG_NEG_INF;
                if (G.scores) G.scores[((size_t)s.cell0 + k) * C + c] = l;
                work[(size_t)k * C] = w;
                T = k == 0 ? w : T + w;
                if (w > 0.0) last = k;
            }
            int pick = -1;
            if (!stuck) {
                const double x = u * T;
                double run = 0.0;
                for (int k = 0; k < s.K; ++k) {
                    const double w = work[(size_t)k * C];
                    run = k == 0 ? w : run + w;
                    if (pick < 0 && x < run) pick = k;
                    const size_t o = ((size_t)s.cell0 + k) * C + c;
                    const double p = w / T;
                    G.prob_sum[o] += p;                      // one writer per word
                    if (G.cond) G.cond[o] = p;
                }
                if (pick < 0) pick = last;
                *slot = fg_as_double(s.lo + pick);
            } else {
                *slot = fg_as_double(old);
                if (G.cond) for (int k = 0; k < s.K; ++k) G.cond[((size_t)s.cell0 + k) * C + c] = NAN;
            }
            // 4. the counters: integers, one atomic per lane that has something to add
            unsigned long long *cnt = G.counts + (size_t)i * FG_GIBBS_COUNTS;
            if (!stuck && s.lo + pick != old) atomicAdd(cnt + 0, 1ull);
            if (stuck) atomicAdd(cnt + 1, 1ull);
            if (n_nan) atomicAdd(cnt + 2, (unsigned long long)n_nan);
            if (n_ninf) atomicAdd(cnt + 3, (unsigned long long)n_ninf);
        } else *slot = fg_as_double(old);
    }
    if (live) {
        for (int i = 0; i < G.n_sites; ++i) X.values[(size_t)G.tab[i].site * C + c] = fg_as_i64(slots[G.tab[i].slot * tw]);
        if (G.rec) for (int r = 0; r < G.n_rec; ++r) G.rec[(size_t)r * C + c] = fg_as_i64(slots[G.rec_slot[r] * tw]);
    }
}

struct fg_gibbs {
    fg_engine *e = nullptr;
    FgGibbsPlan plan;
    long long t = 0;             // the sweep index of the next sweep
    long long sweeps_run = 0;
    FgGibbsSiteDev *d_tab = nullptr;
    double *d_work = nullptr, *d_prob = nullptr;
    unsigned long long *d_counts = nullptr;
    double *tree[2] = { nullptr, nullptr };
    int *d_rec_slot = nullptr; std::vector<int> rec_slot;   // the LDS slots of the sites last recorded, on the device and as uploaded
};

static int gibbs_need(const fg_gibbs *g, const char *who) {
    if (!g || !g->e) { fg_set_error(std::string(who) + ": null handle"); return FG_E_BAD_ARG; }
    if (hipSetDevice(g->e->device) != hipSuccess) { fg_set_error("hipSetDevice failed"); return FG_E_HIP; }
    return FG_OK;
}
static int gibbs_counts(fg_gibbs *g, std::vector<unsigned long long> &h) {
    h.resize(g->plan.sites.size() * FG_GIBBS_COUNTS);
    HIPCHK(hipMemcpyAsync(h.data(), g->d_counts, h.size() * 8, hipMemcpyDeviceToHost, g->e->stream));
    HIPCHK(hipStreamSynchronize(g->e->stream));
    return FG_OK;
}

extern "C" {

int fg_gibbs_new(fg_engine *e, const int32_t *h_sites, int n_sites, fg_gibbs **out) {
    if (!out) { fg_set_error("fg_gibbs_new: null out"); return FG_E_BAD_ARG; }
    *out = nullptr;
    if (!e) { fg_set_error("fg_gibbs_new: null engine"); return FG_E_BAD_ARG; }
    const fg_program *p = e->prog;
    std::vector<FgGibbsSiteInfo> info((size_t)e->S);
    for (int j = 0; j < e->S; ++j) {
        FgGibbsSiteInfo &I = info[(size_t)j];
        I.name = p->stmts[(size_t)p->sorted_stmt[(size_t)j]].addr;
        I.vtype = p->site_vtype[(size_t)j];
        int64_t lo = 0, hi = -1;
        I.has_support = fg_program_site_support(p, j, &lo, &hi) == 1;
        I.lo = lo; I.hi = hi;
    }
    FgGibbsPlan pl;
    std::string err;
    if (int rc = fg_gibbs_plan(info, h_sites, n_sites, e->C, &pl, &err)) { fg_set_error(err); return rc; }
    if (e->gt) { fg_set_error("fg_gibbs_new: the program's tile lives in global memory (beyond a CU's LDS): not supported by k_gibbs_sweep"); return FG_E_LIMIT; }
    NEED_ENGINE(e);
    if (int rc = set_lds(k_gibbs_sweep, e->lds_score)) return rc;
    fg_gibbs *g = new fg_gibbs();
    g->e = e; g->plan = pl;
    std::vector<FgGibbsSiteDev> tab;
    for (const FgGibbsSite &s : pl.sites) tab.push_back(FgGibbsSiteDev{ p->site_slot[(size_t)s.site], s.K, s.lo, s.cell0, s.site, 0 });
    const size_t tree_words = (size_t)pl.n_cells * (size_t)pl.levels[0].m_out;
    if (dev_upload(&g->d_tab, tab) || dev_alloc(&g->d_work, pl.work_bytes / 8) || dev_alloc(&g->d_prob, pl.cell_bytes / 8) ||
        dev_alloc(&g->d_counts, tab.size() * FG_GIBBS_COUNTS) || dev_alloc(&g->tree[0], tree_words) || dev_alloc(&g->tree[1], tree_words)) {
        fg_gibbs_free(g);
        return FG_E_HIP;
    }
    *out = g;
    return FG_OK;
}

int fg_gibbs_n_sites(const fg_gibbs *g) {
    if (!g) { fg_set_error("fg_gibbs_n_sites: null handle"); return FG_E_BAD_ARG; }
    return (int)g->plan.sites.size();
}
int64_t fg_gibbs_n_cells(const fg_gibbs *g) { return g ? (int64_t)g->plan.n_cells : -1; }

int fg_gibbs_layout(const fg_gibbs *g, int32_t *h_site, int64_t *h_lo, int32_t *h_K, int64_t *h_cell0) {
    if (!g) { fg_set_error("fg_gibbs_layout: null handle"); return FG_E_BAD_ARG; }
    for (size_t i = 0; i < g->plan.sites.size(); ++i) {
        const FgGibbsSite &s = g->plan.sites[i];
        if (h_site) h_site[i] = s.site;
        if (h_lo) h_lo[i] = s.lo;
        if (h_K) h_K[i] = s.K;
        if (h_cell0) h_cell0[i] = s.cell0;
    }
    return FG_OK;
}

int fg_gibbs_sweep(fg_gibbs *g, int n_sweeps, const int32_t *h_rec_sites, int n_rec, int64_t *d_rec, double *d_scores, double *d_cond) {
    if (!g || !g->e) { fg_set_error("fg_gibbs_sweep: null handle"); return FG_E_BAD_ARG; }
    fg_engine *e = g->e;
    std::string err;
    if (int rc = fg_gibbs_check_sweeps(g->t, n_sweeps, &err)) { fg_set_error(err); return rc; }
    if (int rc = fg_gibbs_check_rec(e->S, h_rec_sites, n_rec, &err)) { fg_set_error(err); return rc; }
    if (d_rec && n_rec == 0) { fg_set_error("fg_gibbs_sweep: d_rec without recorded sites"); return FG_E_BAD_ARG; }
    if (int rc = gibbs_need(g, "fg_gibbs_sweep")) return rc;
    if (n_sweeps == 0) return FG_OK;
    const bool rec = d_rec != nullptr;
    if (rec) {                                                     // the slot list lives on the handle: a driver records the same sites every call
        std::vector<int> slot((size_t)n_rec);
        for (int r = 0; r < n_rec; ++r) slot[(size_t)r] = e->prog->site_slot[(size_t)h_rec_sites[r]];
        if (slot != g->rec_slot) {
            HIPCHK(hipStreamSynchronize(e->stream));               // a sweep in flight may still read the old list
            if (g->d_rec_slot) { HIPCHK(hipFree(g->d_rec_slot)); g->d_rec_slot = nullptr; g->rec_slot.clear(); }
            if (int rc = dev_upload(&g->d_rec_slot, slot)) return rc;
            g->rec_slot = slot;
        }
    }
    for (int k = 0; k < n_sweeps; ++k) {
        const bool last = k + 1 == n_sweeps;
        FgGibbsDev G = { g->d_tab, (int)g->plan.sites.size(), (uint32_t)g->t, g->d_work, g->d_prob, last ? d_scores : nullptr, last ? d_cond : nullptr,
                         g->d_counts, g->d_rec_slot, rec ? n_rec : 0, rec ? (long long *)d_rec + (size_t)k * (size_t)n_rec * (size_t)e->C : nullptr };
        hipLaunchKernelGGL(k_gibbs_sweep, dim3(g->plan.grid), dim3(FG_WAVE), e->lds_score, e->stream, e->P, e->X, G);
        HIPCHK(hipGetLastError());
        ++g->t; ++g->sweeps_run;
    }
    return fg_internal_rescore_sessions(e);
}

int64_t fg_gibbs_count(const fg_gibbs *g) { return g ? (int64_t)g->t : -1; }

int fg_gibbs_seek(fg_gibbs *g, int64_t t) {
    if (!g) { fg_set_error("fg_gibbs_seek: null handle"); return FG_E_BAD_ARG; }
    if (t < 0 || t > 0xffffffffLL) { fg_set_error("fg_gibbs_seek: the sweep index must lie in [0, 2^32)"); return FG_E_BAD_ARG; }
    g->t = t;
    return FG_OK;
}

int fg_gibbs_stats(fg_gibbs *g, int64_t *h_counts) {
    if (!g || !g->e || !h_counts) { fg_set_error("fg_gibbs_stats: null handle or output"); return FG_E_BAD_ARG; }
    if (int rc = gibbs_need(g, "fg_gibbs_stats")) return rc;
    std::vector<unsigned long long> h;
    if (int rc = gibbs_counts(g, h)) return rc;
    for (size_t k = 0; k < h.size(); ++k) h_counts[k] = (int64_t)h[k];
    return FG_OK;
}

int fg_gibbs_probs(fg_gibbs *g, double *h_mean, int64_t *h_n) {
    if (!g || !g->e) { fg_set_error("fg_gibbs_probs: null handle"); return FG_E_BAD_ARG; }
    if (g->sweeps_run == 0) { fg_set_error("fg_gibbs_probs: no sweep has run (call fg_gibbs_sweep first)"); return FG_E_STATE; }
    if (int rc = gibbs_need(g, "fg_gibbs_probs")) return rc;
    std::vector<unsigned long long> cnt;
    if (int rc = gibbs_counts(g, cnt)) return rc;
    std::vector<double> pooled;
    if (h_mean)
        if (int rc = fg_chain_pool_run<FgGibbsPool>(g->e->stream, g->plan.levels, g->plan.slices, g->d_prob, 0ll, g->tree, pooled)) return rc;
    for (size_t i = 0; i < g->plan.sites.size(); ++i) {
        const FgGibbsSite &s = g->plan.sites[i];
        const long long n = g->sweeps_run * g->plan.C - (long long)cnt[i * FG_GIBBS_COUNTS + 1];
        if (h_n) h_n[i] = n;
        if (h_mean) for (int k = 0; k < s.K; ++k) h_mean[(size_t)s.cell0 + k] = n > 0 ? pooled[(size_t)s.cell0 + k] / (double)n : NAN;
    }
    return FG_OK;
}

void fg_gibbs_free(fg_gibbs *g) {
    if (!g) return;
    if (g->e && hipSetDevice(g->e->device) == hipSuccess) {
        if (g->e->stream) (void)hipStreamSynchronize(g->e->stream);
        for (void *p : { (void *)g->d_tab, (void *)g->d_work, (void *)g->d_prob, (void *)g->d_counts, (void *)g->tree[0], (void *)g->tree[1], (void *)g->d_rec_slot })
            if (p) (void)hipFree(p);
    }
    delete g;
}

}  // extern "C"
