// fg_gibbs_plan.h -- the host side of the exact Gibbs moves of the discrete sites (fg_gibbs.hip) ahead of their launches: the site table,
// the cells of the probability sums, the work table, the launch grid, the refusals, and the rule itself.
// Plain C++ (no HIP): tests/test_gibbs_cpu.py drives it through tests/cpp/gibbs_plan_driver.cpp under -fsanitize=address,undefined.
//
// hmc.rs:68-71 holds every discrete site at its prior draw and says "compose with `mh` to also move discrete sites"; this is that
// composition with the proposal replaced by the exact conditional, so every move is accepted.
//
// THE RULE (tests/gibbs_restatement.py restates it).  A handle owns an ordered list of sites g_0 .. g_{G-1}; site g_i has
// the support lo_i .. lo_i + K_i - 1 and the cells cell0_i .. cell0_i + K_i - 1 (cell0_0 = 0, cell0_{i+1} = cell0_i + K_i).  One sweep of
// chain c with sweep index t visits the sites in list order.  For site g_i:
//   1. l_k, k = 0 .. K_i - 1: the total log weight (prior + likelihood + factors in that order, fg_total) of the chain's trace with
//      g_i := lo_i + k, every other site at its current value (g_0 .. g_{i-1} at what this sweep has just given them), by the run
//      k_log_joint and k_grid_eval do: fg_exec<FG_MODE_SCORE, false> over P.ins_fast.  The candidate enters the site's LDS slot as
//      fg_load_values would have put it there: the 8-byte cell of the site's vtype (an integer; FG_BOOL 0 / 1), its bits read as a double.
//   2. m = the fmax fold of l_0, l_1, ... from -inf in index order (NaN never wins).  m = -inf or +inf: the site is STUCK -- it keeps
//      its value, `stuck` counts it, nothing is added to the probability sums (the conditional read-out of its cells is NaN).
//   3. w_k = exp(l_k - m) (ocml's exp), +0.0 for a NaN l_k; s_0 = w_0, s_k = s_{k-1} + w_k, T = s_{K-1} >= 1; p_k = w_k / T;
//      u = the first word of block i of the stream (seed, chain_offset + c, t, FG_RNG_GIBBS = 13), i.e. the (i + 1)-th fg_rng_u01;
//      x = u T (one rounding); pick = the smallest k with x < s_k, else the largest k with w_k > 0.  The slot takes lo_i + pick.
//   4. prob_sum[cell0_i + k][c] += p_k (one writer per word, sweeps in order); per site the integer counters moved (the pick differs
//      from the old value), stuck, nan_cells, neg_inf_cells (NaN / -inf scores among all K_i of every chain, stuck or not).
// After the last site the listed sites' cells go back to the engine's values.  Nothing depends on C, on the cut of the chains into
// engines (chain_offset), or on how many sweeps a call runs; there are no floating-point atomics.
// Read-out: prob_sum pooled over the chains by fg_chain_pool.h's fixed tree (FgGibbsPool: one double, a + b), divided by the
// contributing (sweep, chain) pairs of the cell's site = sweeps run x C - stuck.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "fg_chain_pool.h"

#define FG_GIBBS_WAVE 64
/* FG_GIBBS_K_CAP (4096 values of one site) and FG_GIBBS_COUNTS (4) are the header's: include/fugue_amd.h */
#define FG_GIBBS_MAX_GRID_X 0x7fffffffLL

struct FgGibbsSite { int site; int K; long long lo; long long cell0; };

// what the program says of one site: its address, its value type and, when has_support, the support [lo, hi] known from constants
struct FgGibbsSiteInfo { std::string name; int vtype = 0; int has_support = 0; long long lo = 0, hi = 0; };

struct FgGibbsPlan {
    std::vector<FgGibbsSite> sites;
    long long n_cells = 0;
    int K_max = 0;
    long long C = 0;
    unsigned grid = 0;                   // k_gibbs_sweep: waves of 64 chains
    size_t work_bytes = 0;               // the work table [K_max][C] of doubles
    size_t cell_bytes = 0;               // a table [n_cells][C] of doubles (prob_sum; the read-outs of the caller)
    std::vector<FgPoolLevel> levels;     // the pooling tree of prob_sum: items = cells
    std::vector<FgPoolSlice> slices;
};

// the values of a support, 0 when it is empty or has 2^63 values or more
inline unsigned long long fg_gibbs_support_size(long long lo, long long hi) {
    if (hi < lo) return 0;
    const unsigned long long span = (unsigned long long)hi - (unsigned long long)lo;
    return span >= 0x7fffffffffffffffULL ? 0 : span + 1;
}

// n_sites == 0: every site with a known support of at most FG_GIBBS_K_CAP values, in site order.  Else the sites of h_sites in that order.
// FG_E_BAD_ARG (the message names the site): n_sites < 0, a null list, a site outside [0, S), a site that is not discrete, a site without a
// finite constant support, a site listed twice, an empty resulting list, C < 1.  FG_E_LIMIT: a listed site with more than FG_GIBBS_K_CAP values.
inline int fg_gibbs_plan(const std::vector<FgGibbsSiteInfo> &info, const int32_t *h_sites, int n_sites, long long C, FgGibbsPlan *out, std::string *err) {
    auto fail = [&](int rc, const std::string &m) { if (err) *err = "fg_gibbs_new: " + m; return rc; };
    if (!out) return fail(FG_E_BAD_ARG, "null plan");
    if (n_sites < 0) return fail(FG_E_BAD_ARG, "n_sites < 0");
    if (n_sites > 0 && !h_sites) return fail(FG_E_BAD_ARG, "null site list");
    if (C < 1) return fail(FG_E_BAD_ARG, "no chains");
    const int S = (int)info.size();
    std::vector<int> list;
    if (n_sites == 0) {
        for (int j = 0; j < S; ++j) {
            const FgGibbsSiteInfo &I = info[(size_t)j];
            if (I.vtype == FG_F64 || !I.has_support) continue;
            const unsigned long long K = fg_gibbs_support_size(I.lo, I.hi);
            if (K >= 1 && K <= FG_GIBBS_K_CAP) list.push_back(j);
        }
        if (list.empty()) return fail(FG_E_BAD_ARG, "the model has no discrete site with a finite constant support of at most " + std::to_string(FG_GIBBS_K_CAP) + " values");
    } else list.assign(h_sites, h_sites + n_sites);
    FgGibbsPlan p;
    std::vector<unsigned char> seen((size_t)S, 0);
    for (int j : list) {
        if (j < 0 || j >= S) return fail(FG_E_BAD_ARG, "site #" + std::to_string(j) + " is outside [0, " + std::to_string(S) + ")");
        const FgGibbsSiteInfo &I = info[(size_t)j];
        if (I.vtype == FG_F64) return fail(FG_E_BAD_ARG, "site `" + I.name + "` is not a discrete site");
        const unsigned long long K = I.has_support ? fg_gibbs_support_size(I.lo, I.hi) : 0;
        if (K < 1) return fail(FG_E_BAD_ARG, "site `" + I.name + "` has no finite support known from constants");
        if (K > FG_GIBBS_K_CAP) return fail(FG_E_LIMIT, "site `" + I.name + "` has " + std::to_string(K) + " values, beyond " + std::to_string(FG_GIBBS_K_CAP));
        if (seen[(size_t)j]++) return fail(FG_E_BAD_ARG, "site `" + I.name + "` is listed twice");
        FgGibbsSite s;
        s.site = j; s.K = (int)K; s.lo = I.lo; s.cell0 = p.n_cells;
        p.sites.push_back(s);
        p.n_cells += (long long)K;
        if ((int)K > p.K_max) p.K_max = (int)K;
    }
    const long long waves = (C + FG_GIBBS_WAVE - 1) / FG_GIBBS_WAVE;
    if (waves > FG_GIBBS_MAX_GRID_X) return fail(FG_E_LIMIT, "2^37 chains or more");
    p.C = C;
    p.grid = (unsigned)waves;
    p.work_bytes = (size_t)p.K_max * (size_t)C * 8;
    p.cell_bytes = (size_t)p.n_cells * (size_t)C * 8;
    p.levels = fg_pool_levels(C);
    p.slices = fg_pool_slices(p.n_cells, FG_POOL_MAX_GRID_Y);
    *out = p;
    return FG_OK;
}
// the chain of (wave, lane) in k_gibbs_sweep, or -1 (a dead lane of the tail wave: clamped to the last chain, stores nothing)
inline long long fg_gibbs_chain(const FgGibbsPlan &p, unsigned wave, int lane) {
    const long long c = (long long)wave * FG_GIBBS_WAVE + lane;
    return c < p.C ? c : -1;
}
// the sites whose cells a call records after every sweep: any sites of the program, repeats allowed
inline int fg_gibbs_check_rec(int S, const int32_t *h_rec_sites, int n_rec, std::string *err) {
    if (n_rec < 0 || (n_rec > 0 && !h_rec_sites)) { if (err) *err = "fg_gibbs_sweep: n_rec < 0, or a null list of recorded sites"; return FG_E_BAD_ARG; }
    for (int r = 0; r < n_rec; ++r)
        if (h_rec_sites[r] < 0 || h_rec_sites[r] >= S) { if (err) *err = "fg_gibbs_sweep: recorded site #" + std::to_string(h_rec_sites[r]) + " is outside [0, " + std::to_string(S) + ")"; return FG_E_BAD_ARG; }
    return FG_OK;
}
// the sweep counter is the RNG's 32-bit iteration word: [t, t + n) must stay inside it
inline int fg_gibbs_check_sweeps(long long t, long long n, std::string *err) {
    if (n < 0) { if (err) *err = "fg_gibbs_sweep: n_sweeps < 0"; return FG_E_BAD_ARG; }
    if (t < 0 || t > 0xffffffffLL || n > 0x100000000LL - t) { if (err) *err = "fg_gibbs_sweep: the sweep index would pass 2^32"; return FG_E_LIMIT; }
    return FG_OK;
}

// prob_sum's pooling element: the sum of a cell's column over chains.  +0.0 is the identity of the sums met here (every term is >= +0.0).
struct FgGibbsPool {
    typedef double Elem;
    typedef double State;
    enum { WORDS = 1 };
    static FG_HD Elem empty() { return 0.0; }
    static FG_HD void state_load(State &s, const double *w, long long) { s = w[0]; }
    static FG_HD Elem leaf(const State &s) { return s; }
    static FG_HD Elem merge(const Elem &a, const Elem &b) { return a + b; }
    static FG_HD Elem elem_load(const double *w) { return w[0]; }
    static FG_HD void elem_store(const Elem &e, double *w) { w[0] = e; }
};
