// fg_ppc_stream_plan.h -- the posterior predictive check stream (fg_ppc_stream.hip): the replicate table d_yrep [n][n_rows][C] that
// fg_predict_eval writes, handed over one chunk at a time and never stored, reduced to test statistics of every replicated data set
// and compared with the observed ones (the last step of the reference's workflows: tests/end_to_end_workflows.rs:650-745,
// tests/inference_integration.rs:717-740, examples/bayesian_coin_flip.rs:211-).  Plain C++ (no HIP, no engine): the
// device code, the host (for T_obs) and tests/cpp/ppc_stream_driver.cpp run the functions below, the last with host loops in place
// of the kernels.
//
// A CHECK is a group of K >= 1 rows of the table (its members, in the order given) and an observed vector y[K]; a SLOT is a (check,
// statistic) pair the caller asked for through the check's 5-bit mask, numbered in check order, then in statistic order.  Per
// (slot, chain) the stream keeps FG_PPC_WORDS 8-byte words, stored [word][n_slots][C], all zero at creation:
//   0 n_lt | n_eq << 32      1 n_gt | n_nan << 32      (u32 counters of T_rep <, ==, > T_obs and of NaN draws: n_total < 2^31)
//   2 n_fin                  3 pivot, the first finite T_rep            4 s1 = sum (T - pivot)            5 s2 = sum (T - pivot)^2
// State size: 48 bytes per (slot, chain) -- 3.1 MB per slot at C = 65 536, 16 GB for a five-statistic check of each of 1 024 observe
// statements: a model with that many selects the checks it needs.  A column has one writer and is walked in draw order, so the state
// after a run does not depend on the chunking, bit for bit.  The pivoted sums are k_diag_stream_update's.
//
// Read-out: counters pool over chains by integer addition and the moments by (n, mean, ssd) merges, along fg_chain_pool.h's fixed tree
// on the chain index, FgPpcPool its elements.
#pragma once
#include <math.h>
#include <stdint.h>

#include <cmath>

#include "fg_chain_pool.h"

#if defined(__HIPCC__)
#define FG_PPC_UNROLL _Pragma("unroll 8")   // the member loads of several iterations in flight; the sums stay in member order
#else
#define FG_PPC_UNROLL
#endif
#define FG_PPC_WORDS 6               // state words per (slot, chain)
#define FG_PPC_ELEM 7                // a tree element in memory: n, mean, ssd, then n_lt, n_eq, n_gt, n_nan as int64 bits
#define FG_PPC_THREADS 256           // of the statistics and the update kernel
#define FG_PPC_SCRATCH_DRAWS 16      // draws whose statistics the scratch table holds: a longer chunk is walked in pieces of that many
#define FG_PPC_COPY 0                // conversion of a member's cells, as fg_diag_cells_f64: f64 bits copied
#define FG_PPC_UNSIGNED 1            // (double)(uint64_t)
#define FG_PPC_SIGNED 2              // (double)(int64_t): bool, usize, i64

// one cell as a double: `x as f64` by the row's value type (diagnostics.rs:153-191, fg_diag_cells_f64)
FG_HD double fg_ppc_cell(uint64_t v, int how) {
    if (how == FG_PPC_COPY) { double x; __builtin_memcpy(&x, &v, 8); return x; }
    return how == FG_PPC_UNSIGNED ? (double)v : (double)(int64_t)v;
}

FG_HD double fg_ppc_nan() { const uint64_t q = 0x7ff8000000000000ull; double x; __builtin_memcpy(&x, &q, 8); return x; }

// The five statistics of one data set of K members, cell(i) the i-th member as a double, in member order (every product and sum is
// rounded: -ffp-contract=off).  mean: the in-order sum onto +0.0 over (double)K (end_to_end_workflows.rs:700-703); var: a second
// in-order pass of (x - mean)(x - mean) onto +0.0 over (double)(K - 1) (:720-726; K = 1 is 0/0 = NaN), left out when !want_var
// (T[FG_PPC_VAR] is NaN then); min / max from the first member by x < m ? x : m, x > m ? x : m; sum: the in-order sum (the number of
// heads of Bernoulli rows, bayesian_coin_flip.rs:211-).  A NaN member makes all five NaN wherever it sits; every NaN that comes out
// is the one quiet NaN 0x7ff8000000000000.
template <class Cell>
FG_HD void fg_ppc_stats(int K, Cell cell, bool want_var, double *T /*[FG_PPC_N_STATS]*/) {
    double x = cell(0);
    double sum = 0.0 + x, mn = x, mx = x;
    bool nan = x != x;
    FG_PPC_UNROLL
    for (int i = 1; i < K; ++i) {
        x = cell(i);
        sum += x;
        mn = x < mn ? x : mn;
        mx = x > mx ? x : mx;
        nan = nan || x != x;
    }
    const double mean = sum / (double)K;
    double var = fg_ppc_nan();
    if (want_var) {
        double ss = 0.0;
        FG_PPC_UNROLL
        for (int i = 0; i < K; ++i) { const double d = cell(i) - mean; ss += d * d; }
        var = ss / (double)(K - 1);
    }
    T[FG_PPC_MEAN] = mean; T[FG_PPC_VAR] = var; T[FG_PPC_MIN] = mn; T[FG_PPC_MAX] = mx; T[FG_PPC_SUM] = sum;
    for (int i = 0; i < FG_PPC_N_STATS; ++i) if (nan || T[i] != T[i]) T[i] = fg_ppc_nan();
}

struct FgPpcState {                  // a (slot, chain) column while a chunk is walked
    uint32_t n_lt, n_eq, n_gt, n_nan;
    uint64_t n_fin;
    double pivot, s1, s2;
};

FG_HD void fg_ppc_state_load(FgPpcState &s, const double *w, long long stride) {
    uint64_t a, b;                                             // the counter words hold integer bits
    __builtin_memcpy(&a, w, 8); __builtin_memcpy(&b, w + stride, 8); __builtin_memcpy(&s.n_fin, w + 2 * stride, 8);
    s.n_lt = (uint32_t)a; s.n_eq = (uint32_t)(a >> 32); s.n_gt = (uint32_t)b; s.n_nan = (uint32_t)(b >> 32);
    s.pivot = w[3 * stride]; s.s1 = w[4 * stride]; s.s2 = w[5 * stride];
}
FG_HD void fg_ppc_state_store(const FgPpcState &s, double *w, long long stride) {
    const uint64_t a = (uint64_t)s.n_lt | ((uint64_t)s.n_eq << 32), b = (uint64_t)s.n_gt | ((uint64_t)s.n_nan << 32);
    __builtin_memcpy(w, &a, 8); __builtin_memcpy(w + stride, &b, 8); __builtin_memcpy(w + 2 * stride, &s.n_fin, 8);
    w[3 * stride] = s.pivot; w[4 * stride] = s.s1; w[5 * stride] = s.s2;
}

// one draw's statistic T against the slot's observed one.  A NaN on either side counts in n_nan and in none of lt / eq / gt
// (-0.0 == +0.0; infinities compare as IEEE compares them); a finite T enters the pivoted sums whatever T_obs is -- the mean and
// spread of the replicated statistic do not depend on the data.
FG_HD void fg_ppc_update(FgPpcState &s, double T, double t_obs) {
    if (T != T || t_obs != t_obs) ++s.n_nan;
    else if (T < t_obs) ++s.n_lt;
    else if (T == t_obs) ++s.n_eq;
    else ++s.n_gt;
    if (T != T || T == INFINITY || T == -INFINITY) return;
    if (s.n_fin == 0) { s.pivot = T; s.s1 = 0.0; s.s2 = 0.0; }
    const double d = T - s.pivot;
    s.s1 += d; s.s2 += d * d; s.n_fin += 1;
}

struct FgPpcElem {                   // a tree element: a chain, or chains pooled
    FgMoments m;                     // of the finite draws
    int64_t n_lt = 0, n_eq = 0, n_gt = 0, n_nan = 0;
};

struct FgPpcPool {
    typedef FgPpcElem Elem;
    typedef FgPpcState State;
    enum { WORDS = FG_PPC_ELEM };
    static FG_HD Elem empty() { return Elem(); }
    static FG_HD void state_load(State &s, const double *w, long long stride) { fg_ppc_state_load(s, w, stride); }
    // a chain as a tree leaf
    static FG_HD Elem leaf(const State &s) {
        Elem e;
        e.m = fg_moments_leaf((double)s.n_fin, s.pivot, s.s1, s.s2);
        e.n_lt = (int64_t)s.n_lt; e.n_eq = (int64_t)s.n_eq; e.n_gt = (int64_t)s.n_gt; e.n_nan = (int64_t)s.n_nan;
        return e;
    }
    // element i takes in element i + s: counters add, the moments merge
    static FG_HD Elem merge(const Elem &a, const Elem &b) {
        Elem r;
        r.m = fg_moments_merge(a.m, b.m);
        r.n_lt = a.n_lt + b.n_lt; r.n_eq = a.n_eq + b.n_eq; r.n_gt = a.n_gt + b.n_gt; r.n_nan = a.n_nan + b.n_nan;
        return r;
    }
    static FG_HD void elem_store(const Elem &e, double *w) {
        w[0] = e.m.n; w[1] = e.m.mean; w[2] = e.m.ssd;
        __builtin_memcpy(w + 3, &e.n_lt, 8); __builtin_memcpy(w + 4, &e.n_eq, 8); __builtin_memcpy(w + 5, &e.n_gt, 8); __builtin_memcpy(w + 6, &e.n_nan, 8);
    }
    static FG_HD Elem elem_load(const double *w) {
        Elem e;
        e.m.n = w[0]; e.m.mean = w[1]; e.m.ssd = w[2];
        __builtin_memcpy(&e.n_lt, w + 3, 8); __builtin_memcpy(&e.n_eq, w + 4, 8); __builtin_memcpy(&e.n_gt, w + 5, 8); __builtin_memcpy(&e.n_nan, w + 6, 8);
        return e;
    }
};

// ------------------------------------------------------------------ host side

struct FgPpcPlan {
    FgDraws draws;
    int n_rows = 0, n_checks = 0, n_slots = 0, scratch_draws = 0;
    long long C = 0, max_grid_y = FG_POOL_MAX_GRID_Y;
    std::vector<int32_t> offsets;                             // [n_checks + 1] into members
    std::vector<int32_t> members;                             // row << 2 | conversion, the CSR list the statistics kernel reads
    std::vector<int32_t> mask, slot0;                         // [n_checks]: the statistics asked for, the check's first slot
    std::vector<double> t_obs;                                // [n_slots]: fg_ppc_stats of the observed vectors
    std::vector<FgPoolLaunch> launches;                       // chain ranges of every statistics / update launch
    std::vector<FgPoolLevel> levels;                          // of the pooling tree
    std::vector<FgPoolSlice> slices;                          // slot ranges of an update launch and of every tree level
};

inline size_t fg_ppc_state_words(const FgPpcPlan &P) { return (size_t)FG_PPC_WORDS * (size_t)P.n_slots * (size_t)P.C; }
inline size_t fg_ppc_scratch_words(const FgPpcPlan &P) { return (size_t)P.scratch_draws * (size_t)P.n_slots * (size_t)P.C; }
inline long long fg_ppc_tree_elems(const FgPpcPlan &P) { return P.levels.empty() ? 1 : P.levels[0].m_out; }

inline int fg_ppc_how(int vtype) {
    return vtype == FG_F64 ? FG_PPC_COPY : vtype == FG_U64 ? FG_PPC_UNSIGNED : (vtype == FG_BOOL || vtype == FG_USIZE || vtype == FG_I64) ? FG_PPC_SIGNED : -1;
}

// max_grid_x / max_grid_y: the tests pass small ones to see the cuts
inline int fg_ppc_init(FgPpcPlan &P, int n_total, long long C, int n_rows, const int32_t *vtypes, int n_checks, const int32_t *offsets, const int32_t *members,
                       const int32_t *stat_mask, const double *observed, std::string *err, long long max_grid_x = FG_POOL_MAX_GRID_X,
                       long long max_grid_y = FG_POOL_MAX_GRID_Y) {
    std::string bad;
    if (n_total < 1) bad = "n_total < 1";
    else if (C < 1) bad = "no chains";
    else if (n_rows < 1 || n_rows >= (1 << 29)) bad = "n_rows outside [1, 2^29)";
    else if (n_checks < 1) bad = "no check";
    else if (!vtypes || !offsets || !members || !stat_mask || !observed) bad = "a null table";
    else if (max_grid_x < 1 || max_grid_y < 1) bad = "a grid limit below 1";
    else if (offsets[0] != 0) bad = "offsets[0] is not 0";
    for (int r = 0; bad.empty() && r < n_rows; ++r)
        if (fg_ppc_how(vtypes[r]) < 0) bad = "unknown value type " + std::to_string(vtypes[r]) + " of row " + std::to_string(r);
    for (int q = 0; bad.empty() && q < n_checks; ++q) {
        if (offsets[q + 1] < offsets[q]) bad = "offsets decrease at check " + std::to_string(q);
        else if (offsets[q + 1] == offsets[q]) bad = "check " + std::to_string(q) + " is empty";
        else if (stat_mask[q] == 0) bad = "check " + std::to_string(q) + " asks for no statistic";
        else if (stat_mask[q] < 0 || stat_mask[q] >= (1 << FG_PPC_N_STATS)) bad = "check " + std::to_string(q) + " has a mask bit beyond the " + std::to_string(FG_PPC_N_STATS) + " statistics";
        for (int i = offsets[q]; bad.empty() && i < offsets[q + 1]; ++i)
            if (members[i] < 0 || members[i] >= n_rows) bad = "member " + std::to_string(i) + " names row " + std::to_string(members[i]) + " outside [0, n_rows)";
    }
    if (!bad.empty()) { if (err) *err = "fg_ppc_stream_new: " + bad; return FG_E_BAD_ARG; }
    P = FgPpcPlan();
    P.draws.n_total = n_total; P.n_rows = n_rows; P.n_checks = n_checks; P.C = C; P.max_grid_y = max_grid_y;
    P.scratch_draws = std::min(n_total, FG_PPC_SCRATCH_DRAWS);
    P.offsets.assign(offsets, offsets + n_checks + 1);
    for (int q = 0; q < n_checks; ++q) {
        P.mask.push_back(stat_mask[q]);
        P.slot0.push_back(P.n_slots);
        const int o0 = offsets[q], K = offsets[q + 1] - o0;
        for (int i = 0; i < K; ++i) P.members.push_back((int32_t)(((uint32_t)members[o0 + i] << 2) | (uint32_t)fg_ppc_how(vtypes[members[o0 + i]])));
        double T[FG_PPC_N_STATS];
        fg_ppc_stats(K, [&](int i) { return observed[o0 + i]; }, (stat_mask[q] >> FG_PPC_VAR) & 1, T);
        for (int st = 0; st < FG_PPC_N_STATS; ++st)
            if ((stat_mask[q] >> st) & 1) { P.t_obs.push_back(T[st]); ++P.n_slots; }
    }
    P.launches = fg_pool_launches(C, FG_PPC_THREADS, max_grid_x);
    P.levels = fg_pool_levels(C);
    P.slices = fg_pool_slices(P.n_slots, max_grid_y);
    return FG_OK;
}

// the (draw, check) pairs of a piece of n_piece draws, cut at the grid limit: pair p is draw p / n_checks, check p % n_checks
inline std::vector<FgPoolSlice> fg_ppc_pair_slices(const FgPpcPlan &P, int n_piece) { return fg_pool_slices((long long)n_piece * P.n_checks, P.max_grid_y); }

// a pooled element as the read-out hands it over: counts lt eq gt nan fin, moments mean ssd (NaN without a finite draw)
inline void fg_ppc_finish(const FgPpcElem &e, int64_t *counts /*[5]*/, double *moments /*[2]*/) {
    counts[0] = e.n_lt; counts[1] = e.n_eq; counts[2] = e.n_gt; counts[3] = e.n_nan; counts[4] = (int64_t)e.m.n;
    moments[0] = e.m.n == 0.0 ? fg_ppc_nan() : e.m.mean;
    moments[1] = e.m.n == 0.0 ? fg_ppc_nan() : e.m.ssd;
}
