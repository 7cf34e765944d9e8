// fg_wpop_eval_plan.h -- predictive checks and WAIC / IS-LOO of a WEIGHTED population (fg_wpop_eval.hip): what the
// reference's workflows do after every sampler they have, SMC included (tests/end_to_end_workflows.rs:330-400 compares models,
// :650-745 checks replicated data), for the particles ABCSMCResult::weighted_mean (abc.rs:476) and the doc example (smc.rs:445-453)
// walk on the host.  Rows [rows][N], particle-fastest, stay on the device.  Plain C++ (no HIP, no engine): the device code and
// tests/cpp/wpop_eval_driver.cpp both call it, the latter with host loops in place of the kernels.
//
// Checks.  The statistics of a particle's data set, the cell conversion, the CSR list and the slot numbering are fg_ppc_stream_plan.h's
// (a population is one draw of N chains).  Per slot the particles fall into four CATEGORIES by the IEEE compare of T_rep(i) with T_obs
// (lt, eq, gt; -0.0 == +0.0) or nan (either side NaN); a particle adds its units q_i to exactly one category's u64 sum and, when
// q_i > 0, 1 to that category's element count.  Integers: the same whatever the order.  A slot's four sums must add up to T.  The
// moments of T_rep are fg_wpop_plan.h's, run on a scratch table [slots][N] the statistics are written to.
//
// Log-likelihood.  A particle takes part in a row iff its weight is good and > 0 (fg_wpe_weight; the moments' leaf rule without the
// cell).  Per row: counters of participating cells by kind; mx / mn the exact max / min of the finite participating cells; the pooled
// FgWpElem (W_fin, mean, ssd, n) of the leaves (fg_wp_leaf_weight: a non-finite cell is no leaf); and five sums over the same fixed
// tree (FgWpSumPool) of terms staged per particle, 0 where it is no leaf:
//   W2 = sum w^2     sp = sum w exp(x - mx)     sn = sum w exp(mn - x)     sn2 = sum (w exp(mn - x))^2     tmax = the exact max of sn's terms
// W, one number per handle: the sum of the participating weights whatever the cell, over the same tree.
#pragma once
#include "fg_loglik_stream_plan.h"
#include "fg_ppc_stream_plan.h"
#include "fg_wpop_plan.h"

#define FG_WPE_THREADS 256
#define FG_WPE_LT 0
#define FG_WPE_EQ 1
#define FG_WPE_GT 2
#define FG_WPE_NAN 3
// FG_WPOP_CATS (fugue_amd.h) = 4 categories per slot; FG_WLL_WORDS = 12 words and FG_WLL_COUNTS = 4 counters per row
enum { FG_WLL_W = 0, FG_WLL_W_FIN = 1, FG_WLL_W2 = 2, FG_WLL_MEAN = 3, FG_WLL_SSD = 4, FG_WLL_N_USED = 5, FG_WLL_MX = 6, FG_WLL_MN = 7, FG_WLL_SP = 8, FG_WLL_SN = 9,
       FG_WLL_SN2 = 10, FG_WLL_TMAX = 11 };
enum { FG_WLL_FIN = 0, FG_WLL_NEG_INF = 1, FG_WLL_POS_INF = 2, FG_WLL_NAN = 3 };
#define FG_WLL_STAGE 3               // staged words per (row, particle)
static_assert(FG_WLL_FIGURES == FG_LL_FIGURES, "fg_wll_finish writes its figures by the FG_LL_* indices of fg_loglik_stream_plan.h");

// ------------------------------------------------------------------ checks
FG_HD int fg_wpe_category(double T, double t_obs) {
    if (T != T || t_obs != t_obs) return FG_WPE_NAN;
    return T < t_obs ? FG_WPE_LT : (T == t_obs ? FG_WPE_EQ : FG_WPE_GT);
}

// the slots `n_checks` masks ask for, or FG_E_BAD_ARG
inline int fg_wpe_n_slots(int n_checks, const int32_t *stat_mask, std::string *err) {
    if (n_checks < 1 || !stat_mask) { if (err) *err = "fg_wpop_checks: no check"; return FG_E_BAD_ARG; }
    long long n = 0;
    for (int q = 0; q < n_checks; ++q) {
        if (stat_mask[q] <= 0 || stat_mask[q] >= (1 << FG_PPC_N_STATS)) { if (err) *err = "fg_wpop_checks: check " + std::to_string(q) + " has no statistic or a mask bit beyond the " + std::to_string(FG_PPC_N_STATS) + " statistics"; return FG_E_BAD_ARG; }
        n += __builtin_popcount((unsigned)stat_mask[q]);
    }
    if (n > 65535) { if (err) *err = "fg_wpop_checks: n_slots must lie in [1, 65535]"; return FG_E_BAD_ARG; }
    return (int)n;
}

// fg_ppc_init of one draw and N chains under this entry's name, with the limits of the weighted form
inline int fg_wpe_checks_init(FgPpcPlan &P, long long N, int n_rows, const int32_t *vtypes, int n_checks, const int32_t *offsets, const int32_t *members,
                              const int32_t *stat_mask, const double *observed, std::string *err) {
    if (n_rows < 1 || n_rows > 65535) { if (err) *err = "fg_wpop_checks: n_rows must lie in [1, 65535]"; return FG_E_BAD_ARG; }
    std::string e;
    const int rc = fg_ppc_init(P, 1, N, n_rows, vtypes, n_checks, offsets, members, stat_mask, observed, &e);
    if (rc) {                                                  // the same message under this entry's name
        const std::string theirs = "fg_ppc_stream_new: ";
        if (err) *err = "fg_wpop_checks: " + (e.compare(0, theirs.size(), theirs) == 0 ? e.substr(theirs.size()) : e);
        return rc;
    }
    if (P.n_slots > 65535) { if (err) *err = "fg_wpop_checks: n_slots must lie in [1, 65535]"; return FG_E_BAD_ARG; }
    return FG_OK;
}
// the CSR list the kernel reads: offsets [n_checks + 1] | mask [n_checks] | slot0 [n_checks] | members (fg_ppc_stream's layout)
inline std::vector<int32_t> fg_wpe_csr(const FgPpcPlan &P) {
    std::vector<int32_t> csr(P.offsets);
    csr.insert(csr.end(), P.mask.begin(), P.mask.end());
    csr.insert(csr.end(), P.slot0.begin(), P.slot0.end());
    csr.insert(csr.end(), P.members.begin(), P.members.end());
    return csr;
}
// slots of a slice: the scratch table [slots][N] stays within the moments' staging budget
inline long long fg_wpe_slot_rows(long long N, long long n_slots) { return fg_wp_moment_rows(N, n_slots); }
// the checks [q0, q1) that own a slot of [s0, s0 + ns)
inline void fg_wpe_slice_checks(const FgPpcPlan &P, long long s0, long long ns, int *q0, int *q1) {
    int a = 0, b = P.n_checks;
    while (a + 1 < P.n_checks && P.slot0[(size_t)a + 1] <= s0) ++a;
    while (b > a + 1 && P.slot0[(size_t)b - 1] >= s0 + ns) --b;
    *q0 = a; *q1 = b;
}
// FG_E_STATE when a slot's unit sums do not add up to T
inline int fg_wpe_checks_verify(int n_slots, const uint64_t *units /*[n_slots][4]*/, uint64_t T, std::string *err) {
    for (int k = 0; k < n_slots; ++k) {
        const uint64_t *u = units + 4 * (size_t)k;
        const uint64_t tot = u[0] + u[1] + u[2] + u[3];
        if (tot != T) {
            if (err) *err = "fg_wpop_checks: slot " + std::to_string(k) + " counted " + std::to_string(tot) + " units where the population holds " + std::to_string(T);
            return FG_E_STATE;
        }
    }
    return FG_OK;
}
// p_ge, p_gt, p_mid of a slot from its unit sums; integers first, one division each; a denominator of 0 gives NaN
inline void fg_wpe_p_values(const uint64_t *u /*[4]*/, double *p /*[3]*/) {
    const uint64_t den = u[FG_WPE_LT] + u[FG_WPE_EQ] + u[FG_WPE_GT];
    if (den == 0) { p[0] = p[1] = p[2] = fg_ppc_nan(); return; }
    p[0] = (double)(u[FG_WPE_GT] + u[FG_WPE_EQ]) / (double)den;
    p[1] = (double)u[FG_WPE_GT] / (double)den;
    p[2] = (double)(2 * u[FG_WPE_GT] + u[FG_WPE_EQ]) / (double)(2 * den);
}

// ------------------------------------------------------------------ log-likelihood
inline int fg_wll_check(long long n_sel, std::string *err) {
    if (n_sel < 1 || n_sel > 65535) { if (err) *err = "fg_wpop_loglik: n_sel must lie in [1, 65535]"; return FG_E_BAD_ARG; }
    return FG_OK;
}
// the weight a particle takes part with: w when good and above zero, else 0
FG_HD double fg_wpe_weight(double w) { return fg_wp_good(w) && w > 0.0 ? w : 0.0; }
FG_HD int fg_wll_kind(double x) { return x != x ? FG_WLL_NAN : (x == INFINITY ? FG_WLL_POS_INF : (x == -INFINITY ? FG_WLL_NEG_INF : FG_WLL_FIN)); }
// the staged terms of a particle with leaf weight lw (0: no leaf, every term +0.0)
FG_HD double fg_wll_w2_term(double lw) { return lw > 0.0 ? lw * lw : 0.0; }
FG_HD double fg_wll_sp_term(double lw, double x, double mx) { return lw > 0.0 ? lw * exp(x - mx) : 0.0; }
FG_HD double fg_wll_sn_term(double lw, double x, double mn) { return lw > 0.0 ? lw * exp(mn - x) : 0.0; }
// rows of a slice: FG_WLL_STAGE staged words per (row, particle), each word within the moments' budget
inline long long fg_wll_rows(long long N, long long n_sel) { return fg_wp_moment_rows(N, n_sel); }

// The figures of one row from its words and counters (fg_ll_finish's table with W in place of N; host std::log).
inline void fg_wll_finish(const double *w /*[FG_WLL_WORDS]*/, const int64_t *c /*[FG_WLL_COUNTS]*/, double *fig /*[FG_WLL_FIGURES]*/) {
    const double nan = std::nan(""), inf = INFINITY;
    const int64_t a = c[FG_WLL_NEG_INF], b = c[FG_WLL_POS_INF];
    if (c[FG_WLL_NAN] > 0 || c[FG_WLL_FIN] == 0) { for (int i = 0; i < FG_WLL_FIGURES; ++i) fig[i] = nan; return; }
    const double W = w[FG_WLL_W], Wf = w[FG_WLL_W_FIN];
    fig[FG_LL_LPPD] = b > 0 ? inf : w[FG_WLL_MX] + std::log(w[FG_WLL_SP] / W);
    fig[FG_LL_ELPD_LOO] = a > 0 ? -inf : w[FG_WLL_MN] - std::log(w[FG_WLL_SN] / W);
    fig[FG_LL_MEAN_LL] = a > 0 && b > 0 ? nan : (a > 0 ? -inf : (b > 0 ? inf : w[FG_WLL_MEAN]));
    const double den = Wf - w[FG_WLL_W2] / Wf;
    fig[FG_LL_P_WAIC] = a == 0 && b == 0 && w[FG_WLL_N_USED] >= 2.0 && den > 0.0 ? w[FG_WLL_SSD] / den : nan;
    fig[FG_LL_ELPD_WAIC] = fig[FG_LL_LPPD] - fig[FG_LL_P_WAIC];
    fig[FG_LL_P_LOO] = fig[FG_LL_LPPD] - fig[FG_LL_ELPD_LOO];
    fig[FG_LL_IS_ESS] = a == 0 ? w[FG_WLL_SN] * w[FG_WLL_SN] / w[FG_WLL_SN2] : nan;
    fig[FG_LL_MAX_WEIGHT] = a == 0 ? w[FG_WLL_TMAX] / w[FG_WLL_SN] : nan;
}
// the words of a row from what the passes left; FG_E_STATE when the tree's leaves are not the finite cells the counters saw
inline int fg_wll_words(double W, const FgWpElem &e, double W2, uint64_t mn_nkey, uint64_t mx_key, double sp, double sn, double sn2, uint64_t tmax_bits, const int64_t *c,
                        long long row, double *w, std::string *err) {
    if (e.n != c[FG_WLL_FIN]) {
        if (err) *err = "fg_wpop_loglik: row " + std::to_string(row) + " pooled " + std::to_string(e.n) + " leaves where " + std::to_string(c[FG_WLL_FIN]) + " finite cells take part";
        return FG_E_STATE;
    }
    const bool any = e.n > 0;
    w[FG_WLL_W] = W; w[FG_WLL_W_FIN] = e.W; w[FG_WLL_W2] = W2; w[FG_WLL_MEAN] = any ? e.mean : std::nan(""); w[FG_WLL_SSD] = any ? e.ssd : std::nan("");
    w[FG_WLL_N_USED] = (double)e.n;
    w[FG_WLL_MX] = any ? fg_qs_unkey(mx_key) : std::nan(""); w[FG_WLL_MN] = any ? fg_qs_unkey(~mn_nkey) : std::nan("");
    w[FG_WLL_SP] = sp; w[FG_WLL_SN] = sn; w[FG_WLL_SN2] = sn2;
    __builtin_memcpy(&w[FG_WLL_TMAX], &tmax_bits, 8);
    return FG_OK;
}
