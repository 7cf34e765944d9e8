// fg_wpop_plan.h -- the summary of a WEIGHTED population (fg_wpop.hip): what the reference leaves to ABCSMCResult::weighted_mean
// (abc.rs:476) and to the doc example that walks the particles by hand (smc.rs:445-453), for rows x [d][N] and normalised weights
// w [N] that stay on the device.  Plain C++ (no HIP, no engine): the device code and tests/cpp/wpop_driver.cpp both call it, the
// latter with host loops in place of the kernels.  DESIGN 3.18.
//
// Units.  q_i = (uint64) rint(w_i 2^52) (half to even) for 0 <= w_i <= 1; any other weight (NaN, negative, above 1, infinite) is BAD:
// q_i = 0, counted in n_bad.  n_zero: the good weights of zero units.  T = sum q_i, kept as the two sums of the high and low 32 bits,
// so a population that is not normalised (T >= 2^53) is an error instead of a wrapped integer.  Quantiles and tables are sums of units:
// integers, the same whatever the order of the additions.  An element of zero units takes no part in either.
//
// Quantile of p: t = min(T, max(1, ceil(p (double)T))), the answer the smallest value v of the row with sum_{key(x_j) <= key(v)} q_j >= t
// (fg_qs_key's order).  An inverse weighted CDF -- NOT the reference's sorted[round((len - 1) p)] of equal weights.  T == 0: NaN.
// Found by radix select: a SLOT is one (row, probability); its state the b decided leading key bits, their prefix, the target t
// inside the bucket, and the bucket's element count m and units u.  Live slots of a row with equal prefix share a GROUP; a group
// with m <= capacity COLLECTS its (key, units) pairs, any other counts the next w = min(digit_bits, 64 - b) bits: units and elements
// per digit, the smallest and largest key.  Before a step the totals of a group must be the (m, u) the previous pass left: FG_E_STATE.
//
// Moments use the doubles w_i over fg_chain_pool.h's fixed tree on the particle index (FgWpPool), then a plain sum over the same
// tree (FgWpSumPool) of (w_i (x_i - mean))^2 for the Monte Carlo error.  Both pools read leaves STAGED as [2][rows][N] / [1][rows][N].
#pragma once
#include <math.h>

#include <utility>

#include "fg_chain_pool.h"
#include "fg_diag_cstream_plan.h"
#include "fg_diag_qstream_plan.h"

#define FG_WP_UNIT_SCALE 4503599627370496.0   // 2^52
#define FG_WP_THREADS 256
#define FG_WP_BLOCKS 2048                     // blocks of a launch, over all groups / rows
#define FG_WP_MAX_ITERS ((1ll << 24) - 1)     // elements a thread takes of a launch: a block sees fewer than 2^32 (its u32 LDS counts cannot wrap)
#define FG_WP_MAX_GROUPS 1024                 // groups of a quantile pass: rows are taken max(1, 1024 / n_probs) at a time
#define FG_WP_STAGE_WORDS (1ll << 24)         // staged leaves of a moments slice, per word
// FG_WPOP_MOMENTS (fugue_amd.h) = 6 doubles per row: W, mean, var, std, mcse, n_used

FG_HD bool fg_wp_good(double w) { return w >= 0.0 && w <= 1.0; }
FG_HD uint64_t fg_wp_units(double w) { return fg_wp_good(w) ? (uint64_t)rint(w * FG_WP_UNIT_SCALE) : 0ull; }
// fg_qs_key, for host and device
FG_HD uint64_t fg_wp_key(double v) {
    uint64_t u;
    __builtin_memcpy(&u, &v, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
FG_HD bool fg_wp_match(uint64_t key, uint64_t prefix, int b) { return b == 0 || ((key ^ prefix) >> (64 - b)) == 0; }

inline int fg_wp_new_check(long long n, std::string *err) {
    if (n < 1) { if (err) *err = "fg_wpop_new: n < 1"; return FG_E_BAD_ARG; }
    return FG_OK;
}
inline int fg_wp_m_check(long long d, std::string *err) {
    if (d < 1 || d > 65535) { if (err) *err = "fg_wpop_moments: d must lie in [1, 65535]"; return FG_E_BAD_ARG; }
    return FG_OK;
}
// T from the sums of the units' high and low halves (each below 2^32 N); FG_E_BAD_ARG at 2^53 and above
inline int fg_wp_total(uint64_t sum_hi, uint64_t sum_lo, uint64_t *T, std::string *err) {
    const uint64_t hi = sum_hi + (sum_lo >> 32);
    if (hi >= (1ull << 21)) { if (err) *err = "fg_wpop_new: the weights are not normalised: their units sum to 2^53 or more"; return FG_E_BAD_ARG; }
    *T = (hi << 32) | (sum_lo & 0xffffffffull);
    return FG_OK;
}

// ------------------------------------------------------------------ moments
struct FgWpElem { double W = 0.0, mean = 0.0, ssd = 0.0; int64_t n = 0; };    // n: the leaves below (n == 0: the empty element)
struct FgWpState { double w, x; };

// the staged leaf weight: w_i where the particle counts (good weight above zero, finite cell), else 0
FG_HD double fg_wp_leaf_weight(double w, double x) { return fg_wp_good(w) && w > 0.0 && x - x == 0.0 ? w : 0.0; }
// the staged term of the second pass
FG_HD double fg_wp_mcse_term(double lw, double x, double mean) {
    if (!(lw > 0.0)) return 0.0;
    const double u = lw * (x - mean);
    return u * u;
}

struct FgWpPool {
    typedef FgWpElem Elem;
    typedef FgWpState State;
    enum { WORDS = 4 };
    static FG_HD Elem empty() { return Elem(); }
    static FG_HD void state_load(State &s, const double *w, long long stride) { s.w = w[0]; s.x = w[stride]; }
    static FG_HD Elem leaf(const State &s) {
        Elem e;
        if (!(s.w > 0.0)) return e;
        e.W = s.w; e.mean = s.x; e.n = 1;
        return e;
    }
    // fg_moments_merge with weights in place of counts; regroup nothing
    static FG_HD Elem merge(const Elem &a, const Elem &b) {
        if (a.n == 0) return b;
        if (b.n == 0) return a;
        Elem r;
        const double W = a.W + b.W, delta = b.mean - a.mean;
        r.W = W;
        r.mean = a.mean + delta * (b.W / W);
        r.ssd = a.ssd + b.ssd + delta * delta * (a.W * b.W / W);
        r.n = a.n + b.n;
        return r;
    }
    static FG_HD void elem_store(const Elem &e, double *w) { w[0] = e.W; w[1] = e.mean; w[2] = e.ssd; __builtin_memcpy(w + 3, &e.n, 8); }
    static FG_HD Elem elem_load(const double *w) { Elem e; e.W = w[0]; e.mean = w[1]; e.ssd = w[2]; __builtin_memcpy(&e.n, w + 3, 8); return e; }
};

// a sum of terms >= +0.0 over the same tree (+0.0 is the empty element: a + 0.0 == a for every such a, bit for bit)
struct FgWpSumPool {
    typedef double Elem;
    typedef double State;
    enum { WORDS = 1 };
    static FG_HD Elem empty() { return 0.0; }
    static FG_HD void state_load(State &s, const double *w, long long) { s = w[0]; }
    static FG_HD Elem leaf(const State &s) { return s; }
    static FG_HD Elem merge(const Elem &a, const Elem &b) { return a + b; }
    static FG_HD void elem_store(const Elem &e, double *w) { w[0] = e; }
    static FG_HD Elem elem_load(const double *w) { return w[0]; }
};

// rows of a moments slice: as many as keep the staged leaves within FG_WP_STAGE_WORDS per word, at least one, at most the grid's y
inline long long fg_wp_moment_rows(long long N, long long d) {
    return std::max<long long>(1, std::min<long long>(std::min<long long>(d, FG_POOL_MAX_GRID_Y), FG_WP_STAGE_WORDS / std::max<long long>(N, 1)));
}
// W, mean, var, std, mcse, n_used from the pooled element and the pooled second-pass sum
inline void fg_wp_finish(const FgWpElem &e, double s2, double *out) {
    const double nan = std::nan("");
    out[5] = (double)e.n;
    if (e.n == 0) { out[0] = 0.0; out[1] = out[2] = out[3] = out[4] = nan; return; }
    out[0] = e.W; out[1] = e.mean;
    out[2] = e.ssd / e.W;
    out[3] = std::sqrt(out[2]);
    out[4] = std::sqrt(s2) / e.W;
}

// ------------------------------------------------------------------ quantiles
struct FgWpSlot {
    int b = 0; uint64_t prefix = 0, t = 0, m = 0, u = 0;
    bool done = false, none = false; uint64_t answer = 0; int passes = 0;   // none: T == 0, the quantile is NaN
    int mode = FG_QS_HIST, group = -1;
};
struct FgWpGroup { int row = 0; uint64_t prefix = 0, m = 0, u = 0, off = 0; };   // off (collect): of its pairs in the pass's pair buffer

struct FgWpQPlan {
    int d = 0, n_probs = 0, digit_bits = 0; int64_t capacity = 0;
    std::vector<FgWpSlot> slot;                                 // [d][n_probs]
    int b = 0, w = 0, passes = 0; bool done = false, failed = false;
    std::vector<FgWpGroup> hist, col;                           // of the current pass
    uint64_t col_pairs = 0;                                     // pairs the collect groups hold together
};
typedef std::vector<std::pair<uint64_t, uint64_t>> FgWpPairs;    // (key, units)
// what a pass leaves: units and elements per digit [n_hist][1 << w], mn / mx [n_hist], cursor [n_col], pairs [n_col]
struct FgWpPassData {
    const uint64_t *units = nullptr, *elems = nullptr, *mn = nullptr, *mx = nullptr, *cursor = nullptr;
    std::vector<FgWpPairs> *pairs = nullptr;
};

inline int fg_wp_q_check(long long d, const double *probs, int n_probs, int digit_bits, int64_t capacity, std::string *err) {
    const char *bad = nullptr;
    if (d < 1 || d > 65535) bad = "d must lie in [1, 65535]";
    else if (!probs || n_probs < 1 || n_probs > FG_QS_MAX_PROBS) bad = "n_probs must lie in [1, 8]";
    else if (digit_bits < 1 || digit_bits > FG_QS_MAX_BITS) bad = "digit_bits must lie in [1, 12]";
    else if (capacity < 0) bad = "capacity < 0";
    for (int q = 0; !bad && q < n_probs; ++q) if (!(probs[q] >= 0.0 && probs[q] <= 1.0)) bad = "probabilities must lie in [0, 1]";
    if (bad) { if (err) *err = std::string("fg_wpop_quantiles: ") + bad; return FG_E_BAD_ARG; }
    return FG_OK;
}
inline uint64_t fg_wp_target(uint64_t T, double p) {
    const double c = std::ceil(p * (double)T);
    const uint64_t t = c < 1.0 ? 1ull : (uint64_t)c;
    return std::min(T, t);
}

inline void fg_wp_begin_pass(FgWpQPlan &P) {
    const int np = P.n_probs;
    P.hist.clear(); P.col.clear(); P.col_pairs = 0;
    P.b = 0;
    for (const FgWpSlot &s : P.slot) if (!s.done) P.b = s.b;    // one value: every live slot has been through every pass
    P.w = std::min(P.digit_bits, 64 - P.b);
    for (int i = 0; i < P.d; ++i)
        for (int q = 0; q < np; ++q) {
            FgWpSlot &s = P.slot[(size_t)i * np + q];
            if (s.done) continue;
            s.mode = (int64_t)std::min<uint64_t>(s.m, (uint64_t)INT64_MAX) <= P.capacity ? FG_QS_COLLECT : FG_QS_HIST;
            std::vector<FgWpGroup> &G = s.mode == FG_QS_COLLECT ? P.col : P.hist;
            int g = (int)G.size() - 1;                          // the groups of row i are the tail of the list
            while (g >= 0 && G[(size_t)g].row == i && G[(size_t)g].prefix != s.prefix) --g;
            if (g < 0 || G[(size_t)g].row != i) {
                FgWpGroup n;
                n.row = i; n.prefix = s.prefix; n.m = s.m; n.u = s.u;
                if (s.mode == FG_QS_COLLECT) { n.off = P.col_pairs; P.col_pairs += s.m; }
                g = (int)G.size();
                G.push_back(n);
            }
            s.group = g;
        }
}

// rows [0, d) of a population of T units on n_live elements of non-zero units; the arguments have passed fg_wp_q_check
inline void fg_wp_q_init(FgWpQPlan &P, int d, const double *probs, int n_probs, int digit_bits, int64_t capacity, uint64_t T, uint64_t n_live) {
    P = FgWpQPlan();
    P.d = d; P.n_probs = n_probs; P.digit_bits = digit_bits; P.capacity = capacity;
    P.slot.assign((size_t)d * n_probs, FgWpSlot());
    for (int i = 0; i < d; ++i)
        for (int q = 0; q < n_probs; ++q) {
            FgWpSlot &s = P.slot[(size_t)i * n_probs + q];
            if (T == 0) { s.done = s.none = true; continue; }
            s.m = n_live; s.u = T; s.t = fg_wp_target(T, probs[q]);
        }
    P.done = T == 0;
    if (!P.done) fg_wp_begin_pass(P);
}

// The end of a pass: the integrity check of every group, then per slot the selection step.  Begins the next pass unless done.
inline int fg_wp_end_pass(FgWpQPlan &P, const FgWpPassData &D, std::string *err) {
    if (P.done || P.failed) { if (err) *err = "fg_wpop_quantiles: no pass is open"; return FG_E_STATE; }
    const int np = P.n_probs, nb = 1 << P.w;
    auto diverged = [&](const FgWpGroup &g, const char *what, uint64_t elems, uint64_t units) {
        if (err) *err = "fg_wpop_quantiles: pass " + std::to_string(P.passes + 1) + " did not reproduce the previous one: row " + std::to_string(g.row) + ", " + what + " " +
                        std::to_string(elems) + " elements of " + std::to_string(units) + " units where " + std::to_string(g.m) + " of " + std::to_string(g.u) + " matched before";
        P.failed = true;
        return FG_E_STATE;
    };
    for (size_t g = 0; g < P.hist.size(); ++g) {
        uint64_t ne = 0, nu = 0;
        for (int k = 0; k < nb; ++k) { ne += D.elems[g * nb + k]; nu += D.units[g * nb + k]; }
        if (ne != P.hist[g].m || nu != P.hist[g].u) return diverged(P.hist[g], "histogram totals", ne, nu);
    }
    for (size_t g = 0; g < P.col.size(); ++g) {
        FgWpPairs &pr = (*D.pairs)[g];
        uint64_t nu = 0;
        for (const auto &kq : pr) nu += kq.second;
        if (D.cursor[g] != P.col[g].m || pr.size() != D.cursor[g] || nu != P.col[g].u) return diverged(P.col[g], "collected", D.cursor[g], nu);
        std::sort(pr.begin(), pr.end());                       // by key; pairs of one key are one value
    }
    bool all = true;
    for (int i = 0; i < P.d; ++i)
        for (int q = 0; q < np; ++q) {
            FgWpSlot &s = P.slot[(size_t)i * np + q];
            if (s.done) continue;
            ++s.passes;
            const size_t g = (size_t)s.group;
            if (s.mode == FG_QS_COLLECT) {
                uint64_t cum = 0;
                for (const auto &kq : (*D.pairs)[g]) { cum += kq.second; if (cum >= s.t) { s.answer = kq.first; break; } }
                s.done = true;                                  // cum reaches u >= t: the totals were checked above
                continue;
            }
            if (D.mn[g] == D.mx[g]) { s.answer = D.mn[g]; s.done = true; continue; }          // 1. the bucket holds one value
            const uint64_t *hu = D.units + g * nb, *he = D.elems + g * nb;                    // 2. the first digit that reaches t
            uint64_t cum = 0; int dg = 0;
            for (; dg < nb - 1; ++dg) { if (cum + hu[dg] >= s.t) break; cum += hu[dg]; }
            s.t -= cum;
            s.prefix |= (uint64_t)dg << (64 - s.b - P.w);
            s.b += P.w;
            s.m = he[dg]; s.u = hu[dg];
            if (s.b == 64) { s.answer = s.prefix; s.done = true; continue; }                  // 3. every bit is decided
            all = false;
        }
    ++P.passes;
    P.done = all;
    if (!all) fg_wp_begin_pass(P);
    return FG_OK;
}

// h_out [d][n_probs] doubles, h_passes [d][n_probs] or NULL: the passes each slot took part in
inline void fg_wp_q_result(const FgWpQPlan &P, double *h_out, int32_t *h_passes) {
    for (size_t k = 0; k < P.slot.size(); ++k) {
        h_out[k] = P.slot[k].none ? std::nan("") : fg_qs_unkey(P.slot[k].answer);
        if (h_passes) h_passes[k] = P.slot[k].passes;
    }
}

// blocks along x of a launch over N elements that runs `rows` grid rows: a share of FG_WP_BLOCKS, no more than the elements need,
// no fewer than keep a thread within FG_WP_MAX_ITERS
inline unsigned fg_wp_blocks(long long N, long long rows) {
    long long nb = std::max<long long>(1, FG_WP_BLOCKS / std::max<long long>(rows, 1));
    nb = std::min(nb, (N + FG_WP_THREADS - 1) / FG_WP_THREADS);
    const long long per = FG_WP_THREADS * FG_WP_MAX_ITERS;
    nb = std::max(nb, (N + per - 1) / per);
    return (unsigned)std::max<long long>(nb, 1);
}

// ------------------------------------------------------------------ tables
// The rows' forms, keys and counter offsets are fg_diag_cstream_plan.h's (a row of cells [N] is a chunk of one draw and N chains);
// the counter table holds units: units [B] | below [n_rows] | above [n_rows] | mn (as ~key under max) | mx (key under max).
inline int fg_wp_c_init(FgCsPlan &P, long long N, int n_rows, const int32_t *vtypes, const int64_t *lo, const int32_t *bins, std::string *err) {
    if (n_rows < 1 || n_rows > 65535) { if (err) *err = "fg_wpop_counts: n_rows must lie in [1, 65535]"; return FG_E_BAD_ARG; }
    std::vector<int32_t> rows((size_t)n_rows);
    for (int k = 0; k < n_rows; ++k) rows[(size_t)k] = k;
    std::string e;
    const int rc = fg_cs_init(P, 1, N, n_rows, rows.data(), vtypes, lo, bins, n_rows, FG_CS_FORCE_WIDE, &e);
    if (rc && err) *err = "fg_wpop_counts: " + e.substr(e.find(": ") + 2);
    return rc;
}
// FG_E_STATE when a row's units do not add up to T
inline int fg_wp_c_result(const FgCsPlan &P, const uint64_t *ctr, uint64_t T, uint64_t *h_units, uint64_t *h_below, uint64_t *h_above, int64_t *h_min, int64_t *h_max,
                          std::string *err) {
    const size_t nw = (size_t)P.n_watch;
    const uint64_t *below = ctr + P.n_bins, *above = below + nw, *mn = above + nw, *mx = mn + nw;
    for (size_t k = 0; k < nw; ++k) {
        const FgCsRow &r = P.rows[k];
        uint64_t tot = below[k] + above[k];
        for (int j = 0; j < r.bins; ++j) tot += ctr[r.off + (size_t)j];
        if (tot != T) {
            if (err) *err = "fg_wpop_counts: row " + std::to_string(k) + " counted " + std::to_string(tot) + " units where the population holds " + std::to_string(T);
            return FG_E_STATE;
        }
    }
    std::memcpy(h_units, ctr, P.n_bins * 8);
    for (size_t k = 0; k < nw; ++k) {
        h_below[k] = below[k]; h_above[k] = above[k];
        const bool any = T > 0;                                  // min / max over the cells of non-zero units; 0 without one
        h_min[k] = any ? (int64_t)(~mn[k] ^ P.rows[k].flip) : 0;
        h_max[k] = any ? (int64_t)(mx[k] ^ P.rows[k].flip) : 0;
    }
    return FG_OK;
}
