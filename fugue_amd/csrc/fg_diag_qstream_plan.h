// fg_diag_qstream_plan.h -- the host side of the streamed quantile selector (fg_diag_qstream.hip): summarize_f64_parameter's
// sorted[round((len - 1) p)] (diagnostics.rs:355-371) of a run that is presented once per pass and never stored.  Plain C++ (no HIP,
// no engine): the device code and tests/cpp/qstream_driver.cpp both call it, the latter with host loops in place of the kernels.
//
// A slot is one (coordinate, probability).  Its state: b decided leading bits of the order-preserving key, their prefix (top-aligned,
// the undecided bits 0), the rank r among the elements that match the prefix, and their exact count m.  A pass presents all n_total
// draws.  At its start every live slot is put into a group of its coordinate -- slots with equal (b, prefix) share one -- and the
// group into a mode: COLLECT when m <= capacity (the pass appends every matching key to a buffer of `capacity` keys, the answer is
// the r-th smallest of them), HISTOGRAM otherwise (the pass counts the next w = min(digit_bits, 64 - b) bits of every matching key
// and keeps the smallest and largest matching key).  Every live slot takes part in every pass, so b is one number per pass.
// At the end of a pass the matching count of every group (histogram total / collect cursor) must be the m the previous pass left:
// a replay that did not reproduce the run is FG_E_STATE, never a quantile.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/fugue_amd.h"

#define FG_QS_MAX_PROBS 8
#define FG_QS_MAX_BITS 12
#define FG_QS_HIST 0
#define FG_QS_COLLECT 1

// ascending in the double's order: -0.0 just below +0.0, positive-sign NaN above +inf (fg_sort_key of fg_diag.hip)
inline uint64_t fg_qs_key(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
inline double fg_qs_unkey(uint64_t key) {
    const uint64_t u = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
    double v;
    std::memcpy(&v, &u, 8);
    return v;
}
// f64::round: half away from zero, as fg_diag_quantiles
inline uint64_t fg_qs_rank(uint64_t len, double p) { return (uint64_t)std::round((double)(len - 1) * p); }
// the leading b bits of key and prefix agree
inline bool fg_qs_match(uint64_t key, uint64_t prefix, int b) { return b == 0 || ((key ^ prefix) >> (64 - b)) == 0; }

struct FgQsSlot {
    int b = 0; uint64_t prefix = 0, r = 0, m = 0;
    bool done = false; uint64_t answer = 0; int passes = 0;     // passes: those the slot took part in
    int mode = FG_QS_HIST, group = -1;                          // of the current pass: the group's index within its coordinate and mode
};

struct FgQsPlan {
    int n_total = 0, d = 0, n_probs = 0, digit_bits = 0; int64_t capacity = 0; uint64_t len = 0;
    std::vector<FgQsSlot> slot;                                 // [d][n_probs]
    int count = 0, passes = 0; bool done = false, failed = false;
    // the current pass: decided bits, digit width, and per coordinate the groups of either mode ([d][n_probs], the first n_* used)
    int b = 0, w = 0;
    std::vector<uint64_t> hist_prefix, col_prefix;
    std::vector<int> n_hist, n_col;
    std::vector<uint64_t> hist_m, col_m;                        // the count every group must reach
};

// what a pass leaves, indexed like the plan's group tables: hist [d][n_probs][1 << w], mn / mx / cursor [d][n_probs]; keys
// [d * n_probs] vectors of the first min(cursor, capacity) collected keys of each collect group (reordered by the selection)
struct FgQsPassData {
    const uint64_t *hist = nullptr, *mn = nullptr, *mx = nullptr, *cursor = nullptr;
    std::vector<std::vector<uint64_t>> *keys = nullptr;
};

inline void fg_qs_begin_pass(FgQsPlan &P) {
    const int np = P.n_probs;
    P.count = 0;
    std::fill(P.n_hist.begin(), P.n_hist.end(), 0);
    std::fill(P.n_col.begin(), P.n_col.end(), 0);
    P.b = 0;
    for (const FgQsSlot &s : P.slot) if (!s.done) P.b = s.b;    // one value: every live slot has been through every pass
    P.w = std::min(P.digit_bits, 64 - P.b);
    for (int i = 0; i < P.d; ++i)
        for (int q = 0; q < np; ++q) {
            FgQsSlot &s = P.slot[(size_t)i * np + q];
            if (s.done) continue;
            s.mode = (int64_t)std::min<uint64_t>(s.m, (uint64_t)INT64_MAX) <= P.capacity ? FG_QS_COLLECT : FG_QS_HIST;
            std::vector<uint64_t> &pf = s.mode == FG_QS_COLLECT ? P.col_prefix : P.hist_prefix, &gm = s.mode == FG_QS_COLLECT ? P.col_m : P.hist_m;
            int &n = s.mode == FG_QS_COLLECT ? P.n_col[i] : P.n_hist[i];
            int g = 0;
            while (g < n && pf[(size_t)i * np + g] != s.prefix) ++g;
            if (g == n) { pf[(size_t)i * np + g] = s.prefix; gm[(size_t)i * np + g] = s.m; ++n; }
            s.group = g;
        }
}

// FG_E_BAD_ARG with *err set, or FG_OK and the first pass begun.  C: the chains of one draw.
inline int fg_qs_init(FgQsPlan &P, int n_total, long long C, int d, const double *probs, int n_probs, int digit_bits, int64_t capacity, std::string *err) {
    const char *bad = nullptr;
    if (n_total < 1) bad = "n_total < 1";
    else if (C < 1) bad = "no chains";
    else if (d < 1 || d > 65535) bad = "d must lie in [1, 65535]";
    else if (!probs || n_probs < 1 || n_probs > FG_QS_MAX_PROBS) bad = "n_probs must lie in [1, 8]";
    else if (digit_bits < 1 || digit_bits > FG_QS_MAX_BITS) bad = "digit_bits must lie in [1, 12]";
    else if (capacity < 0) bad = "capacity < 0";
    for (int q = 0; !bad && q < n_probs; ++q) if (!(probs[q] >= 0.0 && probs[q] <= 1.0)) bad = "probabilities must lie in [0, 1]";
    if (bad) { if (err) *err = std::string("fg_diag_qstream_new: ") + bad; return FG_E_BAD_ARG; }
    P = FgQsPlan();
    P.n_total = n_total; P.d = d; P.n_probs = n_probs; P.digit_bits = digit_bits; P.capacity = capacity;
    P.len = (uint64_t)n_total * (uint64_t)C;
    const size_t ns = (size_t)d * n_probs;
    P.slot.assign(ns, FgQsSlot());
    for (int i = 0; i < d; ++i)
        for (int q = 0; q < n_probs; ++q) { FgQsSlot &s = P.slot[(size_t)i * n_probs + q]; s.m = P.len; s.r = fg_qs_rank(P.len, probs[q]); }
    P.hist_prefix.assign(ns, 0); P.col_prefix.assign(ns, 0); P.hist_m.assign(ns, 0); P.col_m.assign(ns, 0);
    P.n_hist.assign(d, 0); P.n_col.assign(d, 0);
    fg_qs_begin_pass(P);
    return FG_OK;
}

// n_chunk more draws of the current pass: FG_E_STATE past n_total or once the selection is done (or has failed)
inline int fg_qs_take(FgQsPlan &P, int n_chunk, std::string *err) {
    if (n_chunk < 1) { if (err) *err = "fg_diag_qstream_update: n_chunk < 1"; return FG_E_BAD_ARG; }
    if (P.done || P.failed) { if (err) *err = P.done ? "fg_diag_qstream_update: every quantile is selected" : "fg_diag_qstream_update: the stream has failed its integrity check"; return FG_E_STATE; }
    if (n_chunk > P.n_total - P.count) {
        if (err) *err = "fg_diag_qstream_update: " + std::to_string(P.count) + " + " + std::to_string(n_chunk) + " draws pass n_total = " + std::to_string(P.n_total);
        return FG_E_STATE;
    }
    P.count += n_chunk;
    return FG_OK;
}

// may end_pass run?
inline int fg_qs_pass_complete(const FgQsPlan &P, std::string *err) {
    if (P.done || P.failed) { if (err) *err = P.done ? "fg_diag_qstream_end_pass: every quantile is selected" : "fg_diag_qstream_end_pass: the stream has failed its integrity check"; return FG_E_STATE; }
    if (P.count != P.n_total) {
        if (err) *err = "fg_diag_qstream_end_pass: " + std::to_string(P.count) + " of " + std::to_string(P.n_total) + " draws have arrived";
        return FG_E_STATE;
    }
    return FG_OK;
}

// The end of a pass: the integrity check of every group, then per slot the selection step.  Begins the next pass unless done.
inline int fg_qs_end_pass(FgQsPlan &P, const FgQsPassData &D, std::string *err) {
    int rc = fg_qs_pass_complete(P, err);
    if (rc) return rc;
    const int np = P.n_probs, nb = 1 << P.w;
    auto diverged = [&](int i, const char *what, uint64_t got, uint64_t want) {
        if (err) *err = "fg_diag_qstream_end_pass: pass " + std::to_string(P.passes + 1) + " did not reproduce the previous one: coordinate " + std::to_string(i) +
                        ", " + what + " " + std::to_string(got) + " where " + std::to_string(want) + " elements matched before";
        P.failed = true;
        return FG_E_STATE;
    };
    for (int i = 0; i < P.d; ++i) {
        for (int g = 0; g < P.n_hist[i]; ++g) {
            const uint64_t *h = D.hist + ((size_t)i * np + g) * nb;
            uint64_t tot = 0;
            for (int k = 0; k < nb; ++k) tot += h[k];
            if (tot != P.hist_m[(size_t)i * np + g]) return diverged(i, "histogram total", tot, P.hist_m[(size_t)i * np + g]);
        }
        for (int g = 0; g < P.n_col[i]; ++g) {
            const uint64_t cur = D.cursor[(size_t)i * np + g];
            if (cur != P.col_m[(size_t)i * np + g] || cur > (uint64_t)P.capacity || (*D.keys)[(size_t)i * np + g].size() != cur)
                return diverged(i, "collect cursor", cur, P.col_m[(size_t)i * np + g]);
        }
    }
    bool all = true;
    for (int i = 0; i < P.d; ++i)
        for (int q = 0; q < np; ++q) {
            FgQsSlot &s = P.slot[(size_t)i * np + q];
            if (s.done) continue;
            ++s.passes;
            const size_t gi = (size_t)i * np + s.group;
            if (s.mode == FG_QS_COLLECT) {
                std::vector<uint64_t> &k = (*D.keys)[gi];
                std::nth_element(k.begin(), k.begin() + (ptrdiff_t)s.r, k.end());
                s.answer = k[(size_t)s.r]; s.done = true;
                continue;
            }
            if (D.mn[gi] == D.mx[gi]) { s.answer = D.mn[gi]; s.done = true; continue; }       // 1. the bucket holds one value
            const uint64_t *h = D.hist + gi * nb;                                            // 2. the digit that holds rank r
            uint64_t cum = 0; int dg = 0;
            for (; dg < nb - 1; ++dg) { if (cum + h[dg] > s.r) break; cum += h[dg]; }
            s.r -= cum;
            s.prefix |= (uint64_t)dg << (64 - s.b - P.w);
            s.b += P.w;
            s.m = h[dg];
            if (s.b == 64) { s.answer = s.prefix; s.done = true; continue; }                 // 3. every bit is decided
            all = false;
        }
    ++P.passes;
    P.done = all;
    if (!all) fg_qs_begin_pass(P);
    return FG_OK;
}

// h_out [d][n_probs] doubles, h_slot_passes [d][n_probs] or NULL
inline int fg_qs_result(const FgQsPlan &P, double *h_out, int32_t *h_slot_passes, std::string *err) {
    if (!P.done) { if (err) *err = "fg_diag_qstream_result: " + std::to_string(P.passes) + " passes have ended and slots are still open"; return FG_E_STATE; }
    if (!h_out) return FG_E_BAD_ARG;
    for (size_t k = 0; k < P.slot.size(); ++k) {
        h_out[k] = fg_qs_unkey(P.slot[k].answer);
        if (h_slot_passes) h_slot_passes[k] = P.slot[k].passes;
    }
    return FG_OK;
}
