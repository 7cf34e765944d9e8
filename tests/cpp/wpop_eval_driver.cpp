// wpop_eval_driver.cpp -- fg_wpop_eval_plan.h without a GPU: host loops stand where fg_wpop_eval.hip has kernels (the statistics and
// the unit sums of a check, the staged leaves and terms of a log-likelihood row, the counters and the key min / max), everything else
// -- the argument checks, the CSR list, the slices, the pools and the tree, the integrity rule, the finish step -- is the plan
// headers' own code.  tests/test_wpop_eval_cpu.py builds it with g++ (and once more under AddressSanitizer / UBSan) and compares its
// output with tests/wpop_eval_restatement.py.
//
//   wpop_eval_driver N w.f64 n_rows cells.u64|- vtypes offsets members masks observed n_sel ll.f64|- [slot_rows ll_rows]
// prints  units T n_bad n_zero | slot k <t_obs hex> <4 unit sums> <4 counts> <6 moment hex words> <3 p-value hex words> |
//         ll k <8 figure hex words> <12 word hex words> <4 counts> <index of the largest sn term, -1 without one>   and exits 0;
// or  error <code> <message>  and exits 2.  slot_rows / ll_rows (0: the plan's) cut the slices elsewhere: the output must not change.
// WPOP_EVAL_DRIVER_CORRUPT=1 in the environment drops one unit of slot 0 before the integrity rule.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <sstream>

#include "../../fugue_amd/csrc/fg_wpop_eval_plan.h"

static int fail(int rc, const std::string &msg) { std::printf("error %d %s\n", rc, msg.c_str()); return 2; }
static uint64_t bits(double v) { uint64_t u; std::memcpy(&u, &v, 8); return u; }

template <typename T>
static bool read_file(const char *path, std::vector<T> &out, size_t n) {
    out.assign(n, T());
    FILE *f = std::fopen(path, "rb");
    if (!f) return false;
    const size_t got = std::fread(out.data(), sizeof(T), n, f);
    std::fclose(f);
    return got == n;
}
static std::vector<int32_t> ints_of(const char *text) {
    std::vector<int32_t> out;
    std::stringstream ss(text);
    std::string item;
    while (std::getline(ss, item, ',')) if (!item.empty()) out.push_back((int32_t)std::strtoll(item.c_str(), nullptr, 10));
    return out;
}
static std::vector<double> doubles_of(const char *text) {
    std::vector<double> out;
    std::stringstream ss(text);
    std::string item;
    while (std::getline(ss, item, ',')) if (!item.empty()) out.push_back(std::strtod(item.c_str(), nullptr));
    return out;
}

// fg_wpop_moments of rows x [d][N] as tests/cpp/wpop_driver.cpp runs it: k_wpop_leaves, the tree, k_wpop_terms, the tree again
static void moments_rows(const double *x, const std::vector<double> &w, long long N, long long d, double *out) {
    const std::vector<FgPoolLevel> levels = fg_pool_levels(N);
    const long long rows_per = fg_wp_moment_rows(N, d);
    for (long long r0 = 0; r0 < d; r0 += rows_per) {
        const long long rows = std::min(rows_per, d - r0);
        const std::vector<FgPoolSlice> slices = fg_pool_slices(rows, FG_POOL_MAX_GRID_Y);
        std::vector<double> st((size_t)(2 * rows * N));
        for (long long k = 0; k < rows; ++k)
            for (long long i = 0; i < N; ++i) {
                const double xi = x[(size_t)((r0 + k) * N + i)];
                st[(size_t)(k * N + i)] = fg_wp_leaf_weight(w[(size_t)i], xi);
                st[(size_t)((rows + k) * N + i)] = xi;
            }
        const std::vector<FgWpElem> e1 = fg_pool_host<FgWpPool>(levels, slices, st.data(), rows * N);
        for (long long k = 0; k < rows; ++k) {
            const double mu = e1[(size_t)k].n ? e1[(size_t)k].mean : std::nan("");
            for (long long i = 0; i < N; ++i) st[(size_t)(k * N + i)] = fg_wp_mcse_term(st[(size_t)(k * N + i)], st[(size_t)((rows + k) * N + i)], mu);
        }
        const std::vector<double> e2 = fg_pool_host<FgWpSumPool>(levels, slices, st.data(), 0);
        for (long long k = 0; k < rows; ++k) fg_wp_finish(e1[(size_t)k], e2[(size_t)k], out + (r0 + k) * FG_WPOP_MOMENTS);
    }
}

int main(int argc, char **argv) {
    if (argc != 12 && argc != 14) {
        std::fprintf(stderr, "usage: wpop_eval_driver N w.f64 n_rows cells.u64|- vtypes offsets members masks observed n_sel ll.f64|- [slot_rows ll_rows]\n");
        return 1;
    }
    const long long N = std::atoll(argv[1]);
    const int n_rows = std::atoi(argv[3]), n_sel = std::atoi(argv[10]);
    const bool do_checks = std::string(argv[4]) != "-", do_ll = std::string(argv[11]) != "-";
    const long long slot_rows = argc == 14 ? std::atoll(argv[12]) : 0, ll_rows = argc == 14 ? std::atoll(argv[13]) : 0;
    std::string err;
    if (int rc = fg_wp_new_check(N, &err)) return fail(rc, err);
    // the order of the ABI: fg_wpop_new, then the argument checks of fg_wpop_checks and fg_wpop_loglik, before anything is read
    FgPpcPlan P;
    if (do_checks) {
        const std::vector<int32_t> vt = ints_of(argv[5]), off = ints_of(argv[6]), mem = ints_of(argv[7]), mask = ints_of(argv[8]);
        const std::vector<double> obs = doubles_of(argv[9]);
        const int n_checks = (int)mask.size();
        const int32_t no_member = 0;                                           // an empty list is still a list: the plan names the empty check
        const double no_value = 0.0;
        const bool sized = n_rows >= 1 && (size_t)n_rows == vt.size() && off.size() == (size_t)n_checks + 1 && mem.size() == obs.size() && !off.empty() &&
                           (size_t)std::max(0, off.back()) <= mem.size();
        const int ns = fg_wpe_n_slots(n_checks, mask.data(), &err);
        if (ns < 0) return fail(ns, err);
        if (int rc = fg_wpe_checks_init(P, N, n_rows, sized ? vt.data() : nullptr, n_checks, sized ? off.data() : nullptr, sized ? (mem.empty() ? &no_member : mem.data()) : nullptr,
                                        sized ? mask.data() : nullptr, sized ? (obs.empty() ? &no_value : obs.data()) : nullptr, &err))
            return fail(rc, err);
        if (ns != P.n_slots) return fail(FG_E_STATE, "fg_wpop_checks_n_slots disagrees with the plan");
    }
    if (do_ll) if (int rc = fg_wll_check(n_sel, &err)) return fail(rc, err);
    std::vector<double> w;
    if (!read_file(argv[2], w, (size_t)N)) { std::fprintf(stderr, "cannot read the weights\n"); return 1; }

    // ---- k_wpop_units
    std::vector<uint64_t> q((size_t)N);
    uint64_t n_bad = 0, n_zero = 0, hi = 0, lo32 = 0, T = 0;
    for (long long i = 0; i < N; ++i) {
        const bool good = fg_wp_good(w[(size_t)i]);
        const uint64_t u = fg_wp_units(w[(size_t)i]);
        q[(size_t)i] = u;
        n_bad += good ? 0 : 1; n_zero += good && u == 0 ? 1 : 0; hi += u >> 32; lo32 += u & 0xffffffffull;
    }
    if (int rc = fg_wp_total(hi, lo32, &T, &err)) return fail(rc, err);
    std::printf("units %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", T, n_bad, n_zero);

    // ---- fg_wpop_checks: per slice of slots k_wpe_checks as loops over (check, particle), then the moments of the scratch table
    if (do_checks) {
        std::vector<uint64_t> cells;
        if (!read_file(argv[4], cells, (size_t)n_rows * (size_t)N)) { std::fprintf(stderr, "cannot read the cells\n"); return 1; }
        const std::vector<int32_t> csr = fg_wpe_csr(P);
        const int nc = P.n_checks;
        const long long n_slots = P.n_slots, per = slot_rows > 0 ? slot_rows : fg_wpe_slot_rows(N, n_slots);
        std::vector<uint64_t> units((size_t)n_slots * 4, 0);
        std::vector<int64_t> counts((size_t)n_slots * 4, 0);
        std::vector<double> mom((size_t)n_slots * FG_WPOP_MOMENTS);
        for (long long s0 = 0; s0 < n_slots; s0 += per) {
            const long long ns = std::min(per, n_slots - s0);
            std::vector<double> scratch((size_t)(ns * N));
            int q0 = 0, q1 = 0;
            fg_wpe_slice_checks(P, s0, ns, &q0, &q1);
            for (int c = 0; c < nc; ++c) {                                     // a check outside [q0, q1) owns no slot of the slice
                const int o0 = csr[(size_t)c], K = csr[(size_t)c + 1] - o0, mask = csr[(size_t)(nc + 1 + c)], slot0 = csr[(size_t)(2 * nc + 1 + c)];
                const int32_t *members = csr.data() + 3 * nc + 1 + o0;
                bool owns = false;
                for (int st = 0, sl = slot0; st < FG_PPC_N_STATS; ++st) if ((mask >> st) & 1) { owns = owns || (sl >= s0 && sl < s0 + ns); ++sl; }
                if (owns != (c >= q0 && c < q1)) return fail(FG_E_STATE, "fg_wpe_slice_checks misses a check of the slice");
                if (!owns) continue;
                for (long long i = N - 1; i >= 0; --i) {                       // integers have no order: here the reverse one
                    double Ts[FG_PPC_N_STATS];
                    fg_ppc_stats(K, [&](int m) { const int mm = members[m]; return fg_ppc_cell(cells[(size_t)(mm >> 2) * (size_t)N + (size_t)i], mm & 3); }, (mask >> FG_PPC_VAR) & 1, Ts);
                    int sl = slot0;
                    for (int st = 0; st < FG_PPC_N_STATS; ++st) {
                        if (!((mask >> st) & 1)) continue;
                        if (sl >= s0 && sl < s0 + ns) {
                            scratch[(size_t)((sl - s0) * N + i)] = Ts[st];
                            const int g = fg_wpe_category(Ts[st], P.t_obs[(size_t)sl]);
                            units[(size_t)sl * 4 + (size_t)g] += q[(size_t)i];
                            counts[(size_t)sl * 4 + (size_t)g] += q[(size_t)i] ? 1 : 0;
                        }
                        ++sl;
                    }
                }
            }
            moments_rows(scratch.data(), w, N, ns, mom.data() + s0 * FG_WPOP_MOMENTS);
        }
        if (std::getenv("WPOP_EVAL_DRIVER_CORRUPT")) units[0] -= 1;
        if (int rc = fg_wpe_checks_verify((int)n_slots, units.data(), T, &err)) return fail(rc, err);
        for (long long k = 0; k < n_slots; ++k) {
            double p[3];
            fg_wpe_p_values(&units[(size_t)k * 4], p);
            std::printf("slot %lld %" PRIx64, k, bits(P.t_obs[(size_t)k]));
            for (int g = 0; g < 4; ++g) std::printf(" %" PRIu64, units[(size_t)k * 4 + (size_t)g]);
            for (int g = 0; g < 4; ++g) std::printf(" %" PRId64, counts[(size_t)k * 4 + (size_t)g]);
            for (int j = 0; j < FG_WPOP_MOMENTS; ++j) std::printf(" %" PRIx64, bits(mom[(size_t)k * FG_WPOP_MOMENTS + (size_t)j]));
            for (int j = 0; j < 3; ++j) std::printf(" %" PRIx64, bits(p[j]));
            std::printf("\n");
        }
    }

    // ---- fg_wpop_loglik: k_wpe_weights and its tree; per slice k_wpe_ll_stage, the pools, k_wpe_ll_terms, the three sums
    if (do_ll) {
        std::vector<double> ll;
        if (!read_file(argv[11], ll, (size_t)n_sel * (size_t)N)) { std::fprintf(stderr, "cannot read the log-likelihood\n"); return 1; }
        const std::vector<FgPoolLevel> levels = fg_pool_levels(N);
        std::vector<double> pw((size_t)N);
        for (long long i = 0; i < N; ++i) pw[(size_t)i] = fg_wpe_weight(w[(size_t)i]);
        const double W = fg_pool_host<FgWpSumPool>(levels, fg_pool_slices(1, FG_POOL_MAX_GRID_Y), pw.data(), 0)[0];
        const long long per = ll_rows > 0 ? ll_rows : fg_wll_rows(N, n_sel);
        for (long long r0 = 0; r0 < n_sel; r0 += per) {
            const long long rows = std::min<long long>(per, n_sel - r0);
            const std::vector<FgPoolSlice> slices = fg_pool_slices(rows, FG_POOL_MAX_GRID_Y);
            std::vector<double> st((size_t)(FG_WLL_STAGE * rows * N));
            std::vector<uint64_t> ctr((size_t)rows * 7, 0);                    // fin, -inf, +inf, nan, ~min key, max key, the bits of tmax
            for (long long k = 0; k < rows; ++k)
                for (long long i = 0; i < N; ++i) {
                    const double xi = ll[(size_t)((r0 + k) * N + i)], wi = w[(size_t)i], lw = fg_wp_leaf_weight(wi, xi);
                    st[(size_t)(k * N + i)] = lw; st[(size_t)((rows + k) * N + i)] = xi; st[(size_t)((2 * rows + k) * N + i)] = fg_wll_w2_term(lw);
                    if (fg_wpe_weight(wi) > 0.0) {
                        const int kind = fg_wll_kind(xi);
                        ctr[(size_t)k * 7 + (size_t)kind] += 1;
                        if (kind == FG_WLL_FIN) { const uint64_t key = fg_wp_key(xi); ctr[(size_t)k * 7 + 4] = std::max(ctr[(size_t)k * 7 + 4], ~key); ctr[(size_t)k * 7 + 5] = std::max(ctr[(size_t)k * 7 + 5], key); }
                    }
                }
            const std::vector<FgWpElem> e1 = fg_pool_host<FgWpPool>(levels, slices, st.data(), rows * N);
            const std::vector<double> w2 = fg_pool_host<FgWpSumPool>(levels, slices, st.data() + 2 * rows * N, 0);
            std::vector<long long> arg((size_t)rows, -1);
            for (long long k = 0; k < rows; ++k) {
                const bool any = ctr[(size_t)k * 7] > 0;
                const double mx = any ? fg_qs_unkey(ctr[(size_t)k * 7 + 5]) : 0.0, mn = any ? fg_qs_unkey(~ctr[(size_t)k * 7 + 4]) : 0.0;
                for (long long i = 0; i < N; ++i) {
                    const double lw = st[(size_t)(k * N + i)], xi = st[(size_t)((rows + k) * N + i)], tn = fg_wll_sn_term(lw, xi, mn);
                    st[(size_t)(k * N + i)] = fg_wll_sp_term(lw, xi, mx); st[(size_t)((rows + k) * N + i)] = tn; st[(size_t)((2 * rows + k) * N + i)] = tn * tn;
                    if (bits(tn) > ctr[(size_t)k * 7 + 6]) { ctr[(size_t)k * 7 + 6] = bits(tn); arg[(size_t)k] = i; }
                }
            }
            std::vector<double> s[3];
            for (int j = 0; j < 3; ++j) s[j] = fg_pool_host<FgWpSumPool>(levels, slices, st.data() + j * rows * N, 0);
            for (long long k = 0; k < rows; ++k) {
                const uint64_t *cr = &ctr[(size_t)k * 7];
                const int64_t c[FG_WLL_COUNTS] = {(int64_t)cr[0], (int64_t)cr[1], (int64_t)cr[2], (int64_t)cr[3]};
                double wd[FG_WLL_WORDS], fig[FG_WLL_FIGURES];
                if (int rc = fg_wll_words(W, e1[(size_t)k], w2[(size_t)k], cr[4], cr[5], s[0][(size_t)k], s[1][(size_t)k], s[2][(size_t)k], cr[6], c, r0 + k, wd, &err)) return fail(rc, err);
                fg_wll_finish(wd, c, fig);
                std::printf("ll %lld", r0 + k);
                for (int j = 0; j < FG_WLL_FIGURES; ++j) std::printf(" %" PRIx64, bits(fig[j]));
                for (int j = 0; j < FG_WLL_WORDS; ++j) std::printf(" %" PRIx64, bits(wd[j]));
                for (int j = 0; j < FG_WLL_COUNTS; ++j) std::printf(" %" PRId64, c[j]);
                std::printf(" %lld\n", arg[(size_t)k]);
            }
        }
    }
    return 0;
}
