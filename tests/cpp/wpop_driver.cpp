// wpop_driver.cpp -- fg_wpop_plan.h without a GPU: host loops stand where fg_wpop.hip has kernels (units, staged leaves, one histogram
// or collect walk per group and pass, the tables), everything else -- the argument checks, the pools and the tree, the selection
// step with its integrity check, the read-outs -- is the plan header's own code.  tests/test_wpop_cpu.py builds it with g++ (and
// once more under AddressSanitizer / UBSan) and compares its output with tests/wpop_restatement.py bit for bit.
//
//   wpop_driver N d x.f64 w.f64 probs digit_bits capacity [n_rows cells.u64 vtypes lo bins]
// prints  units T n_bad n_zero | q <hex> ... | moments k <6 hex words> | quant k <hex> ... | passes k <int> ... |
//         table k below above min max <units> ...   and exits 0;  or  error <code> <message>  and exits 2.
// WPOP_DRIVER_CORRUPT_PASS=k in the environment spoils the totals of pass k (one unit, or one cursor step) before the selection step.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <sstream>

#include "../../fugue_amd/csrc/fg_wpop_plan.h"

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
template <typename T>
static std::vector<T> list_of(const char *text) {
    std::vector<T> out;
    std::stringstream ss(text);
    std::string item;
    while (std::getline(ss, item, ',')) if (!item.empty()) out.push_back((T)std::strtod(item.c_str(), nullptr));
    return out;
}
static std::vector<int64_t> int_list_of(const char *text) {
    std::vector<int64_t> out;
    std::stringstream ss(text);
    std::string item;
    while (std::getline(ss, item, ',')) if (!item.empty()) out.push_back((int64_t)std::strtoll(item.c_str(), nullptr, 10));
    return out;
}

int main(int argc, char **argv) {
    if (argc != 8 && argc != 13) { std::fprintf(stderr, "usage: wpop_driver N d x.f64 w.f64 probs digit_bits capacity [n_rows cells.u64 vtypes lo bins]\n"); return 1; }
    const long long N = std::atoll(argv[1]), d = std::atoll(argv[2]);
    const std::vector<double> probs = list_of<double>(argv[5]);
    const int digit_bits = std::atoi(argv[6]);
    const int64_t capacity = std::atoll(argv[7]);
    std::string err;
    // the order of the ABI: fg_wpop_new, fg_wpop_moments, fg_wpop_quantiles, fg_wpop_counts
    if (int rc = fg_wp_new_check(N, &err)) return fail(rc, err);
    if (int rc = fg_wp_m_check(d, &err)) return fail(rc, err);
    if (int rc = fg_wp_q_check(d, probs.data(), (int)probs.size(), digit_bits, capacity, &err)) return fail(rc, err);
    const int n_rows = argc == 13 ? std::atoi(argv[8]) : 0;
    FgCsPlan C;
    if (argc == 13) {
        const std::vector<int64_t> vt = int_list_of(argv[10]), lo = int_list_of(argv[11]), bn = int_list_of(argv[12]);
        std::vector<int32_t> vt32(vt.begin(), vt.end()), bn32(bn.begin(), bn.end());
        const bool sized = n_rows >= 1 && (size_t)n_rows == vt.size() && vt.size() == lo.size() && lo.size() == bn.size();
        if (int rc = fg_wp_c_init(C, N, n_rows, sized ? vt32.data() : nullptr, sized ? lo.data() : nullptr, sized ? bn32.data() : nullptr, &err)) return fail(rc, err);
    }
    std::vector<double> x, w;
    if (!read_file(argv[3], x, (size_t)(d * N)) || !read_file(argv[4], w, (size_t)N)) { std::fprintf(stderr, "cannot read the inputs\n"); return 1; }

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
    std::printf("units %" PRIu64 " %" PRIu64 " %" PRIu64 "\nq", T, n_bad, n_zero);
    for (long long i = 0; i < N; ++i) std::printf(" %" PRIx64, q[(size_t)i]);
    std::printf("\n");

    // ---- moments: k_wpop_leaves, the tree, k_wpop_terms, the tree again; slices as fg_wpop_moments cuts them
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
        for (long long k = 0; k < rows; ++k) {
            double out[FG_WPOP_MOMENTS];
            fg_wp_finish(e1[(size_t)k], e2[(size_t)k], out);
            std::printf("moments %lld", r0 + k);
            for (int j = 0; j < FG_WPOP_MOMENTS; ++j) std::printf(" %" PRIx64, bits(out[j]));
            std::printf("\n");
        }
    }

    // ---- quantiles: per pass k_wpop_hist / k_wpop_collect as loops, the selection step the plan's
    const uint64_t n_live = (uint64_t)N - n_bad - n_zero;
    const int np = (int)probs.size();
    const char *corrupt = std::getenv("WPOP_DRIVER_CORRUPT_PASS");               // the integrity check's test: spoil the totals of that pass
    const int corrupt_pass = corrupt ? std::atoi(corrupt) : 0;
    FgWpQPlan P;
    fg_wp_q_init(P, (int)d, probs.data(), np, digit_bits, capacity, T, n_live);
    while (!P.done) {
        const size_t H = P.hist.size(), K = P.col.size(), nb = (size_t)1 << P.w;
        std::vector<uint64_t> units(H * nb, 0), elems(H * nb, 0), mn(H, ~0ull), mx(H, 0), cursor(K, 0);
        std::vector<FgWpPairs> pairs(K);
        for (size_t g = 0; g < H; ++g)
            for (long long i = 0; i < N; ++i) {
                if (!q[(size_t)i]) continue;
                const uint64_t key = fg_wp_key(x[(size_t)(P.hist[g].row * N + i)]);
                if (!fg_wp_match(key, P.hist[g].prefix, P.b)) continue;
                const size_t digit = (size_t)((key >> (64 - P.b - P.w)) & (nb - 1));
                units[g * nb + digit] += q[(size_t)i]; elems[g * nb + digit] += 1;
                mn[g] = std::min(mn[g], key); mx[g] = std::max(mx[g], key);
            }
        for (size_t g = 0; g < K; ++g)
            for (long long i = N - 1; i >= 0; --i) {                      // any order of arrival: here the reverse one
                if (!q[(size_t)i]) continue;
                const uint64_t key = fg_wp_key(x[(size_t)(P.col[g].row * N + i)]);
                if (!fg_wp_match(key, P.col[g].prefix, P.b)) continue;
                if (cursor[g]++ < P.col[g].m) pairs[g].emplace_back(key, q[(size_t)i]);
            }
        if (corrupt_pass == P.passes + 1) {                                   // a pass that did not see what the previous one left
            if (H) units[0] += 1;
            else cursor[0] += 1;
        }
        FgWpPassData D;
        D.units = units.data(); D.elems = elems.data(); D.mn = mn.data(); D.mx = mx.data(); D.cursor = cursor.data(); D.pairs = &pairs;
        if (int rc = fg_wp_end_pass(P, D, &err)) return fail(rc, err);
    }
    std::vector<double> qv((size_t)(d * np));
    std::vector<int32_t> qp((size_t)(d * np));
    fg_wp_q_result(P, qv.data(), qp.data());
    for (long long k = 0; k < d; ++k) {
        std::printf("quant %lld", k);
        for (int j = 0; j < np; ++j) std::printf(" %" PRIx64, bits(qv[(size_t)(k * np + j)]));
        std::printf("\npasses %lld", k);
        for (int j = 0; j < np; ++j) std::printf(" %d", qp[(size_t)(k * np + j)]);
        std::printf("\n");
    }

    // ---- tables: k_wpop_counts as a loop
    if (argc == 13) {
        std::vector<uint64_t> cells;
        if (!read_file(argv[9], cells, (size_t)n_rows * (size_t)N)) { std::fprintf(stderr, "cannot read the cells\n"); return 1; }
        const size_t nw = (size_t)n_rows;
        std::vector<uint64_t> ctr(fg_cs_words(C), 0);
        uint64_t *below = ctr.data() + C.n_bins, *above = below + nw, *mnk = above + nw, *mxk = mnk + nw;
        for (size_t k = 0; k < nw; ++k) {
            const FgCsRow &r = C.rows[k];
            for (long long i = 0; i < N; ++i) {
                if (!q[(size_t)i]) continue;
                const uint64_t key = cells[k * (size_t)N + (size_t)i] ^ r.flip;
                const int bin = fg_cs_bin(key, r.klo, r.bins);
                if (bin < 0) below[k] += q[(size_t)i];
                else if (bin == r.bins) above[k] += q[(size_t)i];
                else ctr[r.off + (size_t)bin] += q[(size_t)i];
                mnk[k] = std::max(mnk[k], ~key); mxk[k] = std::max(mxk[k], key);
            }
        }
        std::vector<uint64_t> units(C.n_bins), hb(nw), ha(nw);
        std::vector<int64_t> hmin(nw), hmax(nw);
        if (int rc = fg_wp_c_result(C, ctr.data(), T, units.data(), hb.data(), ha.data(), hmin.data(), hmax.data(), &err)) return fail(rc, err);
        for (size_t k = 0; k < nw; ++k) {
            std::printf("table %zu %" PRIu64 " %" PRIu64 " %" PRId64 " %" PRId64, k, hb[k], ha[k], hmin[k], hmax[k]);
            for (int j = 0; j < C.rows[k].bins; ++j) std::printf(" %" PRIu64, units[C.rows[k].off + (size_t)j]);
            std::printf("\n");
        }
    }
    return 0;
}
