// loglik_stream_driver.cpp -- the log-likelihood stream on the host: fg_loglik_stream_plan.h and fg_chain_pool.h (the update, merge and
// finish functions the device code runs, the launch cuts and the tree schedule) with k_loglik_stream_update and k_chain_pool replaced
// by plain loops.  tests/test_loglik_stream_cpu.py builds it with g++ (once more with -fsanitize=address,undefined) and compares its
// output bit for bit with the Python restatement.
//
//   loglik_stream_driver N_TOTAL N_SEL C FILE C1,C2,... [MAX_GRID_X MAX_GRID_Y]
//
// FILE: N_TOTAL x N_SEL x C doubles ([n][n_sel][C], raw), fed in chunks of C1, C2, ... draws.  Prints per statement k
// "pooled K" + the FG_LL_POOLED words as 16 hex digits, "counts K A B Z", "figures K" + the FG_LL_FIGURES figures as hex; then
// "launches L levels V slices S".  An error of the plan is printed as "error RC MESSAGE" with exit status 2.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fugue_amd/csrc/fg_loglik_stream_plan.h"

static int fail(int rc, const std::string &msg) { std::printf("error %d %s\n", rc, msg.c_str()); return 2; }

static unsigned long long bits(double v) { unsigned long long u; std::memcpy(&u, &v, 8); return u; }

int main(int argc, char **argv) {
    if (argc < 6) { std::fprintf(stderr, "usage: loglik_stream_driver N_TOTAL N_SEL C FILE C1,C2,... [MAX_GRID_X MAX_GRID_Y]\n"); return 1; }
    const int n_total = std::atoi(argv[1]), n_sel = std::atoi(argv[2]);
    const long long C = std::atoll(argv[3]);
    const long long gx = argc > 6 ? std::atoll(argv[6]) : FG_POOL_MAX_GRID_X;
    const long long gy = argc > 7 ? std::atoll(argv[7]) : FG_POOL_MAX_GRID_Y;
    FgLlPlan P;
    std::string err;
    int rc = fg_ll_init(P, n_total, C, n_sel, &err, gx, gy);
    if (rc) return fail(rc, err);
    const long long stride = (long long)n_sel * C;
    std::vector<double> x((size_t)n_total * (size_t)stride);
    FILE *f = std::fopen(argv[4], "rb");
    if (!f || std::fread(x.data(), 8, x.size(), f) != x.size()) { std::fprintf(stderr, "cannot read %s\n", argv[4]); return 1; }
    std::fclose(f);
    std::vector<double> state(fg_ll_state_words(P), 0.0);                         // zeroed, as the device state
    long long t0 = 0;
    const std::string chunks = argv[5];
    for (size_t at = 0; at < chunks.size();) {
        size_t end = chunks.find(',', at);
        if (end == std::string::npos) end = chunks.size();
        const int n_c = std::atoi(chunks.substr(at, end - at).c_str());
        at = end + 1;
        rc = P.draws.take(n_c, "fg_loglik_stream_update", &err);
        if (rc) return fail(rc, err);
        if (n_c == 0) continue;
        const double *chunk = x.data() + (size_t)t0 * (size_t)stride;
        for (const FgPoolLaunch &L : P.launches)                                   // k_loglik_stream_update
            for (long long j = 0; j < L.cols; ++j) {
                const long long col = L.col0 + j;
                FgLlState s;
                fg_ll_state_load(s, state.data() + col, stride);
                for (int t = 0; t < n_c; ++t) fg_ll_update(s, chunk[(long long)t * stride + col]);
                fg_ll_state_store(s, state.data() + col, stride);
            }
        t0 += n_c;
    }
    rc = P.draws.complete("fg_loglik_stream_result", &err);
    if (rc) return fail(rc, err);
    const std::vector<FgLlElem> cur = fg_pool_host<FgLlPool>(P.levels, P.slices, state.data(), stride);      // k_chain_pool, level by level
    const double N = (double)n_total * (double)C;
    for (int k = 0; k < n_sel; ++k) {
        double w[FG_LL_ELEM], fig[FG_LL_FIGURES];
        FgLlPool::elem_store(cur[(size_t)k], w);
        const FgLlElem e = FgLlPool::elem_load(w);
        std::printf("pooled %d", k);
        for (int i = 0; i < FG_LL_POOLED; ++i) std::printf(" %016llx", bits(w[i]));
        std::printf("\ncounts %d %lld %lld %lld\n", k, (long long)e.n_neg_inf, (long long)e.n_pos_inf, (long long)e.n_nan);
        fg_ll_finish(e, N, fig);
        std::printf("figures %d", k);
        for (int i = 0; i < FG_LL_FIGURES; ++i) std::printf(" %016llx", bits(fig[i]));
        std::printf("\n");
    }
    std::printf("launches %zu levels %zu slices %zu\n", P.launches.size(), P.levels.size(), P.slices.size());
    return 0;
}
