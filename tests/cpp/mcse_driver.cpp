// Runs the rule of the MCSE / ESS figures (fugue_amd/csrc/fg_diag_mcse_plan.h, what fg_diag_mcse.hip's kernels and host code share) on the host.
//   mcse_driver coord <file of S doubles> <file of parameters> <out file>
//       parameters (doubles): n_probs, the probabilities, mean, sd, rhat, ess_mean, then ess [R], pooled mean [R] and pooled std [R] of the
//       R = 2 + n_probs rows (the combination's figures, which the test takes from the oracle).  One coordinate's pooled cells through the
//       rule: keys, a stable sort of the keys (the plan's own radix sort is tests/cpp/rank_driver.cpp's subject), the rows, the gathered
//       order statistics, the folded sort, the Beta rule and fg_mcse_figures.  Writes doubles: rows [R][S], sorted [S], the words
//       [fg_mcse_words], the counts [fg_mcse_counts] (radix passes: 0, the sort here is not the radix sort).
//       Prints:  coord S R | ok|FAIL <what>
//   mcse_driver beta <a> <b> <y> ...        one line per three:  beta | <x with 17 digits>
//   mcse_driver ranks <S> <p> <ess> ...     one line per three:  ranks | rc i_lo i_hi
//   mcse_driver plan <n> <C> <d> <j0> <n_j> <n_probs> <max_out_bytes> ...    one line per seven (probabilities: (i + 1) / (n_probs + 1)):
//       plan | rc S rows words counts block | ok
//   mcse_driver refusals
// tests/test_diag_mcse_cpu.py reads the lines.  Built stand-alone, a second time with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fugue_amd/csrc/fg_diag_mcse_plan.h"

static std::vector<double> read_doubles(const char *path) {
    std::vector<double> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
    double b[1024];
    size_t g;
    while ((g = std::fread(b, 8, 1024, f)) > 0) v.insert(v.end(), b, b + g);
    std::fclose(f);
    return v;
}

static int cmd_coord(const char *in, const char *par, const char *out) {
    const std::vector<double> x = read_doubles(in), q = read_doubles(par);
    const long long S = (long long)x.size();
    if (q.empty()) { std::printf("coord %lld 0 | FAIL no parameters\n", S); return 1; }
    const int n_probs = (int)q[0];
    if (n_probs < 1 || n_probs > FG_MCSE_MAX_PROBS || (long long)q.size() != 1 + n_probs + 4 + 3 * (2 + n_probs)) { std::printf("coord %lld 0 | FAIL parameters\n", S); return 1; }
    const double *probs = &q[1], *raw4 = probs + n_probs;
    FgMcsePlan P;
    const int rc = fg_mcse_plan(S, 1, 1, 0, 1, probs, n_probs, &P);
    if (rc) { std::printf("coord %lld 0 | FAIL plan rc %d\n", S, rc); return 1; }
    const int R = P.rows, nw = fg_mcse_words(n_probs), nc = fg_mcse_counts(n_probs), pairs = fg_mcse_pairs(n_probs);
    const double *ess = raw4 + 4, *mean_rows = ess + R, *std_rows = mean_rows + R;
    std::vector<uint64_t> keys(S), sorted;
    long long n_nan = 0, n_ninf = 0, n_pinf = 0, n_nanf = 0;
    for (long long i = 0; i < S; ++i) { keys[i] = fg_rank_key(x[i]); n_nan += x[i] != x[i]; n_ninf += x[i] == -INFINITY; n_pinf += x[i] == INFINITY; }
    sorted = keys;
    std::stable_sort(sorted.begin(), sorted.end());
    // the block's first gather: the median positions, k_p and its upper neighbour
    std::vector<double> at(pairs);
    at[0] = fg_rank_unkey(sorted[(S - 1) / 2]); at[1] = fg_rank_unkey(sorted[S / 2]);
    for (int i = 0; i < n_probs; ++i) {
        if (P.k_p[i] < 0 || P.k_p[i] >= S) { std::printf("coord %lld %d | FAIL k_p outside [0, S)\n", S, R); return 1; }
        at[2 + 2 * i] = fg_rank_unkey(sorted[P.k_p[i]]);
        at[3 + 2 * i] = fg_rank_unkey(sorted[std::min<long long>(P.k_p[i] + 1, S - 1)]);
    }
    const double med = fg_rank_median(at[0], at[1]);
    std::vector<double> o((size_t)R * S + S + nw + nc);
    std::vector<uint64_t> fkeys(S);
    for (long long i = 0; i < S; ++i) {
        const double c = fg_mcse_centre(x[i], raw4[0]);
        o[i] = fg_mcse_row_abs(c);
        o[S + i] = fg_mcse_row_sq(c);
        for (int p = 0; p < n_probs; ++p) o[(size_t)(2 + p) * S + i] = fg_mcse_indicator(keys[i], sorted[P.k_p[p]]);
        const double f = fg_rank_fold(x[i], med);
        fkeys[i] = fg_rank_key(f);
        n_nanf += f != f;
    }
    std::stable_sort(fkeys.begin(), fkeys.end());
    for (long long i = 0; i < S; ++i) o[(size_t)R * S + i] = fg_rank_unkey(sorted[i]);
    std::vector<int64_t> counts(nc);
    counts[0] = S; counts[1] = n_nan; counts[2] = n_ninf; counts[3] = n_pinf; counts[4] = n_nanf; counts[5] = 0;
    std::vector<double> th((size_t)2 * n_probs, 0.0);
    for (int i = 0; i < n_probs; ++i) {
        int64_t lo = -1, hi = -1;
        if (fg_mcse_ranks(S, probs[i], ess[2 + i], &lo, &hi)) lo = hi = -1;
        else if (lo < 0 || hi < 0 || lo >= S || hi >= S) { std::printf("coord %lld %d | FAIL a position outside [0, S)\n", S, R); return 1; }
        counts[FG_MCSE_FIXED_COUNTS + 3 * i] = P.k_p[i]; counts[FG_MCSE_FIXED_COUNTS + 3 * i + 1] = lo; counts[FG_MCSE_FIXED_COUNTS + 3 * i + 2] = hi;
        if (lo >= 0) { th[2 * i] = fg_rank_unkey(sorted[lo]); th[2 * i + 1] = fg_rank_unkey(sorted[hi]); }
    }
    const double mad = fg_mcse_mad(fg_rank_unkey(fkeys[(S - 1) / 2]), fg_rank_unkey(fkeys[S / 2]), n_nanf);
    fg_mcse_figures(P, probs, raw4, ess, mean_rows, std_rows, at.data(), mad, th.data(), counts.data(), &o[(size_t)R * S + S]);
    for (int i = 0; i < nc; ++i) o[(size_t)R * S + S + nw + i] = (double)counts[i];
    FILE *f = std::fopen(out, "wb");
    if (!f || std::fwrite(o.data(), 8, o.size(), f) != o.size()) { std::printf("coord %lld %d | FAIL write\n", S, R); return 1; }
    std::fclose(f);
    std::printf("coord %lld %d | ok\n", S, R);
    return 0;
}

static int cmd_beta(int argc, char **argv) {
    for (int a = 2; a + 2 < argc; a += 3) {
        const double x = fg_mcse_betaincinv(std::atof(argv[a]), std::atof(argv[a + 1]), std::atof(argv[a + 2]));
        if (!(x >= 0.0 && x <= 1.0)) { std::printf("beta | FAIL outside [0, 1]\n"); return 1; }
        std::printf("beta | %.17g\n", x);
    }
    return 0;
}

static int cmd_ranks(int argc, char **argv) {
    for (int a = 2; a + 2 < argc; a += 3) {
        int64_t lo = -7, hi = -7;
        const int rc = fg_mcse_ranks(std::atoll(argv[a]), std::atof(argv[a + 1]), std::atof(argv[a + 2]), &lo, &hi);
        std::printf("ranks | %d %lld %lld\n", rc, (long long)lo, (long long)hi);
    }
    return 0;
}

static int cmd_plan(int argc, char **argv) {
    int bad = 0;
    for (int a = 2; a + 6 < argc; a += 7) {
        const long long n = std::atoll(argv[a]), C = std::atoll(argv[a + 1]), d = std::atoll(argv[a + 2]), j0 = std::atoll(argv[a + 3]), nj = std::atoll(argv[a + 4]);
        const int n_probs = std::atoi(argv[a + 5]);
        const long long mob = std::atoll(argv[a + 6]);
        double probs[FG_MCSE_MAX_PROBS];
        for (int i = 0; i < FG_MCSE_MAX_PROBS; ++i) probs[i] = (double)(i + 1) / (double)((n_probs > 0 ? n_probs : 1) + 1);
        FgMcsePlan P;
        std::memset(&P, 0, sizeof P);
        const int rc = fg_mcse_plan(n, C, d, j0, nj, probs, n_probs, &P);
        std::string ok = "ok";
        long long blk = 0;
        if (!rc) {
            blk = fg_mcse_block(P, d, mob);
            if (P.rank.S != n * C || P.rows != 2 + n_probs) ok = "FAIL shape";
            if (P.b_coord_out != (size_t)n * C * 8 * P.rows || P.b_coord_keys != (size_t)P.rank.S * 8) ok = "FAIL bytes";
            if (blk < 1 || blk > d || blk * P.rows > 65535 || fg_mcse_block(P, d, 1) != 1) ok = "FAIL block of coordinates";
            for (int i = 0; i < n_probs; ++i) if (P.k_p[i] < 0 || P.k_p[i] >= P.rank.S) ok = "FAIL k_p";
        }
        if (ok != "ok") bad = 1;
        std::printf("plan | %d %lld %d %d %d %lld | %s\n", rc, rc ? 0ll : P.rank.S, rc ? 0 : P.rows, rc ? 0 : fg_mcse_words(n_probs), rc ? 0 : fg_mcse_counts(n_probs), blk, ok.c_str());
    }
    return bad;
}

static int cmd_refusals() {
    FgMcsePlan P;
    const double ok3[3] = { 0.05, 0.5, 0.95 }, edge[2] = { 0.0, 1.0 }, neg[2] = { 0.5, -0.1 }, big[1] = { 1.5 }, nanp[3] = { 0.1, NAN, 0.9 };
    const double eight[8] = { 0.0, 0.1, 0.2, 0.3, 0.5, 0.7, 0.9, 1.0 }, nine[9] = { 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9 };
    struct { long long n, C, d, j0, nj; const double *p; int np; int want; } t[] = {
        { 0, 4, 1, 0, 1, ok3, 3, FG_E_BAD_ARG }, { 4, 0, 1, 0, 1, ok3, 3, FG_E_BAD_ARG }, { 4, 4, 0, 0, 1, ok3, 3, FG_E_BAD_ARG }, { 4, 4, 65536, 0, 1, ok3, 3, FG_E_BAD_ARG },
        { 4, 4, 3, 3, 1, ok3, 3, FG_E_BAD_ARG }, { 4, 4, 3, -1, 1, ok3, 3, FG_E_BAD_ARG }, { 4, 4, 3, 1, 3, ok3, 3, FG_E_BAD_ARG }, { 4, 4, 3, 0, 0, ok3, 3, FG_E_BAD_ARG },
        { 4, 4, 3, 0, 3, ok3, 0, FG_E_BAD_ARG }, { 4, 4, 3, 0, 3, nine, 9, FG_E_BAD_ARG }, { 4, 4, 3, 0, 3, nullptr, 3, FG_E_BAD_ARG }, { 4, 4, 3, 0, 3, neg, 2, FG_E_BAD_ARG },
        { 4, 4, 3, 0, 3, big, 1, FG_E_BAD_ARG }, { 4, 4, 3, 0, 3, nanp, 3, FG_E_BAD_ARG }, { 65536, 32768, 1, 0, 1, ok3, 3, FG_E_LIMIT }, { 1ll << 40, 1ll << 40, 1, 0, 1, ok3, 3, FG_E_LIMIT },
        { 32767, 65536, 1, 0, 1, ok3, 3, FG_OK }, { 4, 4, 65535, 65534, 1, edge, 2, FG_OK }, { 1, 1, 1, 0, 1, eight, 8, FG_OK },
    };
    int bad = 0;
    for (auto &c : t) {
        const int rc = fg_mcse_plan(c.n, c.C, c.d, c.j0, c.nj, c.p, c.np, &P);
        std::printf("refusal n %lld C %lld d %lld j0 %lld n_j %lld n_probs %d | rc %d want %d\n", c.n, c.C, c.d, c.j0, c.nj, c.np, rc, c.want);
        bad |= rc != c.want;
    }
    int64_t lo, hi;
    struct { long long S; double p, ess; int want; } r[] = {
        { 0, 0.5, 10.0, FG_E_BAD_ARG }, { 10, -0.1, 10.0, FG_E_BAD_ARG }, { 10, 1.1, 10.0, FG_E_BAD_ARG }, { 10, NAN, 10.0, FG_E_BAD_ARG }, { 10, 0.5, 0.0, FG_E_BAD_ARG },
        { 10, 0.5, -3.0, FG_E_BAD_ARG }, { 10, 0.5, NAN, FG_E_BAD_ARG }, { 10, 0.5, INFINITY, FG_E_BAD_ARG }, { 1, 0.0, 0.5, FG_OK }, { 10, 1.0, 1e9, FG_OK },
    };
    for (auto &c : r) {
        const int rc = fg_mcse_ranks(c.S, c.p, c.ess, &lo, &hi);
        std::printf("refusal S %lld p %g ess %g | rc %d want %d\n", c.S, c.p, c.ess, rc, c.want);
        bad |= rc != c.want;
        if (!rc && !(lo >= 0 && lo <= hi && hi < c.S)) { std::printf("refusal | FAIL positions %lld %lld\n", (long long)lo, (long long)hi); bad = 1; }
    }
    bad |= fg_mcse_ranks(10, 0.5, 10.0, nullptr, &hi) != FG_E_BAD_ARG || fg_mcse_ranks(10, 0.5, 10.0, &lo, nullptr) != FG_E_BAD_ARG;
    return bad;
}

int main(int argc, char **argv) {
    if (argc >= 5 && !std::strcmp(argv[1], "coord")) return cmd_coord(argv[2], argv[3], argv[4]);
    if (argc >= 2 && !std::strcmp(argv[1], "beta")) return cmd_beta(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "ranks")) return cmd_ranks(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "plan")) return cmd_plan(argc, argv);
    if (argc >= 2 && !std::strcmp(argv[1], "refusals")) return cmd_refusals();
    std::fprintf(stderr, "usage: mcse_driver coord|beta|ranks|plan|refusals ...\n");
    return 2;
}
