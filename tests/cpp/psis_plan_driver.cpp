// Walks fg_psis_plan (fugue_amd/csrc/fg_psis_plan.h, the planner fg_psis.hip calls) and checks what the launches rely on.
//   psis_plan_driver plan <n> <C> <n_sel> ...      one line per triple:
//       plan n C n_sel | rc S M G tstar P rank nb nbp passes rows_per b_row | ok|FAIL <what>
//     M against its definition (the bracketing squares, no floating point); P a power of two holding M; the pass widths covering the
//     64 key bits once; every pooled cell owned by exactly one (block, thread, slot) and every tail term by one (lane, slot) (S up to
//     2^22); the work buffers of a slice adding up to rows_per rows within the budget, the grid's y within 65 535.
//   psis_plan_driver select <file of S doubles>     the radix select by host loops over fg_psis_pick_bin / fg_psis_advance in place of
//     the kernels, against std::sort on the keys:  select S M | cutoff key, below, equal | ok|FAIL
//   psis_plan_driver refusals
//   psis_plan_driver dd                             fg_psis_dd.h's exp, expm1, log, log1p, quotient and sqrt against long double on a fixed walk of
//     arguments (within 2^-60 relative: long double's own resolution), and the corners exp(0) = 1, exp(-inf) = 0, exp(NaN)
// tests/test_psis_cpu.py reads the lines.  Built stand-alone with -fsanitize=address,undefined.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../fugue_amd/csrc/fg_psis_plan.h"
#include "../../fugue_amd/csrc/fg_psis_dd.h"

static uint64_t key_of(double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

static std::string check_plan(long long n, long long C, long long n_sel, FgPsisPlan &P, int *rc_out) {
    const int rc = *rc_out = fg_psis_plan(n, C, n_sel, &P);
    if (n < 1 || C < 1 || n_sel < 1) return rc == FG_E_BAD_ARG ? "ok" : "a bad argument was planned";
    if ((__int128)n * C > FG_PSIS_S_MAX) return rc == FG_E_LIMIT ? "ok" : "S >= 2^31 was planned";
    if (rc) return "plan rc " + std::to_string(rc);
    const long long S = n * C, M = P.M;
    if (P.S != S) return "S";
    const long long a = (S + 4) / 5;
    long long b = 0;
    while ((__int128)b * b < (__int128)9 * S) ++b;                              // by counting: independent of the bisection
    if (M != std::min(a, b) || M != fg_psis_tail(S) || M < 1 || M > S) return "M";
    long long r = 0;
    while ((r + 1) * (r + 1) <= M) ++r;
    if (P.G != 30 + r || P.G > FG_PSIS_G_MAX) return "G";
    if (P.tstar != (M + 2) / 4 || P.tstar > M) return "tstar";
    if (P.P < M || P.P < 2 || (P.P & (P.P - 1)) || (P.P >= 4 && P.P / 2 >= M)) return "P";
    if (P.rank != std::min(M + 1, S)) return "rank";
    int bits = 0;
    for (int p = 0; p < P.passes; ++p) { const int w = fg_psis_pass_width(p); if (w < 1 || w > FG_PSIS_DIGIT_BITS) return "pass width"; bits += w; }
    if (bits != 64) return "the passes do not cover the key";
    if (P.nb < 1 || P.nb > FG_PSIS_MAX_BLOCKS || P.nb != fg_psis_blocks(S) || P.nbp < P.nb || (P.nbp & (P.nbp - 1)) || P.nbp >= 2 * P.nb + (P.nb == 0)) return "blocks";
    if (S <= (1ll << 22)) {
        std::vector<unsigned char> own((size_t)S, 0);
        const long long slots = (S + (long long)P.nb * FG_PSIS_THREADS - 1) / ((long long)P.nb * FG_PSIS_THREADS);
        for (unsigned blk = 0; blk < P.nb; ++blk)
            for (int t = 0; t < FG_PSIS_THREADS; ++t)
                for (long long s = 0; s <= slots; ++s) {
                    const long long i = fg_psis_cell(P, blk, t, s);
                    if (i == -1) continue;
                    if (i < 0 || i >= S) return "a cell outside [0, S)";
                    if (own[(size_t)i]++) return "cell " + std::to_string(i) + " owned twice";
                }
        for (long long i = 0; i < S; ++i) if (!own[(size_t)i]) return "cell " + std::to_string(i) + " owned by nobody";
        std::vector<unsigned char> tw((size_t)M, 0);
        for (int l = 0; l < 64; ++l)
            for (long long s = 0; s <= (M + 63) / 64; ++s) {
                const long long j = fg_psis_tail_term(P, l, s);
                if (j == -1) continue;
                if (j < 0 || j >= M || tw[(size_t)j]++) return "tail term " + std::to_string(j);
            }
        for (long long j = 0; j < M; ++j) if (!tw[(size_t)j]) return "tail term " + std::to_string(j) + " owned by nobody";
    }
    if (P.rows_per < 1 || P.rows_per > FG_PSIS_MAX_GRID_Y || P.rows_per > n_sel) return "rows_per";
    const size_t sum = P.b_state + P.b_class + P.b_hist + P.b_part + P.b_tail + P.b_sort + P.b_t + P.b_fig + P.b_cnt;
    if (sum != (size_t)P.rows_per * P.b_row || sum > (size_t)FG_PSIS_WORK_BYTES) return "the work buffers";
    if (P.b_tail != (size_t)P.rows_per * M * 8 || P.b_sort != (size_t)P.rows_per * P.P * 8 || P.b_part != (size_t)P.rows_per * P.nb * 16 || P.b_t != (size_t)P.rows_per * M * 16) return "a buffer";
    return "ok";
}

static int run_select(const char *path) {
    std::vector<double> x;
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::printf("select FAIL cannot open %s\n", path); return 1; }
    double v;
    while (std::fread(&v, 8, 1, f) == 1) x.push_back(v);
    std::fclose(f);
    FgPsisPlan P;
    if (fg_psis_plan(1, (long long)x.size(), 1, &P)) { std::printf("select FAIL plan\n"); return 1; }
    unsigned long long st[FG_PSIS_STATE_WORDS] = {0};
    st[FG_PSIS_ST_RANK] = (unsigned long long)P.rank;
    std::vector<unsigned int> hist((size_t)1 << FG_PSIS_DIGIT_BITS), part(FG_PSIS_THREADS);
    for (int p = 0; p < P.passes; ++p) {
        const int b = p * FG_PSIS_DIGIT_BITS, w = fg_psis_pass_width(p), lo = 64 - b - w;
        std::fill(hist.begin(), hist.end(), 0u);
        for (double xv : x) {
            const uint64_t key = key_of(xv);
            if (b == 0 || ((key ^ st[FG_PSIS_ST_PREFIX]) >> (64 - b)) == 0) hist[(size_t)((key >> lo) & ((1ull << w) - 1))]++;
        }
        for (int g = 0; g < FG_PSIS_THREADS; ++g) {
            part[(size_t)g] = 0;
            for (int j = 0; j < FG_PSIS_PICK_GROUP; ++j) part[(size_t)g] += hist[(size_t)g * FG_PSIS_PICK_GROUP + j];
        }
        unsigned long long c1, c2;
        const int g = fg_psis_pick_bin(part.data(), FG_PSIS_THREADS, st[FG_PSIS_ST_RANK], &c1);
        const int d = fg_psis_pick_bin(hist.data() + (size_t)g * FG_PSIS_PICK_GROUP, FG_PSIS_PICK_GROUP, st[FG_PSIS_ST_RANK] - c1, &c2);
        fg_psis_advance(st, b, w, g * FG_PSIS_PICK_GROUP + d, c1 + c2, hist[(size_t)g * FG_PSIS_PICK_GROUP + d]);
    }
    std::vector<uint64_t> keys;
    for (double xv : x) keys.push_back(key_of(xv));
    std::sort(keys.begin(), keys.end());
    const uint64_t want = keys[(size_t)P.rank - 1];
    const unsigned long long below = (unsigned long long)(std::lower_bound(keys.begin(), keys.end(), want) - keys.begin());
    const unsigned long long equal = (unsigned long long)(std::upper_bound(keys.begin(), keys.end(), want) - keys.begin()) - below;
    const bool ok = st[FG_PSIS_ST_PREFIX] == want && st[FG_PSIS_ST_BELOW] == below && st[FG_PSIS_ST_EQUAL] == equal && below <= (unsigned long long)P.M &&
                    ((long long)x.size() <= P.M || below + equal >= (unsigned long long)P.M);
    std::printf("select %zu %lld | %016llx %llu %llu | %s\n", x.size(), P.M, (unsigned long long)st[FG_PSIS_ST_PREFIX], (unsigned long long)st[FG_PSIS_ST_BELOW],
                (unsigned long long)st[FG_PSIS_ST_EQUAL], ok ? "ok" : "FAIL");
    return ok ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc >= 2 && !std::strcmp(argv[1], "select")) {
        int bad = 0;
        for (int a = 2; a < argc; ++a) bad += run_select(argv[a]);
        return bad ? 1 : 0;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "dd")) {
        long double worst[6] = {0, 0, 0, 0, 0, 0};
        auto rel = [](FgDD got, long double want) { const long double g = (long double)got.hi + got.lo; return want == 0 ? fabsl(g) : fabsl(g - want) / fabsl(want); };
        unsigned long long seed = 88172645463325252ull;
        auto u01 = [&]() { seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17; return (double)(seed >> 11) / 9007199254740992.0; };
        for (int i = 0; i < 100000; ++i) {
            const double a = -40.0 + 80.0 * u01(), b = 1e-12 + 50.0 * u01(), c = (-0.999 + 6.0 * u01()) * (i % 2 ? 1e-3 : 1.0);
            worst[0] = fmaxl(worst[0], rel(fg_dd_exp(fg_dd(a)), expl((long double)a)));
            worst[1] = fmaxl(worst[1], rel(fg_dd_log(fg_dd(b)), logl((long double)b)));
            if (c != 0.0) { worst[2] = fmaxl(worst[2], rel(fg_dd_log1p(fg_dd(c)), log1pl((long double)c))); worst[3] = fmaxl(worst[3], rel(fg_dd_expm1(fg_dd(c)), expm1l((long double)c))); }
            worst[4] = fmaxl(worst[4], rel(fg_dd_div(fg_dd(a), fg_dd(b)), (long double)a / b));
            worst[5] = fmaxl(worst[5], rel(fg_dd_sqrt(fg_dd(b)), sqrtl((long double)b)));
        }
        const long double lim = ldexpl(1.0L, -60);
        bool ok = true;
        for (long double w : worst) ok = ok && w <= lim;
        const FgDD one = fg_dd_exp(fg_dd(0.0)), nan = fg_dd_exp(fg_dd(NAN));
        ok = ok && one.hi == 1.0 && one.lo == 0.0 && fg_dd_exp(fg_dd(-INFINITY)).hi == 0.0 && fg_dd_exp(fg_dd(-800.0)).hi == 0.0 && nan.hi != nan.hi && fg_dd_log(fg_dd(0.0)).hi == -INFINITY;
        const FgDD s1 = fg_dd_add(fg_dd(1.0), fg_dd(1e-30)), s2 = fg_dd_add(fg_dd(1e-30), fg_dd(1.0));
        ok = ok && s1.hi == s2.hi && s1.lo == s2.lo && s1.lo == 1e-30;
        std::printf("dd exp %.2Le log %.2Le log1p %.2Le expm1 %.2Le div %.2Le sqrt %.2Le | %s\n", worst[0], worst[1], worst[2], worst[3], worst[4], worst[5], ok ? "ok" : "FAIL");
        return ok ? 0 : 1;
    }
    if (argc >= 2 && !std::strcmp(argv[1], "refusals")) {
        FgPsisPlan P;
        const bool ok = fg_psis_plan(0, 4, 1, &P) == FG_E_BAD_ARG && fg_psis_plan(4, 0, 1, &P) == FG_E_BAD_ARG && fg_psis_plan(4, 4, 0, &P) == FG_E_BAD_ARG &&
                        fg_psis_plan(-1, 4, 1, &P) == FG_E_BAD_ARG && fg_psis_plan(1ll << 31, 1, 1, &P) == FG_E_LIMIT && fg_psis_plan(1 << 16, 1 << 15, 1, &P) == FG_E_LIMIT &&
                        fg_psis_plan(1ll << 40, 1ll << 40, 1, &P) == FG_E_LIMIT && fg_psis_plan(32767, 65536, 1, &P) == FG_OK && fg_psis_tail(0) == FG_E_BAD_ARG &&
                        fg_psis_tail(-3) == FG_E_BAD_ARG && fg_psis_tail(1ll << 31) == FG_E_LIMIT && fg_psis_tail((1ll << 31) - 1) > 0;
        std::printf("refusals %s\n", ok ? "ok" : "FAIL");
        return ok ? 0 : 1;
    }
    if (argc < 2 || std::strcmp(argv[1], "plan") || (argc - 2) % 3) { std::fprintf(stderr, "usage: plan <n> <C> <n_sel> ... | select <file> ... | refusals | dd\n"); return 2; }
    int bad = 0;
    for (int a = 2; a + 2 < argc; a += 3) {
        const long long n = std::atoll(argv[a]), C = std::atoll(argv[a + 1]), n_sel = std::atoll(argv[a + 2]);
        FgPsisPlan P = {};
        int rc = 0;
        const std::string r = check_plan(n, C, n_sel, P, &rc);
        std::printf("plan %lld %lld %lld | %d %lld %lld %d %lld %lld %lld %u %u %d %lld %zu | %s\n", n, C, n_sel, rc, P.S, P.M, P.G, P.tstar, P.P, P.rank, P.nb, P.nbp, P.passes, P.rows_per,
                    P.b_row, r == "ok" ? "ok" : ("FAIL " + r).c_str());
        bad += r != "ok";
    }
    return bad ? 1 : 0;
}
