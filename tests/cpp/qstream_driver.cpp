// qstream_driver.cpp -- the streamed quantile selector on the host: fg_diag_qstream_plan.h (the planner the device code calls)
// with the two kernels of fg_diag_qstream.hip replaced by plain loops.  tests/test_diag_qstream_cpu.py builds it with g++ (once
// more with -fsanitize=address,undefined) and compares its output with the numpy restatement and a key sort.
//
//   qstream_driver N_TOTAL D C DIGIT_BITS CAPACITY P1,P2,... PASS [PASS ...]
//
// PASS = FILE@C1,C2,...: a file of N_TOTAL x D x C doubles ([n][d][C], raw) and the chunk lengths it is fed in.  Pass k reads the
// k-th PASS, the last one again when there are fewer.  Prints "slot I Q KEYBITS PASSES" per slot and "passes N"; an error of the
// planner is printed as "error RC MESSAGE" with exit status 2.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../fugue_amd/csrc/fg_diag_qstream_plan.h"

static std::vector<double> split_doubles(const std::string &s) {
    std::vector<double> out;
    size_t at = 0;
    while (at < s.size()) {
        size_t end = s.find(',', at);
        if (end == std::string::npos) end = s.size();
        out.push_back(std::strtod(s.substr(at, end - at).c_str(), nullptr));
        at = end + 1;
    }
    return out;
}

static int fail(int rc, const std::string &msg) { std::printf("error %d %s\n", rc, msg.c_str()); return 2; }

int main(int argc, char **argv) {
    if (argc < 8) { std::fprintf(stderr, "usage: qstream_driver N_TOTAL D C DIGIT_BITS CAPACITY P1,P2,... FILE@C1,C2,... [...]\n"); return 1; }
    const int n_total = std::atoi(argv[1]), d = std::atoi(argv[2]);
    const long long C = std::atoll(argv[3]);
    const int bits = std::atoi(argv[4]);
    const int64_t capacity = std::atoll(argv[5]);
    const std::vector<double> probs = split_doubles(argv[6]);
    FgQsPlan P;
    std::string err;
    int rc = fg_qs_init(P, n_total, C, d, probs.data(), (int)probs.size(), bits, capacity, &err);
    if (rc) return fail(rc, err);
    const int np = P.n_probs;
    const size_t ns = (size_t)d * np;
    for (int pass = 0; !P.done; ++pass) {
        const std::string spec = argv[std::min(7 + pass, argc - 1)];
        const size_t at = spec.rfind('@');
        if (at == std::string::npos) { std::fprintf(stderr, "PASS needs FILE@CHUNKS\n"); return 1; }
        std::vector<double> x((size_t)n_total * d * C);
        FILE *f = std::fopen(spec.substr(0, at).c_str(), "rb");
        if (!f || std::fread(x.data(), 8, x.size(), f) != x.size()) { std::fprintf(stderr, "cannot read %s\n", spec.c_str()); return 1; }
        std::fclose(f);
        // the device state of a pass
        std::vector<uint64_t> hist(ns << P.w, 0), mn(ns, ~0ull), mx(ns, 0), cursor(ns, 0);
        std::vector<std::vector<uint64_t>> keys(ns);
        for (auto &k : keys) k.resize((size_t)capacity);
        long long t0 = 0;
        for (double cl : split_doubles(spec.substr(at + 1))) {
            const int n_c = (int)cl;
            rc = fg_qs_take(P, n_c, &err);
            if (rc) return fail(rc, err);
            const double *chunk = x.data() + (size_t)t0 * d * C;
            for (int i = 0; i < d; ++i)
                for (long long e = 0; e < (long long)n_c * C; ++e) {
                    const long long t = e / C, c = e - t * C;
                    const uint64_t key = fg_qs_key(chunk[(t * d + i) * C + c]);
                    const uint64_t digit = (key >> (64 - P.b - P.w)) & ((1ull << P.w) - 1);
                    for (int g = 0; g < P.n_hist[i]; ++g)                       // k_diag_qstream_hist
                        if (fg_qs_match(key, P.hist_prefix[(size_t)i * np + g], P.b)) {
                            const size_t gi = (size_t)i * np + g;
                            ++hist[(gi << P.w) + digit];
                            mn[gi] = std::min(mn[gi], key); mx[gi] = std::max(mx[gi], key);
                        }
                    for (int g = 0; g < P.n_col[i]; ++g)                        // k_diag_qstream_collect
                        if (fg_qs_match(key, P.col_prefix[(size_t)i * np + g], P.b)) {
                            const size_t gi = (size_t)i * np + g;
                            const uint64_t pos = cursor[gi]++;
                            if (pos < (uint64_t)capacity) keys[gi][(size_t)pos] = key;
                        }
                }
            t0 += n_c;
        }
        for (size_t k = 0; k < ns; ++k) keys[k].resize((size_t)std::min<uint64_t>(cursor[k], (uint64_t)capacity));
        FgQsPassData D;
        D.hist = hist.data(); D.mn = mn.data(); D.mx = mx.data(); D.cursor = cursor.data(); D.keys = &keys;
        rc = fg_qs_end_pass(P, D, &err);
        if (rc) return fail(rc, err);
    }
    std::vector<double> out(ns);
    std::vector<int32_t> sp(ns);
    rc = fg_qs_result(P, out.data(), sp.data(), &err);
    if (rc) return fail(rc, err);
    for (int i = 0; i < d; ++i)
        for (int q = 0; q < np; ++q) {
            uint64_t u;
            std::memcpy(&u, &out[(size_t)i * np + q], 8);
            std::printf("slot %d %d %016llx %d\n", i, q, (unsigned long long)u, (int)sp[(size_t)i * np + q]);
        }
    std::printf("passes %d\n", P.passes);
    return 0;
}
