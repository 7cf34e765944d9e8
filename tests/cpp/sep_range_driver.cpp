// Driver of tests/test_sep_range_cpu.py for fg_sep_range_bound / fg_sep_range_prove (fugue_amd/csrc/fg_sep_range.h).  Lines on stdin:
//     bound <h> <nrec> (<c> <s> <lns>) x nrec                      ->  <verdict 0|1> <bound>
//     prove <h> <ncoord> (<nrec> (<c> <s> <lns>) x nrec) x ncoord  ->  <verdict 0|1> <worst bound>
//     n <h> <q> <u0 0|1> <nrec> (<c> <s> <lns>) x nrec             ->  <n>   the numerator tp - tm of one step of the folded loop as the
//                        kernel forms it (fg_hmc_sep.hip, FG_SEP_DUALS / FG_SEP_LPF_U: s a power of two, nhs2 = -0.5 s^2; u0: record 0 is N(0, 1))
// Every double travels as its 16-digit hexadecimal bit pattern.  Compiled with -ffp-contract=off like the library.  With --self-check
// it runs a small check of its own instead (the sanitizer build's second run).
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../fugue_amd/csrc/fg_sep_range.h"

static double from_bits(uint64_t u) { double d; std::memcpy(&d, &u, 8); return d; }
static uint64_t to_bits(double d) { uint64_t u; std::memcpy(&u, &d, 8); return u; }
static bool rd(double *x) { uint64_t u; if (std::scanf("%" SCNx64, &u) != 1) return false; *x = from_bits(u); return true; }

struct Recs { std::vector<double> c, s, lns; };
static bool rd_recs(int nrec, Recs *r) {
    for (int k = 0; k < nrec; ++k) {
        double c, s, l;
        if (!rd(&c) || !rd(&s) || !rd(&l)) return false;
        r->c.push_back(c); r->s.push_back(s); r->lns.push_back(l);
    }
    return true;
}

static const double K = FG_SEP_RANGE_HALF_LN_2PI;
static double side(double x, bool u0, const Recs &r) {           // one side of the folded loop: log_prior + log_likelihood at x
    const int nrec = (int)r.c.size();
    auto term = [&](int k) { const double d = x - r.c[k]; return std::fma(-0.5 * r.s[k] * r.s[k], d * d, -r.lns[k]) - K; };
    double t = u0 ? std::fma(-0.5, x * x, -K) : term(0);
    if (nrec > 1) {
        double sp = term(1);
        if (nrec > 2) sp += term(2);
        if (nrec > 3) sp += term(3);
        t = t + sp;
    }
    return t;
}

static int self_check() {
    const double c[2] = {0.0, 1.0}, s[2] = {1.0, 2.0}, l[2] = {0.0, std::log(0.5)};
    const int off[1] = {0}, n[1] = {2};
    double w = -1.0;
    if (!fg_sep_range_prove(1e-5, 1, off, n, c, s, l, &w) || !(w > 0x1p70 && w < 0x1p90)) return 1;
    const double cb[2] = {0.0, 0x1.8p510};
    if (fg_sep_range_prove(1e-5, 1, off, n, cb, s, l, &w)) return 1;
    if (fg_sep_range_prove(0.0, 1, off, n, c, s, l, &w) || fg_sep_range_prove(1e-5, 0, off, n, c, s, l, &w)) return 1;
    std::printf("self-check ok\n");
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && !std::strcmp(argv[1], "--self-check")) return self_check();
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        double h;
        int a = 0, b = 0;
        if (!std::strcmp(cmd, "bound")) {
            Recs r;
            if (!rd(&h) || std::scanf("%d", &a) != 1 || a < 0 || a > 64 || !rd_recs(a, &r)) return 2;
            const double bd = fg_sep_range_bound(h, a, r.c.data(), r.s.data(), r.lns.data());
            std::printf("%d %016" PRIx64 "\n", fg_sep_range_ok(h, bd) ? 1 : 0, to_bits(bd));
        } else if (!std::strcmp(cmd, "prove")) {
            Recs r;
            std::vector<int> off, n;
            if (!rd(&h) || std::scanf("%d", &a) != 1 || a < 0 || a > 4096) return 2;
            for (int j = 0; j < a; ++j) {
                if (std::scanf("%d", &b) != 1 || b < 0 || b > 64) return 2;
                off.push_back((int)r.c.size()); n.push_back(b);
                if (!rd_recs(b, &r)) return 2;
            }
            double w = -1.0;
            const bool ok = fg_sep_range_prove(h, (size_t)a, off.data(), n.data(), r.c.data(), r.s.data(), r.lns.data(), &w);
            std::printf("%d %016" PRIx64 "\n", ok ? 1 : 0, to_bits(w));
        } else if (!std::strcmp(cmd, "n")) {
            Recs r;
            double q;
            if (!rd(&h) || !rd(&q) || std::scanf("%d %d", &b, &a) != 2 || a < 1 || a > 4 || !rd_recs(a, &r)) return 2;
            const double qp = q + h, qm = q - h;
            std::printf("%016" PRIx64 "\n", to_bits(side(qp, b != 0, r) - side(qm, b != 0, r)));
        } else return 2;
    }
    return 0;
}
