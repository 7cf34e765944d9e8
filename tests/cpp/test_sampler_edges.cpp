// Host check of the samplers behind fg_sample_dist (fugue_amd/csrc/fg_math.h), meant for a build with
//   -ffp-contract=off -fsanitize=undefined,float-cast-overflow -fno-sanitize-recover=all
// so that any float-to-integer conversion out of range, signed overflow or other undefined behaviour ends the program:
//   1. the edge parameters of tests/sampler_cases.py (EDGES): the cell and the number of Philox blocks consumed;
//   2. 1e5 random valid parameter sets per family (the 16 families fg_sample_dist serves): discrete draws inside their support, no
//      NaN from a continuous family.
// Prints "sampler edges ok" and returns 0 when everything held.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include "../../fugue_amd/csrc/fg_math.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; if (failures < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

enum { BERNOULLI = 0, BETA = 1, BINOMIAL = 2, CAUCHY = 4, CHISQ = 5, DISCRETE_UNIFORM = 6, EXPONENTIAL = 7, GAMMA = 8, INVGAMMA = 9,
       LAPLACE = 10, LOGNORMAL = 11, NORMAL = 12, POISSON = 13, STUDENTT = 14, UNIFORM = 15, WEIBULL = 16 };

static void edge(const char *name, uint32_t kind, double p0, double p1, long long want, int want_blocks) {
    for (uint32_t chain = 0; chain < 64; chain++) {
        FgStream s = fg_stream(5, chain, 0, 1);
        const long long got = fg_sample_dist(kind, false, p0, p1, 0.0, s);
        CHECK(got == want, "%s chain %u: cell %lld, expected %lld", name, chain, got, want);
        if (want_blocks >= 0) CHECK((int)s.c1 == want_blocks, "%s chain %u: %u blocks, expected %d", name, chain, s.c1, want_blocks);
        else CHECK(s.c1 >= 1u && s.c1 < 100000u, "%s chain %u: %u blocks", name, chain, s.c1);
    }
}

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    edge("Binomial(0, 0.3)", BINOMIAL, 0.0, 0.3, 0, 0);
    edge("Binomial(7, 0)", BINOMIAL, 7.0, 0.0, 0, 0);
    edge("Binomial(7, 1)", BINOMIAL, 7.0, 1.0, 7, 0);
    edge("Poisson(inf)", POISSON, inf, 0.0, 0, 0);
    edge("Poisson(1e-300)", POISSON, 1e-300, 0.0, 0, 1);
    edge("Binomial(10, NaN)", BINOMIAL, 10.0, nan, 0, 0);
    edge("Binomial(10, +inf)", BINOMIAL, 10.0, inf, 0, 0);
    edge("Binomial(10, -inf)", BINOMIAL, 10.0, -inf, 0, 0);
    edge("Poisson(NaN)", POISSON, nan, 0.0, 0, 0);
    edge("Poisson(1e19)", POISSON, 1e19, 0.0, FG_I64_MAX, -1);          // every candidate lies above 2^63: saturates
    edge("Poisson(1e300)", POISSON, 1e300, 0.0, FG_I64_MAX, -1);
    edge("Poisson(f64 max)", POISSON, FG_F64_MAX, 0.0, FG_I64_MAX, -1);

    std::mt19937_64 g(20240607);
    auto unif = [&](double lo, double hi) { return lo + (hi - lo) * ((double)(g() >> 11) * 0x1.0p-53); };
    auto logu = [&](double lo, double hi) { return std::exp(unif(std::log(lo), std::log(hi))); };
    const int N = 100000;
    long long checksum = 0;
    for (int i = 0; i < N; i++) {
        const uint32_t chain = (uint32_t)i;
        auto f64 = [&](uint32_t kind, double p0, double p1, double p2, const char *name) {
            FgStream s = fg_stream(11, chain, (uint32_t)kind, 1);
            const long long c = fg_sample_dist(kind, false, p0, p1, p2, s);
            const double x = fg_as_double(c);
            CHECK(x == x, "%s(%.17g, %.17g, %.17g) chain %u: NaN", name, p0, p1, p2, chain);
            CHECK(s.c1 >= 1u && s.c1 < 4000u, "%s chain %u: %u blocks", name, chain, s.c1);
            checksum ^= c;
            return x;
        };
        f64(NORMAL, unif(-5, 5), logu(1e-2, 10), 0, "Normal");
        { const double lo = unif(-5, 5); const double x = f64(UNIFORM, lo, lo + logu(1e-3, 10), 0, "Uniform"); CHECK(x >= lo, "Uniform below lo"); }
        CHECK(f64(LOGNORMAL, unif(-2, 2), logu(1e-2, 2), 0, "LogNormal") > 0.0, "LogNormal <= 0");
        CHECK(f64(EXPONENTIAL, logu(1e-3, 1e3), 0, 0, "Exponential") >= 0.0, "Exponential < 0");
        { const double x = f64(BETA, logu(0.05, 100), logu(0.05, 100), 0, "Beta"); CHECK(x >= 0.0 && x <= 1.0, "Beta outside [0, 1]: %.17g", x); }
        CHECK(f64(GAMMA, logu(1e-2, 1e3), logu(1e-3, 1e3), 0, "Gamma") >= 0.0, "Gamma < 0");
        f64(STUDENTT, logu(0.1, 100), unif(-5, 5), logu(1e-2, 10), "StudentT");
        f64(CAUCHY, unif(-5, 5), logu(1e-2, 10), 0, "Cauchy");
        f64(LAPLACE, unif(-5, 5), logu(1e-2, 10), 0, "Laplace");
        CHECK(f64(WEIBULL, logu(0.1, 10), logu(1e-2, 10), 0, "Weibull") >= 0.0, "Weibull < 0");
        CHECK(f64(CHISQ, logu(1e-2, 100), 0, 0, "ChiSquared") >= 0.0, "ChiSquared < 0");
        CHECK(f64(INVGAMMA, logu(0.1, 100), logu(1e-3, 1e3), 0, "InverseGamma") >= 0.0, "InverseGamma < 0");
        {   // Bernoulli, the end points now and then
            const double p = (i % 97 == 0) ? 0.0 : (i % 89 == 0) ? 1.0 : unif(0, 1);
            FgStream s = fg_stream(11, chain, BERNOULLI, 1);
            const long long c = fg_sample_dist(BERNOULLI, false, p, 0, 0, s);
            CHECK((c == 0 || c == 1) && s.c1 == 1u, "Bernoulli(%.17g): %lld after %u blocks", p, c, s.c1);
            checksum ^= c;
        }
        {   // Binomial: n from 1 to 1e9, p over [0, 1] with the end points, 1/2 and its neighbours now and then
            const double n = std::floor(logu(1.0, 1e9));
            double p = unif(0, 1);
            if (i % 97 == 0) p = 0.0; else if (i % 89 == 0) p = 1.0; else if (i % 83 == 0) p = 0.5; else if (i % 79 == 0) p = std::nextafter(0.5, 1.0);
            else if (i % 5 == 0) p = logu(1e-12, 0.5); else if (i % 7 == 0) p = 1.0 - logu(1e-12, 0.5);
            FgStream s = fg_stream(11, chain, BINOMIAL, 1);
            const long long c = fg_sample_dist(BINOMIAL, false, n, p, 0, s);
            CHECK(c >= 0 && c <= (long long)n && s.c1 < 1000u, "Binomial(%.0f, %.17g): %lld after %u blocks", n, p, c, s.c1);
            checksum ^= c;
        }
        {   // Poisson: both branches, 30 and its predecessor now and then, up to 1e18 (below 2^63: no saturation for a valid draw)
            double lam = logu(1e-3, 1e18);
            if (i % 97 == 0) lam = 30.0; else if (i % 89 == 0) lam = std::nextafter(30.0, 0.0); else if (i % 3 == 0) lam = logu(1e-3, 60.0);
            FgStream s = fg_stream(11, chain, POISSON, 1);
            const long long c = fg_sample_dist(POISSON, false, lam, 0, 0, s);
            CHECK(c >= 0 && c < FG_I64_MAX && s.c1 >= 1u && s.c1 < 1000u, "Poisson(%.17g): %lld after %u blocks", lam, c, s.c1);
            if (lam > 1e3) CHECK(std::fabs((double)c - lam) < 12.0 * std::sqrt(lam), "Poisson(%.17g): %lld is more than 12 sd from the mean", lam, c);
            checksum ^= c;
        }
        {   // DiscreteUniform: bounds as doubles (site-fed form) and as exact bit patterns (hoisted form), the full range included
            long long lo = (long long)g(), hi = (long long)g();
            if (i % 5 == 0) { lo = (long long)(g() % 2001) - 1000; hi = lo + (long long)(g() % 1000); }
            if (lo > hi) { const long long t = lo; lo = hi; hi = t; }
            if (i % 97 == 0) { lo = FG_I64_MIN; hi = FG_I64_MAX; }
            FgStream s = fg_stream(11, chain, DISCRETE_UNIFORM, 1);
            const long long c = fg_sample_dist(DISCRETE_UNIFORM, true, fg_as_double(lo), fg_as_double(hi), 0, s);
            CHECK(c >= lo && c <= hi && s.c1 == 1u, "DiscreteUniform[%lld, %lld] hoisted: %lld", lo, hi, c);
            FgStream s2 = fg_stream(11, chain, DISCRETE_UNIFORM, 1);
            const long long lo2 = fg_f2i_sat((double)lo), hi2 = fg_f2i_sat((double)hi);
            const long long c2 = fg_sample_dist(DISCRETE_UNIFORM, false, (double)lo, (double)hi, 0, s2);
            CHECK((hi2 < lo2 && c2 == lo2) || (c2 >= lo2 && c2 <= hi2), "DiscreteUniform[%lld, %lld] as doubles: %lld", lo, hi, c2);
            checksum ^= c ^ c2;
        }
    }
    std::printf("checksum %016llx, failures %d\n", (unsigned long long)checksum, failures);
    if (failures) return 1;
    std::printf("sampler edges ok\n");
    return 0;
}
