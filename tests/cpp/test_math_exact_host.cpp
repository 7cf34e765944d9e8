// Host build of the primitives that tests/test_gpu_math_exact.py holds to exact values on the device, with the same assertions
// (tests/test_math_exact_cpu.py compiles and runs this): the window of fg_div_const's bitwise claim, and fg_digamma against the exact
// values of tests/golden/math_exact.json, which the Python side passes as a text file of "a hi lo" hex words (argv[1]).
//
// fg_div_const(a, b, RN(1/b)) for an admitted divisor (fg_div_const_ok):
//   * inside the window -- the IEEE quotient finite and normal, |a| >= 2^-968, |a / b| < 2^1020 -- it is a / b bit for bit;
//   * where a / b overflows, it is not finite;
//   * below the window (|a| < 2^-968) the residual a - q b is no longer exact in the FMA, the result is finite and within two ulps of
//     a / b, and within 2^-1022 of it wherever |a / b| < 2^-970 (two ulps there are less).  The window's lower edge is needed: some
//     quotients below it are misrounded.
// Compiled with -ffp-contract=off like the library.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "../../fugue_amd/csrc/fg_math.h"

static uint64_t s[2] = {0x9E3779B97F4A7C15ull, 0xD1B54A32D192ED03ull};
static uint64_t nxt() { uint64_t a = s[0], b = s[1]; s[0] = b; a ^= a << 23; s[1] = a ^ b ^ (a >> 17) ^ (b >> 26); return s[1] + b; }
static double rnd(int emin, int emax) {
    uint64_t bits = ((uint64_t)(emin + (int)(nxt() % (uint64_t)(emax - emin + 1)) + 1023) << 52) | (nxt() & 0xFFFFFFFFFFFFFull);
    if (nxt() & 1) bits |= 1ull << 63;
    double d; memcpy(&d, &bits, 8); return d;
}
static double ulp_of(double q) { int e; frexp(q, &e); return ldexp(1.0, (e - 53 < -1074) ? -1074 : e - 53); }

int main(int argc, char **argv) {
    // ---- DIV ----
    const int ranges[][4] = {{-968, -940, -399, 399}, {-968, -940, -40, 40}, {-1022, 1023, -399, 399}, {-1022, -990, -40, 40}, {-1022, -969, -399, 399}};
    long bad = 0, n_in = 0, n_below = 0, n_over = 0, misrounded_below = 0;
    for (const auto &R : ranges)
        for (long i = 0; i < 400000; i++) {
            const double b = rnd(R[2], R[3]);
            if (!fg_div_const_ok(b)) continue;
            const double a = rnd(R[0], R[1]), q = a / b, g = fg_div_const(a, b, 1.0 / b);
            if (!std::isfinite(q)) { n_over++; if (std::isfinite(g)) bad++; continue; }
            if (std::fabs(a) >= 0x1p-968) {
                if (std::fabs(q) >= 0x1p-1022 && std::fabs(q) < 0x1p1020) { n_in++; if (g != q) bad++; }
                continue;
            }
            n_below++;
            if (g != q) misrounded_below++;
            if (!std::isfinite(g)) { bad++; continue; }
            const double e = std::fabs(g - q);
            if (e > 2.0 * ulp_of(q) || (std::fabs(q) < 0x1p-970 && e > 0x1p-1022)) bad++;
        }
    if (n_in < 900000 || n_below < 500000 || n_over < 1000 || misrounded_below == 0) bad++;
    std::printf("div: %ld in the window, %ld below it (%ld misrounded), %ld overflowing, failures %ld\n", n_in, n_below, misrounded_below, n_over, bad);

    // ---- DIGAMMA ----
    long n_dg = 0, bad_dg = 0;
    double worst = 0.0, worst_at = 0.0;
    if (argc > 1) {
        FILE *f = std::fopen(argv[1], "r");
        if (!f) { std::printf("cannot read %s\n", argv[1]); return 2; }
        unsigned long long ua, uh; unsigned ul;
        while (std::fscanf(f, "%llx %llx %x", &ua, &uh, &ul) == 3) {
            double a, hi; float lo;
            memcpy(&a, &ua, 8); memcpy(&hi, &uh, 8); memcpy(&lo, &ul, 4);
            const double err = std::fabs((fg_digamma(a) - hi) - (double)lo), rel = err / std::fmax(1.0, std::fabs(hi));
            if (!(rel <= 1e-12)) bad_dg++;
            if (rel > worst) { worst = rel; worst_at = a; }
            n_dg++;
        }
        std::fclose(f);
        if (n_dg < 100) bad_dg++;
    }
    std::printf("digamma: %ld points, worst |err| / max(1, |psi|) %.3g at %.17g, failures %ld\n", n_dg, worst, worst_at, bad_dg);
    if (bad == 0 && bad_dg == 0) std::printf("math exact host ok\n");
    return (bad || bad_dg) ? 1 : 0;
}
