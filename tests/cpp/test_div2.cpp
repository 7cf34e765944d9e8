// fg_div2 (fugue_amd/csrc/fg_div2.h: fma(a, Ch, RN(a Cl))) must give the bits of IEEE division for every divisor that
// fg_div2_prove accepts: 2e7 quotients over the divisors the engine uses (2h for the usual h, sigmas such as 0.8, 2.5, 0.7, 1/3)
// and a pool of random accepted divisors -- numerators random over the binades of [2^-823, 2^953), numerators b (k + 1/2), and
// numerators solved from the congruence of the proof for odd |delta| up to 255 (the closest to a midpoint that exist).
// The five divisors known to fail must be refused, with the edge cases.  Compiled with -ffp-contract=off like the library.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../fugue_amd/csrc/fg_div2.h"

static uint64_t s[2] = {0x9E3779B97F4A7C15ull, 0xD1B54A32D192ED03ull};
static uint64_t nxt() { uint64_t a = s[0], b = s[1]; s[0] = b; a ^= a << 23; s[1] = a ^ b ^ (a >> 17) ^ (b >> 26); return s[1] + b; }
static double rnd(int emin, int emax) {
    uint64_t bits = ((uint64_t)(emin + (int)(nxt() % (uint64_t)(emax - emin + 1)) + 1023) << 52) | (nxt() & 0xFFFFFFFFFFFFFull);
    if (nxt() & 1) bits |= 1ull << 63;
    double d; memcpy(&d, &bits, 8); return d;
}
struct Div { double b, ch, cl; uint64_t B; int z; uint64_t inv[2]; };

int main() {
    typedef unsigned __int128 u128;
    const double fixed[] = {2e-5, 2e-4, 2e-6, 2e-3, 6e-5, 2e-7, 1e-5, 0.8, 2.5, 0.7, 1.0 / 3.0, 3.0, 0.3, 0.1, 7.0, 1e5};
    const double failing[] = {0x1.f86664b036c57p-11, 0x1.adff816a7d897p-6, 0x1.7a243b2332317p-22, 0x1.b555b9e69c5a7p-14, 0x1.ab9b08cf72eafp-15};
    long bad = 0, n = 0, refused = 0;
    std::vector<Div> pool;
    auto admit = [&](double b) {
        Div d; d.b = b;
        if (!fg_div2_prove(b, &d.ch, &d.cl)) { refused++; return false; }
        uint64_t u; memcpy(&u, &b, 8);
        d.B = (u & 0xfffffffffffffull) | (1ull << 52); d.z = 0;
        while (!(d.B & 1ull)) { d.B >>= 1; d.z++; }
        for (int sc = 0; sc < 2; sc++) {
            uint64_t inv = 1 % d.B; const uint64_t inv2 = (d.B + 1) >> 1;
            for (int k = 0; k < 52 - d.z + sc; k++) inv = (uint64_t)((u128)inv * inv2 % d.B);
            d.inv[sc] = inv;
        }
        pool.push_back(d); return true;
    };
    for (double b : fixed) if (!admit(b)) { std::printf("refused an engine divisor %a\n", b); bad++; }
    const long n_fixed = (long)pool.size();
    for (int i = 0; i < 6000; i++) admit(std::fabs(rnd(-40, 40)));
    for (long i = 0; i < 20000000L; i++) {
        const Div &d = (i % 4 == 0) ? pool[(size_t)((i / 4) % n_fixed)] : pool[(size_t)(nxt() % pool.size())];
        double a = rnd(-823, 952);
        if (i % 3 == 0) { const double k = (double)(nxt() & 0xFFFFFFFFFFFFull) + 0.5; a = d.b * k; }           // quotient near a midpoint
        else if (i % 3 == 1 && d.B >= (1ull << 40)) {                                                             // the nearest there are: |delta| odd, <= 255
            const int sc = (int)(nxt() & 1), delta = (int)(nxt() % 256) | 1;
            const uint64_t t = (nxt() & 2) ? (d.B - (uint64_t)delta) >> 1 : (d.B + (uint64_t)delta) >> 1;
            uint64_t X = (uint64_t)((u128)(t % d.B) * d.inv[sc] % d.B);
            if (X < (1ull << 52)) X += ((1ull << 52) - X + d.B - 1) / d.B * d.B;
            if (X < (1ull << 53)) { a = std::ldexp((double)X, -52 + (int)(nxt() % 1700) - 823); if (nxt() & 1) a = -a; }
        }
        const double aa = std::fabs(a);
        if (!(aa >= 0x1p-823 && aa < 0x1p953)) continue;
        if (fg_div2(a, d.ch, d.cl) != a / d.b) { if (bad < 10) std::printf("mismatch: %a / %a\n", a, d.b); bad++; }
        n++;
    }
    // the known failing divisors, an all-ones significand, exponents outside [-70, 147], zero, negative and non-finite divisors are refused
    for (double b : failing) if (fg_div2_prove(b, nullptr, nullptr)) bad++;
    uint64_t ones = 0x3FEFFFFFFFFFFFFFull; double bo; memcpy(&bo, &ones, 8);
    if (fg_div2_prove(bo, nullptr, nullptr) || fg_div2_prove(0x1p-71, nullptr, nullptr) || fg_div2_prove(0x1p148, nullptr, nullptr) ||
        fg_div2_prove(0.0, nullptr, nullptr) || fg_div2_prove(-2e-5, nullptr, nullptr) || fg_div2_prove(INFINITY, nullptr, nullptr) ||
        fg_div2_prove(NAN, nullptr, nullptr) || !fg_div2_prove(0x1p-70, nullptr, nullptr) || !fg_div2_prove(0x1.8p147, nullptr, nullptr)) bad++;
    std::printf("checked %ld quotients over %zu divisors (%ld refused), mismatches %ld\n", n, pool.size(), refused, bad);
    return bad ? 1 : 0;
}
