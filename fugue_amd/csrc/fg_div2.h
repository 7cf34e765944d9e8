// fg_div2.h -- host only: the proof that a / b, for ONE divisor b that stays fixed for a run, is the two-instruction
//     fg_div2(a, Ch, Cl) = fma(a, Ch, RN(a Cl)),   Ch = RN(1 / b), Cl = RN(1 / b - Ch)
// bit for bit (Brisebarre & Muller, "Correctly rounded multiplication by arbitrary precision constants", IEEE TC 2008,
// here with C = 1 / b).  Plain C++ without a HIP call: the engine runs it once per configuration (fg_internal_hmc_set_cfg)
// and tests/cpp/div2_driver.cpp builds it with g++.  Build with -ffp-contract=off like the rest.
//
// The argument ("The short quotient"):
//   * r = fma(-Ch, b, 1) is exact and (1 / b - Ch) = r / b, so Cl = r / b IS RN(1 / b - Ch).
//   * the form computes RN(a / b + E), |E| <= |a| |1 / b - Ch| (2^-52 + 2^-106) < (2^-52 + 2^-106) ulp(a / b): it can differ
//     from RN(a / b) only when a / b lies that close to a midpoint between two doubles.
//   * with b's significand B 2^z (B odd), a's significand X in [2^52, 2^53) and the scaling s in {52 - z, 53 - z} that puts
//     X 2^s / B in [2^52, 2^53), write X 2^(s+1) = (2k + 1) B + delta: a / b is |delta| / (2 B) ulp from the midpoint k + 1/2.
//     delta is odd (the left side is even, B is odd), and B < 2^53: the distance is above |delta| 2^-54 ulp, only |delta| <= 4
//     can fail.  A divisor with B < 2^50 has no numerator within 2^-51 ulp of a midpoint at all.
//   * so: for every odd delta in [-8, 8] (twice the need) with |delta| <= B 2^-50 and both scalings, every solution X in the
//     binade of X 2^s = (B + delta) / 2 (mod B) -- at most five per class -- is put through both forms here.  All agree: the
//     form is correctly rounded for every a whose quotient stays clear of under- and overflow.  One disagrees: refused.
//   * range: callers keep |a| in [2^-823, 2^953) (fg_sep_trajectory's window).  The unbiased exponent e of b must lie in
//     [-70, 147]: e >= -70 keeps a / b < 2^1023, and e <= 147 keeps a / b >= 2^-971, where ulp(a / b) >= 2^-1023 -- an a Cl
//     that underflows is off by at most 2^-1075 <= 2^-52 ulp(a / b), which the doubled delta range covers (every numerator
//     not tested lies more than 2^-51 ulp from a midpoint: 2^-51 > 2^-52 + 2^-106 + 2^-52).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include "fg_math.h"

// the two-instruction quotient as the kernels issue it (host build: tests and the proof)
inline double fg_div2(double a, double ch, double cl) { return std::fma(a, ch, a * cl); }

inline bool fg_div2_prove(double b, double *hi, double *lo) {
    if (hi) *hi = 0.0;
    if (lo) *lo = 0.0;
    if (!(b > 0.0) || !std::isfinite(b) || !fg_div_const_ok(b)) return false;      // (zero, negative, NaN, inf, all-ones significand, |e| >= 400)
    uint64_t u; std::memcpy(&u, &b, 8);
    const int e = (int)((u >> 52) & 0x7ffu) - 1023;
    if (e < -70 || e > 147) return false;
    const double ch = 1.0 / b;
    const double r = std::fma(-ch, b, 1.0);
    const double cl = r / b;
    uint64_t B = (u & 0xfffffffffffffull) | (1ull << 52);
    int z = 0;
    while (!(B & 1ull)) { B >>= 1; ++z; }
    typedef unsigned __int128 u128;
    const uint64_t inv2 = (B + 1) >> 1;                                             // 2^-1 mod B (B odd; B = 1: 0)
    for (int sc = 0; sc < 2 && B > 1; ++sc) {
        const int s = 52 - z + sc;
        uint64_t inv = 1 % B;                                                       // 2^-s mod B
        for (int k = 0; k < s; ++k) inv = (uint64_t)((u128)inv * inv2 % B);
        for (int delta = -7; delta <= 7; delta += 2) {
            const uint64_t ad = (uint64_t)(delta < 0 ? -delta : delta);
            if ((ad << 50) > B) continue;                                           // |delta| / (2 B) > 2^-51 ulp: never near enough
            const uint64_t t = delta < 0 ? (B - ad) >> 1 : (B + ad) >> 1;          // (B + delta) / 2, in [0, B]
            uint64_t X = (uint64_t)((u128)(t % B) * inv % B);                       // X = t 2^-s (mod B)
            if (X < (1ull << 52)) X += ((1ull << 52) - X + B - 1) / B * B;          // the first solution in the binade
            for (; X < (1ull << 53); X += B) {
                const double a = std::ldexp((double)X, -52);                        // in [1, 2): a / b and a Cl are normal for every admitted e
                if (fg_div2(a, ch, cl) != a / b || fg_div2(-a, ch, cl) != -a / b) return false;
            }
        }
    }
    if (hi) *hi = ch;
    if (lo) *lo = cl;
    return true;
}
