// Driver of tests/test_div2_cpu.py for fg_div2_prove / fg_div2 (fugue_amd/csrc/fg_div2.h).  Lines on stdin:
//     prove <b>          ->  <verdict 0|1> <Ch> <Cl>
//     eval <b> <a>       ->  <fma(a, Ch, a * Cl)> <a / b>        (Ch, Cl formed as the proof forms them, whatever its verdict)
// Every double travels as its 16-digit hexadecimal bit pattern.  Compiled with -ffp-contract=off like the library.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include "../../fugue_amd/csrc/fg_div2.h"

static double from_bits(uint64_t u) { double d; std::memcpy(&d, &u, 8); return d; }
static uint64_t to_bits(double d) { uint64_t u; std::memcpy(&u, &d, 8); return u; }

int main() {
    char cmd[16];
    uint64_t ub, ua;
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "prove")) {
            if (std::scanf("%" SCNx64, &ub) != 1) return 2;
            double hi = -1.0, lo = -1.0;
            const bool ok = fg_div2_prove(from_bits(ub), &hi, &lo);
            std::printf("%d %016" PRIx64 " %016" PRIx64 "\n", ok ? 1 : 0, to_bits(hi), to_bits(lo));
        } else if (!std::strcmp(cmd, "eval")) {
            if (std::scanf("%" SCNx64 " %" SCNx64, &ub, &ua) != 2) return 2;
            const double b = from_bits(ub), a = from_bits(ua);
            const double ch = 1.0 / b, cl = std::fma(-ch, b, 1.0) / b;
            std::printf("%016" PRIx64 " %016" PRIx64 "\n", to_bits(fg_div2(a, ch, cl)), to_bits(a / b));
        } else return 2;
    }
    return 0;
}
