// fg_rng_debug.hip -- a debug entry point (not in the public header, like fg_debug_hmc_prof) that evaluates the momentum draw of the
// samplers in its earlier and its present form side by side, for tests/test_gpu_rng_identity.py.
//
// "old": the pair as it was before the key schedule went scalar -- the generic Philox (vector keys, two xors per round), log and sincos
// with the compiler's own choice of constant operands, ocml's sqrt with its range scaling.  It is reachable from here only.
// "new": fg_cold_normal_pair / fg_cold_u01_pair / fg_philox4x32_10_ukey / fg_sqrt_pos as the units that define FG_COLD_UKEY compile them
// (fg_hmc_sep.hip, fg_hmc_lin.hip; here this unit's own static copies, compiled with the library's flags).
#include <hip/hip_runtime.h>
#define FG_COLD_UKEY 1        /* the short forms are what this unit is about; k_rng_debug passes a kernel argument as the key */
#include "fg_cold.h"

static __device__ __noinline__ void fg_old_words(uint32_t k0, uint32_t k1, uint32_t chain, uint32_t block, uint32_t iter, uint32_t purpose,
                                                 unsigned long long &a, unsigned long long &b) {
    FgStream s; s.k0 = k0; s.k1 = k1; s.c0 = chain; s.c1 = block; s.c2 = iter; s.c3 = purpose;
    fg_rng_block(s, a, b);
}
static __device__ __noinline__ FgD2 fg_old_pair_of(unsigned long long a, unsigned long long b) {
    double u1 = ((double)(a >> 11) + 1.0) * 0x1.0p-53;
    double u2 = fg_u01_of(b);
    double r = sqrt(-2.0 * fg_fast_log(u1));
    double th = 2.0 * M_PI * u2;
    double sn, cs;
    fg_fast_sincos(th, sn, cs);
    FgD2 z; z.a = r * cs; z.b = r * sn;
    return z;
}
static __device__ __noinline__ FgD2 fg_old_normal_pair(uint32_t k0, uint32_t k1, uint32_t chain, uint32_t block, uint32_t iter, uint32_t purpose) {
    FgStream s; s.k0 = k0; s.k1 = k1; s.c0 = chain; s.c1 = block; s.c2 = iter; s.c3 = purpose;
    unsigned long long a, b;
    fg_rng_block(s, a, b);
    return fg_old_pair_of(a, b);
}
static __device__ __noinline__ FgD2 fg_new_pair_of(unsigned long long a, unsigned long long b) {
    FgD2 z;
    fg_normal_pair_of<true>(a, b, z.a, z.b);
    return z;
}

// out: FG_RNG_DEBUG_ROWS rows of n 64-bit cells (doubles as their bits).
// mode 0 (counters; lane i is chain chain0 + i):  0, 1 old normal pair | 2, 3 new normal pair | 4, 5 old Philox words | 6, 7 new Philox words |
//                                                 8, 9 old uniforms | 10, 11 new uniforms (fg_cold_u01_pair)
// mode 1 (the two words given, wa / wb):          0, 1 old normal pair | 2, 3 new normal pair | 4 the root's argument -2 ln u1 |
//                                                 5 fg_sqrt_pos of it | 6 sqrt of it
// mode 2 (wa holds the bits of a double x):       0 fg_sqrt_pos(x) | 1 sqrt(x)
#define FG_RNG_DEBUG_ROWS 12
__global__ __launch_bounds__(256) void k_rng_debug(int mode, long long n, uint32_t k0, uint32_t k1, uint32_t chain0, uint32_t block, uint32_t iter, uint32_t purpose,
                                                   const unsigned long long *wa, const unsigned long long *wb, unsigned long long *out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;                                   // a partial last wave: the cold functions run with inactive lanes
    auto put = [&](int row, double v) { out[(long long)row * n + i] = (unsigned long long)fg_as_i64(v); };
    if (mode == 0) {
        const uint32_t chain = chain0 + (uint32_t)i;
        const FgD2 zo = fg_old_normal_pair(k0, k1, chain, block, iter, purpose), zn = fg_cold_normal_pair(k0, k1, chain, block, iter, purpose);
        put(0, zo.a); put(1, zo.b); put(2, zn.a); put(3, zn.b);
        unsigned long long a, b;
        fg_old_words(k0, k1, chain, block, iter, purpose, a, b);
        uint32_t o[4];
        fg_philox4x32_10_ukey(chain, block, iter, purpose, k0, k1, o);
        out[4 * n + i] = a; out[5 * n + i] = b;
        out[6 * n + i] = (unsigned long long)o[0] | ((unsigned long long)o[1] << 32);
        out[7 * n + i] = (unsigned long long)o[2] | ((unsigned long long)o[3] << 32);
        const FgD2 un = fg_cold_u01_pair(k0, k1, chain, block, iter, purpose);
        put(8, fg_u01_of(a)); put(9, fg_u01_of(b)); put(10, un.a); put(11, un.b);
    } else if (mode == 1) {
        const unsigned long long a = wa[i], b = wb[i];
        const FgD2 zo = fg_old_pair_of(a, b), zn = fg_new_pair_of(a, b);
        put(0, zo.a); put(1, zo.b); put(2, zn.a); put(3, zn.b);
        const double x = -2.0 * fg_fast_log(((double)(a >> 11) + 1.0) * 0x1.0p-53);
        put(4, x); put(5, fg_sqrt_pos(x)); put(6, sqrt(x));
    } else {
        const double x = fg_as_double((long long)wa[i]);
        put(0, fg_sqrt_pos(x)); put(1, sqrt(x));
    }
}

// Host side: out is a host buffer of FG_RNG_DEBUG_ROWS * n cells; wa / wb are host arrays of n words (modes 1, 2) or null.
extern "C" int fg_debug_rng_pairs(int mode, long long n, unsigned long long seed, uint32_t chain0, uint32_t block, uint32_t iter, uint32_t purpose,
                                  const unsigned long long *wa, const unsigned long long *wb, unsigned long long *out) {
    if (n <= 0 || mode < 0 || mode > 2 || !out || (mode >= 1 && !wa) || (mode == 1 && !wb)) return -1;
    unsigned long long *d_a = nullptr, *d_b = nullptr, *d_out = nullptr;
    const size_t wbytes = (size_t)n * 8, obytes = (size_t)FG_RNG_DEBUG_ROWS * wbytes;
    int rc = -1;
    do {
        if (hipMalloc(&d_out, obytes) != hipSuccess || hipMemset(d_out, 0, obytes) != hipSuccess) break;
        if (wa && (hipMalloc(&d_a, wbytes) != hipSuccess || hipMemcpy(d_a, wa, wbytes, hipMemcpyHostToDevice) != hipSuccess)) break;
        if (wb && (hipMalloc(&d_b, wbytes) != hipSuccess || hipMemcpy(d_b, wb, wbytes, hipMemcpyHostToDevice) != hipSuccess)) break;
        hipLaunchKernelGGL(k_rng_debug, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, mode, n, (uint32_t)seed, (uint32_t)(seed >> 32), chain0, block, iter,
                           purpose, d_a, d_b, d_out);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) break;
        if (hipMemcpy(out, d_out, obytes, hipMemcpyDeviceToHost) != hipSuccess) break;
        rc = 0;
    } while (0);
    if (d_a) (void)hipFree(d_a);
    if (d_b) (void)hipFree(d_b);
    if (d_out) (void)hipFree(d_out);
    return rc;
}
