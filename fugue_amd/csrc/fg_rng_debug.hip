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

// fg_debug_math -- the device's arithmetic primitives on the caller's operands, for tests/test_gpu_math_exact.py, which holds them to exact
// values (tests/golden/math_exact.json).  out: FG_DEBUG_MATH_ROWS rows of n 64-bit cells (doubles as their bits); rows an op does not
// name stay zero.  a, b, c: host arrays of n doubles (PAIR: a, b are the two 64-bit words of a Philox block).
// op 0 DIV (a, b, c = 1.0 / b formed on the host, as fg_program.cpp does): 0 fg_div_const(a, b, c) | 1 a / b
// op 1 LOG (a):      0 fg_fast_log_t<false> | 1 fg_fast_log_t<true> | 2 log
// op 2 SINCOS (a):   0, 1 sin, cos of fg_fast_sincos_t<false> | 2, 3 of fg_fast_sincos_t<true>
// op 3 PAIR (a, b):  0, 1 fg_normal_pair_of<false> | 2, 3 fg_normal_pair_of<true> | 4 fg_gaussian_z_of
// op 4 OCML (a, b):  0 log(a) | 1 log1p(a) | 2 lgamma(a) | 3 exp(a) | 4 pow(a, b) | 5 tan(a) -- what fg_logpdf and the samplers call
// op 5 DIGAMMA (a):  0 fg_digamma
#define FG_DEBUG_MATH_ROWS 6
#define FG_DEBUG_MATH_OPS 6
__global__ __launch_bounds__(256) void k_debug_math(int op, long long n, const double *a, const double *b, const double *c, unsigned long long *out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    auto put = [&](int row, double v) { out[(long long)row * n + i] = (unsigned long long)fg_as_i64(v); };
    if (op == 0) {
        const double x = a[i], d = b[i];
        put(0, fg_div_const(x, d, c[i])); put(1, x / d);
    } else if (op == 1) {
        const double x = a[i];
        put(0, fg_fast_log_t<false>(x)); put(1, fg_fast_log_t<true>(x)); put(2, log(x));
    } else if (op == 2) {
        const double x = a[i];
        double sn, cs;
        fg_fast_sincos_t<false>(x, sn, cs); put(0, sn); put(1, cs);
        fg_fast_sincos_t<true>(x, sn, cs); put(2, sn); put(3, cs);
    } else if (op == 3) {
        const unsigned long long wa = (unsigned long long)fg_as_i64(a[i]), wb = (unsigned long long)fg_as_i64(b[i]);
        double z0, z1;
        fg_normal_pair_of<false>(wa, wb, z0, z1); put(0, z0); put(1, z1);
        fg_normal_pair_of<true>(wa, wb, z0, z1); put(2, z0); put(3, z1);
        put(4, fg_gaussian_z_of(wa, wb));
    } else if (op == 4) {
        const double x = a[i];
        put(0, log(x)); put(1, log1p(x)); put(2, fg_lgamma(x)); put(3, exp(x)); put(4, pow(x, b[i])); put(5, tan(x));
    } else {
        put(0, fg_digamma(a[i]));
    }
}

// Host side: out is a host buffer of FG_DEBUG_MATH_ROWS * n cells; a (every op), b (DIV, PAIR, OCML) and c (DIV) are host arrays of n doubles.
extern "C" int fg_debug_math(int op, long long n, const double *a, const double *b, const double *c, unsigned long long *out) {
    if (n <= 0 || op < 0 || op >= FG_DEBUG_MATH_OPS || !out || !a || ((op == 0 || op == 3 || op == 4) && !b) || (op == 0 && !c)) return -1;
    double *d_in[3] = {nullptr, nullptr, nullptr};
    const double *h_in[3] = {a, b, c};
    unsigned long long *d_out = nullptr;
    const size_t wbytes = (size_t)n * 8, obytes = (size_t)FG_DEBUG_MATH_ROWS * wbytes;
    int rc = -1;
    do {
        if (hipMalloc(&d_out, obytes) != hipSuccess || hipMemset(d_out, 0, obytes) != hipSuccess) break;
        bool ok = true;
        for (int k = 0; k < 3 && ok; k++)
            if (h_in[k]) ok = hipMalloc(&d_in[k], wbytes) == hipSuccess && hipMemcpy(d_in[k], h_in[k], wbytes, hipMemcpyHostToDevice) == hipSuccess;
        if (!ok) break;
        hipLaunchKernelGGL(k_debug_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, n, d_in[0], d_in[1], d_in[2], d_out);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) break;
        if (hipMemcpy(out, d_out, obytes, hipMemcpyDeviceToHost) != hipSuccess) break;
        rc = 0;
    } while (0);
    for (int k = 0; k < 3; k++)
        if (d_in[k]) (void)hipFree(d_in[k]);
    if (d_out) (void)hipFree(d_out);
    return rc;
}
