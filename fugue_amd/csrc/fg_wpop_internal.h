// fg_wpop_internal.h -- what the units that work on a fg_wpop handle share (fg_wpop.hip: moments, quantiles, tables; fg_wpop_eval.hip:
// predictive checks and WAIC / IS-LOO): the handle itself, the device buffers of one call, the block's min / max of keys.
#pragma once
#include "fg_engine_internal.h"
#include "fg_wpop_plan.h"

#define FG_WP_WAVES (FG_WP_THREADS / 64)

struct fg_wpop {
    fg_engine *e = nullptr;
    long long n = 0;
    double *d_w = nullptr;                   // [n] the weights as they were at fg_wpop_new
    unsigned long long *d_q = nullptr;       // [n] their units
    uint64_t T = 0, n_bad = 0, n_zero = 0;
};

// min / max of a block's keys: wave reduction, LDS, then thread 0 holds them (a > z: the block saw none)
__device__ __forceinline__ void wp_block_minmax(unsigned long long &a, unsigned long long &z, unsigned long long (*mm)[2]) {
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long a2 = __shfl_down(a, o, 64), z2 = __shfl_down(z, o, 64);
        a = a2 < a ? a2 : a; z = z2 > z ? z2 : z;
    }
    if ((threadIdx.x & 63) == 0) { mm[threadIdx.x >> 6][0] = a; mm[threadIdx.x >> 6][1] = z; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int v = 1; v < FG_WP_WAVES; ++v) { a = mm[v][0] < a ? mm[v][0] : a; z = mm[v][1] > z ? mm[v][1] : z; }
}

namespace {

struct WpScope {                             // device buffers of one call
    std::vector<void *> p;
    ~WpScope() { for (void *q : p) (void)hipFree(q); }
    template <typename T>
    int alloc(T **out, size_t n, const char *what) {
        if (hipMalloc((void **)out, (n ? n : 1) * sizeof(T)) != hipSuccess) { fg_set_error(std::string("fg_wpop: no device memory for ") + what); return FG_E_HIP; }
        p.push_back(*out);
        return FG_OK;
    }
};

int need_wpop(const fg_wpop *h) {
    if (!h || !h->e) { fg_set_error("null weighted population"); return FG_E_BAD_ARG; }
    if (hipSetDevice(h->e->device) != hipSuccess) { fg_set_error("hipSetDevice failed"); return FG_E_HIP; }
    return FG_OK;
}

}  // namespace
