// fg_diag_qstream.hip -- summarize_f64_parameter's quantiles (diagnostics.rs:355-371) without stored draws: an exact radix select
// over a run that is presented once per pass (the sampling phase replayed from fg_state_export's blob) and never stored.  The
// selection rule, the slot state and both ends of a pass are fg_diag_qstream_plan.h's (plain C++); here are the two kernels that
// see the draws, the device tables of a pass and the C ABI.  This engine's chains only: sharded runs keep fg_diag_quantiles.
//
// Device state of a pass, all 64-bit words, zeroed at its start (np = n_probs, nb = 2^digit_bits):
//   tab  [2 d np + d]   histogram prefixes [d][np], collect prefixes [d][np], per coordinate n_hist | n_collect << 8
//   ctr  hist [d][np][nb] | mn [d][np] (as ~key under atomicMax, so 0 is "none yet") | mx [d][np] | cursor [d][np]
//   keys [d][np][capacity]
#include "fg_engine_internal.h"
#include "fg_diag_qstream_plan.h"

#define FG_QS_LDS_BYTES 65536
#define FG_QS_BLOCKS 1024            // blocks of a launch, over all coordinates

struct fg_diag_qstream {
    fg_engine *e = nullptr;
    FgQsPlan plan;
    unsigned long long *tab = nullptr, *ctr = nullptr, *keys = nullptr;
    size_t n_ctr = 0;
    bool staged = false;             // the tables of the current pass are on the device
};

__device__ __forceinline__ unsigned long long fg_qs_dev_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// One block row per coordinate (blockIdx.y), grid-stride over the chunk's n_c * C elements of it, chains fastest.  Each element is
// keyed once; the groups of a coordinate have distinct prefixes of one length b, so it matches at most one.  The first n_lds groups
// count into u32 histograms in LDS (a block sees fewer than 2^32 elements), the others straight into the global counters; the
// non-zero bins are flushed with 64-bit atomics, min and max go through a wave reduction and the (reused) LDS to one atomic per
// block and group.
__global__ __launch_bounds__(256) void k_diag_qstream_hist(const double *chunk, int n_c, int d, long long C, int np, int b, int w, int n_lds,
                                                           const unsigned long long *tab, unsigned long long *ctr) {
    extern __shared__ unsigned int sh[];
    const int i = blockIdx.y;
    const int ng = (int)(tab[2ll * d * np + i] & 255ull);
    if (ng == 0) return;
    const int nl = ng < n_lds ? ng : n_lds;
    for (int k = threadIdx.x; k < (nl << w); k += blockDim.x) sh[k] = 0u;
    unsigned long long pf[FG_QS_MAX_PROBS], mn[FG_QS_MAX_PROBS], mx[FG_QS_MAX_PROBS];
#pragma unroll
    for (int g = 0; g < FG_QS_MAX_PROBS; ++g) { pf[g] = g < ng ? tab[(long long)i * np + g] : 0ull; mn[g] = ~0ull; mx[g] = 0ull; }
    __syncthreads();
    unsigned long long *hist = ctr + ((long long)i * np << w);
    const int lo = 64 - b - w;
    const unsigned int mask = (1u << w) - 1u;
    const long long total = (long long)n_c * C;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long t = e / C, c = e - t * C;
        const unsigned long long key = fg_qs_dev_key(chunk[(t * d + i) * C + c]);
        const unsigned int digit = (unsigned int)(key >> lo) & mask;
#pragma unroll
        for (int g = 0; g < FG_QS_MAX_PROBS; ++g) {
            if (g < ng && (b == 0 || ((key ^ pf[g]) >> (64 - b)) == 0ull)) {
                if (g < nl) atomicAdd(&sh[(g << w) + digit], 1u);
                else atomicAdd(&hist[((long long)g << w) + digit], 1ull);
                mn[g] = key < mn[g] ? key : mn[g];
                mx[g] = key > mx[g] ? key : mx[g];
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < (nl << w); k += blockDim.x)
        if (sh[k]) atomicAdd(&hist[k], (unsigned long long)sh[k]);
    __syncthreads();                                                           // the histograms are flushed: their LDS carries min / max now
    unsigned long long *red = (unsigned long long *)sh;                        // [4 waves][8 groups][2]
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int g = 0; g < FG_QS_MAX_PROBS; ++g) {
        unsigned long long a = mn[g], z = mx[g];
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long a2 = __shfl_down(a, o, 64), z2 = __shfl_down(z, o, 64);
            a = a2 < a ? a2 : a; z = z2 > z ? z2 : z;
        }
        if ((threadIdx.x & 63) == 0) { red[(wave * FG_QS_MAX_PROBS + g) * 2] = a; red[(wave * FG_QS_MAX_PROBS + g) * 2 + 1] = z; }
    }
    __syncthreads();
    if ((int)threadIdx.x < ng) {
        const int g = threadIdx.x;
        unsigned long long a = ~0ull, z = 0ull;
        for (int v = 0; v < (int)(blockDim.x >> 6); ++v) {
            const unsigned long long a2 = red[(v * FG_QS_MAX_PROBS + g) * 2], z2 = red[(v * FG_QS_MAX_PROBS + g) * 2 + 1];
            a = a2 < a ? a2 : a; z = z2 > z ? z2 : z;
        }
        if (a <= z) {                                                          // the block saw an element of the group
            unsigned long long *mm = ctr + ((long long)d * np << w);
            atomicMax(&mm[(long long)i * np + g], ~a);
            atomicMax(&mm[(long long)d * np + (long long)i * np + g], z);
        }
    }
}

// The same walk over the chunk for the collect groups: a matching key reserves a position with atomicAdd on the group's cursor and
// is stored only when the position lies below `capacity` (a cursor past it is the host's integrity error, never a write).  Keys
// arrive in any order; the selection does not depend on it.
__global__ __launch_bounds__(256) void k_diag_qstream_collect(const double *chunk, int n_c, int d, long long C, int np, int b, int w, long long capacity,
                                                              const unsigned long long *tab, unsigned long long *ctr, unsigned long long *keys) {
    const int i = blockIdx.y;
    const int ng = (int)((tab[2ll * d * np + i] >> 8) & 255ull);
    if (ng == 0) return;
    unsigned long long pf[FG_QS_MAX_PROBS];
#pragma unroll
    for (int g = 0; g < FG_QS_MAX_PROBS; ++g) pf[g] = g < ng ? tab[(long long)d * np + (long long)i * np + g] : 0ull;
    unsigned long long *cursor = ctr + ((long long)d * np << w) + 2ll * d * np + (long long)i * np;
    const long long total = (long long)n_c * C;
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
        const long long t = e / C, c = e - t * C;
        const unsigned long long key = fg_qs_dev_key(chunk[(t * d + i) * C + c]);
#pragma unroll
        for (int g = 0; g < FG_QS_MAX_PROBS; ++g) {
            if (g < ng && (b == 0 || ((key ^ pf[g]) >> (64 - b)) == 0ull)) {
                const unsigned long long pos = atomicAdd(&cursor[g], 1ull);
                if (pos < (unsigned long long)capacity) keys[((long long)i * np + g) * capacity + (long long)pos] = key;
            }
        }
    }
}

// the tables and zeroed counters of the plan's current pass
static int qs_stage(fg_diag_qstream *s) {
    const FgQsPlan &P = s->plan;
    fg_engine *e = s->e;
    const size_t ns = (size_t)P.d * P.n_probs;
    std::vector<unsigned long long> tab(2 * ns + P.d);
    for (size_t k = 0; k < ns; ++k) { tab[k] = P.hist_prefix[k]; tab[ns + k] = P.col_prefix[k]; }
    for (int i = 0; i < P.d; ++i) tab[2 * ns + i] = (unsigned long long)P.n_hist[i] | ((unsigned long long)P.n_col[i] << 8);
    HIPCHK(hipMemcpyAsync(s->tab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemsetAsync(s->ctr, 0, s->n_ctr * 8, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));                                   // `tab` is a local
    s->staged = true;
    return FG_OK;
}

extern "C" {

int fg_diag_qstream_new(fg_engine *e, int n_total, int d, const double *h_probs, int n_probs, int digit_bits, int64_t capacity, fg_diag_qstream **out) {
    NEED_ENGINE(e);
    if (!out) return FG_E_BAD_ARG;
    *out = nullptr;
    fg_diag_qstream *s = new fg_diag_qstream;
    std::string err;
    int rc = fg_qs_init(s->plan, n_total, e->C, d, h_probs, n_probs, digit_bits, capacity, &err);
    if (rc) { fg_set_error(err); delete s; return rc; }
    s->e = e;
    const size_t ns = (size_t)d * n_probs;
    s->n_ctr = (ns << digit_bits) + 3 * ns;
    if (capacity > 0 && (uint64_t)capacity > (UINT64_MAX / 8) / ns) { fg_set_error("fg_diag_qstream_new: d x n_probs x capacity keys do not fit"); delete s; return FG_E_LIMIT; }
    rc = dev_alloc(&s->tab, 2 * ns + d);
    if (!rc) rc = dev_alloc(&s->ctr, s->n_ctr);
    if (!rc && capacity > 0) {                                                 // never read before written: no memset
        if (hipMalloc((void **)&s->keys, ns * (size_t)capacity * 8) != hipSuccess) { fg_set_error("fg_diag_qstream_new: no memory for d x n_probs x capacity keys"); rc = FG_E_HIP; }
    }
    if (rc) { fg_diag_qstream_free(s); return rc; }
    *out = s;
    return FG_OK;
}

int fg_diag_qstream_update(fg_diag_qstream *s, const double *d_draws, int n_chunk) {
    if (!s) { fg_set_error("null stream"); return FG_E_BAD_ARG; }
    NEED_ENGINE(s->e);
    if (!d_draws) return FG_E_BAD_ARG;
    std::string err;
    FgQsPlan &P = s->plan;
    int rc = fg_qs_take(P, n_chunk, &err);
    if (rc) { fg_set_error(err); return rc; }
    fg_engine *e = s->e;
    if (!s->staged && (rc = qs_stage(s))) { P.count -= n_chunk; return rc; }
    bool any_hist = false, any_col = false;
    for (int i = 0; i < P.d; ++i) { any_hist |= P.n_hist[i] > 0; any_col |= P.n_col[i] > 0; }
    const long long total = (long long)n_chunk * e->C;
    const long long want = std::max(1, (FG_QS_BLOCKS + P.d - 1) / P.d);
    const unsigned nb = (unsigned)std::max<long long>(1, std::min<long long>(want, (total + 255) / 256));
    if (any_hist) {
        const int n_lds = std::min(FG_QS_MAX_PROBS, FG_QS_LDS_BYTES / (4 << P.w));
        int most = 0;
        for (int i = 0; i < P.d; ++i) most = std::max(most, std::min(P.n_hist[i], n_lds));
        const size_t lds = std::max<size_t>((size_t)most * (4u << P.w), 4 * FG_QS_MAX_PROBS * 2 * 8);      // the histograms, then the min / max rows of four waves
        hipLaunchKernelGGL(k_diag_qstream_hist, dim3(nb, (unsigned)P.d), dim3(256), lds, e->stream, d_draws, n_chunk, P.d, e->C, P.n_probs, P.b, P.w, n_lds,
                           (const unsigned long long *)s->tab, s->ctr);
        HIPCHK(hipGetLastError());
    }
    if (any_col) {
        hipLaunchKernelGGL(k_diag_qstream_collect, dim3(nb, (unsigned)P.d), dim3(256), 0, e->stream, d_draws, n_chunk, P.d, e->C, P.n_probs, P.b, P.w,
                           (long long)P.capacity, (const unsigned long long *)s->tab, s->ctr, s->keys);
        HIPCHK(hipGetLastError());
    }
    return FG_OK;
}

int fg_diag_qstream_count(const fg_diag_qstream *s) { return s ? s->plan.count : 0; }

int fg_diag_qstream_end_pass(fg_diag_qstream *s, int *out_done) {
    if (!s) { fg_set_error("null stream"); return FG_E_BAD_ARG; }
    NEED_ENGINE(s->e);
    if (!out_done) return FG_E_BAD_ARG;
    std::string err;
    FgQsPlan &P = s->plan;
    int rc = fg_qs_pass_complete(P, &err);
    if (rc) { fg_set_error(err); return rc; }
    fg_engine *e = s->e;
    const size_t ns = (size_t)P.d * P.n_probs;
    std::vector<unsigned long long> ctr(s->n_ctr);
    HIPCHK(hipMemcpyAsync(ctr.data(), s->ctr, s->n_ctr * 8, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    // the plan's view: histograms at stride 2^w (the device's stride, the pass's digit width), min back from its complement
    const size_t hist_words = ns << P.w;
    std::vector<uint64_t> hist(ctr.begin(), ctr.begin() + hist_words), mn(ns), mx(ns), cursor(ns);
    for (size_t k = 0; k < ns; ++k) { mn[k] = ~ctr[hist_words + k]; mx[k] = ctr[hist_words + ns + k]; cursor[k] = ctr[hist_words + 2 * ns + k]; }
    std::vector<std::vector<uint64_t>> keys(ns);
    for (int i = 0; i < P.d; ++i)
        for (int g = 0; g < P.n_col[i]; ++g) {
            const size_t k = (size_t)i * P.n_probs + g;
            if (cursor[k] > (uint64_t)P.capacity) continue;                    // the plan reports it
            keys[k].resize((size_t)cursor[k]);
            if (cursor[k]) HIPCHK(hipMemcpy(keys[k].data(), s->keys + k * (size_t)P.capacity, (size_t)cursor[k] * 8, hipMemcpyDeviceToHost));
        }
    FgQsPassData D;
    D.hist = hist.data(); D.mn = mn.data(); D.mx = mx.data(); D.cursor = cursor.data(); D.keys = &keys;
    rc = fg_qs_end_pass(P, D, &err);
    s->staged = false;
    if (rc) { fg_set_error(err); return rc; }
    *out_done = P.done ? 1 : 0;
    return FG_OK;
}

int fg_diag_qstream_passes(const fg_diag_qstream *s) { return s ? s->plan.passes : 0; }

int fg_diag_qstream_result(fg_diag_qstream *s, double *h_out, int32_t *h_slot_passes) {
    if (!s) { fg_set_error("null stream"); return FG_E_BAD_ARG; }
    std::string err;
    const int rc = fg_qs_result(s->plan, h_out, h_slot_passes, &err);
    if (rc && !err.empty()) fg_set_error(err);
    return rc;
}

void fg_diag_qstream_free(fg_diag_qstream *s) {
    if (!s) return;
    if (s->e && hipSetDevice(s->e->device) == hipSuccess) {
        if (s->tab) (void)hipFree(s->tab);
        if (s->ctr) (void)hipFree(s->ctr);
        if (s->keys) (void)hipFree(s->keys);
    }
    delete s;
}

}  // extern "C"
