// fg_diag_cstream.hip -- discrete sites without stored draws.  fg_diag_cstream: exact frequency tables of the integer rows of a run
// handed over one chunk at a time (what the reference's callers make of extract_bool_values / extract_u64_values /
// extract_usize_values / extract_i64_values, diagnostics.rs:76-98).  fg_diag_cells_f64: a gather of chunk rows into f64 rows
// (`x as f64`, the Diagnostics<u64> implementation of diagnostics.rs:153-191), the input fg_diag_stream / fg_diag_qstream take.
// Validation, the form of every watched row, the counter table, the launch split and the read-out are fg_diag_cstream_plan.h's
// (plain C++); here are the two kernels and the C ABI.  This engine's chains only: counts of ranks add on the host.
#include <cstdlib>

#include "fg_engine_internal.h"
#include "fg_diag_cstream_plan.h"

#define FG_CS_WAVES (FG_CS_THREADS / 64)
#define FG_CS_PEEL 8                 // WIDE: match sets combined per element-wave before the lanes left over add 1 each

struct fg_diag_cstream {
    fg_engine *e = nullptr;
    FgCsPlan plan;
    unsigned long long *tab = nullptr, *ctr = nullptr;
};

// One grid row per watched row (blockIdx.y), grid-stride over the launch's n_c * C cells of it, chains fastest.  Every trip of the
// loop is taken by whole waves (a lane past the end carries valid = false), so the ballots below see all 64 lanes.
//   NARROW (bins <= 8): per element-wave one ballot per bin and one each for below / above, their populations added to wave-uniform
//     counters; no LDS atomics.  At the end one flush per wave through LDS, then one 64-bit atomic per block and non-zero counter.
//   WIDE: a u32 histogram in dynamic LDS (sized by the stream's widest WIDE row; a stream of NARROW rows reserves none).  Equal
//     values of a wave are combined first: the leader of a match set adds its population (the first FG_CS_PEEL sets of an
//     element-wave; lanes still left add 1 each).  Non-zero bins are flushed with 64-bit atomics.
// Both forms count below / above by ballot and take min / max of the keys by wave reduction, then LDS, then one atomic per block.
// A block sees fewer than 2^32 elements (fg_cs_split), so no u32 counter wraps.
__global__ __launch_bounds__(FG_CS_THREADS) void k_diag_cstream_count(const unsigned long long *cells, int n_c, int n_rec, long long C,
                                                                       const unsigned long long *tab, unsigned long long *ctr, long long n_bins, int n_watch) {
    extern __shared__ unsigned int hist[];                                     // fg_cs_lds_bins words: the widest WIDE row of the stream (none: 0)
    __shared__ unsigned int wcnt[FG_CS_WAVES][FG_CS_NARROW_BINS + 2];
    __shared__ unsigned long long wmm[FG_CS_WAVES][2];
    const int k = blockIdx.y;
    const unsigned long long *t5 = tab + (long long)k * FG_CS_TAB_WORDS;
    const long long row = (long long)t5[0];
    const unsigned long long klo = t5[1], flip = t5[4];
    const int bins = (int)(t5[2] & 0xffffffffull), form = (int)(t5[2] >> 32);
    const long long off = (long long)t5[3];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (form == FG_CS_WIDE) {
        for (int j = threadIdx.x; j < bins; j += FG_CS_THREADS) hist[j] = 0u;
        __syncthreads();
    }
    unsigned int cnt[FG_CS_NARROW_BINS], n_below = 0u, n_above = 0u;             // wave-uniform
#pragma unroll
    for (int j = 0; j < FG_CS_NARROW_BINS; ++j) cnt[j] = 0u;
    unsigned long long kmin = ~0ull, kmax = 0ull;
    bool any = false;
    const long long total = (long long)n_c * C, stride = (long long)gridDim.x * FG_CS_THREADS;
    const long long st = stride / C, sc = stride - st * C;                       // the stride as (draws, chains)
    const long long e0 = (long long)blockIdx.x * FG_CS_THREADS + threadIdx.x;
    long long t = e0 / C, c = e0 - t * C;
    for (long long base = e0 - lane; base < total; base += stride) {            // base: the wave's first element
        const bool valid = base + lane < total;
        unsigned long long key = 0ull;
        int b = -2;
        if (valid) {
            key = cells[(t * n_rec + row) * C + c] ^ flip;
            b = fg_cs_bin(key, klo, bins);
            kmin = key < kmin ? key : kmin;
            kmax = key > kmax ? key : kmax;
            any = true;
        }
        n_below += (unsigned int)__popcll(__ballot(b == -1));
        n_above += (unsigned int)__popcll(__ballot(b == bins));
        if (form == FG_CS_NARROW) {
#pragma unroll
            for (int j = 0; j < FG_CS_NARROW_BINS; ++j)
                if (j < bins) cnt[j] += (unsigned int)__popcll(__ballot(b == j));
        } else {
            const bool in = b >= 0 && b < bins;
            unsigned long long todo = __ballot(in);
            for (int round = 0; round < FG_CS_PEEL && todo; ++round) {
                const int leader = __ffsll((long long)todo) - 1;
                const int lb = __shfl(b, leader, 64);
                const unsigned long long set = __ballot(in && b == lb);
                if (lane == leader) atomicAdd(&hist[lb], (unsigned int)__popcll(set));
                todo &= ~set;
            }
            if (in && ((todo >> lane) & 1ull)) atomicAdd(&hist[b], 1u);
        }
        t += st; c += sc;
        if (c >= C) { c -= C; ++t; }
    }
    // min / max: wave, then block
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long a2 = __shfl_down(kmin, o, 64), z2 = __shfl_down(kmax, o, 64);
        const int y2 = __shfl_down((int)any, o, 64);
        kmin = a2 < kmin ? a2 : kmin; kmax = z2 > kmax ? z2 : kmax; any = any || y2;
    }
    if (lane == 0) {
        wmm[wave][0] = any ? kmin : ~0ull; wmm[wave][1] = any ? kmax : 0ull;
#pragma unroll
        for (int j = 0; j < FG_CS_NARROW_BINS; ++j) wcnt[wave][j] = cnt[j];
        wcnt[wave][FG_CS_NARROW_BINS] = n_below; wcnt[wave][FG_CS_NARROW_BINS + 1] = n_above;
    }
    __syncthreads();
    unsigned long long *below = ctr + n_bins, *above = below + n_watch, *mn = above + n_watch, *mx = mn + n_watch;
    if (threadIdx.x < FG_CS_NARROW_BINS + 2) {
        const int j = threadIdx.x;
        unsigned long long s = 0ull;
        for (int w = 0; w < FG_CS_WAVES; ++w) s += wcnt[w][j];
        if (s) {
            if (j == FG_CS_NARROW_BINS) atomicAdd(&below[k], s);
            else if (j == FG_CS_NARROW_BINS + 1) atomicAdd(&above[k], s);
            else if (form == FG_CS_NARROW && j < bins) atomicAdd(&ctr[off + j], s);
        }
    } else if (threadIdx.x == 64) {
        unsigned long long a = ~0ull, z = 0ull;
        for (int w = 0; w < FG_CS_WAVES; ++w) { a = wmm[w][0] < a ? wmm[w][0] : a; z = wmm[w][1] > z ? wmm[w][1] : z; }
        if (a <= z) { atomicMax(&mn[k], ~a); atomicMax(&mx[k], z); }           // the block saw an element
    }
    if (form == FG_CS_WIDE)
        for (int j = threadIdx.x; j < bins; j += FG_CS_THREADS)
            if (hist[j]) atomicAdd(&ctr[off + j], (unsigned long long)hist[j]);
}

// fg_diag_cells_f64: up to FG_CELLS_SEL selected rows travel as a kernel argument (row << 2 | conversion), so a call stages nothing
#define FG_CELLS_SEL 120
#define FG_CELLS_COPY 0
#define FG_CELLS_UNSIGNED 1
#define FG_CELLS_SIGNED 2
struct FgCellsSel { int32_t e[FG_CELLS_SEL]; };

__device__ __forceinline__ double fg_cell_f64(unsigned long long v, int how) {
    return how == FG_CELLS_COPY ? __longlong_as_double((long long)v) : how == FG_CELLS_UNSIGNED ? (double)v : (double)(long long)v;
}

// Grid y strides over the (draw, selected row) pairs of this launch, grid x over the chains of one: two cells per thread through
// 16-byte loads and stores when `vec` (C even and both buffers 16-byte aligned), one otherwise.
__global__ __launch_bounds__(256) void k_diag_cells_f64(const unsigned long long *cells, int n, int n_rec, long long C, FgCellsSel sel, int k0, int nk, int n_sel,
                                                        int vec, double *out) {
    const long long pairs = (long long)n * nk;
    for (long long r = blockIdx.y; r < pairs; r += gridDim.y) {
        const long long t = r / nk;
        const int k = (int)(r - t * nk);
        const int entry = sel.e[k], how = entry & 3;
        const unsigned long long *src = cells + (t * n_rec + (entry >> 2)) * C;
        double *dst = out + (t * n_sel + k0 + k) * C;
        if (vec) {
            const long long C2 = C >> 1;
            for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < C2; c += (long long)gridDim.x * blockDim.x) {
                const ulonglong2 v = ((const ulonglong2 *)src)[c];
                double2 o;
                o.x = fg_cell_f64(v.x, how); o.y = fg_cell_f64(v.y, how);
                ((double2 *)dst)[c] = o;
            }
        } else {
            for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < C; c += (long long)gridDim.x * blockDim.x)
                dst[c] = fg_cell_f64(src[c], how);
        }
    }
}

static int cs_force_from_env() {
    const char *v = std::getenv("FG_DIAG_CSTREAM_FORM");
    if (!v) return FG_CS_FORCE_NONE;
    if (!std::strcmp(v, "narrow")) return FG_CS_FORCE_NARROW;
    if (!std::strcmp(v, "wide")) return FG_CS_FORCE_WIDE;
    return FG_CS_FORCE_NONE;
}

extern "C" {

int fg_diag_cstream_new(fg_engine *e, int n_total, int n_rec, const int32_t *h_rows, const int32_t *h_vtypes, const int64_t *h_lo, const int32_t *h_bins,
                        int n_watch, fg_diag_cstream **out) {
    NEED_ENGINE(e);
    if (!out) { fg_set_error("fg_diag_cstream_new: null out"); return FG_E_BAD_ARG; }
    *out = nullptr;
    fg_diag_cstream *s = new fg_diag_cstream;
    std::string err;
    int rc = fg_cs_init(s->plan, n_total, e->C, n_rec, h_rows, h_vtypes, h_lo, h_bins, n_watch, cs_force_from_env(), &err);
    if (rc) { fg_set_error(err); delete s; return rc; }
    s->e = e;
    std::vector<uint64_t> tab;
    fg_cs_table(s->plan, tab);
    std::vector<unsigned long long> tab_dev(tab.begin(), tab.end());
    rc = dev_upload(&s->tab, tab_dev);
    if (!rc) rc = dev_alloc(&s->ctr, fg_cs_words(s->plan));                    // zeroed
    if (rc) { fg_diag_cstream_free(s); return rc; }
    *out = s;
    return FG_OK;
}

int fg_diag_cstream_update(fg_diag_cstream *s, const void *d_cells, int n_chunk) {
    if (!s) { fg_set_error("null stream"); return FG_E_BAD_ARG; }
    NEED_ENGINE(s->e);
    if (!d_cells) { fg_set_error("fg_diag_cstream_update: null d_cells"); return FG_E_BAD_ARG; }
    std::string err;
    FgCsPlan &P = s->plan;
    int rc = fg_cs_take(P, n_chunk, &err);
    if (rc) { fg_set_error(err); return rc; }
    fg_engine *e = s->e;
    unsigned blocks = 1;
    std::vector<FgCsLaunch> launches;
    fg_cs_split(P, n_chunk, &blocks, launches);
    const size_t lds = (size_t)fg_cs_lds_bins(P) * sizeof(unsigned int);
    for (const FgCsLaunch &L : launches) {
        const unsigned long long *at = (const unsigned long long *)d_cells + (long long)L.t0 * P.n_rec * P.C;
        hipLaunchKernelGGL(k_diag_cstream_count, dim3(blocks, (unsigned)P.n_watch), dim3(FG_CS_THREADS), lds, e->stream, at, L.n, P.n_rec, P.C,
                           (const unsigned long long *)s->tab, s->ctr, (long long)P.n_bins, P.n_watch);
        const hipError_t he = hipGetLastError();
        if (he != hipSuccess) {
            // Nothing of this launch ran.  A first launch that fails leaves the stream where it was; after an earlier launch of the
            // chunk the draws stay counted as taken, and the read-out's integrity check reports the cells that are missing.
            if (L.t0 == 0) fg_cs_untake(P, n_chunk);
            fg_set_error(std::string("fg_diag_cstream_update: k_diag_cstream_count: ") + hipGetErrorString(he));
            return FG_E_HIP;
        }
    }
    return FG_OK;
}

int fg_diag_cstream_count(const fg_diag_cstream *s) { return s ? s->plan.count : 0; }

int fg_diag_cstream_result(fg_diag_cstream *s, uint64_t *h_counts, uint64_t *h_below, uint64_t *h_above, int64_t *h_min, int64_t *h_max) {
    if (!s) { fg_set_error("null stream"); return FG_E_BAD_ARG; }
    NEED_ENGINE(s->e);
    const FgCsPlan &P = s->plan;
    std::string err;
    if (P.count != P.n_total) {                                                // the plan's message, before anything is copied
        const int rc = fg_cs_result(P, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &err);
        fg_set_error(err);
        return rc;
    }
    std::vector<unsigned long long> ctr(fg_cs_words(P));
    HIPCHK(hipMemcpyAsync(ctr.data(), s->ctr, ctr.size() * 8, hipMemcpyDeviceToHost, s->e->stream));
    HIPCHK(hipStreamSynchronize(s->e->stream));
    std::vector<uint64_t> words(ctr.begin(), ctr.end());
    const int rc = fg_cs_result(P, words.data(), h_counts, h_below, h_above, h_min, h_max, &err);
    if (rc) fg_set_error(err);
    return rc;
}

void fg_diag_cstream_free(fg_diag_cstream *s) {
    if (!s) return;
    if (s->e && hipSetDevice(s->e->device) == hipSuccess) {
        if (s->tab) (void)hipFree(s->tab);
        if (s->ctr) (void)hipFree(s->ctr);
    }
    delete s;
}

int fg_diag_cells_f64(fg_engine *e, const void *d_cells, int n, int n_rec, const int32_t *h_rows, const int32_t *h_vtypes, int n_sel, double *d_out) {
    NEED_ENGINE(e);
    if (n < 0 || n_rec < 1 || n_sel < 1 || !h_rows || !h_vtypes) { fg_set_error("fg_diag_cells_f64: n < 0, n_rec < 1, n_sel < 1 or a null table"); return FG_E_BAD_ARG; }
    std::vector<int32_t> entry((size_t)n_sel);
    for (int k = 0; k < n_sel; ++k) {
        const int vt = h_vtypes[k];
        if (h_rows[k] < 0 || h_rows[k] >= n_rec || h_rows[k] >= (1 << 29)) { fg_set_error("fg_diag_cells_f64: selected row " + std::to_string(k) + " lies outside [0, n_rec)"); return FG_E_BAD_ARG; }
        if (vt != FG_F64 && vt != FG_BOOL && vt != FG_U64 && vt != FG_USIZE && vt != FG_I64) { fg_set_error("fg_diag_cells_f64: unknown value type " + std::to_string(vt)); return FG_E_BAD_ARG; }
        entry[(size_t)k] = (h_rows[k] << 2) | (vt == FG_F64 ? FG_CELLS_COPY : vt == FG_U64 ? FG_CELLS_UNSIGNED : FG_CELLS_SIGNED);
    }
    if (n == 0) return FG_OK;
    if (!d_cells || !d_out) { fg_set_error("fg_diag_cells_f64: null d_cells or d_out"); return FG_E_BAD_ARG; }
    const long long C = e->C;
    const int vec = (C % 2 == 0) && ((uintptr_t)d_cells % 16 == 0) && ((uintptr_t)d_out % 16 == 0);
    const long long units = vec ? C / 2 : C, xmax = (units + 255) / 256;
    for (int k0 = 0; k0 < n_sel; k0 += FG_CELLS_SEL) {
        const int nk = std::min(FG_CELLS_SEL, n_sel - k0);
        FgCellsSel sel;
        for (int k = 0; k < FG_CELLS_SEL; ++k) sel.e[k] = k < nk ? entry[(size_t)(k0 + k)] : 0;
        const long long pairs = (long long)n * nk;
        const unsigned gy = (unsigned)std::min<long long>(pairs, 65535);
        const unsigned gx = (unsigned)std::max<long long>(1, std::min<long long>(xmax, 8192 / gy));
        hipLaunchKernelGGL(k_diag_cells_f64, dim3(gx, gy), dim3(256), 0, e->stream, (const unsigned long long *)d_cells, n, n_rec, C, sel, k0, nk, n_sel, vec, d_out);
        HIPCHK(hipGetLastError());
    }
    return FG_OK;
}

}  // extern "C"
