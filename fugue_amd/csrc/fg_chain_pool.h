// fg_chain_pool.h -- what the streams that keep one writer per (item, chain) column and then pool the chains have in common
// (fg_loglik_stream_plan.h: an item is a selected observe statement; fg_ppc_stream_plan.h: a (check, statistic) slot):
// the count of the draws that have arrived, the launch cuts, the (n, mean, ssd) triple, and the FIXED binary tree on the chain index.
// Plain C++ above the __HIPCC__ line (g++ builds the host drivers under tests/cpp from it), the kernel and its launcher below it.
//
// The tree: for stride s = 1, 2, 4, ... element i (a multiple of 2 s) takes in element i + s when i + s < C and passes through
// unchanged otherwise, so the pooled words are a function of the columns and of C alone.  A missing partner is the empty element, and
// merging with it is the identity, bit for bit; so a block of FG_POOL_THREADS consecutive elements is a subtree whatever C is, and the
// tree is run level by level: level 0 turns C columns into ceil(C / 256) elements, level 1 those into ceil(. / 256), ... down to one.
// Device, host driver and the Python restatements agree bit for bit because the pairs and the order of the operations inside a
// merge are the same everywhere (-ffp-contract=off): regroup no product or quotient below.
//
// A stream describes its elements by a Pool: Elem (a chain, or chains pooled), State (a column), WORDS (8-byte words of an element in
// memory), empty(), leaf(State), merge(a, b), state_load(State &, words, stride), elem_load(words), elem_store(Elem, words).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/fugue_amd.h"

#ifndef FG_HD
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FG_HD __host__ __device__ __forceinline__
#else
#define FG_HD inline
#endif
#endif

#define FG_POOL_THREADS 256          // elements per block of a tree level; a power of two (the block is a subtree)
#define FG_POOL_MAX_GRID_X 0x7fffff  // blocks along x of one launch: threads stay below 2^31
#define FG_POOL_MAX_GRID_Y 65535

// The draws of a stream: n_chunk more (FG_E_STATE past n_total; n_chunk == 0 is FG_OK, the caller launches nothing), a launch that
// never ran gives its draws back, and a read-out wants them all.  `who`: the C entry point, the prefix of the message.
struct FgDraws {
    int n_total = 0, count = 0;
    int take(int n_chunk, const char *who, std::string *err) {
        if (n_chunk < 0) { if (err) *err = std::string(who) + ": n_chunk < 0"; return FG_E_BAD_ARG; }
        if (n_chunk > n_total - count) {
            if (err) *err = std::string(who) + ": " + std::to_string(count) + " + " + std::to_string(n_chunk) + " draws pass n_total = " + std::to_string(n_total);
            return FG_E_STATE;
        }
        count += n_chunk;
        return FG_OK;
    }
    void untake(int n_chunk) { count -= n_chunk; }
    int complete(const char *who, std::string *err) const {
        if (count == n_total) return FG_OK;
        if (err) *err = std::string(who) + ": " + std::to_string(count) + " of " + std::to_string(n_total) + " draws have arrived";
        return FG_E_STATE;
    }
};

struct FgPoolLaunch { long long col0 = 0, cols = 0; };        // columns [col0, col0 + cols) of a launch with one thread per column (grid x)
struct FgPoolLevel { long long m_in = 0, m_out = 0; };        // a tree level: m_in elements per item -> m_out = ceil(m_in / 256)
struct FgPoolSlice { long long k0 = 0, nk = 0; };             // items [k0, k0 + nk) of a launch (grid y)

inline std::vector<FgPoolLaunch> fg_pool_launches(long long n_cols, int threads, long long max_grid_x) {
    std::vector<FgPoolLaunch> out;
    const long long per = max_grid_x * threads;
    for (long long c0 = 0; c0 < n_cols; c0 += per) {
        FgPoolLaunch L;
        L.col0 = c0; L.cols = std::min(per, n_cols - c0);
        out.push_back(L);
    }
    return out;
}
inline std::vector<FgPoolLevel> fg_pool_levels(long long C) {
    std::vector<FgPoolLevel> out;
    long long m = C;
    do {
        FgPoolLevel L;
        L.m_in = m; L.m_out = (m + FG_POOL_THREADS - 1) / FG_POOL_THREADS;
        out.push_back(L);
        m = L.m_out;
    } while (m > 1);
    return out;
}
inline std::vector<FgPoolSlice> fg_pool_slices(long long n_items, long long max_grid_y) {
    std::vector<FgPoolSlice> out;
    for (long long k0 = 0; k0 < n_items; k0 += max_grid_y) {
        FgPoolSlice S;
        S.k0 = k0; S.nk = std::min(max_grid_y, n_items - k0);
        out.push_back(S);
    }
    return out;
}

// The finite values of a chain, or of chains pooled: their number (below 2^47, exact), mean and sum of squared deviations.
struct FgMoments { double n = 0.0, mean = 0.0, ssd = 0.0; };

// a column's pivoted sums s1 = sum (x - pivot), s2 = sum (x - pivot)^2 by fg_diag_stream's identities
FG_HD FgMoments fg_moments_leaf(double n_fin, double pivot, double s1, double s2) {
    FgMoments m;
    if (n_fin == 0.0) return m;
    m.n = n_fin;
    const double mu = s1 / m.n;
    m.mean = pivot + mu;
    m.ssd = s2 - s1 * mu;
    return m;
}
// a side without finite values passes the other through untouched; else Chan's formulas
FG_HD FgMoments fg_moments_merge(const FgMoments &a, const FgMoments &b) {
    if (a.n == 0.0) return b;
    if (b.n == 0.0) return a;
    FgMoments r;
    const double n = a.n + b.n, delta = b.mean - a.mean;
    r.n = n;
    r.mean = a.mean + delta * (b.n / n);
    r.ssd = a.ssd + b.ssd + delta * delta * (a.n * b.n / n);
    return r;
}

// One block of a tree level on the host: elements e[0 .. n) (n <= 256) by the stride rule; the result is e[0].  The device block
// runs the same pairs with the missing partners as empty elements.
template <class Pool>
typename Pool::Elem fg_pool_block_tree(typename Pool::Elem *e, int n) {
    for (int s = 1; s < n; s *= 2)
        for (int i = 0; i + s < n; i += 2 * s) e[i] = Pool::merge(e[i], e[i + s]);
    return e[0];
}

// The whole tree on the host, block by block as fg_chain_pool_run launches it: state [.][n_items][C] -> the pooled element of every item
template <class Pool>
std::vector<typename Pool::Elem> fg_pool_host(const std::vector<FgPoolLevel> &levels, const std::vector<FgPoolSlice> &slices, const double *state, long long stride) {
    const size_t n_items = (size_t)(slices.back().k0 + slices.back().nk);
    std::vector<typename Pool::Elem> cur, next;
    for (size_t l = 0; l < levels.size(); ++l) {
        const FgPoolLevel &L = levels[l];
        next.assign(n_items * (size_t)L.m_out, Pool::empty());
        for (const FgPoolSlice &S : slices)
            for (long long k = S.k0; k < S.k0 + S.nk; ++k)
                for (long long blk = 0; blk < L.m_out; ++blk) {
                    typename Pool::Elem e[FG_POOL_THREADS];
                    const long long i0 = blk * FG_POOL_THREADS;
                    const int n = (int)std::min<long long>(FG_POOL_THREADS, L.m_in - i0);
                    for (int i = 0; i < n; ++i) {
                        if (l == 0) {
                            typename Pool::State s;
                            Pool::state_load(s, state + k * L.m_in + i0 + i, stride);
                            e[i] = Pool::leaf(s);
                        } else e[i] = cur[(size_t)k * (size_t)L.m_in + (size_t)(i0 + i)];
                    }
                    next[(size_t)k * (size_t)L.m_out + (size_t)blk] = fg_pool_block_tree<Pool>(e, n);
                }
        cur.swap(next);
    }
    return cur;
}

#if defined(__HIPCC__)
#include "fg_engine_internal.h"

static_assert(FG_POOL_THREADS == 4 * 64, "k_chain_pool merges the four waves of a block by hand: sh[0] with sh[1], sh[2] with sh[3]");

// One level: element i of item k0 + blockIdx.y is the state column (LEAF) or in[k][i]; a block pools 256 consecutive elements (an
// index past m_in: the empty element, whose merge is the identity) by strides 1 .. 32 inside each wave, 64 and 128 through LDS, and
// writes out[k][blockIdx.x].  The pairs are those of the stride rule on the chain index, whatever the grid.  An element crosses
// lanes as its WORDS memory words, each moved as a 64-bit integer: the counter words hold integer bits.
template <class Pool, bool LEAF>
__global__ __launch_bounds__(FG_POOL_THREADS) void k_chain_pool(const double *in, long long m_in, long long stride, long long k0, double *out, long long m_out) {
    typedef typename Pool::Elem Elem;
    __shared__ double sh[FG_POOL_THREADS / 64][Pool::WORDS];
    const long long i = (long long)blockIdx.x * FG_POOL_THREADS + threadIdx.x;
    const long long k = k0 + blockIdx.y;
    Elem e = Pool::empty();
    if (i < m_in) {
        if (LEAF) {
            typename Pool::State s;
            Pool::state_load(s, in + k * m_in + i, stride);
            e = Pool::leaf(s);
        } else e = Pool::elem_load(in + (k * m_in + i) * Pool::WORDS);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll 1                     // the private array below makes the unroller eager, and six copies of a merge only cost registers
    for (int s = 1; s < 64; s *= 2) {
        double w[Pool::WORDS];
        Pool::elem_store(e, w);
#pragma unroll
        for (int j = 0; j < Pool::WORDS; ++j) w[j] = __longlong_as_double(__shfl_down(__double_as_longlong(w[j]), s, 64));
        if ((lane & (2 * s - 1)) == 0) e = Pool::merge(e, Pool::elem_load(w));
    }
    if (lane == 0) Pool::elem_store(e, sh[wave]);
    __syncthreads();
    if (threadIdx.x == 0) {
        const Elem lo = Pool::merge(Pool::elem_load(sh[0]), Pool::elem_load(sh[1]));
        const Elem hi = Pool::merge(Pool::elem_load(sh[2]), Pool::elem_load(sh[3]));
        Pool::elem_store(Pool::merge(lo, hi), out + (k * m_out + blockIdx.x) * Pool::WORDS);
    }
}

// The tree level by level, one launch per (level, slice), between the two buffers tree[0 / 1] ([n_items][levels[0].m_out][WORDS]
// each); the pooled elements [n_items][WORDS] on the host.  leaf_stride: the distance between two state words of a column.
template <class Pool>
int fg_chain_pool_run(hipStream_t stream, const std::vector<FgPoolLevel> &levels, const std::vector<FgPoolSlice> &slices, const double *state, long long leaf_stride,
                      double *const tree[2], std::vector<double> &h) {
    const double *in = state;
    int side = 0;
    for (size_t l = 0; l < levels.size(); ++l) {
        const FgPoolLevel &L = levels[l];
        for (const FgPoolSlice &S : slices) {
            const dim3 grid((unsigned)L.m_out, (unsigned)S.nk), block(FG_POOL_THREADS);
            if (l == 0) hipLaunchKernelGGL((k_chain_pool<Pool, true>), grid, block, 0, stream, in, L.m_in, leaf_stride, S.k0, tree[side], L.m_out);
            else hipLaunchKernelGGL((k_chain_pool<Pool, false>), grid, block, 0, stream, in, L.m_in, 0ll, S.k0, tree[side], L.m_out);
            HIPCHK(hipGetLastError());
        }
        in = tree[side];
        side ^= 1;
    }
    h.resize((size_t)(slices.back().k0 + slices.back().nk) * Pool::WORDS);
    HIPCHK(hipMemcpyAsync(h.data(), in, h.size() * 8, hipMemcpyDeviceToHost, stream));
    HIPCHK(hipStreamSynchronize(stream));
    return FG_OK;
}

// a stream handle S { fg_engine *e; Plan P with FgDraws draws; ... }: usable at all / with every draw in (a read-out)
template <class S>
int fg_need_stream(const S *s) {
    if (!s || !s->e) { fg_set_error("null stream"); return FG_E_BAD_ARG; }
    if (hipSetDevice(s->e->device) != hipSuccess) { fg_set_error("hipSetDevice failed"); return FG_E_HIP; }
    return FG_OK;
}
template <class S>
int fg_stream_ready(const S *s, const char *who) {
    int rc = fg_need_stream(s);
    if (rc) return rc;
    std::string err;
    rc = s->P.draws.complete(who, &err);
    if (rc) fg_set_error(err);
    return rc;
}
#endif
