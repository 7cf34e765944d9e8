// fg_diag_rank.hip -- rank-normalised split R-hat, bulk ESS, folded R-hat and tail ESS (Vehtari, Gelman, Simpson, Carpenter, Buerkner
// 2021; what the R `posterior` package and Stan report; the reference has none of it) of stored draws d_draws [n][d][C] on the device.
// The rule, the sort's ownership of positions and every limit are fg_diag_rank_plan.h's; here are the kernels and the C ABI.  Nothing is
// replayed and no engine state changes: the calls read the engine's chain count, device and stream.  This engine's chains only.
//
//   k_rank_keys     the S = n C cells of one coordinate (chains fastest, as k_diag_qhist reads them) -> key [S] u64, index [S] u32
//                   (t C + c), the histograms of all eight 8-bit digits (LDS, integer atomics) and the -inf / +inf / NaN cell counts;
//                   the folded form keys |x - med| instead and, in the same read, writes the tail indicators I_p = key(x) <= key(sorted[k_p])
//                   (lo(x) <= k_p exactly when x's key does not exceed the key at sorted position k_p) into the caller's rows, coalesced
//   k_rank_count    one radix pass: the digit counts of every block's tile -> table [256][blocks]
//   k_rank_scan     table -> exclusive offsets in (digit, block) order: one workgroup per digit, its base from the pass's histogram
//   k_rank_scatter  the stable scatter of a pass: a wave ranks its 64 cells of a round by match sets out of eight ballots, one lane
//                   of each set advances the wave's digit counter in LDS; the waves of a block are stacked in wave order
//   k_rank_runs     over the sorted keys: run starts / ends; a max scan forward and a min scan backward give lo / hi per position
//                   (block aggregates first, k_rank_carry scans them in block order, then the final form), r2 = lo + hi + 1, the
//                   normal score, and the scatter by cell index into the caller's row
// Integer atomics only, and only where order cannot matter (counts, a maximum).  No floating-point atomics.
#include "fg_diag_rank_internal.h"

__device__ __forceinline__ double rank_cell(const double *draws, u32 i, u32 C, long long d, long long j) {
    const u32 t = i / C, c = i - t * C;
    return draws[((long long)t * d + j) * (long long)C + (long long)c];
}

template <bool FOLD>
__global__ __launch_bounds__(FG_RANK_THREADS) void k_rank_keys(const double *draws, u32 S, u32 C, long long d, long long j, double med, u64 *keys, u32 *idx,
                                                                u32 *hist /*[8][256]*/, u32 *stat, double *out, long long rows, long long row0, u64 key_lo, u64 key_hi) {
    __shared__ u32 sh[FG_RANK_PASSES * FG_RANK_BINS];
    for (int k = threadIdx.x; k < FG_RANK_PASSES * FG_RANK_BINS; k += FG_RANK_THREADS) sh[k] = 0u;
    __syncthreads();
    u32 c0 = 0u, c1 = 0u, c2 = 0u;
    const u64 stride = (u64)gridDim.x * FG_RANK_THREADS;
    for (u64 i = (u64)blockIdx.x * FG_RANK_THREADS + threadIdx.x; i < S; i += stride) {
        double x = rank_cell(draws, (u32)i, C, d, j);
        if (FOLD) {
            const u64 k0 = fg_rank_key(x);
            const u32 t = (u32)i / C, c = (u32)i - t * C;
            double *o = out + ((long long)t * rows + row0) * (long long)C + (long long)c;
            o[2 * (long long)C] = k0 <= key_lo ? 1.0 : 0.0;
            o[3 * (long long)C] = k0 <= key_hi ? 1.0 : 0.0;
            x = fg_rank_fold(x, med);
        }
        const u64 key = fg_rank_key(x);
        keys[i] = key;
        idx[i] = (u32)i;
#pragma unroll
        for (int p = 0; p < FG_RANK_PASSES; ++p) atomicAdd(&sh[p * FG_RANK_BINS + ((u32)(key >> (8 * p)) & 255u)], 1u);
        c0 += x == -INFINITY ? 1u : 0u; c1 += x == INFINITY ? 1u : 0u; c2 += x != x ? 1u : 0u;
    }
    __syncthreads();
    for (int k = threadIdx.x; k < FG_RANK_PASSES * FG_RANK_BINS; k += FG_RANK_THREADS)
        if (sh[k]) atomicAdd(&hist[k], sh[k]);
    for (int o = 32; o > 0; o >>= 1) { c0 += __shfl_down(c0, o, 64); c1 += __shfl_down(c1, o, 64); c2 += __shfl_down(c2, o, 64); }
    if ((threadIdx.x & 63) == 0) {
        if (c0) atomicAdd(&stat[0], c0);
        if (c1) atomicAdd(&stat[1], c1);
        if (c2) atomicAdd(&stat[2], c2);
    }
}

__global__ __launch_bounds__(FG_RANK_THREADS) void k_rank_count(const u64 *keys, u32 S, int shift, u32 *table, u32 nb) {
    __shared__ u32 sh[FG_RANK_BINS];
    sh[threadIdx.x] = 0u;
    __syncthreads();
    const u64 base = (u64)blockIdx.x * FG_RANK_TILE;
    for (int k = 0; k < FG_RANK_ITEMS; ++k) {
        const u64 i = base + (u64)k * FG_RANK_THREADS + threadIdx.x;
        if (i < S) atomicAdd(&sh[(u32)(keys[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    table[(size_t)threadIdx.x * nb + blockIdx.x] = sh[threadIdx.x];
}

// table [256][nb] counts -> exclusive offsets in (digit, block) order.  Workgroup = digit; thread t owns the blocks [t per, (t + 1) per).
__global__ __launch_bounds__(FG_RANK_THREADS) void k_rank_scan(u32 *table, u32 nb, const u32 *hist256) {
    __shared__ u32 part[FG_RANK_THREADS];
    __shared__ u32 base_s;
    const u32 digit = blockIdx.x, tid = threadIdx.x;
    part[tid] = tid < digit ? hist256[tid] : 0u;
    __syncthreads();
    if (tid == 0) { u32 b = 0u; for (int k = 0; k < FG_RANK_THREADS; ++k) b += part[k]; base_s = b; }
    __syncthreads();
    const u32 base = base_s;
    const u32 per = (nb + FG_RANK_THREADS - 1) / FG_RANK_THREADS;
    const u32 b0 = tid * per < nb ? tid * per : nb, b1 = b0 + per < nb ? b0 + per : nb;
    u32 *row = table + (size_t)digit * nb;
    u32 s = 0u;
    for (u32 b = b0; b < b1; ++b) s += row[b];
    __syncthreads();
    part[tid] = s;
    __syncthreads();
    if (tid == 0) { u32 run = base; for (int k = 0; k < FG_RANK_THREADS; ++k) { const u32 v = part[k]; part[k] = run; run += v; } }
    __syncthreads();
    u32 run = part[tid];
    for (u32 b = b0; b < b1; ++b) { const u32 v = row[b]; row[b] = run; run += v; }
}

__global__ __launch_bounds__(FG_RANK_THREADS) void k_rank_scatter(const u64 *kin, const u32 *iin, u64 *kout, u32 *iout, u32 S, int shift, const u32 *table, u32 nb) {
    __shared__ volatile u32 wcnt[FG_RANK_WAVES][FG_RANK_BINS];
    __shared__ u32 off[FG_RANK_WAVES][FG_RANK_BINS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int w = 0; w < FG_RANK_WAVES; ++w) wcnt[w][tid] = 0u;
    __syncthreads();
    const u64 wbase = (u64)blockIdx.x * FG_RANK_TILE + (u64)wave * FG_RANK_WAVE_TILE;
    const u64 below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    u64 key[FG_RANK_ITEMS];
    u32 id[FG_RANK_ITEMS], rk[FG_RANK_ITEMS];
#pragma unroll
    for (int k = 0; k < FG_RANK_ITEMS; ++k) {
        const u64 i = wbase + (u64)k * 64 + lane;
        const bool valid = i < S;
        key[k] = valid ? kin[i] : 0ull;
        id[k] = valid ? iin[i] : 0u;
        const u32 digit = (u32)(key[k] >> shift) & 255u;
        u64 peers = __ballot(valid);                               // the lanes of this round that hold this lane's digit
#pragma unroll
        for (int b = 0; b < FG_RANK_DIGIT_BITS; ++b) {
            const bool bit = (digit >> b) & 1u;
            const u64 m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const int leader = peers ? __ffsll((long long)peers) - 1 : 0;
        u32 pre = 0u;
        if (valid && lane == leader) { pre = wcnt[wave][digit]; wcnt[wave][digit] = pre + (u32)__popcll(peers); }
        pre = __shfl(pre, leader, 64);
        rk[k] = pre + (u32)__popcll(peers & below);
    }
    __syncthreads();
    {
        u32 run = table[(size_t)tid * nb + blockIdx.x];
        for (int w = 0; w < FG_RANK_WAVES; ++w) { off[w][tid] = run; run += wcnt[w][tid]; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < FG_RANK_ITEMS; ++k) {
        const u64 i = wbase + (u64)k * 64 + lane;
        if (i < S) {
            const u32 pos = off[wave][(u32)(key[k] >> shift) & 255u] + rk[k];
            if (pos < S) { kout[pos] = key[k]; iout[pos] = id[k]; }       // counts that disagree are the host's integrity error, never a write
        }
    }
}

struct FgRankRunArgs {
    const u64 *keys; const u32 *idx; u32 S, C;
    int *bs; u32 *be;                              // [blocks]: block aggregates, then (after k_rank_carry) the carries into a block
    u32 *stat;
    double *out; u32 *rank2; long long rows, row0, nj, k; int folded;
};
#define FG_RANK_NO_END 0xffffffffu

template <bool FINAL>
__global__ __launch_bounds__(FG_RANK_RUN_THREADS) void k_rank_runs(FgRankRunArgs A) {
    __shared__ int ws[FG_RANK_RUN_THREADS / 64];
    __shared__ u32 we[FG_RANK_RUN_THREADS / 64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const u64 S = A.S, base = (u64)blockIdx.x * FG_RANK_RUN_TILE + (u64)tid * FG_RANK_RUN_ITEMS;
    u64 k[FG_RANK_RUN_ITEMS + 2];
#pragma unroll
    for (int m = 0; m < FG_RANK_RUN_ITEMS + 2; ++m) {
        const u64 i = base + m;                                    // position i - 1
        k[m] = (i >= 1 && i - 1 < S) ? A.keys[i - 1] : 0ull;
    }
    int s[FG_RANK_RUN_ITEMS], smax = -1;
    u32 e[FG_RANK_RUN_ITEMS], emin = FG_RANK_NO_END;
#pragma unroll
    for (int m = 0; m < FG_RANK_RUN_ITEMS; ++m) {
        const u64 i = base + m;
        const bool valid = i < S;
        const bool start = valid && (i == 0 || k[m] != k[m + 1]), end = valid && (i == S - 1 || k[m + 1] != k[m + 2]);
        s[m] = start ? (int)i : -1;
        e[m] = end ? (u32)(i + 1) : FG_RANK_NO_END;
        smax = s[m] > smax ? s[m] : smax;
        emin = e[m] < emin ? e[m] : emin;
    }
    // inclusive scans over the block's threads: the last start at or before a thread, the first end at or after it
    int vs = smax;
    u32 ve = emin;
    for (int o = 1; o < 64; o <<= 1) {
        const int t1 = __shfl_up(vs, o, 64);
        const u32 t2 = __shfl_down(ve, o, 64);
        if (lane >= o) vs = t1 > vs ? t1 : vs;
        if (lane + o < 64) ve = t2 < ve ? t2 : ve;
    }
    if (lane == 63) ws[wave] = vs;
    if (lane == 0) we[wave] = ve;
    __syncthreads();
    if (!FINAL) {
        if (tid == 0) {
            int a = -1; u32 b = FG_RANK_NO_END;
            for (int w = 0; w < FG_RANK_RUN_THREADS / 64; ++w) { a = ws[w] > a ? ws[w] : a; b = we[w] < b ? we[w] : b; }
            A.bs[blockIdx.x] = a; A.be[blockIdx.x] = b;
        }
        return;
    }
    int ps = A.bs[blockIdx.x];
    u32 pe = A.be[blockIdx.x];
    for (int w = 0; w < wave; ++w) ps = ws[w] > ps ? ws[w] : ps;
    for (int w = wave + 1; w < FG_RANK_RUN_THREADS / 64; ++w) pe = we[w] < pe ? we[w] : pe;
    const int us = __shfl_up(vs, 1, 64);
    const u32 ue = __shfl_down(ve, 1, 64);
    int run_s = lane > 0 ? (us > ps ? us : ps) : ps;
    u32 run_e = lane < 63 ? (ue < pe ? ue : pe) : pe;
    u32 lo[FG_RANK_RUN_ITEMS], hi[FG_RANK_RUN_ITEMS];
#pragma unroll
    for (int m = 0; m < FG_RANK_RUN_ITEMS; ++m) { if (s[m] >= 0) run_s = s[m]; lo[m] = (u32)run_s; }
#pragma unroll
    for (int m = FG_RANK_RUN_ITEMS - 1; m >= 0; --m) { if (e[m] != FG_RANK_NO_END) run_e = e[m]; hi[m] = run_e; }
    u32 n_runs = 0u, longest = 0u;
#pragma unroll
    for (int m = 0; m < FG_RANK_RUN_ITEMS; ++m) {
        const u64 i = base + m;
        if (i < S) {
            const long long r2 = (long long)lo[m] + (long long)hi[m] + 1;
            const double z = fg_rank_z(r2, (long long)S);
            const u32 id = A.idx[i], t = id / A.C, c = id - t * A.C;
            if (id >= A.S) continue;                                       // a cell index past S is never a write
            double *o = A.out + ((long long)t * A.rows + A.row0) * (long long)A.C + (long long)c;
            if (A.folded) o[(long long)A.C] = z;
            else {
                o[0] = z;
                if (A.rank2) A.rank2[((long long)t * A.nj + A.k) * (long long)A.C + (long long)c] = (u32)r2;
            }
            if (s[m] >= 0) { n_runs += 1u; const u32 len = hi[m] - lo[m]; longest = len > longest ? len : longest; }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        n_runs += __shfl_down(n_runs, o, 64);
        const u32 l2 = __shfl_down(longest, o, 64);
        longest = l2 > longest ? l2 : longest;
    }
    if (lane == 0 && n_runs) { atomicAdd(&A.stat[3], n_runs); atomicMax(&A.stat[4], longest); }
}

// the block aggregates -> the carry INTO each block: the last start in the blocks before it (-1: none), the first end in the blocks
// after it.  One workgroup; thread t owns the blocks [t per, (t + 1) per); block order throughout.
__global__ __launch_bounds__(FG_RANK_RUN_THREADS) void k_rank_carry(int *bs, u32 *be, u32 nb) {
    __shared__ int ps[FG_RANK_RUN_THREADS];
    __shared__ u32 pe[FG_RANK_RUN_THREADS];
    const u32 tid = threadIdx.x, per = (nb + FG_RANK_RUN_THREADS - 1) / FG_RANK_RUN_THREADS;
    const u32 b0 = tid * per < nb ? tid * per : nb, b1 = b0 + per < nb ? b0 + per : nb;
    int a = -1; u32 z = FG_RANK_NO_END;
    for (u32 b = b0; b < b1; ++b) { a = bs[b] > a ? bs[b] : a; z = be[b] < z ? be[b] : z; }
    ps[tid] = a; pe[tid] = z;
    __syncthreads();
    if (tid == 0) {
        int run = -1;
        for (int k = 0; k < FG_RANK_RUN_THREADS; ++k) { const int v = ps[k]; ps[k] = run; run = v > run ? v : run; }
        u32 rue = FG_RANK_NO_END;
        for (int k = FG_RANK_RUN_THREADS - 1; k >= 0; --k) { const u32 v = pe[k]; pe[k] = rue; rue = v < rue ? v : rue; }
    }
    __syncthreads();
    int run = ps[tid];
    for (u32 b = b0; b < b1; ++b) { const int v = bs[b]; bs[b] = run; run = v > run ? v : run; }
    u32 rue = pe[tid];
    for (u32 b = b1; b > b0; --b) { const u32 v = be[b - 1]; be[b - 1] = rue; rue = v < rue ? v : rue; }
}

// the radix passes on (key[0], idx[0]); returns the buffer that holds the sorted pairs through *cur and adds the passes run
int rank_sort(fg_engine *e, const FgRankPlan &P, RankWork &W, int *cur, long long *passes_run) {
    std::vector<u32> hist((size_t)FG_RANK_PASSES * FG_RANK_BINS);
    HIPCHK(hipMemcpyAsync(hist.data(), W.hist, P.b_hist, hipMemcpyDeviceToHost, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    const u32 S = (u32)P.S;
    int c = 0;
    for (int p = 0; p < FG_RANK_PASSES; ++p) {
        const u32 *h = &hist[(size_t)p * FG_RANK_BINS];
        unsigned long long tot = 0;
        for (int b = 0; b < FG_RANK_BINS; ++b) tot += h[b];
        if (tot != (unsigned long long)P.S) { fg_set_error("fg_diag_rank: a digit histogram counts " + std::to_string(tot) + " cells of " + std::to_string(P.S)); return FG_E_STATE; }
        if (fg_rank_pass_skipped(h, P.S)) continue;
        const int shift = FG_RANK_DIGIT_BITS * p;
        hipLaunchKernelGGL(k_rank_count, dim3(P.nb), dim3(FG_RANK_THREADS), 0, e->stream, (const u64 *)W.key[c], S, shift, W.table, P.nb);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_rank_scan, dim3(FG_RANK_BINS), dim3(FG_RANK_THREADS), 0, e->stream, W.table, P.nb, (const u32 *)(W.hist + (size_t)p * FG_RANK_BINS));
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_rank_scatter, dim3(P.nb), dim3(FG_RANK_THREADS), 0, e->stream, (const u64 *)W.key[c], (const u32 *)W.idx[c], W.key[1 - c], W.idx[1 - c], S, shift,
                           (const u32 *)W.table, P.nb);
        HIPCHK(hipGetLastError());
        c = 1 - c;
        *passes_run += 1;
    }
    *cur = c;
    return FG_OK;
}

int rank_keys(fg_engine *e, const FgRankPlan &P, RankWork &W, const double *d_draws, int d, long long j) {
    hipLaunchKernelGGL(k_rank_keys<false>, dim3(P.nb_key), dim3(FG_RANK_THREADS), 0, e->stream, d_draws, (u32)P.S, (u32)e->C, (long long)d, j, 0.0, W.key[0], W.idx[0], W.hist, W.stat,
                       (double *)nullptr, 0ll, 0ll, (u64)0, (u64)0);
    HIPCHK(hipGetLastError());
    return FG_OK;
}

namespace {

int rank_runs(fg_engine *e, const FgRankPlan &P, RankWork &W, int cur, FgRankRunArgs A) {
    A.keys = W.key[cur]; A.idx = W.idx[cur]; A.S = (u32)P.S; A.bs = W.bs; A.be = W.be;
    hipLaunchKernelGGL(k_rank_runs<false>, dim3(P.nb_run), dim3(FG_RANK_RUN_THREADS), 0, e->stream, A);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_rank_carry, dim3(1), dim3(FG_RANK_RUN_THREADS), 0, e->stream, W.bs, W.be, P.nb_run);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_rank_runs<true>, dim3(P.nb_run), dim3(FG_RANK_RUN_THREADS), 0, e->stream, A);
    HIPCHK(hipGetLastError());
    return FG_OK;
}

// coordinates [j0, j0 + n_j) -> d_out [n][FG_RANK_ROWS n_j][C]; h_median / h_xq ([n_j][2]: x_lo, x_hi) / h_counts may not be null
int rank_transform(fg_engine *e, const FgRankPlan &P, RankWork &W, const double *d_draws, int n, int d, int j0, int n_j, double *d_out, u32 *d_rank2,
                   double *h_median, double *h_xq, int64_t *h_counts) {
    const u32 S = (u32)P.S, C = (u32)e->C;
    for (int k = 0; k < n_j; ++k) {
        const long long j = (long long)j0 + k;
        long long passes = 0;
        HIPCHK(hipMemsetAsync(W.hist, 0, P.b_hist, e->stream));
        HIPCHK(hipMemsetAsync(W.stat, 0, 2 * P.b_stat, e->stream));
        if (int rc = rank_keys(e, P, W, d_draws, d, j)) return rc;
        int cur = 0;
        if (int rc = rank_sort(e, P, W, &cur, &passes)) return rc;
        FgRankRunArgs A;
        A.C = C; A.stat = W.stat; A.out = d_out; A.rank2 = d_rank2; A.rows = (long long)FG_RANK_ROWS * n_j; A.row0 = (long long)FG_RANK_ROWS * k; A.nj = n_j; A.k = k;
        A.folded = 0;
        if (int rc = rank_runs(e, P, W, cur, A)) return rc;
        u64 q[4];
        const long long at[4] = { (P.S - 1) / 2, P.S / 2, P.k_lo, P.k_hi };
        for (int i = 0; i < 4; ++i) HIPCHK(hipMemcpyAsync(&q[i], W.key[cur] + at[i], 8, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        const double med = fg_rank_median(fg_rank_unkey(q[0]), fg_rank_unkey(q[1]));
        HIPCHK(hipMemsetAsync(W.hist, 0, P.b_hist, e->stream));
        hipLaunchKernelGGL(k_rank_keys<true>, dim3(P.nb_key), dim3(FG_RANK_THREADS), 0, e->stream, d_draws, S, C, (long long)d, j, med, W.key[0], W.idx[0], W.hist,
                           W.stat + FG_RANK_STAT_WORDS, d_out, A.rows, A.row0, (u64)q[2], (u64)q[3]);
        HIPCHK(hipGetLastError());
        if (int rc = rank_sort(e, P, W, &cur, &passes)) return rc;
        A.stat = W.stat + FG_RANK_STAT_WORDS; A.rank2 = nullptr; A.folded = 1;
        if (int rc = rank_runs(e, P, W, cur, A)) return rc;
        u32 st[2 * FG_RANK_STAT_WORDS];
        HIPCHK(hipMemcpyAsync(st, W.stat, sizeof st, hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        h_median[k] = med;
        h_xq[2 * k] = fg_rank_unkey(q[2]); h_xq[2 * k + 1] = fg_rank_unkey(q[3]);
        int64_t *c = h_counts + (size_t)k * FG_RANK_COUNTS;
        c[0] = P.S; c[1] = st[3]; c[2] = st[4]; c[3] = st[2]; c[4] = st[0]; c[5] = st[1]; c[6] = st[FG_RANK_STAT_WORDS + 2]; c[7] = passes;
    }
    return FG_OK;
}

int rank_check(const char *who, bool pointers, int n, int d, int j0, int n_j, double p_lo, double p_hi) {
    if (!pointers) { fg_set_error(std::string(who) + ": null d_draws or output pointer"); return FG_E_BAD_ARG; }
    if (n < 1) { fg_set_error(std::string(who) + ": n must be at least 1"); return FG_E_BAD_ARG; }
    if (d < 1 || d > 65535) { fg_set_error(std::string(who) + ": d outside [1, 65535]"); return FG_E_BAD_ARG; }
    if (j0 < 0 || n_j < 1 || j0 >= d || n_j > d - j0) { fg_set_error(std::string(who) + ": the block of coordinates lies outside [0, d)"); return FG_E_BAD_ARG; }
    if (!(p_lo >= 0.0 && p_lo <= 1.0 && p_hi >= 0.0 && p_hi <= 1.0 && p_lo <= p_hi)) { fg_set_error(std::string(who) + ": probabilities outside [0, 1], or p_lo > p_hi"); return FG_E_BAD_ARG; }
    return FG_OK;
}

int rank_plan_for(const char *who, fg_engine *e, int n, int d, int j0, int n_j, double p_lo, double p_hi, FgRankPlan *P) {
    if (!e) { fg_set_error(std::string(who) + ": null engine"); return FG_E_BAD_ARG; }
    const int rc = fg_rank_plan(n, e->C, d, j0, n_j, p_lo, p_hi, P);
    if (rc == FG_E_LIMIT) fg_set_error(std::string(who) + ": n x chains = " + std::to_string((long long)n * e->C) + " pooled draws: the limit is 2^31 - 1");
    else if (rc) fg_set_error(std::string(who) + ": bad argument");
    return rc;
}

}  // namespace

extern "C" {

int fg_diag_rank_words(void) { return FG_RANK_WORDS; }

int fg_diag_rank_transform(fg_engine *e, const double *d_draws, int n, int d, int j0, int n_j, double p_lo, double p_hi, double *d_out, uint32_t *d_rank2_or_null,
                           double *h_median, int64_t *h_counts) {
    if (int rc = rank_check("fg_diag_rank_transform", d_draws && d_out && h_median && h_counts, n, d, j0, n_j, p_lo, p_hi)) return rc;
    FgRankPlan P;
    if (int rc = rank_plan_for("fg_diag_rank_transform", e, n, d, j0, n_j, p_lo, p_hi, &P)) return rc;
    if (hipSetDevice(e->device) != hipSuccess) { fg_set_error("hipSetDevice failed"); return FG_E_HIP; }
    RankWork W;
    if (int rc = W.init(P)) return rc;
    std::vector<double> xq((size_t)2 * n_j);
    return rank_transform(e, P, W, d_draws, n, d, j0, n_j, d_out, d_rank2_or_null, h_median, xq.data(), h_counts);
}

int fg_diag_rank_rhat_ess(fg_engine *e, const double *d_draws, int n, int d, double p_lo, double p_hi, int64_t max_out_bytes, double *h_figures, int64_t *h_counts) {
    if (int rc = rank_check("fg_diag_rank_rhat_ess", d_draws && h_figures && h_counts, n, d, 0, d < 1 ? 1 : d, p_lo, p_hi)) return rc;
    if (max_out_bytes < 0) { fg_set_error("fg_diag_rank_rhat_ess: max_out_bytes must not be negative"); return FG_E_BAD_ARG; }
    FgRankPlan P;
    if (int rc = rank_plan_for("fg_diag_rank_rhat_ess", e, n, d, 0, d, p_lo, p_hi, &P)) return rc;
    if (hipSetDevice(e->device) != hipSuccess) { fg_set_error("hipSetDevice failed"); return FG_E_HIP; }
    RankWork W;
    if (int rc = W.init(P)) return rc;
    const long long per = fg_rank_block(P, d, max_out_bytes);
    double *d_out = nullptr;
    if (int rc = W.alloc(&d_out, (size_t)per * P.b_coord_out, "the transformed rows")) return rc;
    std::vector<double> med((size_t)per), xq((size_t)2 * per), rhat((size_t)FG_RANK_ROWS * per), ess((size_t)FG_RANK_ROWS * per);
    for (long long j0 = 0; j0 < d; j0 += per) {
        const int nj = (int)std::min<long long>(per, d - j0);
        if (int rc = rank_transform(e, P, W, d_draws, n, d, (int)j0, nj, d_out, nullptr, med.data(), xq.data(), h_counts + (size_t)j0 * FG_RANK_COUNTS)) return rc;
        const long long exchanged = e->diag_bytes;                 // fg_diag_rhat_ess's own read-out: this call leaves it as it was
        const int rc_comb = fg_diag_rhat_ess(e, d_out, n, FG_RANK_ROWS * nj, nullptr, rhat.data(), ess.data(), nullptr, nullptr, nullptr);
        e->diag_bytes = exchanged;
        if (rc_comb) return rc_comb;
        for (int k = 0; k < nj; ++k) {
            const int64_t *c = h_counts + (size_t)(j0 + k) * FG_RANK_COUNTS;
            fg_rank_figures(&rhat[(size_t)FG_RANK_ROWS * k], &ess[(size_t)FG_RANK_ROWS * k], med[k], xq[2 * k], xq[2 * k + 1], c[3], c[6], h_figures + (size_t)(j0 + k) * FG_RANK_WORDS);
        }
    }
    return FG_OK;
}

}  // extern "C"
