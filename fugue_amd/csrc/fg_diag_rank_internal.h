// fg_diag_rank_internal.h -- what fg_diag_rank.hip shares with fg_diag_mcse.hip: the kernels of the exact stable radix sort of one
// coordinate's pooled cells (their code and the sort's ownership of positions: fg_diag_rank.hip, fg_diag_rank_plan.h), the workspace of
// a call and the radix passes.  Both consumers sort through the same code, so the sorted keys are the same bits.
#pragma once
#include "fg_engine_internal.h"
#include "fg_diag_rank_plan.h"

typedef unsigned long long u64;
typedef unsigned int u32;

template <bool FOLD>
__global__ void k_rank_keys(const double *draws, u32 S, u32 C, long long d, long long j, double med, u64 *keys, u32 *idx, u32 *hist /*[8][256]*/, u32 *stat, double *out,
                            long long rows, long long row0, u64 key_lo, u64 key_hi);
__global__ void k_rank_count(const u64 *keys, u32 S, int shift, u32 *table, u32 nb);
__global__ void k_rank_scan(u32 *table, u32 nb, const u32 *hist256);
__global__ void k_rank_scatter(const u64 *kin, const u32 *iin, u64 *kout, u32 *iout, u32 S, int shift, const u32 *table, u32 nb);

struct RankWork {                              // the workspace of one call: reused for every coordinate and both sorts
    u64 *key[2] = { nullptr, nullptr };
    u32 *idx[2] = { nullptr, nullptr };
    u32 *table = nullptr, *hist = nullptr, *stat = nullptr, *be = nullptr;
    int *bs = nullptr;
    std::vector<void *> p;
    ~RankWork() { for (void *q : p) (void)hipFree(q); }
    template <typename T>
    int alloc(T **out, size_t bytes, const char *what) {
        if (hipMalloc((void **)out, bytes ? bytes : 1) != hipSuccess) { fg_set_error(std::string("fg_diag_rank: no device memory for ") + what); return FG_E_HIP; }
        p.push_back(*out);
        return FG_OK;
    }
    int init(const FgRankPlan &P) {
        for (int i = 0; i < 2; ++i)
            if (alloc(&key[i], P.b_keys, "the keys") || alloc(&idx[i], P.b_idx, "the cell indices")) return FG_E_HIP;
        if (alloc(&table, P.b_table, "the scan table") || alloc(&hist, P.b_hist, "the digit histograms") || alloc(&stat, 2 * P.b_stat, "the counters") ||
            alloc(&bs, P.b_carry / 2, "the run carries") || alloc(&be, P.b_carry / 2, "the run carries"))
            return FG_E_HIP;
        return FG_OK;
    }
};

// the first key pass of coordinate j (k_rank_keys<false>) into (key[0], idx[0]), the histograms and the counters W.stat [0, 3)
int rank_keys(fg_engine *e, const FgRankPlan &P, RankWork &W, const double *d_draws, int d, long long j);
// the radix passes on (key[0], idx[0]); returns the buffer that holds the sorted pairs through *cur and adds the passes run
int rank_sort(fg_engine *e, const FgRankPlan &P, RankWork &W, int *cur, long long *passes_run);
