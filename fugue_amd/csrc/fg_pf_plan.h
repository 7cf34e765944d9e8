// fg_pf_plan.h -- the host side of the bootstrap particle filter bank (fg_pf.hip) ahead of its launches: the workgroup of one filter,
// which thread owns which particle, the LDS it declares, the cap on N, the grid, and how a run of T steps is cut into launches.
// Plain C++ (no HIP): tests/test_pf_cpu.py drives it through tests/cpp/pf_plan_driver.cpp under -fsanitize=address,undefined.
//
// One workgroup = one filter, the whole population resident in LDS for the launch: three arrays of N doubles
//   xa, xb  the positions and the buffer a resampling step gathers into (the two swap roles at every resampling step)
//   a       the carried log-weights, then the normalised weights, then -- in a resampling step -- their inclusive prefix sums
// and FG_PF_LDS_RESERVE bytes behind them for the wave totals of the sums and of the scan.
//
// THE SUMMATION ORDER, a function of N alone (tests/pf_restatement.py restates it as `plan_sum` / `plan_cumsum`):
//   a sum over the particles (sum exp(lw - max), sum w, sum w^2, sum w x, sum w (x - mean)^2):
//     1. thread t of `threads` adds its particles t, t + threads, t + 2 threads, ... (< N) in that sequence, starting from +0.0;
//     2. each wave of 64 threads folds its 64 partials by halves: lane l takes v[l] + v[l ^ 32], then ^ 16, ^ 8, ^ 4, ^ 2, ^ 1;
//     3. the wave totals are added in wave order 0, 1, ..., threads / 64 - 1, starting from +0.0.
//   the inclusive scan of the weights (resampling steps):
//     1. thread t owns the run [t per_thread, (t + 1) per_thread) (clipped to N) and adds it up in index order, starting from +0.0;
//     2. the thread totals of a wave are scanned by doubling: lane l adds the value of lane l - o for o = 1, 2, 4, 8, 16, 32;
//     3. a wave's offset is the sum of the totals of the waves before it in wave order, starting from +0.0;
//     4. cum[i] = (wave offset + inclusive value of the lane before, +0.0 for lane 0) + the thread's running sum at i.
// Neither depends on the number of filters, on the cut of T into launches, or on whether a step is recorded.
#pragma once
#include <cstddef>

#include "../../include/fugue_amd.h"

#define FG_PF_WAVE 64
#define FG_PF_MAX_THREADS 1024                    /* one workgroup: 16 waves */
#define FG_PF_TARGET_PER_THREAD 4                 /* particles per thread before the workgroup grows */
#define FG_PF_LDS_BUDGET (160 * 1024)             /* what a workgroup may declare on gfx950 */
#define FG_PF_LDS_RESERVE 1024                    /* wave totals: six rows of 16, one row per sum of a step, and 16 of the scan = 896 bytes; the rest is slack */
#define FG_PF_ARRAYS 3                            /* xa, xb, a */
#define FG_PF_MIN_PARTICLES 2
#define FG_PF_N_CAP ((FG_PF_LDS_BUDGET - FG_PF_LDS_RESERVE) / (FG_PF_ARRAYS * 8) / 2 * 2)   /* 6784 >= the reference's 5000 */
/* particle-steps of one filter in one launch.  Measured: a workgroup's share of a launch is 0.7 ms at n = 5000 (26 steps of
 * 25.6 us), 1.4 ms at n = 1024, 2.4 ms at n = 256 (256 steps of 9.5 us); a launch of B filters lasts that times the rounds of workgroups
 * the bank needs on 256 CUs (n = 5000, B = 4096: 16 rounds, 10 ms).  At least 20 steps at n = 5000: the reference's largest filter over a
 * short series is one launch. */
#define FG_PF_LAUNCH_WORK (1 << 17)
#define FG_PF_MAX_STEPS_PER_LAUNCH 256
static_assert(FG_PF_N_CAP >= 5000, "the reference's largest filter fits one workgroup");

struct FgPfPlan {
    int n;                  // particles of a filter
    int threads;            // workgroup size: a power of two in [64, 1024]
    int per_thread;         // slots of a thread: ceil(n / threads)
    int n_pad;              // doubles of one LDS array (n rounded up to 2: every array starts on 16 bytes)
    size_t lds;             // dynamic LDS bytes of the workgroup
    unsigned grid;          // one workgroup per filter
    int steps_per_launch;   // a run of T steps is ceil(T / steps_per_launch) launches
};

// FG_E_BAD_ARG: n < 2 or n_filters < 1; FG_E_LIMIT: n above FG_PF_N_CAP (a filter spanning several workgroups is out of scope)
inline int fg_pf_plan(long long n, long long n_filters, FgPfPlan *out) {
    if (n < FG_PF_MIN_PARTICLES || n_filters < 1 || n_filters > 0x7fffffffLL) return FG_E_BAD_ARG;
    if (n > FG_PF_N_CAP) return FG_E_LIMIT;
    FgPfPlan p;
    p.n = (int)n;
    p.threads = FG_PF_WAVE;
    while (p.threads < FG_PF_MAX_THREADS && (long long)p.threads * FG_PF_TARGET_PER_THREAD < n) p.threads *= 2;
    p.per_thread = (p.n + p.threads - 1) / p.threads;
    p.n_pad = (p.n + 1) & ~1;
    p.lds = (size_t)FG_PF_ARRAYS * p.n_pad * 8 + FG_PF_LDS_RESERVE;
    p.grid = (unsigned)n_filters;
    const int by_work = FG_PF_LAUNCH_WORK / p.n;
    p.steps_per_launch = by_work < 1 ? 1 : (by_work > FG_PF_MAX_STEPS_PER_LAUNCH ? FG_PF_MAX_STEPS_PER_LAUNCH : by_work);
    *out = p;
    return FG_OK;
}
// the particle of (thread, slot) in the elementwise phases and the sums, or -1: particle i belongs to thread i % threads, slot i / threads
inline int fg_pf_owner(const FgPfPlan &p, int thread, int slot) {
    const long long i = (long long)slot * p.threads + thread;
    return i < p.n ? (int)i : -1;
}
// ... and in the scan: thread t owns the run [t per_thread, (t + 1) per_thread)
inline int fg_pf_scan_owner(const FgPfPlan &p, int thread, int slot) {
    const long long i = (long long)thread * p.per_thread + slot;
    return i < p.n ? (int)i : -1;
}
// launch k of a run of T steps takes steps [first, first + count); count = 0 past the last launch
inline void fg_pf_launch_steps(const FgPfPlan &p, long long T, long long k, long long *first, long long *count) {
    *first = k * p.steps_per_launch;
    const long long left = T - *first;
    *count = left <= 0 ? 0 : (left < p.steps_per_launch ? left : p.steps_per_launch);
}
inline long long fg_pf_n_launches(const FgPfPlan &p, long long T) { return T <= 0 ? 0 : (T + p.steps_per_launch - 1) / p.steps_per_launch; }
