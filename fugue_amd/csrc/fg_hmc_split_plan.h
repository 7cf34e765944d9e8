// fg_hmc_split_plan.h -- the host side, ahead of the launch, of the HMC kernels that share a tile among waves by splitting its work:
// the unit compiled at run time (k_hmc_jit_steps), the interpreter kernel (k_hmc_interp_mw_steps) and the gradient-stream kernel
// (k_hmc_stream_steps) -- waves per tile, which (coordinate, sign) tasks / coordinates each wave owns, the LDS tile, what of the generated
// unit's straight-line code a launch may use, the kernel's name -- and which of them fg_hmc_step asks first.  Plain C++ (no HIP, no
// engine): tests/test_hmc_split_plan_cpu.py pins every field against tests/golden/hmc_split_plans.json through a g++ build of
// tests/cpp/split_plan_driver.cpp.
#pragma once
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "fg_ir.h"
#include "fg_switch.h"
#include "../../include/fugue_amd.h"

#define FG_TSP_WMAX 16            /* = FG_MWI_MAX (fg_hmc_interp.hip) = FG_MW_MAX (fg_interp.h) */
#define FG_TSP_WAVE 64            /* = FG_WAVE (fg_interp.h) */
#define FG_TSP_LDS (160 * 1024)   /* a CU's LDS */

// cost of one interpreted instruction in the split (relative: an out-of-line density with its logs / lgammas against an add)
inline long long fg_task_ins_cost(const FgIns &in) {
    const uint32_t code = FG_INS_OPCODE(in.op);
    if (code == FG_OP_NORMAL_FAST) return 3;
    if (code < 17u) return (in.op & FG_F_HOISTED) ? 10 : 16;
    switch (code) {
    case FG_OP_EXP: case FG_OP_LN: case FG_OP_SIN: case FG_OP_COS: case FG_OP_TANH: return 6;
    case FG_OP_POW: case FG_OP_RPOW: return 14;
    case FG_OP_DIV: case FG_OP_RDIV: case FG_OP_SQRT: return 3;
    case FG_OP_DOT: return 1 + (long long)in.opnd[1] / 2;
    default: return 1;
    }
}

// task costs per coordinate: static weights per interpreted instruction of its sub-program (they track the measured cycles within ~30 %:
// FG_HMC_INTERP_DEBUG).  tcost: the same in the units the one-barrier rule of fg_jit_task_plan was measured in -- the split's costs are the
// interpreter's, where a general density is 10 - 16 against a fast Normal's 3; compiled, the ratio is about twice that
inline void fg_task_coord_costs(const FgCoord *coord, int d, const FgIns *sub, std::vector<long long> &cost, std::vector<long long> &tcost) {
    cost.assign((size_t)d, 1); tcost.assign((size_t)d, 1);
    for (int k = 0; k < d; ++k) {
        long long cs = 0, ts = 0;
        for (int q = 0; q < coord[k].sub_n; ++q) { const FgIns &in = sub[coord[k].sub_off + q]; const long long c = fg_task_ins_cost(in); cs += c; ts += c * ((FG_INS_OPCODE(in.op) < 17u) ? 2 : 1); }
        cost[(size_t)k] = std::max(1LL, cs); tcost[(size_t)k] = std::max(1LL, ts);
    }
}

// The switches of the task splits, each "unset or integer".  fg_task_switches() reads them: once when the compiled unit's module is built,
// once per prepare of the unit that misses the cached split, and at every launch of the interpreter kernel.
struct FgTaskSwitches { FgSwitch waves, occ, ldsprog, jit_occ, fused, tasks, verbose; };   // FG_HMC_INTERP_WAVES, _OCC, _LDSPROG, FG_HMC_JIT_OCC, FG_JIT_FUSED, FG_JIT_TASKS, FG_JIT_VERBOSE
inline FgTaskSwitches fg_task_switches() {
    return FgTaskSwitches{ fg_env_switch("FG_HMC_INTERP_WAVES"), fg_env_switch("FG_HMC_INTERP_OCC"), fg_env_switch("FG_HMC_INTERP_LDSPROG"), fg_env_switch("FG_HMC_JIT_OCC"),
                           fg_env_switch("FG_JIT_FUSED"), fg_env_switch("FG_JIT_TASKS"), fg_env_switch("FG_JIT_VERBOSE") };
}

// bytes of the LDS tile: S site rows (twice with the one-barrier gradient's second copy), `priv` private rows per wave (the interpreter's
// temporaries + 1; the compiled unit has none), d momentum rows, 2 d evaluation rows, 2 + W exchange rows
inline long long fg_task_lds(int S, int d, int W, int priv = 0, bool second_copy = false) {
    return ((long long)S * (second_copy ? 2 : 1) + (long long)W * priv + 3LL * d + 2 + W) * FG_TSP_WAVE * (long long)sizeof(double);
}

// What a split is: wave w owns the tasks order[off[w] .. off[w + 1]) (task 2 k + sign: coordinate k at q_k + h / q_k - h), ascending;
// FG_GRAD_ANALYTIC's one derivative task per coordinate follows in order[2 d ..) under off_an; cbins: whole coordinates per wave (the
// one-barrier gradient), empty when that form is not taken
struct FgTaskSplit { int W = 0; int off[FG_TSP_WMAX + 1] = {}, off_an[FG_TSP_WMAX + 1] = {}; std::vector<int> order; std::vector<std::vector<int>> cbins; };
inline bool fg_same_tasks(const FgTaskSplit &a, const FgTaskSplit &b) { return a.W == b.W && a.order == b.order && std::equal(a.off, a.off + FG_TSP_WMAX + 1, b.off) && std::equal(a.off_an, a.off_an + FG_TSP_WMAX + 1, b.off_an); }
inline bool fg_same_coords(const FgTaskSplit &a, const FgTaskSplit &b) { return !a.cbins.empty() && a.cbins == b.cbins; }
inline bool operator==(const FgTaskSplit &a, const FgTaskSplit &b) { return fg_same_tasks(a, b) && a.cbins == b.cbins; }

// longest-processing-time split of the 2 d tasks (task 2 k + sign costs cost[k]) over W waves, each bin ascending.
// plus_only: the "-" tasks cost nothing and are left out of the bins (FG_GRAD_ANALYTIC in the compiled kernel: one task per coordinate)
inline std::vector<std::vector<int>> fg_task_bins(const std::vector<long long> &cost, int W, bool plus_only = false) {
    const int n_tasks = 2 * (int)cost.size();
    std::vector<int> by;
    for (int k = 0; k < n_tasks; ++k) if (!plus_only || !(k & 1)) by.push_back(k);
    std::stable_sort(by.begin(), by.end(), [&](int a, int b) { return cost[a >> 1] > cost[b >> 1]; });
    std::vector<std::vector<int>> bins(W);
    std::vector<long long> load(W, 0);
    for (int k : by) {
        int best = 0;
        for (int w = 1; w < W; ++w) if (load[w] < load[best]) best = w;
        bins[best].push_back(k); load[best] += cost[k >> 1];
    }
    int lightest = 0;                                           // wave 0 also runs the endpoint score: it gets the lightest bin
    for (int w = 1; w < W; ++w) if (load[w] < load[lightest]) lightest = w;
    std::swap(bins[0], bins[lightest]);
    for (std::vector<int> &b : bins) std::sort(b.begin(), b.end());
    return bins;
}

// bins -> order[at ..) and off[0 .. W); off[W ..] = the end
inline void fg_task_order(const std::vector<std::vector<int>> &bins, std::vector<int> &order, int off[FG_TSP_WMAX + 1]) {
    for (int w = 0; w <= FG_TSP_WMAX; ++w) {
        off[w] = (int)order.size();
        if (w < (int)bins.size()) order.insert(order.end(), bins[(size_t)w].begin(), bins[(size_t)w].end());
    }
}

// ---- the unit compiled at run time (fg_jit.cpp, fg_hmc_jit_body.h) ---------------------------------------------------------------------
// Waves per tile of the compiled HMC kernels and the split of the finite difference's 2 d tasks over them -- a function of the program,
// the chain count and the switches at the time: the unit is generated BEHIND it (fg_jit_wave_tasks)
struct FgJitTaskIn { int d, S; unsigned tiles; int n_simd, mw_override;      // (mw_override: FG_HMC_WAVES)
                     const std::vector<long long> *cost, *tcost;            // fg_task_coord_costs
                     int grad_mode; FgTaskSwitches sw; };
struct FgJitTaskPlan {
    FgTaskSplit split; std::vector<std::vector<int>> bins;                  // bins: split.order's 2 d tasks per wave, as fg_jit_hmc_source takes them
    std::vector<long long> cost;                                            // the costs the tasks were dealt by (dense: every task is the whole program)
    bool by_rule = false; long long total = 0, resident = 0;                // FG_JIT_VERBOSE's figures: W by the several-tiles-per-CU rule, from these;
    long long span_tasks = 0, span_coords = 0, t1 = 0, t2 = 0;              // the longest wave by tasks / by whole coordinates, tiles per CU without / with the second copy of the site rows
};
inline FgJitTaskPlan fg_jit_task_plan(const FgJitTaskIn &in) {
    FgJitTaskPlan p;
    const int d = in.d, n_tasks = 2 * d;
    const bool dense = in.grad_mode == FG_GRAD_FD_DENSE;
    const std::vector<long long> &cost = *in.cost, &tcost = *in.tcost;
    int forced = in.mw_override;
    if (in.sw.waves.set) forced = in.sw.waves.v;
    int jocc = 4;
    if (in.sw.jit_occ.set && in.sw.jit_occ.v >= 2 && in.sw.jit_occ.v <= 4) jocc = in.sw.jit_occ.v;
    const int wcap = std::min(std::min(FG_TSP_WMAX, 4 * jocc), n_tasks);
    int W = 1;
    const long long n_cu = std::max(1, in.n_simd / 4), per_cu = ((long long)in.tiles + n_cu - 1) / n_cu;
    if (forced > 0) W = std::max(1, std::min(forced, wcap));
    else if ((long long)in.tiles <= n_cu) W = wcap;          // a CU has at most one tile: a wave per task (logistic regression, 8 192 chains: W = 6 beats 4 by 45 %)
    else {
        // several tiles per CU: sixteen waves per CU is all that is ever resident (128 VGPRs), so four tiles of four waves where the LDS holds four tiles and a tile has at most sixteen tasks --
        // fewer, longer task lists per wave and half the waves at every barrier (reference_model(8) at 65 536 chains 2.32e10 -> 2.81e10 leapfrog-steps/s,
        // hier 1.75e10 -> 2.05e10, mixture +6 %) -- and eight waves where it holds two or three (reference_model(20): 1.02e10 with four, 1.12e10 with eight;
        // reference_model(32) 6.1e9 / 7.4e9): profiles/round4_hmc_jit_waves.txt
        p.resident = std::min<long long>(FG_TSP_LDS / std::max<long long>(1, fg_task_lds(in.S, d, 8)), per_cu);
        const int target = (p.resident >= 4 && n_tasks <= 16) ? 4 : 8;     // (alldists, 24 heavy tasks, four tiles per CU: 9.3e8 with eight waves, 8.7e8 with four)
        while (2 * W <= std::min(target, wcap)) W *= 2;
        p.by_rule = true;
        for (long long c : cost) p.total += 2 * c;
    }
    p.split.W = W;
    p.bins = fg_task_bins(cost, W);
    // whole coordinates per wave (the one-barrier gradient of fg_jit_wave_grad): both evaluations of a coordinate on one wave.  Taken where the coarser
    // split stretches the longest wave by less than a barrier costs; FG_JIT_FUSED=0 / 1 forces.
    const std::vector<std::vector<int>> pb = fg_task_bins(cost, W, true);
    for (int w = 0; w < W; ++w) {
        long long a = 0, b = 0;
        for (int t : p.bins[(size_t)w]) a += tcost[(size_t)(t >> 1)];
        for (int t : pb[(size_t)w]) b += 2 * tcost[(size_t)(t >> 1)];
        p.span_tasks = std::max(p.span_tasks, a); p.span_coords = std::max(p.span_coords, b);
    }
    const long long lds1 = fg_task_lds(in.S, d, W), lds2 = fg_task_lds(in.S, d, W, 0, true);
    // (a barrier is worth about 96 such units of the longest wave: reference_model(8) 36 -> 48 units +8 %, reference_model(20) 60 -> 120 +7 % / +15 % at 8 192
    // chains, reference_model(32) 96 -> 192 +8 %, hier_scale 74 -> 148 of the split's units (general densities) -8 %, logistic regression 465 -> 930 -29 %; the second copy may cost a resident tile but not the last but one:
    // reference_model(32), two tiles -> one, -14 % -- profiles/round4_hmc_jit_one_barrier.txt)
    p.t1 = std::min<long long>(FG_TSP_LDS / lds1, per_cu); p.t2 = lds2 <= FG_TSP_LDS ? std::min<long long>(FG_TSP_LDS / lds2, per_cu) : 0;
    const bool room = p.t2 >= std::min<long long>(2, p.t1);
    if (!dense) {
        bool ok = room && p.span_coords - p.span_tasks <= 96;
        if (in.sw.fused.set) ok = in.sw.fused.v != 0 && lds2 <= FG_TSP_LDS;
        if (ok) for (int w = 0; w < W; ++w) { p.split.cbins.emplace_back(); for (int t : pb[(size_t)w]) p.split.cbins.back().push_back(t >> 1); }
        p.cost = cost;
    } else {
        // the dense mode's one-barrier gradient: every (coordinate, sign) task is the whole program, so whole coordinates per wave cost nothing exactly when
        // 2 ceil(d / W) = ceil(2 d / W); the second copy of the site rows under the same LDS rule as the sparse form's
        bool ok = room;
        if (in.sw.fused.set) ok = in.sw.fused.v != 0 && lds2 <= FG_TSP_LDS;
        if (ok && 2 * ((d + W - 1) / W) == (2 * d + W - 1) / W) { p.split.cbins.assign((size_t)W, std::vector<int>()); for (int k = 0; k < d; ++k) p.split.cbins[(size_t)(k % W)].push_back(k); }
        p.cost.assign((size_t)d, 1);
        p.bins = fg_task_bins(p.cost, W);
    }
    fg_task_order(p.bins, p.split.order, p.split.off);
    // FG_GRAD_ANALYTIC: one derivative task per coordinate, dealt over the same W waves (the step-size search keeps the split above)
    fg_task_order(fg_task_bins(p.cost, W, true), p.split.order, p.split.off_an);
    return p;
}

// FG_JIT_VERBOSE's lines about a plan
inline std::string fg_jit_task_say(const FgJitTaskPlan &p, int d) {
    char line[2][256] = { "", "" };
    if (p.by_rule) std::snprintf(line[0], sizeof line[0], "fugue_amd: compiled HMC unit: d %d, task cost %lld, resident %lld, W %d\n", d, p.total, p.resident, p.split.W);
    std::snprintf(line[1], sizeof line[1], "fugue_amd: compiled HMC unit: W %d, longest wave %lld (tasks) / %lld (whole coordinates), tiles per CU %lld / %lld\n", p.split.W, p.span_tasks, p.span_coords, p.t1, p.t2);
    return std::string(line[0]) + line[1];
}

// A launch of k_hmc_jit_steps: `baked` -- 1: the unit holds this very split as straight-line code (fg_jit_wave_tasks), 2 / 3: and whole
// coordinates per wave (fg_jit_wave_grad / _dense: a second copy of the site rows), 0: the task list in memory; `gen`: the split of this
// gradient mode the unit was generated behind
struct FgJitLaunchShape { int baked; bool fused, analytic_off; size_t lds; std::string name; };    // analytic_off: the waves take off_an
inline FgJitLaunchShape fg_jit_launch_shape(const FgTaskSplit &cur, const FgTaskSplit &gen, int grad_mode, bool has_ad, int S, int d) {
    FgJitLaunchShape sh;
    const bool dense = grad_mode == FG_GRAD_FD_DENSE;
    sh.baked = (grad_mode == FG_GRAD_FD_SPARSE && fg_same_tasks(cur, gen)) ? 1 : 0;
    sh.fused = (grad_mode == FG_GRAD_FD_SPARSE || dense) && fg_same_coords(cur, gen);
    if (sh.fused) sh.baked = dense ? 3 : 2;
    sh.analytic_off = grad_mode == FG_GRAD_ANALYTIC && has_ad;
    sh.lds = (size_t)fg_task_lds(S, d, cur.W, 0, sh.fused);
    sh.name = "k_hmc_jit_steps W=" + std::to_string(cur.W) + (dense ? (sh.fused ? " (dense; compiled at run time, one barrier per gradient)" : " (dense; compiled at run time)") : sh.fused ? " (compiled at run time, one barrier per gradient)" : " (compiled at run time)");
    return sh;
}

// ---- the interpreter kernel (fg_hmc_interp.hip) -------------------------------------------------------------------------------------------
// waves per SIMD the launch asks for: 4 -- measured (tools/bench_interp_mw.py): 128 VGPRs with the cold paths spilling beats 168 and 198,
// the waves hide more than the spills cost
inline int fg_mwi_occ(const FgTaskSwitches &sw) { return sw.occ.set ? (sw.occ.v <= 2 ? 2 : 4) : 4; }

// once per (engine, gradient mode): waves per tile and the split of the 2 d tasks.  FG_E_UNSUPPORTED: no two waves' tile fits the LDS
struct FgMwiTaskIn { int d, S, n_slots, mw_override; const std::vector<long long> *cost; FgTaskSwitches sw; };
inline int fg_mwi_task_plan(const FgMwiTaskIn &in, FgTaskSplit *out) {
    const int priv = in.n_slots - in.S + 1;
    const int wmax = 4 * fg_mwi_occ(in.sw);                    // a workgroup's waves must fit one CU at that occupancy
    const int wcap = std::min(wmax, 2 * in.d);
    int forced = in.mw_override;
    if (in.sw.waves.set) forced = in.sw.waves.v;
    // waves per tile: eight (two tiles fill a CU's sixteen wave slots, one tile still gives every SIMD two waves), a power of two
    // (measured: 6 and 12 lose to 4 and 8 on every model), never more than the 2 d tasks
    int W = 2;
    if (forced > 0) W = std::max(2, std::min(forced, wcap));
    else while (2 * W <= std::min(8, wcap) && fg_task_lds(in.S, in.d, 2 * W, priv) <= FG_TSP_LDS) W *= 2;
    while (W > 1 && fg_task_lds(in.S, in.d, W, priv) > FG_TSP_LDS) --W;
    if (W < 2) return FG_E_UNSUPPORTED;
    *out = FgTaskSplit();
    out->W = W;
    fg_task_order(fg_task_bins(*in.cost, W), out->order, out->off);
    return FG_OK;
}

// per launch: the occupancy, whether the program is staged in LDS (instruction fetch by ds_read_b32: -5 ... -10 % time) -- when that does
// not cost a resident tile: with two or more tiles per CU the workgroup must stay under half the LDS, a CU's only tile may take all of it --
// the LDS bytes and the name
struct FgMwiLaunchIn { int d, S, n_slots, W; size_t prog_bytes; unsigned tiles; int n_simd; FgTaskSwitches sw; };
struct FgMwiLaunchShape { int occ; bool pl; size_t lds; std::string name; };
inline FgMwiLaunchShape fg_mwi_launch_shape(const FgMwiLaunchIn &in) {
    FgMwiLaunchShape sh;
    const long long n_cu = std::max(1, in.n_simd / 4), per_cu = ((long long)in.tiles + n_cu - 1) / n_cu;
    const size_t rows = (size_t)fg_task_lds(in.S, in.d, in.W, in.n_slots - in.S + 1);
    sh.occ = fg_mwi_occ(in.sw);
    sh.pl = rows + in.prog_bytes <= (size_t)(per_cu >= 2 ? 80 : 160) * 1024;
    if (in.sw.ldsprog.set) sh.pl = in.sw.ldsprog.v != 0 && rows + in.prog_bytes <= (size_t)FG_TSP_LDS;
    sh.lds = rows + (sh.pl ? in.prog_bytes : 0);
    sh.name = "k_hmc_interp_mw_steps W=" + std::to_string(in.W) + (sh.occ != 4 ? " occ=" + std::to_string(sh.occ) : std::string()) + (sh.pl ? std::string() : std::string(" (program in global memory)"));
    return sh;
}

// ---- the gradient-stream kernel (k_hmc_stream_steps, fg_engine.hip) ------------------------------------------------------------------------
struct FgStreamPlanIn { int d; unsigned tiles; int n_simd; size_t lds_bytes; int mw_override, tw; bool gt;
                        const FgGradRec *gs; int nrec;            // the gradient stream; null, 0 without one
                        int sstream_kinds; bool has_sstream; int grad_mode; };
struct FgStreamPlan { int W, c[FG_TSP_WMAX + 1], g[FG_TSP_WMAX + 1], separable;   // FgSeg's: wave w owns coordinates [c[w], c[w + 1]) and records [g[w], g[w + 1])
                      int rk; bool analytic, ss;                                 // the instantiation: record kinds, analytic gradient, the program has a score stream
                      std::string name; };
// FG_E_UNSUPPORTED: not a launch of this kernel
inline int fg_hmc_stream_plan(const FgStreamPlanIn &in, FgStreamPlan *out) {
    const int d = in.d, nrec = in.nrec;
    const FgGradRec *gs = in.gs;
    const bool dense_stream = in.grad_mode == FG_GRAD_FD_DENSE && in.has_sstream && in.sstream_kinds == 0;
    const bool analytic = in.grad_mode == FG_GRAD_ANALYTIC;
    if (!((((in.grad_mode == FG_GRAD_FD_SPARSE || analytic) && gs) || dense_stream) && in.tw == FG_TSP_WAVE && !in.gt)) return FG_E_UNSUPPORTED;
    // waves per tile: aim at 4 waves per SIMD (16 per CU, see k_hmc_stream_steps).  The LDS tile caps the tiles
    // resident on a CU (160 KB / lds_bytes -- 4 for the 32-site model), so the waves have to come from sharing
    // a tile, whatever the chain count; each wave should still own at least 2 coordinates
    int W = in.mw_override > 0 ? std::min(in.mw_override, FG_TSP_WMAX) : 1;
    if (in.mw_override <= 0) {
        const long long n_cu = std::max(1, in.n_simd / 4);
        const long long resident = std::max(1LL, std::min<long long>(FG_TSP_LDS / (long long)in.lds_bytes, ((long long)in.tiles + n_cu - 1) / n_cu));
        while (W < FG_TSP_WMAX && resident * W < 16 && d >= 4 * W) W *= 2;
    }
    FgStreamPlan &seg = *out;
    std::vector<int> cstart(d + 1, nrec);                    // first record of each coordinate
    for (int k = nrec - 1; k >= 0; --k) cstart[gs[k].coord] = k;
    std::vector<long long> cum(nrec + 1, 0);                 // work before record k: a linear predictor costs its terms
    for (int k = 0; k < nrec; ++k) cum[k + 1] = cum[k] + ((gs[k].flags & FG_G_LIN) ? 1 + gs[k].maskm / 2 : 1);
    for (int w = 0; w <= FG_TSP_WMAX; ++w) { seg.c[w] = d; seg.g[w] = nrec; }
    seg.c[0] = 0; seg.g[0] = 0;
    for (int w = 1, k = 0; w < W; ++w) {
        if (dense_stream) { seg.c[w] = (int)((long long)d * w / W); seg.g[w] = 0; continue; }   // every coordinate costs one whole-program pass
        const long long target = cum[nrec] * w / W;           // cut at the coordinate boundary nearest to w/W of the work
        while (k < d && cum[cstart[k]] < target) ++k;
        seg.c[w] = k; seg.g[w] = cstart[k];
    }
    // do the waves interact inside a trajectory?  Not when every record only reads coordinates of its own wave.
    seg.separable = 1;
    for (int w = 0; w < W && !dense_stream; ++w)
        for (int k = seg.g[w]; k < seg.g[w + 1]; ++k) {
            const FgGradRec &r = gs[k];
            const bool x_ok = (r.flags & FG_G_X_CONST) || ((int)r.xi >= seg.c[w] && (int)r.xi < seg.c[w + 1]);
            const bool m_ok = (r.flags & FG_G_M_CONST) || ((int)r.mi >= seg.c[w] && (int)r.mi < seg.c[w + 1]);
            if (!x_ok || !m_ok || (r.flags & FG_G_LIN)) seg.separable = 0;   // a linear predictor reads many coordinates
        }
    int rk = in.sstream_kinds;                               // record kinds present in either stream
    for (int k = 0; k < nrec && rk < 2; ++k) rk = std::max(rk, (gs[k].flags & FG_G_GEN) ? 2 : ((gs[k].flags & FG_G_LIN) ? 1 : 0));
    if (analytic && rk == 2) rk = 0;                         // (the analytic gradient has no general-record instantiation: such a launch has always taken the plain one)
    seg.W = W; seg.rk = rk; seg.analytic = analytic; seg.ss = in.has_sstream;
    seg.name = std::string(dense_stream ? "k_hmc_stream_steps (dense stream) W=" : "k_hmc_stream_steps W=") + std::to_string(W);
    return FG_OK;
}

// ---- which kernel first --------------------------------------------------------------------------------------------------------------------
// does fg_hmc_step run this program through the kernel compiled at run time ahead of the stream kernel (hmc_launch_steps' order: independent
// sites, dense regressions, then the compiled form where it is the faster one, the stream kernel, the compiled form, the interpreter)?
// sep_gate / lin_gate: fg_hmc_sep_gate (fg_hmc_sep_plan.h) / fg_hmc_lin_gate (fg_hmc_lin.hip), the launchers' own first early-outs
struct FgJitFirstIn { int grad_mode, jit_state; bool has_gstream, gt; int tw; bool sep_gate, lin_gate; };
inline bool fg_hmc_jit_first(const FgJitFirstIn &in) {
    if (in.grad_mode != FG_GRAD_FD_SPARSE || in.jit_state < 0) return false;
    if (!in.has_gstream) return true;
    if (in.gt || in.tw != FG_TSP_WAVE) return false;
    if (in.sep_gate || in.lin_gate) return false;              // fg_hmc_sep_launch / fg_hmc_lin_launch takes it
    // Every other gradient-stream program, at every chain count.  Round 3 sent only linear-predictor / general / option-select records here, round 4 first
    // added programs of fewer than eight coordinates and launches of two tiles per CU or fewer (the stream kernel kept 16 % on reference_model(8) at
    // 65 536 chains).  Since the unit holds its task split as straight-line code per wave (fg_jit_wave_tasks: no task list in memory, no dispatch on the
    // coordinate, short sub-programs inlined) it wins everywhere measured -- reference_model(8) 1.85e10 -> 2.26e10 leapfrog-steps/s at 65 536 chains,
    // 2.48e10 -> 2.57e10 at 524 288; reference_model(20) 8.4e9 -> 1.07e10; reference_model(32) 4.5e9 -> 7.2e9 (profiles/round4_jit_vs_stream_tasks.txt).
    // FG_JIT=0 keeps k_hmc_stream_steps (bit-identity tests, a box without hiprtc).
    return true;
}
