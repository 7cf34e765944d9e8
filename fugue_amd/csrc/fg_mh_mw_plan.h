// fg_mh_mw_plan.h -- the host side of the multi-wave MH kernels (fg_mh.hip) ahead of the launch: the launch shape, the row-less
// Categorical tail, the kind-sorted record order and its deal to the waves, what the run-time compiler is asked to generate, the
// instantiation and the kernel's name.  Plain C++ (no HIP, no engine): tests/test_mh_mw_plan_cpu.py pins every field against
// tests/golden/mh_mw_plans.json through a g++ build of tests/cpp/mh_plan_driver.cpp.
#pragma once
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "fg_ir.h"
#include "fg_switch.h"
#include "../../include/fugue_amd.h"

#define FG_MHP_WMAX 16            /* = FG_MH_WMAX (fg_mh_mw_body.h) */
#define FG_MHP_NCLS 6             /* = FG_MH_NCLS */
#define FG_MHP_WAVE 64            /* = FG_WAVE (fg_interp.h) */

// The instantiations of k_mh_mw_steps / k_mh_mw2_steps (PIPE), each named once: X(PIPE, RK, SPLIT); RK: the record kinds the
// instantiation understands (fg_score_one), SPLIT: the two in-order sums on two waves.
#define FG_MH_VARIANTS_P(X, PIPE) X(PIPE, 0, false) X(PIPE, 0, true) X(PIPE, 2, false) X(PIPE, 2, true) X(PIPE, 3, false) X(PIPE, 3, true)
#define FG_MH_VARIANTS(X) FG_MH_VARIANTS_P(X, false) FG_MH_VARIANTS_P(X, true)
struct FgMhMwKey { bool pipe; int rk; bool split; };

// The launch switches, each "unset or integer".  Per launch: pipe, exp, split, prio, prio2, stagger (the shape).  Once per engine, at its
// first launch: catu (the tail); jit, gen_min, gen_all, nseg, nseg_ns, ctl16, bake, jit_any, jit_sums, sums_form (the generated unit).
struct FgMhSwitches {
    FgSwitch pipe, exp, split, prio, prio2, stagger;          // FG_MH_PIPE, _EXP, _SPLIT, _PRIO, _PRIO2, _STAGGER
    FgSwitch catu;                                            // FG_MH_CATU
    FgSwitch jit, gen_min, gen_all, nseg, nseg_ns, ctl16, bake, jit_any, jit_sums, sums_form;   // FG_JIT, FG_MH_GEN_MIN, _GEN_ALL, _NSEG, _NSEG_NS, _CTL16, _BAKE, _JIT_ANY, _JIT_SUMS, _SUMS_FORM
};

struct FgMhPlanIn {
    long long C; int n_simd, n_slots, S, mw_override;         // (mw_override: FG_HMC_WAVES)
    bool has_overrides;                                       // fg_mh_init was given per-site proposal kinds (FgMhDev::ov_kind)
    const int *site_vtype, *site_cat;                         // fg_program's, [S] and [S][2]
    const std::vector<double> *pool;
    const FgGradRec *sstream; int n_s, n_pri;                 // the score stream (n_s records and its readable tail), log_prior rows; null, 0, 0 without one
    int sstream_kinds, sstream_gen; size_t n_ins_fast;        // FgProgramDev's; instructions of the program
};

// Launch shape of the multi-wave kernel for a program of n_s statements: LDS bytes, waves per tile, the experiment / priority mask,
// whether the two in-order sums run on two waves.
struct FgMhMwShape { size_t lds; int W, exp_mask, split_sums, pool_n, pipe, resident; unsigned tiles; };
inline int fg_mh_mw_shape(const FgMhPlanIn &in, int n_s, bool stage_pool, bool pipe_ok, const FgMhSwitches &sw, FgMhMwShape &sh) {
    const size_t pool_size = in.pool->size();
    // the pipelined step loop (fg_mh_mw2_body.h): stream programs
    // -- opt-in (FG_MH_PIPE=1): identical results, but measured 5-20 % slower than the one-control-wave loop at every chain count
    // (profiles/round4_mh_pipeline_experiment.txt): what it takes off the decider's path comes back as the proposer's phase B
    sh.pipe = (pipe_ok && fg_switch_is(sw.pipe, 1) && !sw.exp.set) ? 1 : 0;
    sh.split_sums = sw.split.set ? (sw.split.v != 0 ? 1 : 0) : (n_s >= 64 ? 1 : 0);
    int pipe_bits = 0, xrows = 17;                                          // one-control-wave loop: 2 x 8 exchange rows + the log_likelihood sum
    bool all_f64 = true;
    for (int j = 0; j < in.S; ++j) { if (in.site_vtype[j] == FG_USIZE) pipe_bits |= 512; if (in.site_vtype[j] == FG_BOOL) pipe_bits |= 1024; all_f64 = all_f64 && in.site_vtype[j] == FG_F64; }
    if (sh.pipe) {
        if (all_f64 && !in.has_overrides) pipe_bits |= 2048;                // every proposal is a walk on an f64 site with the support-based kind: the proposer's short path
        const int nr = 3 + ((pipe_bits & 512) ? 1 : 0) + ((pipe_bits & 1024) ? 1 : 0);
        xrows = 2 * nr + 9 + (sh.split_sums ? 2 : 0);                       // fg_mh_mw2_body.h: two random-number buffers, 8 candidate rows, the decision, (sum + tag)
    } else if (pipe_ok && !(pipe_bits & (512 | 1024))) pipe_bits |= 4096;   // a stream program without Categorical / bool sites: nobody reads block 1's uniform (fg_mh_mw_body.h)
    sh.lds = (size_t)(in.n_slots + n_s + xrows) * FG_MHP_WAVE * sizeof(double); // site values, term rows, exchange rows
    if (sh.lds > 160 * 1024) return FG_E_UNSUPPORTED;
    sh.pool_n = 0;                                                          // stage the constant pool into LDS when it is small and the tile leaves room
    if (stage_pool && pool_size * 8 <= 24 * 1024 && sh.lds + pool_size * 8 <= 160 * 1024 &&
        (160 * 1024) / sh.lds == (160 * 1024) / (sh.lds + pool_size * 8)) { sh.pool_n = (int)pool_size; sh.lds += pool_size * 8; }
    sh.tiles = (unsigned)((in.C + FG_MHP_WAVE - 1) / FG_MHP_WAVE);
    const long long n_cu = std::max(1, in.n_simd / 4);
    const long long resident = std::max(1LL, std::min<long long>((160 * 1024) / (long long)sh.lds, ((long long)sh.tiles + n_cu - 1) / n_cu));
    sh.resident = (int)resident;
    int W = in.mw_override > 0 ? in.mw_override : 2;
    // (sixteen waves only pay with >= 6 rows per wave where the rows are a score stream's records: reference_model(20), 39 rows, one tile per CU at 8 192 chains:
    // W = 8 4.30 / 6.24e9 adapting / sampling, W = 16 4.18 / 5.93e9; the statements of a program without a stream are whole expression programs -- rule unchanged)
    if (in.mw_override <= 0) while (W < FG_MHP_WMAX && resident * W < 16 && n_s >= ((pipe_ok && W >= 8) ? 12 : 4) * W) W *= 2;
    sh.W = std::max(W, 2);                                                  // control wave + random-number wave
    sh.exp_mask = (sw.exp.set ? sw.exp.v : 0) | pipe_bits;
    if (fg_switch_is(sw.prio, 0)) sh.exp_mask |= 32;
    else if (resident >= 2) sh.exp_mask |= 64;
    if (resident >= 3 && !fg_switch_is(sw.stagger, 0)) sh.exp_mask |= 128;   // bit 128: the tiles of a CU start a quarter of a step apart (reference_model(20), four tiles per CU: +4.7 %; two tiles: nothing)   // bit 64: phase-B waves ahead of the random-number waves of the OTHER tiles on the CU (reference_model(20) +3 %; a lone tile loses 2 %)
    if (fg_switch_is(sw.prio2, 0)) sh.exp_mask |= 16384;
    // long programs: log_prior and log_likelihood are added by two waves (C5: +11 %); a short one pays more for the extra barrier than
    // the second wave returns (reference_model(20), 4 tiles per CU: -3 %) -- split_sums, above
    return FG_OK;
}

inline long long fg_mhp_bits(double d) { long long i; std::memcpy(&i, &d, 8); return i; }      // (fg_as_i64, fg_math.h)

// Categorical sites with a uniform constant table whose terms are the last rows of log_prior: no rows (FgMhSeg).  n_cu = 0: none.
struct FgMhTailSite { int slot, K; };                                      // = FgMhCatU (fg_mh_mw_body.h)
struct FgMhTail { int n_cu = 0, same = 0; double c0 = 0.0; std::vector<double> c; std::vector<FgMhTailSite> sites; };   // c: the constants, padded as the kernel reads them
inline FgMhTail fg_mh_mw_tail(const FgMhPlanIn &in, const FgMhSwitches &sw) {
    const std::vector<double> &pool = *in.pool;
    const int n_s = in.n_s, n_pri = in.n_pri;
    FgMhTail t;
    std::vector<int> ks;
    for (int k = 0; k < n_s; ++k) if (in.sstream[k].flags & FG_G_CATC) ks.push_back(k);
    int n_tab_sites = 0;
    for (int j = 0; j < in.S; ++j) n_tab_sites += (in.site_vtype[j] == FG_USIZE && in.site_cat[2 * j + 1] > 0) ? 1 : 0;
    const int n_c = (int)ks.size();
    bool ok = n_c >= 4 && n_c == n_tab_sites && n_c <= n_pri && !fg_switch_is(sw.catu, 0);
    std::vector<double> cs; std::vector<FgMhTailSite> info;
    for (int q = 0; q < n_c && ok; ++q) {
        const FgGradRec &r = in.sstream[ks[(size_t)q]];
        uint32_t w[2]; std::memcpy(w, &r.mimm, 8);                       // {pool base, K}: p[0 .. K), then ln p[0 .. K)
        ok = (int)r.coord == n_pri - n_c + q && w[1] >= 1;               // the last rows of log_prior, in program order
        for (uint32_t i = 1; i < w[1] && ok; ++i) ok = fg_mhp_bits(pool[w[0] + w[1] + i]) == fg_mhp_bits(pool[w[0] + w[1]]) && pool[w[0] + i] > 0.0;
        if (ok) ok = pool[w[0]] > 0.0;
        if (ok) { cs.push_back(pool[w[0] + w[1]]); FgMhTailSite cu; cu.slot = (int)r.xi; cu.K = (int)w[1]; info.push_back(cu); }
    }
    if (ok) {
        t.same = 1; t.c0 = cs[0];
        for (double v : cs) if (fg_mhp_bits(v) != fg_mhp_bits(cs[0])) t.same = 0;
        while (cs.size() % 8 || cs.size() < (size_t)n_c + 16) cs.push_back(0.0);      // read eight at a time, eight ahead
        t.c = cs; t.sites = info; t.n_cu = n_c;
    }
    return t;
}

// the class of a score-stream record: 0 option lists of sites, 1 constant Categorical tables, 2 - 4 the operand patterns of a plain
// Normal with sigma = 2^k, 5 everything else (fg_score_one over the record, or a generated statement)
inline int fg_mh_mw_cls(const FgMhPlanIn &in, const FgGradRec &r) {
    const uint32_t zero_slot = (uint32_t)(in.n_slots - 1);
    if (r.flags & FG_G_CATC) return 1;
    if ((r.flags & (FG_G_GEN | FG_G_LIN)) || !(r.flags & FG_G_POW2)) return 5;
    const bool xc = r.xi == zero_slot, mc = r.mi == zero_slot;                // a constant operand reads the always-zero slot and carries its value as the immediate
    if (r.flags & FG_G_NSEL) {                                                 // class 0: an observation against options that are all sites
        uint32_t w[2]; std::memcpy(w, &r.mimm, 8);
        bool sites_only = xc;
        for (uint32_t q = 0; q < w[1] && sites_only; ++q) sites_only = (uint32_t)(fg_mhp_bits((*in.pool)[w[0] + 2 * q]) >> 32) == 0u;
        return sites_only ? 0 : 5;
    }
    if (!xc && !mc && r.ximm == 0.0 && r.mimm == 0.0) return 2;
    if (xc && !mc && r.mimm == 0.0) return 3;
    if (!xc && mc && r.ximm == 0.0) return 4;
    return 5;
}

// statement k's term row once the n_cu row-less terms are gone: log_likelihood rows follow the shortened log_prior
inline int fg_mh_mw_row(const FgMhPlanIn &in, int n_cu, int k) {
    const int row = (int)in.sstream[k].coord;
    return row - ((n_cu > 0 && row >= in.n_pri) ? n_cu : 0);
}

// the kind-sorted order of the score stream, as record indices (the sorted copy's record q is record order[q] with fg_mh_mw_row as its
// `coord`); within a class the records keep their program order; cls_off[c .. c + 1]: class c
inline std::vector<int> fg_mh_mw_order(const FgMhPlanIn &in, int n_cu, int cls_off[FG_MHP_NCLS + 1]) {
    std::vector<int> order;
    cls_off[0] = 0;
    for (int c = 0; c < FG_MHP_NCLS; ++c) {
        for (int k = 0; k < in.n_s; ++k) if (fg_mh_mw_cls(in, in.sstream[k]) == c && !(n_cu > 0 && c == 1)) order.push_back(k);
        cls_off[c + 1] = (int)order.size();
    }
    return order;
}

// FgMhSeg::r: records [r[c][w], r[c][w + 1]) of the sorted stream are wave w's share of class c
inline void fg_mh_mw_segments(const int cls_off[FG_MHP_NCLS + 1], const FgMhMwShape &sh, int r[FG_MHP_NCLS][FG_MHP_WMAX + 1]) {
    const int W = sh.W;
    // in phase B all waves share the records of every class evenly; the remainders of successive classes go to different waves
    int shift = 0;
    // the pipelined loop's proposer spends phase B on the adaptation state and the next step's candidates: no records where the tile has
    // waves to spare, half a share otherwise
    const int w_pro = (sh.pipe && W >= 3) ? ((sh.split_sums && W > 2) ? 2 : 1) : -1;
    for (int c = 0; c < FG_MHP_NCLS; ++c) {
        const int a = cls_off[c], n = cls_off[c + 1] - a;
        int cnt[FG_MHP_WMAX] = {0};
        if (w_pro < 0) {
            for (int w = 0; w < W; ++w) cnt[(w + shift) % W] = (int)((long long)n * (w + 1) / W - (long long)n * w / W);
            shift += n % W;
        } else {                                                            // 2 (W - 1) half shares for the others, one (W < 8) or none for the proposer
            const int units = 2 * (W - 1) + (W < 8 ? 1 : 0);
            int at_u = 0, given = 0;
            for (int q = 0; q < W; ++q) {
                const int w = (q + shift) % W;
                const int u = w == w_pro ? (W < 8 ? 1 : 0) : 2;
                const int upto = (int)((long long)n * (at_u + u) / units);
                cnt[w] = upto - given; given = upto; at_u += u;
            }
            shift += n % W;
        }
        int at = a;
        for (int w = 0; w <= FG_MHP_WMAX; ++w) { r[c][w] = at; if (w < W) at += cnt[w]; }
    }
}

inline FgMhMwKey fg_mh_mw_key(const FgMhPlanIn &in, const FgMhMwShape &sh) {
    return FgMhMwKey{ sh.pipe != 0, in.sstream_kinds == 0 ? 0 : (in.sstream_gen ? 2 : 3), sh.split_sums != 0 };       // record kinds the instantiation understands (fg_score_one)
}

// What fg_jit_mhmw_source (fg_jit.cpp) is told: the unit around fg_mh_mw_body.h / fg_mh_mw2_body.h with statements generated.
struct FgMhJitSpec {
    bool tried = false, unit = false;        // tried: the run-time compiler is asked at all (FG_JIT, FG_MH_EXP, the program's size); unit: and there is a unit to generate
    std::vector<char> generated;             // [statement] its log-density term is a generated statement (else its record, by the hand-written runs)
    std::vector<int> rows;                   // [statement] its term row (a program without a stream: log_prior rows [0, n_pri) first, the n_fac `factor` rows last)
    int rk = 0, split = 0, n_pri = -1, n_fac = 0;
    bool no_stream = false, pipe = false;    // pipe: around fg_mh_mw2_body.h's step loop
    int nseg = 0, ctl16 = 16;                // nseg 2 .. 16: one statement segment per wave of a launch with that many waves per tile, else sixteen; ctl16: the control wave's share of a wave's statements, in sixteenths
    int sum_pri = -1, sum_lik = -1;          // >= 0: the tile's log_prior / log_likelihood term rows -- the control wave's in-order sums as straight-line code
    bool bake = false, bake_rows = true;     // bake: baked[0 .. 7) are literals in the kernel; bake_rows = false (FG_MH_BAKE=2): all but the three row counts
    int baked[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // {row-less terms, term rows, log_prior rows, site slots, waves per tile, exp_mask, pool_n} of every launch of this unit; [7]: sums_form by rule
    int sums_form = 0;                       // fg_jit_sums2: 0 plain statements; 3: pinned, no prefetch; n >= 4: the two chains pinned side by side, rows n pairs ahead (profiles/round4_mh_sums_form.txt)
};

// the program compiled at run time (fg_jit.cpp): the same kernel with the general records (class 5: fg_score_one over the record)
// as sixteen generated statement segments; where they are the minority the operand-pattern classes stay the hand-written
// runs, which are shorter than what the generator writes for them (reference_model(20), all pattern records: 2.08e10
// hand-written, 1.57e10 generated; C5, 8 general records of 136: 4.33e9 with the runs, 3.89e9 all generated)
inline FgMhJitSpec fg_mh_mw_jit_spec(const FgMhPlanIn &in, const FgMhMwShape &sh, int n_cu, const int cls_off[FG_MHP_NCLS + 1], const FgMhSwitches &sw) {
    FgMhJitSpec sp;
    const int n_s = in.n_s, n_pri = in.n_pri, W = sh.W;
    sp.tried = !fg_switch_is(sw.jit, 0) && !sw.exp.set && in.n_ins_fast <= 200000;
    if (!sp.tried) return sp;
    sp.generated.resize((size_t)n_s);
    int n_gen = 0;
    sp.rows.resize((size_t)n_s);
    for (int k = 0; k < n_s; ++k) {
        n_gen += (sp.generated[(size_t)k] = fg_mh_mw_cls(in, in.sstream[k]) == 5 ? 1 : 0);
        sp.rows[(size_t)k] = fg_mh_mw_row(in, n_cu, k);
    }
    // mostly general records: the few pattern records too (their runs' set-up costs more than the generated statements:
    // linreg, 2 pattern records of 22: 2.49e10 all generated, 2.08e10 with the two runs, 1.66e10 hand-written)
    // Programs of pattern records only (plain Normals with sigma = 2^k): round 3 kept the hand-written record runs -- the generated
    // functions read their tile through generic pointers then (FLAT accesses) and lost.  With LDS-qualified pointers the generated
    // statements, one segment per wave, win (reference_model(20): sampling 2.24e10 -> 2.70e10 at 65 536 chains, 3.9e9 -> 4.6e9 at 8 192;
    // reference_model(8) 3.0e10 -> 3.4e10 / 4.4e9 -> 5.6e9; normal32, reference_model(50) +13 %) -- not where phase B is table lookups
    // (C5: -19 %): profiles/round4_mh_generated_statements.txt.  FG_MH_GEN_ALL = 0 / 1 forces either.
    // ... and whatever the mix of pattern and general records, down to two statements (a survey of the test zoo at 65 536 chains,
    // profiles/round4_zoo_mh.txt: a program of 5 pattern + 5 general records 2.3e10 -> 4.0e10, the README model 3.4e10 -> 4.0e10, none slower).
    bool gen_all = n_s >= (sw.gen_min.set ? sw.gen_min.v : 1) && cls_off[2] == 0;              // (no class-0 / class-1 lookup records)
    if (sw.gen_all.set) gen_all = sw.gen_all.v != 0;
    // one segment per wave of this launch shape (all of a wave's statements in one straight-line function) where every statement
    // is generated; the control wave takes `ctl16` sixteenths of a share
    int nseg = W, ctl16 = 16;                                                            // (reference_model(20), 65 536 chains: sampling 2.21e10 -> 2.61e10; linreg +19 %, hier_scale +9 %)
    if (fg_switch_is(sw.nseg, 0)) nseg = 0;
    if (sw.ctl16.set) ctl16 = std::max(0, std::min(16, sw.ctl16.v));
    if (gen_all) n_gen = n_s;
    if (2 * n_gen >= n_s) for (int k = 0; k < n_s; ++k) sp.generated[(size_t)k] = (n_cu > 0 && (in.sstream[k].flags & FG_G_CATC)) ? 0 : 1;   // (row-less terms have no statement to run)
    // the launch shape as literals in the unit (one segment per wave only: the unit is then this W's anyway); FG_MH_BAKE=0: kernel arguments as before
    // [7]: the form of the control wave's in-order sums -- the two chains pinned side by side with the rows requested four pairs ahead where a CU holds ONE
    // tile (nothing else fills the control wave's waits: 8 192 chains +8 %); with two tiles per CU the plain statements measured 4 % faster in the sampling phase
    const int baked[8] = { n_cu, n_s - n_cu, n_pri - n_cu, in.n_slots, W, sh.exp_mask, sh.pool_n, sh.resident <= 1 ? 4 : 0 };
    std::memcpy(sp.baked, baked, sizeof baked);
    sp.bake = nseg == W && !sh.pipe && !fg_switch_is(sw.bake, 0);
    sp.bake_rows = !fg_switch_is(sw.bake, 2);
    // (a handful of general records among many pattern records: the runs alone -- C5 with two tiles on a CU: 7.0e9 against 6.7e9)
    sp.unit = 8 * n_gen >= n_s || (sw.jit_any.set && sw.jit_any.v != 0);
    sp.rk = fg_mh_mw_key(in, sh).rk; sp.split = sh.split_sums; sp.pipe = sh.pipe != 0;
    sp.nseg = (2 * n_gen >= n_s) ? nseg : 0; sp.ctl16 = ctl16;
    // (the control wave's in-order sums as inlined straight-line code with the row counts as literals: reference_model(20) sampling 2.71e10 -> 2.89e10; behind a CALL they lost -- a call drains the adaptation-state gather that is in flight across the sums)
    sp.sum_pri = fg_switch_is(sw.jit_sums, 0) ? -1 : n_pri - n_cu; sp.sum_lik = n_s - n_pri;
    sp.sums_form = sw.sums_form.set ? sw.sums_form.v : baked[7];
    return sp;
}

// ... of a program WITHOUT a score stream: every statement generated, rows in accumulator order (acc[statement]: 0 log_prior,
// 1 log_likelihood, 2 `factor`)
inline FgMhJitSpec fg_mh_mw_jit_spec_nostream(const FgMhPlanIn &in, const FgMhMwShape &sh, const std::vector<unsigned char> &acc, int n_s, const FgMhSwitches &sw) {
    FgMhJitSpec sp;
    if (fg_switch_is(sw.jit, 0) || sw.exp.set || in.n_ins_fast > 200000 || acc.size() != (size_t)n_s) return sp;
    int n_acc[3] = {0, 0, 0};
    for (int k = 0; k < n_s; ++k) { if (acc[(size_t)k] > 2) return sp; n_acc[acc[(size_t)k]] += 1; }
    const int n_pri = n_acc[0], n_fac = n_acc[2];
    sp.tried = sp.unit = true;
    sp.rows.resize((size_t)n_s);
    for (int k = 0, a = 0, b = n_pri, c = n_pri + n_acc[1]; k < n_s; ++k) sp.rows[(size_t)k] = acc[(size_t)k] == 0 ? a++ : acc[(size_t)k] == 1 ? b++ : c++;
    const int nseg_ns = fg_switch_is(sw.nseg_ns, 0) ? 0 : sh.W;       // one statement segment per wave (logistic +12 %, poisson_glm +16 %, hier_logsigma +8 %, alldists level)
    // (the launch shape as literals, as for stream programs above)
    const int baked[8] = { 0, n_s, n_pri, in.n_slots, sh.W, sh.exp_mask, sh.pool_n, 0 };
    std::memcpy(sp.baked, baked, sizeof baked);
    sp.bake = nseg_ns == sh.W && !fg_switch_is(sw.bake, 0);
    sp.bake_rows = !fg_switch_is(sw.bake, 2);
    sp.generated.assign((size_t)n_s, 1);
    sp.rk = 3; sp.split = sh.split_sums; sp.n_pri = n_pri; sp.n_fac = n_fac; sp.no_stream = true; sp.nseg = nseg_ns;
    sp.sums_form = sw.sums_form.set ? sw.sums_form.v : 0;
    return sp;
}

// fg_mh_last_kernel: the library's instantiation, the unit compiled at run time, or that of a program without a record stream
inline std::string fg_mh_mw_name(const FgMhMwShape &sh, bool unit, bool no_stream) {
    const std::string w = " W=" + std::to_string(sh.W);
    if (no_stream) return "k_mh_mw_jit_steps" + w + " (a program without a record stream; statements compiled at run time)";
    if (unit) return std::string(sh.pipe ? "k_mh_mw2_jit_steps" : "k_mh_mw_jit_steps") + w + " (statements compiled at run time)";
    return std::string(sh.pipe ? "k_mh_mw2_steps" : "k_mh_mw_steps") + w;
}
