// fg_mh.hip -- adaptive single-site Metropolis-Hastings (single_site_mh_step x n, src/inference/mh.rs:698-744, 938-1014) with a
// 64-chain tile shared by W waves, for programs whose statements all have a score-stream record.
//
// One MH step of a chain is a short serial recipe -- pick a site, propose, re-run the model (S + O log-densities), accept,
// adapt -- and at 65 536 chains a one-wave-per-tile kernel puts ONE wave on every SIMD: in-order issue, nothing hides the
// random-number generation, the transcendental functions or the gathers of the adaptation state (round 1: 0.03 of the f64
// peak, 390 spilled VGPRs).  Here the step is software-pipelined over the waves of a workgroup:
//
//   phase A   wave 0 (control): finishes step t-1 -- adds the statements' log-density TERMS in program order (log_prior
//             terms, then log_likelihood terms: the same sums in the same order as one scoring run, interpreters.rs:76-163),
//             accept (mh.rs:731-733), DiminishingAdaptation::update (mcmc_utils.rs:88-150), commit / roll back -- and
//             makes the proposal of step t (mh.rs:183-294, 516-530, 557-567) from the random numbers published two
//             barriers earlier;
//             wave W-1 (random numbers), at the same time: Philox blocks 0..2 of step t+1 -> target site, gaussian_z
//             (mh.rs:128-132) and both candidate accept uniforms, into the other half of a double buffer;
//   barrier
//   phase B   every wave: its share of the statements' log-densities at the proposed state -> term rows in LDS;
//   barrier
//
// Two barriers per step; the scalar record fetches, LDS reads and arithmetic of a term are independent of the other
// terms'.  All proposals here are model-independent (random walks on f64 / u64 / i64 sites, the bool flip, prior resampling
// of Categorical sites with a constant table): the engine keeps programs with other needs on k_mh_steps (fg_engine.hip).
// Values and decisions are those of k_mh_steps: the same random numbers, the same operations in the same order.
#include "fg_engine_internal.h"
#include "fg_gradstream.h"
#include "fg_cold.h"
#include "fg_jit.h"
#include "fg_mh_mw_plan.h"

#include "fg_mh_mw_body.h"
#include "fg_mh_mw2_body.h"
#ifdef FG_MH_PROF
extern hipModule_t fg_mh_prof_module;
static inline void fg_mh_prof_set_module(hipModule_t m) { fg_mh_prof_module = m; }
#endif

// the same step with its serial recipe split over waves (round 4, fg_mh_mw2_body.h: decider / speculative proposer); FG_MH_PIPE=0 keeps
// the one-control-wave loop above (A/B, identity tests)
template <int RK, bool SPLIT>
__global__ __launch_bounds__(FG_WAVE * FG_MH_WMAX, 4) void k_mh_mw2_steps(FgProgramDev P, FgChainCtx X, FgMhDev M, const FgGradRec *srt, FgMhSeg seg, int iter0, int n_steps, int n_warmup,
                                                                            long long *draws, int first_sample_t, int exp_mask, int pool_n) {
    fg_mh_mw2_body<RK, SPLIT>(P, X, M, srt, seg, iter0, n_steps, n_warmup, draws, first_sample_t, exp_mask, pool_n);
}

template <int RK, bool SPLIT>
__global__ __launch_bounds__(FG_WAVE * FG_MH_WMAX, 4) void k_mh_mw_steps(FgProgramDev P, FgChainCtx X, FgMhDev M, const FgGradRec *srt, FgMhSeg seg, int iter0, int n_steps, int n_warmup,
                                                                           long long *draws, int first_sample_t, int exp_mask, int pool_n) {
    fg_mh_mw_body<RK, SPLIT>(P, X, M, srt, seg, iter0, n_steps, n_warmup, draws, first_sample_t, exp_mask, pool_n);
}

static_assert(FG_MHP_WMAX == FG_MH_WMAX && FG_MHP_NCLS == FG_MH_NCLS && FG_MHP_WAVE == FG_WAVE && sizeof(FgMhTailSite) == sizeof(FgMhCatU), "fg_mh_mw_plan.h plans for fg_mh_mw_body.h's tile");

using FgMhMwKernel = void (*)(FgProgramDev, FgChainCtx, FgMhDev, const FgGradRec *, FgMhSeg, int, int, int, long long *, int, int, int);
struct FgMhMwVariant { FgMhMwKey key; FgMhMwKernel fn; unsigned long long raised; };       // raised: fg_launch
template <bool PIPE, int RK, bool SPLIT> constexpr FgMhMwKernel fg_mh_mw_kernel() { if constexpr (PIPE) return k_mh_mw2_steps<RK, SPLIT>; else return k_mh_mw_steps<RK, SPLIT>; }
#define FG_MH_ENTRY(PIPE, RK, SPLIT) { { PIPE, RK, SPLIT }, fg_mh_mw_kernel<PIPE, RK, SPLIT>(), 0 },
static FgMhMwVariant fg_mh_mw_variants[] = { FG_MH_VARIANTS(FG_MH_ENTRY) };
#undef FG_MH_ENTRY

// the launch switches, read once per launch after the early returns (FgMhSwitches says which of them only an engine's first launch uses)
static FgMhSwitches mh_mw_switches() {
    return FgMhSwitches{ fg_env_switch("FG_MH_PIPE"), fg_env_switch("FG_MH_EXP"), fg_env_switch("FG_MH_SPLIT"), fg_env_switch("FG_MH_PRIO"), fg_env_switch("FG_MH_PRIO2"), fg_env_switch("FG_MH_STAGGER"),
                         fg_env_switch("FG_MH_CATU"), fg_env_switch("FG_JIT"), fg_env_switch("FG_MH_GEN_MIN"), fg_env_switch("FG_MH_GEN_ALL"), fg_env_switch("FG_MH_NSEG"), fg_env_switch("FG_MH_NSEG_NS"),
                         fg_env_switch("FG_MH_CTL16"), fg_env_switch("FG_MH_BAKE"), fg_env_switch("FG_MH_JIT_ANY"), fg_env_switch("FG_MH_JIT_SUMS"), fg_env_switch("FG_MH_SUMS_FORM") };
}
static FgMhPlanIn mh_mw_plan_in(const fg_engine *e) {
    const fg_program *p = e->prog;
    return FgMhPlanIn{ e->C, e->n_simd, e->n_slots, e->S, e->mw_override, e->M.ov_kind != nullptr, p->site_vtype.data(), p->site_cat.data(), &p->pool,
                       e->P.sstream ? p->sstream.data() : nullptr, e->P.sstream ? e->P.n_sstream : 0, e->P.sstream ? e->P.n_prior_terms : 0, e->P.sstream_kinds, e->P.sstream_gen, p->ins_fast.size() };
}
static bool mh_mw_sites_ok(const fg_engine *e) {     // every site must take a model-independent proposal: Categorical sites need a constant table, no PriorResample override
    if (e->gt || e->S < 1 || e->mh_mw_disabled || e->mh_has_prior_resample) return false;     // (tiles in global memory: the one-wave-per-tile kernels, fg_engine.hip)
    for (int j = 0; j < e->S; j++) if (e->prog->site_vtype[j] == FG_USIZE && e->prog->site_cat[2 * j + 1] <= 0) return false;
    return true;
}

// The unit a spec asks for: generated, compiled (or taken from the cache), loaded, its kernel found and allowed a 160 KB tile, its constant tables bound.
// state 1, or -1 with the HIP error cleared (the caller falls back; the reason is printed under FG_JIT_VERBOSE only).
static void mh_mw_load_unit(fg_engine *e, const FgMhJitSpec &spec, FgMhMwUnit *u) {
    const fg_program *p = e->prog;
    std::vector<long long> cost((size_t)p->n_ins);
    for (int k = 0; k < p->n_ins; ++k) cost[(size_t)k] = fg_mhi_ins_cost(p->ins_fast[(size_t)k]);
    std::vector<double> ctab;
    const std::string src = fg_jit_mhmw_source(p, cost, spec, &ctab);
    std::vector<char> code;
    if (!src.empty() && src.size() <= (6u << 20) && fg_jit_get_code(src, code, e->jit_log) == FG_OK &&
        hipModuleLoadData(&u->mod, code.data()) == hipSuccess &&
        hipModuleGetFunction(&u->fn, u->mod, "k_mh_mw_jit_steps") == hipSuccess &&
        hipFuncSetAttribute((const void *)u->fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess &&
        fg_jit_bind_tables(u->mod, ctab, &u->d_tab, e->stream) == FG_OK) { u->state = 1; return; }
    u->state = -1;
    (void)hipGetLastError();
    if (std::getenv("FG_JIT_VERBOSE")) fprintf(stderr, "fugue_amd: multi-wave MH kernel not compiled at run time (%s)\n", e->jit_log.c_str());
}
// the first launch of an engine: the unit of `spec`, and the launch shape it was generated for
static void mh_mw_first_unit(fg_engine *e, const FgMhJitSpec &spec, FgMhMwUnit *u) {
    u->state = -1;
    if (!spec.tried) return;
    if (spec.bake) { std::memcpy(e->mhmw.baked, spec.baked, sizeof e->mhmw.baked); e->mhmw.has_baked = true; }
    mh_mw_load_unit(e, spec, u);
}
// a launch the unit was not generated for (the shape is a function of the engine and the environment: only when a switch changed between two launches)
static int mh_mw_check_baked(const fg_engine *e, const FgMhMwShape &sh) {
    const int now[4] = { e->n_slots, sh.W, sh.exp_mask, sh.pool_n };             // (baked[0 .. 3), the row counts, are the engine's: decided once)
    if (!e->mhmw.has_baked || std::memcmp(now, e->mhmw.baked + 3, sizeof now) == 0) return FG_OK;
    fg_set_error("the compiled multi-wave MH kernel was generated for another launch shape");
    return FG_E_STATE;
}

// Programs WITHOUT a score stream (expression parameters, ...) on the same kernel: every statement generated (fg_jit_mhmw_source),
// rows in accumulator order (log_prior terms, log_likelihood terms, then the terms of `factor` statements), proposals that need the model (undecided kinds, PriorResample, computed Categorical tables) through the interpreter on
// the target's own statement (`site_ins`, device: [S][2] first instruction and count in the generic program).  Called by
// fg_mh_interp_launch with its statement table.
int fg_mh_mw_nostream_launch(fg_engine *e, int iter0, int n_steps, long long *draws, int first_sample_t, const std::vector<int> &stmt_end,
                             const std::vector<unsigned char> &acc, const int *d_site_ins) {
    FgMhMwUnit &u = e->mhmw.unit_ns;
    if (u.state < 0 || e->gt || e->S < 1 || e->mh_mw_disabled || n_steps < 1 || e->tw != FG_WAVE) return FG_E_UNSUPPORTED;
    const FgMhSwitches sw = mh_mw_switches();
    const FgMhPlanIn in = mh_mw_plan_in(e);
    const int n_s = (int)stmt_end.size();
    FgMhMwShape sh;
    if (fg_mh_mw_shape(in, n_s, false, false, sw, sh) != FG_OK) return FG_E_UNSUPPORTED;
    if (u.state == 0) mh_mw_first_unit(e, fg_mh_mw_jit_spec_nostream(in, sh, acc, n_s, sw), &u);
    if (u.state != 1) return FG_E_UNSUPPORTED;
    if (int rc = mh_mw_check_baked(e, sh)) return rc;
    FgMhSeg seg;
    std::memset(&seg, 0, sizeof(seg));
    int n_warmup = e->mh_warmup;
    const FgGradRec *site_ins_as_srt = (const FgGradRec *)d_site_ins;        // the unit reads its `srt` argument as the site_ins table (FG_MHMW_PROBE)
    void *args[] = { &e->P, &e->X, &e->M, &site_ins_as_srt, &seg, &iter0, &n_steps, &n_warmup, &draws, &first_sample_t, &sh.exp_mask, &sh.pool_n };
    HIPCHK(hipModuleLaunchKernel(u.fn, sh.tiles, 1, 1, FG_WAVE * sh.W, 1, 1, (unsigned)sh.lds, e->stream, args, nullptr));
    e->last_mh_kernel = fg_mh_mw_name(sh, true, true);
    return FG_OK;
}

// Programs with a score stream.  Once per engine: the row-less tail, the kind-sorted copy of the stream, the unit compiled at run time
// (all three for the first launch's shape); per launch: the shape and the records' deal to the waves (fg_mh_mw_plan.h).
int fg_mh_mw_launch(fg_engine *e, int iter0, int n_steps, long long *draws, int first_sample_t) {
    if (!e->P.sstream || n_steps < 1 || !mh_mw_sites_ok(e)) return FG_E_UNSUPPORTED;
    FgMhMwState &st = e->mhmw;
    const FgMhSwitches sw = mh_mw_switches();
    const FgMhPlanIn in = mh_mw_plan_in(e);
    if (st.ncu < 0) {
        st.ncu = 0;
        const FgMhTail t = fg_mh_mw_tail(in, sw);
        if (t.n_cu > 0) {
            FgMhTailSite *d_info = nullptr;
            st.catu_same = t.same; st.catu_c0 = t.c0;
            if (dev_upload(&st.d_catu_c, t.c) || dev_upload(&d_info, t.sites)) return FG_E_HIP;
            st.d_catu = d_info;
            st.ncu = t.n_cu;
        }
    }
    const int n_cu = st.ncu;
    FgMhMwShape sh;
    if (fg_mh_mw_shape(in, in.n_s - n_cu, e->P.sstream_kinds != 0, true, sw, sh) != FG_OK) return FG_E_UNSUPPORTED;      // (the term rows of the tile)
    if (!st.d_srt) {
        std::vector<FgGradRec> srt;
        for (int k : fg_mh_mw_order(in, n_cu, st.cls_off)) { srt.push_back(in.sstream[k]); srt.back().coord = (uint32_t)fg_mh_mw_row(in, n_cu, k); }
        for (int q = 0; q < 4; ++q) srt.push_back(in.sstream[(size_t)in.n_s + (size_t)(q & 1)]);    // readable records past the end (fetched ahead, never evaluated)
        if (dev_upload(&st.d_srt, srt)) return FG_E_HIP;
    }
    FgMhSeg seg;
    fg_mh_mw_segments(st.cls_off, sh, seg.r);
    seg.n_cu = n_cu; seg.catu_c = st.d_catu_c; seg.catu = (const FgMhCatU *)st.d_catu; seg.catu_same = st.catu_same; seg.catu_c0 = st.catu_c0;
    if (st.unit.state == 0) mh_mw_first_unit(e, fg_mh_mw_jit_spec(in, sh, n_cu, st.cls_off, sw), &st.unit);
    if (st.unit.state == 1) {
        if (int rc = mh_mw_check_baked(e, sh)) return rc;
        int n_warmup = e->mh_warmup;
        void *args[] = { &e->P, &e->X, &e->M, &st.d_srt, &seg, &iter0, &n_steps, &n_warmup, &draws, &first_sample_t, &sh.exp_mask, &sh.pool_n };
        HIPCHK(hipModuleLaunchKernel(st.unit.fn, sh.tiles, 1, 1, FG_WAVE * sh.W, 1, 1, (unsigned)sh.lds, e->stream, args, nullptr));
#ifdef FG_MH_PROF
        fg_mh_prof_set_module(st.unit.mod);
#endif
        e->last_mh_kernel = fg_mh_mw_name(sh, true, false);
        return FG_OK;
    }
    const FgMhMwKey key = fg_mh_mw_key(in, sh);
    FgMhMwVariant *v = std::find_if(std::begin(fg_mh_mw_variants), std::end(fg_mh_mw_variants), [&](const FgMhMwVariant &q) { return q.key.pipe == key.pipe && q.key.rk == key.rk && q.key.split == key.split; });
    if (v == std::end(fg_mh_mw_variants)) return FG_E_UNSUPPORTED;
    const int rc = fg_launch(e, v->fn, v->raised, dim3(sh.tiles), dim3(FG_WAVE * sh.W), sh.lds, e->P, e->X, e->M, st.d_srt, seg, iter0, n_steps, e->mh_warmup, draws, first_sample_t, sh.exp_mask, sh.pool_n);
    if (rc != FG_OK) return rc;
#ifdef FG_MH_PROF
    fg_mh_prof_set_module(nullptr);
#endif
    e->last_mh_kernel = fg_mh_mw_name(sh, false, false);
    return FG_OK;
}

#ifdef FG_MH_PROF
hipModule_t fg_mh_prof_module = nullptr;      // the module of the last launch when that was the kernel compiled at run time (its own counters)
extern "C" int fg_debug_mh_prof(unsigned long long *out) {
    if (fg_mh_prof_module) {
        hipDeviceptr_t dp = nullptr; size_t bytes = 0;
        if (hipModuleGetGlobal(&dp, &bytes, fg_mh_prof_module, "fg_mh_prof") != hipSuccess || bytes < sizeof(unsigned long long) * FG_MH_WMAX * 8) return -1;
        return hipMemcpy(out, dp, sizeof(unsigned long long) * FG_MH_WMAX * 8, hipMemcpyDeviceToHost) == hipSuccess ? 0 : -1;
    }
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(fg_mh_prof), sizeof(unsigned long long) * FG_MH_WMAX * 8) == hipSuccess ? 0 : -1;
}
#endif
