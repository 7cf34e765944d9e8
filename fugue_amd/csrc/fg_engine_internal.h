// fg_engine_internal.h -- definitions shared by the engine translation units
// (fg_engine.hip: prior/score/HMC/MH; fg_smc.hip: SMC + reductions; fg_diag.hip: diagnostics).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fg_interp.h"
#include "fg_program.h"
#include "fg_dev_types.h"
#include "fg_hmc_split_plan.h"

#define HIPCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) { \
    fg_set_error(std::string(#expr) + ": " + hipGetErrorString(e_)); return FG_E_HIP; } } while (0)

// ======================================================================================
// kernels
// ======================================================================================
static __global__ void k_fill(double *p, long long n, double v) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// The multi-wave MH launchers' once-per-engine state (fg_mh.hip): the parts of the plan (fg_mh_mw_plan.h) made at the first launch and their device copies.
struct FgMhMwUnit { int state = 0; hipModule_t mod = nullptr; hipFunction_t fn = nullptr; double *d_tab = nullptr; };   // the kernel with statements compiled at run time: 0 not tried, 1 loaded, -1 unavailable; its constant tables (fg_jit_bind_tables)
struct FgMhMwState {
    FgGradRec *d_srt = nullptr; int cls_off[7] = {0, 0, 0, 0, 0, 0, 0};   // kind-sorted score stream, class boundaries
    int ncu = -1, catu_same = 0; double catu_c0 = 0.0; double *d_catu_c = nullptr; void *d_catu = nullptr;   // row-less uniform Categorical terms (FgMhSeg; -1: not decided)
    int baked[7] = {0, 0, 0, 0, 0, 0, 0}; bool has_baked = false;   // the launch shape the unit was generated for (FgMhJitSpec::baked)
    FgMhMwUnit unit, unit_ns;    // of a program with a score stream, phase B generated / of a program without one
};

// The wave-split HMC launchers' once-per-engine state (fg_hmc_interp.hip): the split made at the first launch of a key (fg_hmc_split_plan.h) and
// its device copy, shared by the interpreter kernel and the unit compiled at run time; the splits that unit was generated behind.
enum FgSplitKey { FG_SPLIT_NONE = -1, FG_SPLIT_INTERP_DENSE, FG_SPLIT_INTERP_SPARSE, FG_SPLIT_JIT_SPARSE /* and FG_GRAD_ANALYTIC: off_an */, FG_SPLIT_JIT_DENSE };
struct FgHmcSplitState {
    FgSplitKey key = FG_SPLIT_NONE; FgTaskSplit split; std::vector<long long> cost;   // whose split is cached, the split, the per-coordinate costs it was dealt by
    FgTaskSplit gen_sparse, gen_dense;   // what the compiled unit holds as straight-line code (W = 0: nothing -- FG_JIT_TASKS=0, or no unit yet)
    int *d_mwi_order = nullptr; long long *d_mwi_prof = nullptr; int mwi_calibrated = 0;   // split.order on the device; FG_HMC_INTERP_DEBUG: cycles per task, 0 not clocked / 1 clocked / 2 printed
};

struct fg_engine {
    const fg_program *prog = nullptr;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;
    long long C = 0;
    unsigned long long seed = 0;
    uint32_t chain0 = 0;
    int S = 0, d = 0, n_slots = 0;
    // device copies of the program
    FgIns *d_ins = nullptr, *d_ins_fast = nullptr, *d_sub = nullptr;
    FgCoord *d_coord = nullptr;
    FgGradRec *d_gstream = nullptr, *d_sstream = nullptr;
    FgSepRec *d_sep = nullptr; FgSepCoord *d_sep_coord = nullptr; FgSepFree *d_sep_free = nullptr; uint32_t *d_sobs = nullptr; int *d_site_rec = nullptr;
    bool mh_mw_disabled = false;  // FG_MH_MW=0: keep every program on the one-wave-per-tile MH kernel (A/B tests)
    bool mh_has_prior_resample = false;   // an override asks for PriorResample on some site (needs the model-driven proposal path)
    bool sep_disabled = false;   // FG_HMC_SEP=0: keep independent-sites programs on the gradient-stream kernel (A/B tests)
    bool sep_res_disabled = false;   // FG_HMC_SEP_RESIDENT=0: 64-chain sparse tiles without the resident form of k_hmc_sep_steps (A/B tests)
    bool sep_fold_disabled = false;  // FG_HMC_SEP_FOLD=0: k_hmc_sep_steps's trajectories without the folded loop (A/B tests)
    bool gt = false;             // the program's tile exceeds a CU's LDS: tiles in global memory, one-wave-per-tile kernels only
    double *d_gtile = nullptr;
    bool lin_disabled = false;   // FG_HMC_LIN=0: keep dense regressions on the gradient-stream kernel (A/B tests)
    double *d_lin_tab = nullptr; int *d_lin_meta = nullptr;   // dense-regression table (fg_hmc_lin.hip)
    int *d_sub_off = nullptr, *d_f64_slot = nullptr, *d_site_slot = nullptr, *d_vtype = nullptr, *d_site_cat = nullptr;
    double *d_pool = nullptr;
    FgProgramDev P{};
    FgChainCtx X{};
    long long *d_values = nullptr;
    double *d_acc = nullptr, *d_logp = nullptr;
    // HMC
    bool hmc_ready = false;
    fg_hmc_config cfg{};
    FgHmcDev H{};
    std::vector<void *> hmc_allocs;
    int n_warmup = 0, iter = 0, mass_adapt_at = -1;
    // MH
    bool mh_ready = false;
    FgMhDev M{};
    std::vector<void *> mh_allocs;
    int mh_warmup = 0, mh_iter = 0;
    std::vector<fg_site_proposal> mh_overrides;   // as given to fg_mh_init (site order), for fg_state_export
    int *d_rec = nullptr; int rec_cap = 0;
    bool smc_pop_ready = false;   // the arena holds a particle population (log-weights, weights, log-likelihoods) for the standalone SMC calls
    void *smc_arena = nullptr; size_t smc_arena_bytes = 0;   // scratch of fg_smc_run, allocated once per engine (fg_smc.hip)
    int smc_epoch = 0;            // tags the pass flags of one next_beta search in smc_host
    void *smc_host = nullptr;     // pinned host scalars the SMC kernels write (beta, log-evidence, flags): the host's look at them needs no copy
    double *d_tmp = nullptr;     // [C] scratch
    int *d_itmp = nullptr;       // [3][C] scratch
    size_t lds_bytes = 0;        // LDS tile of the HMC kernels (slots + momentum + exchange rows)
    size_t lds_score = 0;        // LDS tile of the score / prior / MH / SMC kernels (slots only)
    int tw = 64;               // tile width (threads per block)
    int n_simd = 1024;         // SIMDs on the device (4 per CU)
    int diag_mode = 0;         // FG_DIAG_REDUCE / FG_DIAG_GATHER: how fg_diag_rhat_ess exchanges chain statistics between ranks
    long long diag_bytes = 0;  // bytes this rank put into collectives during the last fg_diag_rhat_ess
    std::string last_hmc_kernel;   // kernel (and waves per tile) the last fg_hmc_step launch ran (fg_hmc_last_kernel)
    bool interp_mw_disabled = false;   // FG_HMC_INTERP_MW=0: keep interpreter programs on the one-wave-per-tile HMC kernel (A/B tests)
    FgHmcSplitState hsplit;      // what the wave-split HMC launchers decide once per engine and gradient mode (fg_hmc_interp.hip)
    int mhi_W = 0, mhi_n_stmt = 0, mhi_occ = 2; bool mhi_setup_done = false; size_t mhi_lds = 0; std::vector<int> mhi_ins_off, mhi_stmt_off; unsigned char *d_mhi_acc = nullptr; int *d_mhi_site_ins = nullptr; std::vector<int> mhi_stmt_end; std::vector<unsigned char> mhi_acc_host;   // statement split of k_mh_interp_mw_steps (fg_mh_interp.hip)
    int jit_state = 0;           // run-time compiled HMC kernel of this program: 0 not tried, 1 loaded, -1 unavailable (fg_jit.cpp; FG_JIT=0 switches it off)
    hipModule_t jit_mod = nullptr; hipFunction_t jit_fn = nullptr, jit_fn_eps = nullptr, jit_fn_rejuv = nullptr, jit_fn_prior = nullptr, jit_fn_lj = nullptr; std::string jit_log; bool jit_lds_attr = false, jit_rejuv_attr = false, jit_has_ad = false, jit_has_dense = false, an_jit = false /* FG_GRAD_ANALYTIC runs on the compiled unit's derivative code */; double *d_jit_tab = nullptr, *d_jit_mh_tab = nullptr;   // the modules' constant tables (fg_jit_bind_tables)
    FgMhMwState mhmw;            // what the multi-wave MH launchers decide once per engine (fg_mh.hip)
    int jit_mh_state = 0, jit_mh_W = 1, jit_mh_direct = 0; size_t jit_mh_lds = 0; hipModule_t jit_mh_mod = nullptr; hipFunction_t jit_mh_fn[2] = {nullptr, nullptr};   // ... and its MH kernel (128- and 256-VGPR builds)
    std::string last_mh_kernel;  // kernel the last fg_mh_step launch ran (fg_mh_last_kernel)
    // mean-field VI (fg_vi.hip): factor table, stream ids, per-sample terms, per-wave sums, ELBOs, global tiles -- grown on demand
    std::vector<void *> vi_allocs;
    void *d_vi_tab = nullptr; uint32_t *d_vi_sid = nullptr; double *d_vi_terms = nullptr, *d_vi_partial = nullptr, *d_vi_elbo = nullptr, *d_vi_gtile = nullptr;
    size_t vi_cap_tab = 0, vi_cap_eval = 0, vi_cap_terms = 0;
    int mw_override = 0;       // FG_HMC_WAVES env: force waves per tile of the multi-wave HMC kernel (tests)
    // the model's return value (fg_result.hip): device copies of the result program, made at the first fg_result_eval; the row of the draw
    // each used site comes from as last uploaded; the global scratch of programs whose slice exceeds a CU's LDS, grown on demand
    FgIns *d_res_ins = nullptr; double *d_res_pool = nullptr; int *d_res_site = nullptr, *d_res_row = nullptr; std::vector<int> res_row_host;
    double *d_res_gtile = nullptr; size_t res_gtile_bytes = 0;
    // predictive draws (fg_predict.hip): the row of the draw each site comes from and the table row of each observe statement, as last
    // uploaded (made at the first fg_predict_eval); the global scratch of programs whose slice exceeds a CU's LDS, grown on demand
    int *d_pred_row = nullptr, *d_pred_sel = nullptr; std::vector<int> pred_row_host, pred_sel_host;
    double *d_pred_gtile = nullptr; size_t pred_gtile_bytes = 0;
};

// p0 ~ N(0, M): hmc.rs:436-441.  Box-Muller pairs from the chain's (iteration) stream.
__device__ __forceinline__ void fg_draw_momentum(const FgProgramDev &P, FgStream &rng, double *pl, int tw, const double *mass_sqrt,
                                                 long long C) {
    for (int i = 0; i < P.d; i += 2) {
        double z0, z1;
        fg_rng_normal_pair(rng, z0, z1);
        pl[i * tw] = z0 * (mass_sqrt ? mass_sqrt[(long long)i * C] : 1.0);
        if (i + 1 < P.d) pl[(i + 1) * tw] = z1 * (mass_sqrt ? mass_sqrt[(long long)(i + 1) * C] : 1.0);
    }
}


namespace {

// Tile width = lanes per wave that own a chain = 64.  Spreading 65 536 chains over narrower, half-empty waves was
// measured NOT to help (profiles/round1_occupancy_sweep.txt): an instruction costs the same whatever the number of
// active lanes, and the LDS tile, not the wave count, limits residency.  More waves per SIMD come from SHARING a tile
// between waves instead (k_hmc_stream_steps); the tile stride stays a compile-time constant.
int tile_width_for(long long C) { (void)C; return FG_WAVE; }

template <typename K>
int set_lds(K kernel, size_t bytes) {
    if (bytes > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return FG_OK;
}

template <typename T>
int dev_alloc(T **p, size_t n) {
    HIPCHK(hipMalloc((void **)p, (n ? n : 1) * sizeof(T)));
    HIPCHK(hipMemset(*p, 0, (n ? n : 1) * sizeof(T)));
    return FG_OK;
}
template <typename T>
int dev_upload(T **p, const std::vector<T> &v) {
    int rc = dev_alloc(p, v.size());
    if (rc) return rc;
    if (!v.empty()) HIPCHK(hipMemcpy(*p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
    return FG_OK;
}

// One launch of a library kernel picked from a table of typed pointers (all instantiations of a kernel template have one
// function type: the arguments are checked against it here, once).  A tile above 64 KB needs the function's dynamic-LDS limit
// raised, once per (device, function): `raised` is the table entry's mask of the devices that have it.  LDS_MAX: what it is raised
// to -- a CU's 160 KB less the kernel's static LDS (the runtime refuses a limit that the two together exceed).
template <typename T> struct fg_same { using type = T; };
template <int LDS_MAX = 160 * 1024, typename... P>
int fg_launch(fg_engine *e, void (*fn)(P...), unsigned long long &raised, dim3 grid, dim3 block, size_t lds, const typename fg_same<P>::type &...args) {
    const unsigned long long dev_bit = 1ull << (e->device & 63);
    if (lds > 64 * 1024 && !(raised & dev_bit)) {
        const hipError_t he = hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX);
        if (he != hipSuccess) { fg_set_error(std::string("hipFuncSetAttribute: ") + hipGetErrorString(he)); return FG_E_HIP; }
        raised |= dev_bit;
    }
    void *argv[] = { (void *)&args... };
    (void)hipLaunchKernel((const void *)fn, grid, block, argv, lds, e->stream);
    HIPCHK(hipGetLastError());
    return FG_OK;
}

}  // namespace


#define NEED_ENGINE(e) do { if (!(e)) { fg_set_error("null engine"); return FG_E_BAD_ARG; } \
    if (hipSetDevice((e)->device) != hipSuccess) { fg_set_error("hipSetDevice failed"); return FG_E_HIP; } } while (0)

// fg_hmc_interp.hip: adaptive_smc's rejuvenation move through the model compiled at run time (FG_E_UNSUPPORTED: the interpreter kernel)
struct FgSmcDev; struct FgSmcScalars;
int fg_smc_jit_rejuv_launch(fg_engine *e, const FgSmcDev &M, const FgSmcScalars *st, uint32_t move_id, unsigned *n_blk_out, const long long *vsrc = nullptr, double *pmax = nullptr);
int fg_jit_prior_launch(fg_engine *e, uint32_t iteration, uint32_t purpose, double *d_acc, double *d_lj, bool compile);   // k_prior_jit, or FG_E_UNSUPPORTED
int fg_jit_log_joint_launch(fg_engine *e, double *d_acc, double *d_lj, bool compile);                                     // k_log_joint_jit, or FG_E_UNSUPPORTED
bool fg_hmc_jit_has_ad(fg_engine *e);      // the compiled module holds the forward-mode derivative of every sub-program (FG_GRAD_ANALYTIC for any program)

// fg_hmc_sep.hip: register-resident trajectories for independent-sites programs (FG_E_UNSUPPORTED: not applicable)
int fg_hmc_sep_launch(fg_engine *e, int iter0, int n, int welford_on, double *draws, int first_sample_t, double *pos_all, double *info);

// fg_hmc_lin.hip: observation-major finite-difference gradient for dense regressions (FG_E_UNSUPPORTED: not applicable)
bool fg_hmc_lin_gate(const fg_engine *e);   // the static part of what fg_hmc_lin_launch takes (hmc_jit_first asks too)
int fg_hmc_lin_launch(fg_engine *e, int iter0, int n, int welford_on, double *draws, int first_sample_t, double *pos_all, double *info);

// fg_hmc_interp.hip: the program compiled at run time (fg_jit.cpp) behind the same multi-wave kernel (FG_E_UNSUPPORTED: not applicable)
int fg_hmc_jit_launch(fg_engine *e, int iter0, int n, int welford_on, double *draws, int first_sample_t, double *pos_all, double *info);
int fg_hmc_jit_find_eps(fg_engine *e, uint32_t instance, int injected, double *d_eps_out);
// fg_hmc_interp.hip: interpreter programs with a tile shared by W waves (FG_E_UNSUPPORTED: not applicable)
int fg_hmc_interp_launch(fg_engine *e, int iter0, int n, int welford_on, double *draws, int first_sample_t, double *pos_all, double *info);

// fg_engine.hip internals used by fg_state.hip
extern "C" {
int fg_internal_rescore_sessions(fg_engine *e);   // the cached log-joint of a live MH / HMC session at the engine's values (fg_gibbs.hip)
int fg_internal_hmc_alloc(fg_engine *e, bool mass);
void fg_internal_hmc_set_cfg(fg_engine *e, const fg_hmc_config *cfg);
int fg_internal_hmc_step(fg_engine *e, int n_transitions, double *d_draws, double *d_pos_all, double *d_info);
int fg_internal_mh_alloc(fg_engine *e);
int fg_internal_mh_set_overrides(fg_engine *e, const fg_site_proposal *overrides);
int fg_internal_smc_weights(fg_engine *e, const double **d_w);   // fg_smc.hip, for fg_wpop.hip: FG_E_STATE without a population
}

// fg_mh_interp.hip: multi-wave single-site MH for interpreter programs (FG_E_UNSUPPORTED: not applicable)
long long fg_mhi_ins_cost(const FgIns &in);   // relative cost of an instruction (statement splits)
int fg_mh_interp_launch(fg_engine *e, int iter0, int n_steps, long long *draws, int first_sample_t);

// fg_mh.hip: multi-wave single-site MH for programs with a score stream (FG_E_UNSUPPORTED: not applicable)
int fg_mh_mw_launch(fg_engine *e, int iter0, int n_steps, long long *draws, int first_sample_t);
int fg_mh_mw_nostream_launch(fg_engine *e, int iter0, int n_steps, long long *draws, int first_sample_t, const std::vector<int> &stmt_end,
                             const std::vector<unsigned char> &acc, const int *d_site_ins);

extern "C" int fg_launch_prior(fg_engine *e, uint32_t iteration, uint32_t purpose, double *d_acc, double *d_lj);
