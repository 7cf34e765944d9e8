// fg_hmc_interp.hip -- HmcSession::step (hmc.rs:819-919) for programs that need the interpreter (a parameter that is an expression,
// a guard, a select ...: no gradient stream), with a 64-chain tile shared by W waves.
//
// k_hmc_steps gives such a program ONE wave per tile: at 65 536 chains that is one wave per SIMD, so every instruction fetch, LDS
// round trip, scalar branch and out-of-line density call of the interpreter sits exposed between its f64 instructions (a lone
// wave issues a dependent f64 op every ~6 cycles, two or more one per ~4.4: profiles/round1_f64_issue_microbench.txt), and at 8 192
// chains seven SIMDs in eight are idle.  The finite-difference gradient (hmc.rs:304-329) is 2 d independent model runs: here
// wave w evaluates ITS (coordinate, sign) tasks -- a host-side longest-processing-time split by sub-program cost.  The site rows
// of the tile are shared and read-only inside a gradient; what an evaluation writes -- the perturbed coordinate, expression
// temporaries, Categorical tables, select options -- lives in a small block of rows private to the wave (FgRemap, fg_interp.h:
// the interpreter redirects reads of slot i to the wave's `pert` row and offsets every row above the sites), so a tile costs
// S + W (temporaries + 2) rows of LDS, not W copies.  Every evaluation leaves its log-joint in an LDS row; after a workgroup
// barrier wave k mod W forms g_k, kicks p_k and drifts q_k, and a second barrier publishes it.  The sequential parts
// (Hamiltonians, the endpoint score in program order, accept, dual averaging) run on wave 0 exactly as in k_hmc_stream_steps.
// Per coordinate the operations and their order are those of fg_trajectory (fg_engine.hip), so the kernel is bit-identical to
// k_hmc_steps for every W (tests/test_gpu_parity.py::test_hmc_interp_multiwave_is_bit_identical).
#include "fg_engine_internal.h"
#include "fg_cold.h"
#include "fg_jit.h"
#include "fg_smc_plan.h"

#define FG_MWI_MAX 16         /* waves per tile */

struct FgMwi { int off[FG_MWI_MAX + 1]; const int *order; long long *prof; int n_sub_ins, n_fast_ins; };   // wave w owns the tasks order[off[w] .. off[w + 1]): 2 i + sign = evaluate at q_i + h / q_i - h;
                                                                                  // prof: [2 d] cycles of each task (tile 0, first gradient of the launch) or null

template <bool PL>
__device__ __forceinline__ void fg_hmc_interp_mw_body(const FgProgramDev &P, const FgChainCtx &X, const FgHmcDev &H, const FgMwi &seg, int iter0, int n_steps,
                                                      int n_warmup, int welford_on, double *draws, int first_sample_t,
                                                      double *pos_all /*[n][d][C] or null*/, double *info /*[n][4][C] or null*/) {
    extern __shared__ double lds[];
    constexpr int tw = FG_WAVE;
    const int lane = threadIdx.x & (FG_WAVE - 1);
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int W = (int)(blockDim.x >> 6);
    const long long chain = (long long)blockIdx.x * tw + lane;
    const bool live = chain < X.C;
    const long long c = live ? chain : X.C - 1;
    const int d = P.d, L = H.L;
    const int np = P.n_slots - P.S + 1;                                              // private rows of a wave: temporaries, zero slot, perturbed coordinate
    double *slots = lds + lane;                                                      // site rows [0, S), shared
    double *pl = lds + (long long)(P.S + W * np) * tw + lane;                        // momentum rows, shared
    double *ev_lp = lds + ((long long)(P.S + W * np) + d) * tw + lane;               // log-joint of evaluation (coordinate i, sign): row 2 i + sign
    double *xch = lds + ((long long)(P.S + W * np) + 3 * d) * tw + lane;             // rows: 0 step size, 1 accepted, 2.. per-wave divergence flags
    // PL: the sub-programs and the whole program, staged in LDS behind the rows (instruction fetch = ds_read_b32)
    const FgIns *l_sub = P.sub, *l_fast = P.ins_fast;
    if (PL) {
        uint32_t *dst = (uint32_t *)(lds + ((long long)(P.S + W * np) + 3 * d + 2 + W) * tw);
        const int n_sub_dw = seg.n_sub_ins * 24, n_fast_dw = seg.n_fast_ins * 24;
        for (int k = (int)threadIdx.x; k < n_sub_dw; k += (int)blockDim.x) dst[k] = ((const uint32_t *)P.sub)[k];
        for (int k = (int)threadIdx.x; k < n_fast_dw; k += (int)blockDim.x) dst[n_sub_dw + k] = ((const uint32_t *)P.ins_fast)[k];
        l_sub = (const FgIns *)dst; l_fast = (const FgIns *)(dst + n_sub_dw);
    }
    FgRemap rm;
    rm.pi = 0xffffffffu; rm.n_shared = (uint32_t)P.S; rm.woff = (uint32_t)(wv * np); rm.pert = (uint32_t)(P.n_slots + wv * np);
    const int j0 = seg.off[wv], j1 = seg.off[wv + 1];
    const bool sparse = H.grad_mode != FG_GRAD_FD_DENSE;
    const double *mi = H.use_mass ? H.m_inv + c : nullptr;
    const double *ms = H.use_mass ? H.mass_sqrt + c : nullptr;
    const uint32_t sk0 = (uint32_t)X.seed, sk1 = (uint32_t)(X.seed >> 32), gchain = X.chain0 + (uint32_t)c;
    const double h = H.h;
    for (int j = wv; j < P.S; j += W) slots[P.site_slot[j] * tw] = fg_as_double(X.values[(long long)j * X.C + c]);
    slots[(P.n_slots - 1 + rm.woff) * tw] = 0.0;                                     // the wave's always-zero slot
    // wave 0 owns the per-chain sampler state
    double lj = 0.0, eps = 0.0, frozen = 0.0, da_mu = 0.0, da_leb = 0.0, da_hbar = 0.0, asum = 0.0;
    unsigned long long da_m = 0, ndiv = 0;
    if (wv == 0) {
        lj = H.lj[c]; eps = H.eps[c]; frozen = H.frozen[c];
        da_mu = H.da_mu[c]; da_leb = H.da_leb[c]; da_hbar = H.da_hbar[c]; da_m = H.da_m[c];
    }
    for (int t = 0; t < n_steps; ++t) {
        const int iter = iter0 + t;
        const bool warming = iter < n_warmup;
        double h0 = 0.0, u = 0.0;
        // p0 ~ N(0, M) (hmc.rs:436-441): Box-Muller pair j of the chain's (iteration) stream is Philox block j
        const int n_pairs = (d + 1) >> 1;
        for (int j = wv; j < n_pairs; j += W) {
            const FgD2 zz = fg_cold_normal_pair(sk0, sk1, gchain, (uint32_t)j, (uint32_t)iter, FG_RNG_HMC);
            const int i = 2 * j;
            pl[i * tw] = zz.a * (ms ? ms[(long long)i * X.C] : 1.0);
            if (i + 1 < d) pl[(i + 1) * tw] = zz.b * (ms ? ms[(long long)(i + 1) * X.C] : 1.0);
        }
        if (wv == 0) {
            double e;
            if (warming) e = eps;
            else {                                             // frozen_or_current: hmc.rs:789-798
                if (frozen == frozen) e = frozen;
                else if (n_warmup > 0) e = fg_cold_exp(da_leb);
                else e = eps;
                frozen = e;
            }
            u = fg_cold_u01_pair(sk0, sk1, gchain, (uint32_t)n_pairs, (uint32_t)iter, FG_RNG_HMC).a;
            xch[0] = e;
        }
        __syncthreads();
        if (wv == 0) h0 = -lj + fg_kinetic(P, pl, tw, mi, X.C);  // hmc.rs:442-443 (all of p0, before any kick)
        __syncthreads();
        const double e = xch[0], hk = 0.5 * e;
        // leapfrog (hmc.rs:353-407) + endpoint score (hmc.rs:283-299) as one flat loop of model evaluations around the interpreter's
        // single call site: this wave's (coordinate, sign) tasks for gradients 0 .. L, then (wave 0) the whole program.  An evaluation
        // leaves its log-joint in row 2 i + sign of `ev_lp`; behind the barrier wave k mod W forms g_k, kicks p_k and drifts q_k.
        const int n_evals = (L + 1) * (j1 - j0) + (wv == 0 ? 1 : 0);
        bool bad = false;
        int s = 0, jj = j0;
        double lj_new = FG_NEG_INF;
        for (int ev = 0; ev < n_evals; ++ev) {
            const bool is_final = (wv == 0) && (ev == n_evals - 1);
            const FgIns *prog = l_fast;
            int n = P.n_ins, task = 0;
            rm.pi = 0xffffffffu;
            if (!is_final) {
                // the perturbed value goes to the wave's private row; the shared q_i is only read (hmc.rs:317-319 restores it: here it never changes)
                task = seg.order[jj];
                const FgCoord cd = P.coord[task >> 1];
                const double orig = slots[cd.slot * tw];
                slots[rm.pert * tw] = (task & 1) ? orig - h : orig + h;
                rm.pi = (uint32_t)cd.slot;
                if (sparse) { prog = l_sub + cd.sub_off; n = cd.sub_n; }
            }
            const bool clocked = seg.prof != nullptr && blockIdx.x == 0 && t == 0 && s == 0 && !is_final;
            long long t0 = 0;
            if (clocked) t0 = (long long)clock64();
            FgAcc3 A = {0.0, 0.0, 0.0};
            fg_exec<FG_MODE_SCORE, false, true, PL>(prog, n, P.pool, slots, tw, A, nullptr, nullptr, 0, false, nullptr, &rm);
            const double tot = fg_total(A);
            if (is_final) { lj_new = tot; break; }
            ev_lp[task * tw] = tot;
            if (clocked && lane == 0) seg.prof[task] = (long long)clock64() - t0;
            if (++jj == j1) {
                jj = j0;
                __syncthreads();                                      // every evaluation of this gradient done, every read of q done
                for (int k = wv; k < d; k += W) {
                    const double g = (ev_lp[2 * k * tw] - ev_lp[(2 * k + 1) * tw]) / (2.0 * h);    // hmc.rs:322
                    bad = bad || !fg_finite(g);
                    double p = pl[k * tw];
                    p += hk * g;                                      // hmc.rs:389 / :400
                    if (s > 0 && s < L) p += hk * g;                  // trailing kick of step s + leading kick of s + 1
                    pl[k * tw] = p;
                    if (s < L) {                                      // q += eps * M^-1 p   (hmc.rs:391-393)
                        const double mk = mi ? mi[(long long)k * X.C] : 1.0;
                        slots[k * tw] += e * mk * p;
                    }
                }
                __syncthreads();
                ++s;
            }
        }
        xch[(2 + wv) * tw] = bad ? 1.0 : 0.0;
        __syncthreads();
        if (wv == 0) {
            bool div = false;
            for (int w = 0; w < W; ++w) div = div || xch[(2 + w) * tw] != 0.0;
            div = div || !fg_finite(lj_new);
            double ap = 0.0; bool acc = false;
            if (!div) {
                const double h_new = -lj_new + fg_kinetic(P, pl, tw, mi, X.C);
                ap = fg_cold_accept_prob(h0, h_new);             // hmc.rs:460
                acc = u < ap;                                    // hmc.rs:461
            }
            if (acc) lj = lj_new;
            xch[tw] = acc ? 1.0 : 0.0;
            asum += ap; ndiv += div ? 1ull : 0ull;
            if (live && info) {                                  // HmcStepInfo: hmc.rs:587-602
                double *r = info + (long long)t * 4 * X.C + c;
                r[0] = acc ? 1.0 : 0.0; r[X.C] = div ? 1.0 : 0.0; r[2 * X.C] = ap; r[3 * X.C] = e;
            }
            if (warming) {                                       // DualAveraging::update: hmc.rs:168-178
                da_m += 1ull;
                const FgD3 r = fg_cold_da_update(da_hbar, da_leb, (double)da_m, da_mu, H.target, ap);
                eps = r.a; da_hbar = r.b; da_leb = r.c;
            }
        }
        __syncthreads();
        const bool acc = xch[tw] != 0.0;
        unsigned long long wn = 0;
        if (warming && welford_on) wn = H.w_n[c] + 1ull;          // every wave reads the old count before wave 0 bumps it below
        for (int k = wv; k < d; k += W) {                         // commit or roll back: coordinate k by wave k mod W
            const long long g = (long long)P.f64_site[k] * X.C + c;
            if (acc) { if (live) X.values[g] = fg_as_i64(slots[k * tw]); }
            else slots[k * tw] = fg_as_double(X.values[g]);
            const double x = slots[k * tw];
            if (live && pos_all) pos_all[((long long)t * d + k) * X.C + c] = x;
            if (warming) {
                if (welford_on) {                                 // Welford::push: hmc.rs:202-211
                    const long long gi = (long long)k * X.C + c;
                    const double n = (double)wn;
                    double mean = H.w_mean[gi];
                    const double delta = x - mean;
                    mean += delta / n;
                    const double delta2 = x - mean;
                    if (live) { H.w_mean[gi] = mean; H.w_m2[gi] += delta * delta2; }
                }
            } else if (draws && live) draws[((long long)(t - first_sample_t) * d + k) * X.C + c] = x;   // hmc.rs:577-582
        }
        if (warming && welford_on) {
            __syncthreads();                                      // all waves hold the old count
            if (wv == 0 && live) H.w_n[c] = wn;
        }
    }
    if (wv == 0 && live) {
        H.lj[c] = lj; H.eps[c] = eps; H.frozen[c] = frozen;
        H.da_mu[c] = da_mu; H.da_leb[c] = da_leb; H.da_hbar[c] = da_hbar; H.da_m[c] = da_m;
        H.alpha_sum[c] += asum; H.n_div[c] += ndiv;
    }
}

// OCC = waves per SIMD the register budget allows (2: 256 VGPRs, no spills; 4: 128 with the interpreter's cold paths spilling -- the
// faster one wherever enough waves exist: tools/bench_interp_mw.py); PL: program staged in LDS
#define FG_MWI_KERNEL(OCC, PL, NAME) \
__global__ __attribute__((amdgpu_waves_per_eu(OCC, OCC))) __launch_bounds__(FG_WAVE * 4 * OCC) \
void NAME(FgProgramDev P, FgChainCtx X, FgHmcDev H, FgMwi seg, int iter0, int n_steps, int n_warmup, int welford_on, double *draws, \
          int first_sample_t, double *pos_all, double *info) { \
    fg_hmc_interp_mw_body<PL>(P, X, H, seg, iter0, n_steps, n_warmup, welford_on, draws, first_sample_t, pos_all, info); }
FG_MWI_KERNEL(2, false, k_hmc_interp_mw_steps_occ2)
FG_MWI_KERNEL(4, false, k_hmc_interp_mw_steps_occ4)
FG_MWI_KERNEL(2, true, k_hmc_interp_mw_steps_lds_occ2)
FG_MWI_KERNEL(4, true, k_hmc_interp_mw_steps_lds_occ4)

// Plan (fg_hmc_split_plan.h: the split once per engine and gradient mode, the shape per launch), upload, launch, name.
int fg_hmc_interp_launch(fg_engine *e, int iter0, int n, int welford_on, double *draws, int first_sample_t, double *pos_all, double *info) {
    if (e->interp_mw_disabled || e->gt || e->tw != FG_WAVE || e->d < 2) return FG_E_UNSUPPORTED;
    const unsigned tiles = (unsigned)((e->C + e->tw - 1) / e->tw);
    const bool sparse = e->cfg.grad_mode != FG_GRAD_FD_DENSE;
    for (int j = 0; j < e->S; ++j) if (e->prog->site_slot[j] >= e->S) return FG_E_UNSUPPORTED;    // site rows first, the private rows above them
    for (int k = 0; k < e->d; ++k) if (e->prog->coord[k].slot != k) return FG_E_UNSUPPORTED;
    FgHmcSplitState &st = e->hsplit;
    const FgTaskSwitches sw = fg_task_switches();
    const int n_tasks = 2 * e->d;
    if (!st.d_mwi_order) {
        HIPCHK(hipMalloc((void **)&st.d_mwi_order, (size_t)2 * n_tasks * sizeof(int)));
        HIPCHK(hipMalloc((void **)&st.d_mwi_prof, (size_t)n_tasks * sizeof(long long)));
        HIPCHK(hipMemsetAsync(st.d_mwi_prof, 0, (size_t)n_tasks * sizeof(long long), e->stream));
    }
    const bool debug = std::getenv("FG_HMC_INTERP_DEBUG") != nullptr;
    if (debug && st.mwi_calibrated == 1) {                      // FG_HMC_INTERP_DEBUG: the cycles the previous launch clocked per task, beside the static costs
        std::vector<long long> prof(n_tasks, 0);
        HIPCHK(hipMemcpyAsync(prof.data(), st.d_mwi_prof, (size_t)n_tasks * sizeof(long long), hipMemcpyDeviceToHost, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        for (int k = 0; k < e->d; ++k) fprintf(stderr, "coord %d static %lld measured %lld %lld sub_n %d\n", k, st.cost[k], prof[2 * k], prof[2 * k + 1], e->prog->coord[k].sub_n);
        st.mwi_calibrated = 2;
    }
    const FgSplitKey key = sparse ? FG_SPLIT_INTERP_SPARSE : FG_SPLIT_INTERP_DENSE;
    if (st.key != key) {
        std::vector<long long> tcost;
        st.cost.assign(e->d, 1);
        if (sparse) fg_task_coord_costs(e->prog->coord.data(), e->d, e->prog->sub.data(), st.cost, tcost);
        const FgMwiTaskIn in = { e->d, e->S, e->n_slots, e->mw_override, &st.cost, sw };
        if (int rc = fg_mwi_task_plan(in, &st.split)) return rc;
        HIPCHK(hipMemcpyAsync(st.d_mwi_order, st.split.order.data(), (size_t)n_tasks * sizeof(int), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        st.key = key; st.mwi_calibrated = 0;
    }
    const int W = st.split.W;
    FgMwi seg;
    for (int w = 0; w <= FG_MWI_MAX; ++w) seg.off[w] = st.split.off[w];
    seg.order = st.d_mwi_order;
    seg.prof = (debug && st.mwi_calibrated == 0) ? st.d_mwi_prof : nullptr;
    if (debug && st.mwi_calibrated == 0) st.mwi_calibrated = 1;
    seg.n_sub_ins = (int)e->prog->sub.size(); seg.n_fast_ins = (int)e->prog->ins_fast.size();
    const FgMwiLaunchIn lin = { e->d, e->S, e->n_slots, W, (e->prog->sub.size() + e->prog->ins_fast.size()) * sizeof(FgIns), tiles, e->n_simd, sw };
    const FgMwiLaunchShape sh = fg_mwi_launch_shape(lin);
#define FG_MWI_LAUNCH(K) do { if (int rc = set_lds(K, sh.lds)) return rc; \
    hipLaunchKernelGGL(K, dim3(tiles), dim3(FG_WAVE * W), sh.lds, e->stream, e->P, e->X, e->H, seg, iter0, n, e->n_warmup, welford_on, \
                       draws, first_sample_t, pos_all, info); } while (0)
    if (sh.pl) { if (sh.occ == 4) FG_MWI_LAUNCH(k_hmc_interp_mw_steps_lds_occ4); else FG_MWI_LAUNCH(k_hmc_interp_mw_steps_lds_occ2); }
    else { if (sh.occ == 4) FG_MWI_LAUNCH(k_hmc_interp_mw_steps_occ4); else FG_MWI_LAUNCH(k_hmc_interp_mw_steps_occ2); }
#undef FG_MWI_LAUNCH
    HIPCHK(hipGetLastError());
    e->last_hmc_kernel = sh.name;
    return FG_OK;
}

// ---- the same kernel around a model compiled at run time (fg_jit.cpp, fg_hmc_jit_body.h) --------------------------------------
struct FgJitSeg { int off[FG_MWI_MAX + 1]; const int *order; int baked; };   // (fg_hmc_jit_body.h's)

// the plan of this engine's chain count under the switches `sw` (fg_jit_task_plan); FG_JIT_VERBOSE's lines
static FgJitTaskPlan jit_task_plan(fg_engine *e, unsigned tiles, int grad_mode, const FgTaskSwitches &sw, bool say) {
    std::vector<long long> cost, tcost;
    fg_task_coord_costs(e->prog->coord.data(), e->d, e->prog->sub.data(), cost, tcost);
    const FgJitTaskIn in = { e->d, e->S, tiles, e->n_simd, e->mw_override, &cost, &tcost, grad_mode, sw };
    const FgJitTaskPlan p = fg_jit_task_plan(in);
    if (say && sw.verbose.set) fputs(fg_jit_task_say(p, e->d).c_str(), stderr);
    return p;
}

// the program's compiled module (once per engine): HMC transitions, the step-size search, adaptive_smc's rejuvenation move
static int jit_hmc_module(fg_engine *e) {
    if (e->jit_state < 0 || e->gt || e->tw != FG_WAVE || e->d < 1) return FG_E_UNSUPPORTED;
    if (e->jit_state == 0) {
        e->jit_state = -1;
        if (const char *sp = std::getenv("FG_JIT")) if (std::atoi(sp) == 0) return FG_E_UNSUPPORTED;
        for (int j = 0; j < e->S; ++j) if (e->prog->site_slot[j] >= e->S) return FG_E_UNSUPPORTED;
        for (int k = 0; k < e->d; ++k) if (e->prog->coord[k].slot != k) return FG_E_UNSUPPORTED;
        if (e->prog->sub.size() + e->prog->ins_fast.size() > 64000000) return FG_E_UNSUPPORTED;
        std::vector<double> ctab;
        bool has_ad = false, has_dense = false;
        FgHmcSplitState &st = e->hsplit;
        std::vector<std::vector<int>> bins;
        st.gen_sparse = st.gen_dense = FgTaskSplit();
        const FgTaskSwitches sw = fg_task_switches();
        if (!fg_switch_is(sw.tasks, 0)) {                         // the unit is generated behind the split of this chain count under these switches
            const unsigned tiles0 = (unsigned)((e->C + e->tw - 1) / e->tw);
            const FgJitTaskPlan p = jit_task_plan(e, tiles0, FG_GRAD_FD_SPARSE, sw, true);
            bins = p.bins; st.gen_sparse = p.split;
            st.gen_dense = jit_task_plan(e, tiles0, FG_GRAD_FD_DENSE, sw, false).split;
        }
        const std::string src = fg_jit_hmc_source(e->prog, &ctab, &has_ad, &has_dense, bins.empty() ? nullptr : &bins, st.gen_sparse.cbins.empty() ? nullptr : &st.gen_sparse.cbins,
                                                  st.gen_dense.cbins.empty() ? nullptr : &st.gen_dense.cbins);
        if (src.empty() || src.size() > (6u << 20)) return FG_E_UNSUPPORTED;                            // plates roll into loops; what stays straight-line must stay compilable in seconds
        std::vector<char> code;
        const int rc = fg_jit_get_code(src, code, e->jit_log);
        if (rc != FG_OK) {
            if (std::getenv("FG_JIT_VERBOSE")) fprintf(stderr, "fugue_amd: run-time compilation unavailable (%s): the interpreter kernels take this program\n", e->jit_log.c_str());
            return FG_E_UNSUPPORTED;
        }
        if (hipModuleLoadData(&e->jit_mod, code.data()) != hipSuccess || hipModuleGetFunction(&e->jit_fn, e->jit_mod, "k_hmc_jit_steps") != hipSuccess ||
            hipModuleGetFunction(&e->jit_fn_eps, e->jit_mod, "k_hmc_jit_find_eps") != hipSuccess ||
            hipModuleGetFunction(&e->jit_fn_rejuv, e->jit_mod, "k_smc_jit_rejuv") != hipSuccess ||
            fg_jit_bind_tables(e->jit_mod, ctab, &e->d_jit_tab, e->stream) != FG_OK) {
            e->jit_log = "hipModuleLoadData / hipModuleGetFunction / table upload failed"; (void)hipGetLastError();
            return FG_E_UNSUPPORTED;
        }
        // (optional entry points: a unit whose generic program the generator does not cover has no k_prior_jit)
        if (hipModuleGetFunction(&e->jit_fn_prior, e->jit_mod, "k_prior_jit") != hipSuccess) { e->jit_fn_prior = nullptr; (void)hipGetLastError(); }
        if (hipModuleGetFunction(&e->jit_fn_lj, e->jit_mod, "k_log_joint_jit") != hipSuccess) { e->jit_fn_lj = nullptr; (void)hipGetLastError(); }
        e->jit_state = 1; e->jit_has_ad = has_ad; e->jit_has_dense = has_dense;
    }
    return FG_OK;
}

// run(PriorHandler) / run(ScoreGivenTrace) of every chain through the compiled model (k_prior_jit / k_log_joint_jit): FG_E_UNSUPPORTED when
// there is none (the caller takes the interpreter kernels).  `compile`: build the unit now if it is not there yet (callers for which the
// draw is a visible part of the work: adaptive_smc, sessions of programs that will step through the unit anyway).
static int jit_tile_launch(fg_engine *e, hipFunction_t fn, void **args) {
    const size_t tile = (size_t)e->S * FG_WAVE * sizeof(double);
    if (!fn || tile == 0 || tile > 64 * 1024) return FG_E_UNSUPPORTED;
    const int wpb = (int)std::max<size_t>(1, std::min<size_t>(4, (64 * 1024) / tile));
    const unsigned nblk = (unsigned)((e->C + (long long)FG_WAVE * wpb - 1) / ((long long)FG_WAVE * wpb));
    HIPCHK(hipModuleLaunchKernel(fn, nblk, 1, 1, FG_WAVE * wpb, 1, 1, (unsigned)(tile * wpb), e->stream, args, nullptr));
    return FG_OK;
}
int fg_jit_prior_launch(fg_engine *e, uint32_t iteration, uint32_t purpose, double *d_acc, double *d_lj, bool compile) {
    if (e->jit_state != 1 && !(compile && e->jit_state == 0)) return FG_E_UNSUPPORTED;
    if (int rc = jit_hmc_module(e)) {
        if (std::getenv("FG_JIT_VERBOSE")) fprintf(stderr, "fugue_amd: no compiled prior draw (state %d, d %d, S %d, tw %d, gt %d: %s)\n", e->jit_state, e->d, e->S, e->tw, (int)(e->gt != 0), e->jit_log.c_str());
        return rc;
    }
    if (!e->jit_fn_prior && std::getenv("FG_JIT_VERBOSE")) fprintf(stderr, "fugue_amd: the compiled unit has no k_prior_jit\n");
    void *args[] = { &e->P, &e->X, &iteration, &purpose, &d_acc, &d_lj };
    return jit_tile_launch(e, e->jit_fn_prior, args);
}
int fg_jit_log_joint_launch(fg_engine *e, double *d_acc, double *d_lj, bool compile) {
    if (e->jit_state != 1 && !(compile && e->jit_state == 0)) return FG_E_UNSUPPORTED;
    if (int rc = jit_hmc_module(e)) return rc;
    void *args[] = { &e->P, &e->X, &d_acc, &d_lj };
    return jit_tile_launch(e, e->jit_fn_lj, args);
}

// does the compiled module hold the analytic gradient of this program (FG_GRAD_ANALYTIC beyond Normal force terms)?  Compiles it if need be.
bool fg_hmc_jit_has_ad(fg_engine *e) { return jit_hmc_module(e) == FG_OK && e->jit_has_ad; }

// adaptive_smc's rejuvenation move of a program without a score stream through the compiled model (k_smc_jit_rejuv, fg_hmc_jit_body.h);
// FG_E_UNSUPPORTED: the interpreter kernel k_smc_rejuv<-1> takes it.  n_blk_out: blocks launched (rows of M.blk that k_smc_adapt adds).
int fg_smc_jit_rejuv_launch(fg_engine *e, const FgSmcDev &M, const FgSmcScalars *st, uint32_t move_id, unsigned *n_blk_out, const long long *vsrc, double *pmax) {
    FgSmcJitShape sh;      // (asked ahead of the module: the callers come with 512 n_slots <= 150 KB and n_slots > S, so its tile test refuses nothing the site test let through)
    if (int rc = fg_smc_jit_rejuv_shape(e->S, e->C, &sh)) return rc;
    if (int rc = jit_hmc_module(e)) return rc;
    if (sh.lds > FG_SMC_LDS_PLAIN && !e->jit_rejuv_attr) {
        if (hipFuncSetAttribute((const void *)e->jit_fn_rejuv, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) { (void)hipGetLastError(); return FG_E_UNSUPPORTED; }
        e->jit_rejuv_attr = true;
    }
    FgSmcDev Mv = M;
    void *args[] = { &e->P, &e->X, &Mv, &st, &move_id, &vsrc, &pmax };
    HIPCHK(hipModuleLaunchKernel(e->jit_fn_rejuv, sh.nblk, 1, 1, FG_WAVE * sh.wpb, 1, 1, (unsigned)sh.lds, e->stream, args, nullptr));
    if (n_blk_out) *n_blk_out = sh.nblk;
    return FG_OK;
}

// ... and the task split of its HMC kernels; FG_E_UNSUPPORTED when there is none
static int jit_hmc_prepare(fg_engine *e, unsigned tiles) {
    if (int rc = jit_hmc_module(e)) return rc;
    const bool dense = e->cfg.grad_mode == FG_GRAD_FD_DENSE;
    if (dense && !e->jit_has_dense) return FG_E_UNSUPPORTED;      // (d copies of the program were too much to compile: the interpreter kernels)
    const int n_tasks = 2 * e->d;
    {   // LDS: S site rows + d momentum rows + 2 d evaluation rows + exchange rows; beyond 64 KB the module's functions need the attribute
        if (fg_task_lds(e->S, e->d, FG_MWI_MAX) > 160 * 1024) return FG_E_UNSUPPORTED;
        if (fg_task_lds(e->S, e->d, FG_MWI_MAX, 0, true) > 64 * 1024 && !e->jit_lds_attr) {      // (+ the second copy of the site rows of the one-barrier gradient)
            if (hipFuncSetAttribute((const void *)e->jit_fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess ||
                hipFuncSetAttribute((const void *)e->jit_fn_eps, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) { (void)hipGetLastError(); e->jit_state = -1; return FG_E_UNSUPPORTED; }
            e->jit_lds_attr = true;
        }
    }
    FgHmcSplitState &st = e->hsplit;
    if (!st.d_mwi_order) {
        HIPCHK(hipMalloc((void **)&st.d_mwi_order, (size_t)2 * n_tasks * sizeof(int)));      // (the second half: the split of the analytic mode)
        HIPCHK(hipMalloc((void **)&st.d_mwi_prof, (size_t)n_tasks * sizeof(long long)));
    }
    const FgSplitKey key = dense ? FG_SPLIT_JIT_DENSE : FG_SPLIT_JIT_SPARSE;      // (dense: every task is the whole program)
    if (st.key != key) {
        FgJitTaskPlan p = jit_task_plan(e, tiles, e->cfg.grad_mode, fg_task_switches(), true);
        HIPCHK(hipMemcpyAsync(st.d_mwi_order, p.split.order.data(), p.split.order.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));                // `p` is a local
        st.split = std::move(p.split); st.cost = std::move(p.cost); st.key = key;
    }
    return FG_OK;
}

// find_reasonable_epsilon through the compiled kernel (k_hmc_jit_find_eps)
int fg_hmc_jit_find_eps(fg_engine *e, uint32_t instance, int injected, double *d_eps_out) {
    const unsigned tiles = (unsigned)((e->C + e->tw - 1) / e->tw);
    // the choice of kernel must be the one fg_hmc_step will make: only programs the compiled form takes by default or by force
    if (int rc = jit_hmc_prepare(e, tiles)) return rc;
    const FgTaskSplit &sp = e->hsplit.split;
    const int W = sp.W;
    FgJitSeg seg;
    for (int w = 0; w <= FG_MWI_MAX; ++w) seg.off[w] = sp.off[w];
    seg.order = e->hsplit.d_mwi_order; seg.baked = 0;
    const size_t lds = (size_t)fg_task_lds(e->S, e->d, W);
    void *args[] = { &e->P, &e->X, &e->H, &seg, &instance, &injected, &d_eps_out };
    HIPCHK(hipModuleLaunchKernel(e->jit_fn_eps, tiles, 1, 1, FG_WAVE * W, 1, 1, (unsigned)lds, e->stream, args, nullptr));
    return FG_OK;
}

int fg_hmc_jit_launch(fg_engine *e, int iter0, int n, int welford_on, double *draws, int first_sample_t, double *pos_all, double *info) {
    const unsigned tiles = (unsigned)((e->C + e->tw - 1) / e->tw);
    if (int rc = jit_hmc_prepare(e, tiles)) return rc;
    const FgHmcSplitState &st = e->hsplit;
    const FgJitLaunchShape sh = fg_jit_launch_shape(st.split, e->cfg.grad_mode == FG_GRAD_FD_DENSE ? st.gen_dense : st.gen_sparse, e->cfg.grad_mode, e->jit_has_ad, e->S, e->d);
    FgJitSeg seg;
    for (int w = 0; w <= FG_MWI_MAX; ++w) seg.off[w] = sh.analytic_off ? st.split.off_an[w] : st.split.off[w];
    seg.order = st.d_mwi_order; seg.baked = sh.baked;
    int n_warmup = e->n_warmup;
    void *args[] = { &e->P, &e->X, &e->H, &seg, &iter0, &n, &n_warmup, &welford_on, &draws, &first_sample_t, &pos_all, &info };
    HIPCHK(hipModuleLaunchKernel(e->jit_fn, tiles, 1, 1, FG_WAVE * st.split.W, 1, 1, (unsigned)sh.lds, e->stream, args, nullptr));
    e->last_hmc_kernel = sh.name;
    return FG_OK;
}
