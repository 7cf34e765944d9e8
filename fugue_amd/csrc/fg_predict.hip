// fg_predict.hip -- posterior (and prior) predictive draws on the device.  The reference's workflows end a run by sampling replicated
// data by hand: for every posterior draw, a value from the distribution of each `observe` site at that draw's parameters
// (tests/inference_integration.rs:717-740, tests/end_to_end_workflows.rs:650-700, examples/bayesian_coin_flip.rs:211-).  k_predict_eval
// runs the model's statement list with the latent sites pinned to a draw and the observe sites DRAWN instead of scored: a chunk of
// draws [n][n_rows][C] becomes a chunk of replicates [n][n_sel][C], and, if asked, the table of per-observation log-likelihoods
// (`Choice.logp` of the observe sites: what WAIC / LOO start from) that the scoring run only keeps the sum of.
//
// One lane = one chain; a wave owns one 64-chain tile and a run of consecutive draws (fg_predict_plan.h).  Per draw a lane loads the
// recorded rows into its column of the wave's [n_slots][64] slice (the program's own slot numbering: fg_ir.h), takes the stream
// (seed, chain, iter0 + t, FG_RNG_PREDICT) and walks the program's GENERAL instruction list -- the one FG_MODE_PRIOR runs -- with a
// wave-uniform program counter: instructions come through scalar loads from the constant address space, every branch on an opcode,
// a flag or an operand kind is a scalar branch; lanes part only inside the rejection samplers.  Sites that are not among the draw's
// rows come from the engine's current values, once per wave, before the draws (no statement of this walk writes a site slot).
//   expression opcodes: fg_exec's switch restated, as fg_result.hip restates it (same fg_operand, same out-of-line transcendentals,
//                       same GATHER / DOT forms, same -ffp-contract=off): the parameters are the bits a scoring run sees;
//   sample statements:  nothing is drawn, nothing is scored -- the value is the pinned one;
//   factor statements:  skipped;
//   observe statements: one draw through fg_sample_cold (Categorical: the cumulative walk of FG_MODE_PRIOR), consuming the lane's
//                       one stream in program order as PriorHandler consumes its stream (interpreters.rs:88-104); FG_F_INVALID is
//                       not looked at, as FG_MODE_PRIOR does not look at it for a sample statement (the samplers' own guards give
//                       NaN / 0); and the log-density of the OBSERVED value, the operations of fg_exec<FG_MODE_SCORE> for the
//                       statement in their order.
// Every observe statement is drawn whether its row is stored or not: a selection holds the bits of the full table.
// fg_exec itself is not touched (its register allocation in the sampler kernels stays what it was).
#include "fg_engine_internal.h"
#include "fg_predict_plan.h"

struct FgPredictDev {
    const FgIns *ins;        // the program's general list, n_ins of them (two readable no-ops follow)
    const double *pool;
    const int *site_slot;    // [S] slot of sorted site j
    const int *row;          // [S] row of the draw that holds site j, or -1: the engine's current values
    const int *sel_row;      // [O] row of the tables observe statement k is stored to, or -1
    int n_ins, n_slots, S, n_sel;
    unsigned long long seed; uint32_t chain0, iter0;
};

template <bool GT>
__global__ __launch_bounds__(FG_WAVE * 4, FG_MIN_WAVES) void k_predict_eval(FgPredictDev Q, const long long *values, long long C, const long long *draws, long long n,
                                                              long long n_rows, long long tiles, long long draws_per_wave, long long items, double *gtile,
                                                              long long *yrep, double *loglik) {
    extern __shared__ __attribute__((aligned(16))) double lds_pred[];
    const int lane = (int)(threadIdx.x & (FG_WAVE - 1));
    const long long g = (long long)blockIdx.x * (blockDim.x / FG_WAVE) + (threadIdx.x / FG_WAVE);
    if (g >= items) return;                                 // (no barrier anywhere: the waves of a workgroup share nothing)
    long long tile, t0, t1;
    fg_predict_item(g, tiles, draws_per_wave, n, &tile, &t0, &t1);
    constexpr int tw = FG_WAVE;
    double *slots = (GT ? gtile + (size_t)g * Q.n_slots * FG_WAVE : lds_pred + (size_t)(threadIdx.x / FG_WAVE) * Q.n_slots * FG_WAVE) + lane;
    const long long chain = tile * FG_WAVE + lane;
    const bool live = chain < C;                            // a lane beyond C repeats the last chain's work (bounded samplers on defined
    const long long c = live ? chain : C - 1;               // parameters) and stores nothing
    for (int k = 0; k < Q.n_slots; ++k) slots[k * tw] = 0.0;   // temporaries read before written do not exist; the always-zero slot is the last
    for (int j = 0; j < Q.S; ++j)
        if (Q.row[j] < 0) slots[Q.site_slot[j] * tw] = fg_as_double(values[(long long)j * C + c]);
    const FG_AS4 FgIns *prog = (const FG_AS4 FgIns *)(uintptr_t)Q.ins;
    const double *pool = Q.pool;
    const bool want_ll = loglik != nullptr, want_y = yrep != nullptr;
    for (long long t = t0; t < t1; ++t) {
        for (int j = 0; j < Q.S; ++j) {
            const int row = Q.row[j];
            if (row >= 0) slots[Q.site_slot[j] * tw] = fg_as_double(draws[fg_predict_draw_index(t, n_rows, row, C, c)]);
        }
        FgStream rng = fg_stream(Q.seed, Q.chain0 + (uint32_t)c, Q.iter0 + (uint32_t)t, FG_RNG_PREDICT);
        double acc = 0.0;
        int ko = 0;                                         // observe statements met so far (program order)
        for (int pc = 0; pc < Q.n_ins; ++pc) {
            const FG_AS4 FgIns *I = prog + pc;
            const uint32_t op = I->op;
            const uint32_t code = FG_INS_OPCODE(op);
            if (code < 17u) {
                if (!(op & FG_F_OBSERVE)) continue;         // a latent site: pinned
                const bool hoisted = (op & FG_F_HOISTED) != 0u;
                const uint32_t vtype = FG_INS_VTYPE(op);
                const uint32_t xw = I->opnd[0];
                long long cell;
                double lp = 0.0;
                if (code == 3u) {                           // Categorical: the cumulative walk of FG_MODE_PRIOR (fg_interp.h)
                    const uint32_t bw = I->opnd[1];
                    const int K = (int)I->opnd[2];
                    const bool in_pool = FG_OPND_KIND(bw) == FG_OPND_POOL;
                    const uint32_t base = FG_OPND_IDX(bw);  // a table in slots is a run of temporaries
                    const double u = fg_rng_u01(rng);
                    double cum = 0.0; int idx = K;
                    for (int i = 0; i < K; ++i) {
                        const double pi = in_pool ? pool[base + i] : slots[(base + i) * tw];
                        cum += pi;
                        if (idx == K && !(cum < u)) idx = i;
                    }
                    cell = idx < K - 1 ? idx : K - 1;
                    if (want_ll) {
                        long long xi;
                        if (FG_OPND_KIND(xw) == FG_OPND_SLOT_I) xi = fg_as_i64(slots[FG_OPND_IDX(xw) * tw]);
                        else xi = fg_obs_int_cold(fg_operand(xw, I->imm[0], slots, pool, tw), vtype);
                        if ((op & FG_F_INVALID) != 0u || xi < 0 || xi >= (long long)K) lp = FG_NEG_INF;
                        else if (in_pool) lp = pool[base + K + (int)xi];          // precomputed ln p (or -inf)
                        else { const double p = slots[(base + (int)xi) * tw]; lp = p > 0.0 ? log(p) : FG_NEG_INF; }
                    }
                } else {
                    const double p0 = fg_operand(I->opnd[1], I->imm[1], slots, pool, tw);
                    const double p1 = fg_operand(I->opnd[2], I->imm[2], slots, pool, tw);
                    const double p2 = fg_operand(I->opnd[3], I->imm[3], slots, pool, tw);
                    cell = fg_sample_cold(code, hoisted, p0, p1, p2, &rng);
                    if (want_ll) {
                        double xf = 0.0; long long xi = 0;
                        if (vtype == 0u) xf = fg_operand(xw, I->imm[0], slots, pool, tw);
                        else if (FG_OPND_KIND(xw) == FG_OPND_SLOT_I) xi = fg_as_i64(slots[FG_OPND_IDX(xw) * tw]);
                        else xi = fg_obs_int_cold(fg_operand(xw, I->imm[0], slots, pool, tw), vtype);
                        if ((op & FG_F_INVALID) != 0u) lp = FG_NEG_INF;
                        else if (code == 12u && hoisted) {   // Normal with constant parameters, as fg_exec has it inline
                            if (!fg_finite(xf)) lp = FG_NEG_INF;
                            else {
                                const double z = (op & FG_F_POW2SCALE) ? (xf - p0) * I->h[4] : (xf - p0) / p1;
                                lp = -0.5 * z * z - I->h[0] - 0.5 * FG_LN_2PI;
                            }
                        } else {
                            lp = fg_logpdf_cold(code, hoisted, (op & FG_F_POW2SCALE) != 0u, xf, xi, p0, p1, p2, I->h[0], I->h[1], I->h[2], I->h[3], I->h[4],
                                                (op & FG_F_SCALEHOIST) != 0u, (op & FG_F_XHOIST) != 0u);
                        }
                    }
                }
                const int r = Q.sel_row[ko];
                ++ko;
                if (r >= 0 && live) {
                    const long long o = fg_predict_out_index(t, Q.n_sel, r, C, c);
                    if (want_y) yrep[o] = cell;
                    if (want_ll) loglik[o] = lp;
                }
                continue;
            }
            const double x0 = fg_operand(I->opnd[0], I->imm[0], slots, pool, tw);
            switch (code) {
            case FG_OP_LOAD: acc = x0; break;
            case FG_OP_ADD: acc = acc + x0; break;
            case FG_OP_SUB: acc = acc - x0; break;
            case FG_OP_MUL: acc = acc * x0; break;
            case FG_OP_DIV: acc = acc / x0; break;
            case FG_OP_RSUB: acc = x0 - acc; break;
            case FG_OP_RDIV: acc = x0 / acc; break;
            case FG_OP_NEG: acc = -acc; break;
            case FG_OP_EXP: acc = fg_op_exp(acc); break;
            case FG_OP_LN: acc = fg_op_log(acc); break;
            case FG_OP_SQRT: acc = sqrt(acc); break;
            case FG_OP_ABS: acc = fabs(acc); break;
            case FG_OP_FLOOR: acc = floor(acc); break;
            case FG_OP_SIN: acc = fg_op_sin(acc); break;
            case FG_OP_COS: acc = fg_op_cos(acc); break;
            case FG_OP_TANH: acc = fg_op_tanh(acc); break;
            case FG_OP_POW: acc = fg_op_pow(acc, x0); break;
            case FG_OP_RPOW: acc = fg_op_pow(x0, acc); break;
            case FG_OP_MIN: acc = fmin(acc, x0); break;
            case FG_OP_MAX: acc = fmax(acc, x0); break;
            case FG_OP_CLAMP: acc = fg_clamp(acc, x0, fg_operand(I->opnd[1], I->imm[1], slots, pool, tw)); break;
            case FG_OP_MAC: { const double tm = x0 * fg_operand(I->opnd[1], I->imm[1], slots, pool, tw);
                              acc = acc + tm; break; }
            case FG_OP_STORE: slots[I->aux * tw] = acc; break;
            case FG_OP_GATHER: { const int k = (int)I->opnd[1];
                                 const bool ok = (acc >= 0.0) && (acc < (double)k) && (acc == floor(acc));
                                 const int j = ok ? (int)acc : 0;
                                 const double v = slots[(I->aux + j) * tw];         // the options are a run of temporaries
                                 acc = ok ? v : NAN; break; }
            case FG_OP_DOT: {                              // n MACs (slot x constant), terms fetched 4 at a time by scalar loads
                const int nt = (int)I->opnd[1];
                const FG_AS4 char *tb = (const FG_AS4 char *)(uintptr_t)(pool + I->aux);
                int q4 = 0;
                for (; q4 + 4 <= nt; q4 += 4) {
                    const fg_u32x16 q = *(const FG_AS4 fg_u32x16 *)(tb + 16 * q4);
                    const double v0 = slots[q[0] * tw], v1 = slots[q[4] * tw], v2 = slots[q[8] * tw], v3 = slots[q[12] * tw];
                    acc = acc + v0 * fg_dbl(q[2], q[3]);
                    acc = acc + v1 * fg_dbl(q[6], q[7]);
                    acc = acc + v2 * fg_dbl(q[10], q[11]);
                    acc = acc + v3 * fg_dbl(q[14], q[15]);
                }
                for (; q4 < nt; ++q4) {
                    const fg_u32x4 q = *(const FG_AS4 fg_u32x4 *)(tb + 16 * q4);
                    acc = acc + slots[q[0] * tw] * fg_dbl(q[2], q[3]);
                }
                break; }
            default: break;                                // FG_OP_FACTOR: a factor statement draws nothing and has no pointwise term
            }
        }
    }
}

// the engine's device copies of the two mappings, made at the first call (an engine that never predicts allocates nothing)
static int predict_setup(fg_engine *e) {
    if (e->d_pred_row) return FG_OK;
    int rc = dev_alloc(&e->d_pred_row, (size_t)e->S);
    if (!rc) rc = dev_alloc(&e->d_pred_sel, (size_t)e->prog->n_observes);
    e->pred_row_host.assign(1, -3);                        // (no mapping uploaded yet)
    e->pred_sel_host.assign(1, -3);
    return rc;
}

struct FgPredictVariant { bool gt; void (*fn)(FgPredictDev, const long long *, long long, const long long *, long long, long long, long long, long long, long long, double *,
                                              long long *, double *);
                          unsigned long long raised; };
static FgPredictVariant g_predict_variants[] = { { false, k_predict_eval<false>, 0ull }, { true, k_predict_eval<true>, 0ull } };

extern "C" int fg_predict_eval(fg_engine *e, const void *d_draws, int n, const int32_t *h_rows, int n_rows, uint32_t iter0, const int32_t *h_sel, int n_sel,
                               void *d_yrep, double *d_loglik) {
    NEED_ENGINE(e);
    const fg_program *p = e->prog;
    const int O = p->n_observes;
    if (O == 0) { fg_set_error("fg_predict_eval: the program has no observe statement"); return FG_E_STATE; }
    if (n < 0 || n_rows < 0) { fg_set_error("fg_predict_eval: negative n or n_rows"); return FG_E_BAD_ARG; }
    if (!d_draws && !(n == 1 && n_rows == 0)) { fg_set_error("fg_predict_eval: without draws n must be 1 and n_rows 0 (the engine's current values)"); return FG_E_BAD_ARG; }
    if (d_draws && !h_rows && n_rows != e->d) { fg_set_error("fg_predict_eval: without h_rows the draws hold the d f64 sites: n_rows must be d"); return FG_E_BAD_ARG; }
    std::vector<int> rows((size_t)std::max(1, e->S), -1);  // row of every sorted site (-1: not recorded)
    for (int j = 0; d_draws && j < n_rows; ++j) {
        const int s = h_rows ? h_rows[j] : p->f64_slot[j];
        if (s < 0 || s >= e->S) { fg_set_error("fg_predict_eval: row " + std::to_string(j) + " names site " + std::to_string(s) + " outside [0, S)"); return FG_E_BAD_ARG; }
        if (rows[s] >= 0) { fg_set_error("fg_predict_eval: site " + std::to_string(s) + " is given twice among the rows"); return FG_E_BAD_ARG; }
        rows[s] = j;
    }
    std::vector<int> sel((size_t)O, -1);                   // table row of every observe statement (-1: drawn, not stored)
    if (!h_sel) { n_sel = O; for (int k = 0; k < O; ++k) sel[k] = k; }
    else {
        if (n_sel < 1) { fg_set_error("fg_predict_eval: an empty selection"); return FG_E_BAD_ARG; }
        for (int r = 0; r < n_sel; ++r) {
            const int k = h_sel[r];
            if (k < 0 || k >= O) { fg_set_error("fg_predict_eval: selection " + std::to_string(r) + " names observe statement " + std::to_string(k) + " outside [0, O)"); return FG_E_BAD_ARG; }
            if (sel[k] >= 0) { fg_set_error("fg_predict_eval: observe statement " + std::to_string(k) + " is selected twice"); return FG_E_BAD_ARG; }
            sel[k] = r;
        }
    }
    if (!d_yrep && !d_loglik) { fg_set_error("fg_predict_eval: both outputs are null"); return FG_E_BAD_ARG; }
    if (n == 0) return FG_OK;
    int rc = predict_setup(e);
    if (rc) return rc;
    if (rows != e->pred_row_host || sel != e->pred_sel_host) {   // the kernels in flight read the previous mappings: in stream order, and the vectors are locals
        if (e->S > 0) HIPCHK(hipMemcpyAsync(e->d_pred_row, rows.data(), (size_t)e->S * sizeof(int), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipMemcpyAsync(e->d_pred_sel, sel.data(), (size_t)O * sizeof(int), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        e->pred_row_host = rows; e->pred_sel_host = sel;
    }
    const char *fg_env = std::getenv("FG_PREDICT_GLOBAL_TILE");
    FgPredictPlan pl;
    rc = fg_predict_plan(e->C, n, p->n_slots, std::max(1, p->n_ins), std::max(1, e->n_simd / 4), fg_env && std::atoi(fg_env) != 0, &pl);
    if (rc) { fg_set_error("fg_predict_eval: no launch plan for this shape"); return rc; }
    if (pl.global_tile && pl.scratch_bytes > e->pred_gtile_bytes) {
        HIPCHK(hipStreamSynchronize(e->stream));
        if (e->d_pred_gtile) { HIPCHK(hipFree(e->d_pred_gtile)); e->d_pred_gtile = nullptr; e->pred_gtile_bytes = 0; }
        HIPCHK(hipMalloc((void **)&e->d_pred_gtile, pl.scratch_bytes));
        e->pred_gtile_bytes = pl.scratch_bytes;
    }
    FgPredictDev Q = { e->d_ins, e->d_pool, e->d_site_slot, e->d_pred_row, e->d_pred_sel, p->n_ins, p->n_slots, e->S, n_sel, e->seed, e->chain0, iter0 };
    FgPredictVariant &v = g_predict_variants[pl.global_tile ? 1 : 0];
    return fg_launch(e, v.fn, v.raised, dim3(pl.grid), dim3(FG_WAVE * pl.W), pl.lds, Q, (const long long *)e->d_values, e->C, (const long long *)d_draws, (long long)n,
                     (long long)n_rows, pl.tiles, pl.draws_per_wave, pl.items, e->d_pred_gtile, (long long *)d_yrep, d_loglik);
}
