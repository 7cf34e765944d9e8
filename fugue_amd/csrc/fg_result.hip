// fg_result.hip -- the model's return value on the device.  The reference's drivers return `Vec<(A, Trace)>`: every draw carries the
// `A` its model closed with `pure(a)` (src/core/model.rs; hmc.rs:566-583, mh.rs:921-944, `Particle` in smc.rs).  The program keeps
// `A` as R named scalar expressions (fg_program_result, compiled by fg_program::compile_results); k_result_eval turns a chunk of
// draws [n][n_rows][C] into a chunk of results [n][R][C], so that a run summarised without stored draws (fg_diag_stream,
// fg_diag_qstream) can be summarised by a derived quantity and not only by site.
//
// One lane = one chain; a wave owns one 64-chain tile and a run of consecutive draws (fg_result_plan.h).  Per draw a lane loads the
// rows of the sites the results read into its column of the wave's [n_slots][64] slice (chain fastest: 64 consecutive 8-byte words
// per row), runs the result instruction list with a wave-uniform program counter -- instructions come through scalar loads from the
// constant address space, every branch on an opcode or operand kind is a scalar branch -- and stores the R values, chain fastest.
// Sites that are not among the draw's rows come from the engine's current values, once per wave, before the draws.
//
// The expression switch restates fg_exec's (fg_interp.h) over the same fg_operand, the same out-of-line transcendentals and the same
// GATHER / DOT forms, built with the same -ffp-contract=off: every opcode yields the interpreter's bits, and FG_OP_FACTOR -- the
// statement the same expression compiles to inside `factor(..)` -- hands the value over instead of adding it to log_factors.
// fg_exec itself is not touched (its register allocation in the sampler kernels stays what it was).
#include "fg_engine_internal.h"
#include "fg_result_plan.h"

struct FgResultDev {
    const FgIns *ins;        // res_ins, n_ins of them (two readable no-ops follow)
    const double *pool;      // res_pool: the terms of the fused linear predictors
    const int *site;         // [n_used] sorted site index of slot k
    const int *row;          // [n_used] row of the draw that holds it, or -1: the engine's current values
    int n_ins, n_slots, n_used, R;
};

template <bool GT>
__global__ __launch_bounds__(FG_WAVE * 4) void k_result_eval(FgResultDev Q, const long long *values, long long C, const long long *draws, long long n,
                                                             long long n_rows, long long tiles, long long draws_per_wave, long long items, double *gtile,
                                                             double *out) {
    extern __shared__ __attribute__((aligned(16))) double lds_res[];
    const int lane = (int)(threadIdx.x & (FG_WAVE - 1));
    const long long g = (long long)blockIdx.x * (blockDim.x / FG_WAVE) + (threadIdx.x / FG_WAVE);
    if (g >= items) return;                                 // (no barrier anywhere: the waves of a workgroup share nothing)
    long long tile, t0, t1;
    fg_result_item(g, tiles, draws_per_wave, n, &tile, &t0, &t1);
    constexpr int tw = FG_WAVE;
    double *slots = (GT ? gtile + (size_t)g * Q.n_slots * FG_WAVE : lds_res + (size_t)(threadIdx.x / FG_WAVE) * Q.n_slots * FG_WAVE) + lane;
    const long long c = tile * FG_WAVE + lane;
    const bool live = c < C;                               // a lane beyond C loads nothing and stores nothing
    slots[(Q.n_slots - 1) * tw] = 0.0;                     // the always-zero slot
    for (int k = 0; k < Q.n_used; ++k)
        if (Q.row[k] < 0 && live) slots[k * tw] = fg_as_double(values[(long long)Q.site[k] * C + c]);
    const FG_AS4 FgIns *prog = (const FG_AS4 FgIns *)(uintptr_t)Q.ins;
    const double *pool = Q.pool;
    for (long long t = t0; t < t1; ++t) {
        for (int k = 0; k < Q.n_used; ++k) {
            const int row = Q.row[k];
            if (row >= 0 && live) slots[k * tw] = fg_as_double(draws[fg_result_draw_index(t, n_rows, row, C, c)]);
        }
        double acc = 0.0;
        long long r = 0;
        for (int pc = 0; pc < Q.n_ins; ++pc) {
            const FG_AS4 FgIns *I = prog + pc;
            const uint32_t code = FG_INS_OPCODE(I->op);
            const double x0 = fg_operand(I->opnd[0], I->imm[0], slots, pool, tw);
            switch (code) {
            case FG_OP_FACTOR: if (live) out[fg_result_out_index(t, Q.R, r, C, c)] = x0; ++r; break;
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
            default: break;
            }
        }
    }
}

// the engine's device copies of the result program, made at the first call (an engine that never evaluates a result allocates nothing)
static int result_setup(fg_engine *e) {
    if (e->d_res_ins) return FG_OK;
    const fg_program *p = e->prog;
    int rc = dev_upload(&e->d_res_ins, p->res_ins);
    if (!rc) rc = dev_upload(&e->d_res_pool, p->res_pool);
    if (!rc) rc = dev_upload(&e->d_res_site, p->res_sites);
    if (!rc) rc = dev_alloc(&e->d_res_row, p->res_sites.size());
    e->res_row_host.assign(p->res_sites.size(), -2);      // (no mapping uploaded yet)
    return rc;
}

struct FgResultVariant { bool gt; void (*fn)(FgResultDev, const long long *, long long, const long long *, long long, long long, long long, long long, long long, double *, double *);
                         unsigned long long raised; };
static FgResultVariant g_result_variants[] = { { false, k_result_eval<false>, 0ull }, { true, k_result_eval<true>, 0ull } };

extern "C" int fg_result_eval(fg_engine *e, const void *d_draws, int n, const int32_t *h_rows, int n_rows, double *d_out) {
    NEED_ENGINE(e);
    const fg_program *p = e->prog;
    const int R = (int)p->results.size();
    if (R == 0) { fg_set_error("fg_result_eval: the program has no result (fg_program_result)"); return FG_E_STATE; }
    if (n < 0 || n_rows < 0) { fg_set_error("fg_result_eval: negative n or n_rows"); return FG_E_BAD_ARG; }
    if (!d_draws && !(n == 1 && n_rows == 0)) { fg_set_error("fg_result_eval: without draws n must be 1 and n_rows 0 (the engine's current values)"); return FG_E_BAD_ARG; }
    if (d_draws && !h_rows && n_rows != e->d) { fg_set_error("fg_result_eval: without h_rows the draws hold the d f64 sites: n_rows must be d"); return FG_E_BAD_ARG; }
    // row of every sorted site (-1: not recorded)
    std::vector<int> row_of((size_t)std::max(1, e->S), -1);
    for (int j = 0; d_draws && j < n_rows; ++j) {
        const int s = h_rows ? h_rows[j] : p->f64_slot[j];
        if (s < 0 || s >= e->S) { fg_set_error("fg_result_eval: row " + std::to_string(j) + " names site " + std::to_string(s) + " outside [0, S)"); return FG_E_BAD_ARG; }
        if (row_of[s] >= 0) { fg_set_error("fg_result_eval: site " + std::to_string(s) + " is given twice among the rows"); return FG_E_BAD_ARG; }
        row_of[s] = j;
    }
    if (n == 0) return FG_OK;
    if (!d_out) { fg_set_error("fg_result_eval: null d_out"); return FG_E_BAD_ARG; }
    int rc = result_setup(e);
    if (rc) return rc;
    std::vector<int> rows(p->res_sites.size());
    for (size_t k = 0; k < rows.size(); ++k) rows[k] = row_of[p->res_sites[k]];
    if (rows != e->res_row_host) {                         // the kernels in flight read the previous mapping: in stream order, and `rows` is a local
        if (!rows.empty()) HIPCHK(hipMemcpyAsync(e->d_res_row, rows.data(), rows.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
        HIPCHK(hipStreamSynchronize(e->stream));
        e->res_row_host = rows;
    }
    const char *fg_env = std::getenv("FG_RESULT_GLOBAL_TILE");
    FgResultPlan pl;
    rc = fg_result_plan(e->C, n, p->res_n_slots, p->res_n_ins, std::max(1, e->n_simd / 4), fg_env && std::atoi(fg_env) != 0, &pl);
    if (rc) { fg_set_error("fg_result_eval: no launch plan for this shape"); return rc; }
    if (pl.global_tile && pl.scratch_bytes > e->res_gtile_bytes) {
        HIPCHK(hipStreamSynchronize(e->stream));
        if (e->d_res_gtile) { HIPCHK(hipFree(e->d_res_gtile)); e->d_res_gtile = nullptr; e->res_gtile_bytes = 0; }
        HIPCHK(hipMalloc((void **)&e->d_res_gtile, pl.scratch_bytes));
        e->res_gtile_bytes = pl.scratch_bytes;
    }
    FgResultDev Q = { e->d_res_ins, e->d_res_pool, e->d_res_site, e->d_res_row, p->res_n_ins, p->res_n_slots, (int)p->res_sites.size(), R };
    FgResultVariant &v = g_result_variants[pl.global_tile ? 1 : 0];
    return fg_launch(e, v.fn, v.raised, dim3(pl.grid), dim3(FG_WAVE * pl.W), pl.lds, Q, (const long long *)e->d_values, e->C, (const long long *)d_draws, (long long)n,
                     (long long)n_rows, pl.tiles, pl.draws_per_wave, pl.items, e->d_res_gtile, d_out);
}
