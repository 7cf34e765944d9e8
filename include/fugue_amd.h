/*
 * fugue_amd.h -- C ABI of the MI355X-native many-chain / many-particle engine for
 * Fugue's `src/inference` hot path (hmc_chain, adaptive_mcmc_chain, adaptive_smc).
 *
 * The reference (alexnodeland/fugue, crate fugue-ppl 0.2.0) has no FFI for this path:
 * the boundary today is Rust generics.  Each entry point below names the reference
 * interface it replaces (file:line under /root/reference); INTEGRATION.md shows the
 * `extern "C"` block and the `GpuBackend` shim a maintainer would add on the Rust side.
 *
 * Conventions
 *   - plain C types only; handles are opaque; every `int` return is 0 on success, a
 *     reference `ErrorCode` value (src/error.rs:40-59: 100-106, 301, 302, 500, 600) for
 *     model errors, or a negative FG_E_* for engine / HIP failures.  fg_last_error()
 *     returns a thread-local message.
 *   - `h_` pointers are host memory, `d_` pointers are device (HBM) memory of the
 *     engine's device.  All [a][b] arrays are row-major with the LAST index = chain
 *     (struct-of-arrays: [sites x chains], site-major so a wavefront's 64 lanes read 64
 *     consecutive chains).
 *   - trace cells are 8 bytes: f64 sites hold the double, bool/u64/usize/i64 sites hold
 *     an int64 (bool 0/1) -- the flattened `ChoiceValue` (src/runtime/trace.rs:32-43).
 *   - site order everywhere = lexicographic order of the address strings = the
 *     reference's `BTreeMap<Address, Choice>` order (src/core/address.rs:150-157);
 *     f64 coordinate order (HMC `q`) is that order restricted to f64 sites
 *     (src/inference/hmc.rs:238-248).
 *   - there is NO CPU fallback: every engine call fails with FG_E_NO_DEVICE when no
 *     gfx950 device is usable.
 */
#ifndef FUGUE_AMD_H
#define FUGUE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FG_ABI_VERSION 1

/* engine errors (negative); model errors reuse the reference ErrorCode numbers */
enum {
    FG_OK = 0,
    FG_E_NO_DEVICE = -1,      /* no usable HIP device / wrong arch */
    FG_E_HIP = -2,            /* a HIP runtime call failed */
    FG_E_BAD_ARG = -3,
    FG_E_NOT_FINALIZED = -4,
    FG_E_STATE = -5,          /* call order (e.g. hmc_step before hmc_init) */
    FG_E_UNSUPPORTED = -6,
    FG_E_LIMIT = -7           /* model exceeds an engine limit (LDS budget, K > 64, ...) */
};
enum {
    FG_ERR_INVALID_MEAN = 100, FG_ERR_INVALID_VARIANCE = 101, FG_ERR_INVALID_PROBABILITY = 102, FG_ERR_INVALID_SHAPE = 104, FG_ERR_INVALID_COUNT = 106,
    FG_ERR_ADDRESS_CONFLICT = 301, FG_ERR_UNEXPECTED_STRUCTURE = 302,
    FG_ERR_ADDRESS_NOT_FOUND = 500, FG_ERR_TYPE_MISMATCH = 600
};

/* the 17 distributions, in the order of the crate-root re-export (src/lib.rs:18-22) */
enum {
    FG_BERNOULLI = 0, FG_BETA, FG_BINOMIAL, FG_CATEGORICAL, FG_CAUCHY, FG_CHISQUARED,
    FG_DISCRETEUNIFORM, FG_EXPONENTIAL, FG_GAMMA, FG_INVERSEGAMMA, FG_LAPLACE, FG_LOGNORMAL,
    FG_NORMAL, FG_POISSON, FG_STUDENTT, FG_UNIFORM, FG_WEIBULL, FG_N_DISTS
};
/* ChoiceValue tags (src/runtime/trace.rs:32-43) */
enum { FG_F64 = 0, FG_BOOL = 1, FG_U64 = 2, FG_USIZE = 3, FG_I64 = 4 };

/* ------------------------------------------------------------------ site programs
 * Replaces: `Model<A>` + `Handler` + `run` (src/core/model.rs:20-131,
 * src/runtime/handler.rs:29-209).  A model is flattened ONCE into a fixed-structure
 * site program; parameters that depend on earlier sites are postfix expressions over
 * the DSL's operator set (crates/fugue-wasm/src/dsl.rs:92-102,569-582).            */
enum {
    FG_T_CONST = 0,  /* push imm */
    FG_T_SITE,       /* push value of sample site `a` (handle from fg_program_sample), as f64 */
    FG_T_DATA,       /* push data[a][b] */
    FG_T_NEG, FG_T_EXP, FG_T_LN, FG_T_SQRT, FG_T_ABS, FG_T_FLOOR, FG_T_SIN, FG_T_COS, FG_T_TANH,
    FG_T_ADD, FG_T_SUB, FG_T_MUL, FG_T_DIV, FG_T_POW, FG_T_MIN, FG_T_MAX,
    FG_T_CLAMP,      /* x lo hi -> f64::clamp */
    FG_T_SELECT      /* idx opt0 .. opt{a-1} -> opt[idx]  (a = number of options) */
};
typedef struct fg_tok { int32_t op; int32_t a; int32_t b; int32_t reserved; double imm; } fg_tok;

typedef struct fg_program fg_program;

fg_program *fg_program_new(void);
void        fg_program_free(fg_program *p);
/* named data arrays (DSL `{"y":[...]}`, dsl.rs:1066-1106); returns the array id >= 0 */
int fg_program_data(fg_program *p, const char *name, const double *h_values, int64_t n);
/* `sample(addr, dist)` (src/core/model.rs:144-266).  `toks` holds the parameter
 * expressions back to back, `param_len[i]` tokens each (Categorical: one per
 * probability, 1..64).  Returns the site handle >= 0 (program order), or an error. */
int fg_program_sample(fg_program *p, const char *addr_utf8, int dist, const fg_tok *toks,
                      const int32_t *param_len, int n_params);
/* `observe(addr, dist, value)` (model.rs:381-424) */
int fg_program_observe(fg_program *p, const char *addr_utf8, int dist, const fg_tok *toks,
                       const int32_t *param_len, int n_params, const fg_tok *value, int n_value);
/* `sample(addr, DiscreteUniform::new(lo, hi))` with exact i64 bounds (src/core/distribution.rs:1842-1853 takes i64;
 * the token form above carries them as f64, exact only up to 2^53). */
int fg_program_sample_discrete_uniform(fg_program *p, const char *addr_utf8, int64_t lo, int64_t hi);
/* `factor(logw)` (model.rs:426-431) */
int fg_program_factor(fg_program *p, const fg_tok *toks, int n);
/* sorts sites by address, rejects duplicate addresses (AddressConflict = 301, the panic of
 * src/runtime/interpreters.rs:23-33), compiles the device program. */
int fg_program_finalize(fg_program *p);
int fg_program_n_sites(const fg_program *p);      /* S */
int fg_program_n_f64(const fg_program *p);        /* d */
int fg_program_n_observe(const fg_program *p);    /* O */
int fg_program_n_instructions(const fg_program *p);
int fg_program_n_slots(const fg_program *p);      /* S + expression temporaries */
/* coordinate order == reference BTreeMap order; returns bytes needed incl. NUL */
int fg_program_site_name(const fg_program *p, int sorted_idx, char *buf, int buf_len);
int fg_program_site_vtype(const fg_program *p, int sorted_idx);
int fg_program_site_of_handle(const fg_program *p, int handle);
/* observe statement k in PROGRAM order, 0 <= k < O (the order `run` meets them, handler.rs:124-209; the row order of fg_predict_eval):
 * its address like fg_program_site_name, the value type of its distribution (FG_F64 .. FG_I64), the distribution kind */
int fg_program_observe_name(const fg_program *p, int k, char *buf, int buf_len);
int fg_program_observe_vtype(const fg_program *p, int k);
int fg_program_observe_dist(const fg_program *p, int k);
/* the observed value of observe statement k (program order) where the model states it: returns 1 and *out = the value as the double
 * `x as f64` when it reads no site (a literal or a data element: the `observations` slice of the reference's workflows,
 * tests/end_to_end_workflows.rs:650-745), 0 when it reads a site (its value moves with the draw; *out is left alone).  A discrete
 * statement gives the value AS OBSERVED: the integer its expression converts to (dsl.rs:71-84,985-998: 2.5 -> 0, -2 -> 0 for a count,
 * any non-zero -> 1 for a Bernoulli), which is what replicated cells compare with.  FG_E_BAD_ARG:
 * k outside [0, O), a null argument. */
int fg_program_observe_value(const fg_program *p, int k, double *out);
int fg_program_f64_site(const fg_program *p, int k);
/* number of instructions re-evaluated when f64 coordinate k is perturbed (sparse FD) */
int fg_program_dep_count(const fg_program *p, int k);
/* record streams the compiler could build for the stream kernels (0 = the interpreter kernels are used):
 * which = 0: records of the fused finite-difference gradient stream; 1: records of the score stream;
 * 2: record kinds present (0 fast Normals only, 1 + linear predictors, 2 + general distribution records);
 * 3: records of the register-resident trajectory kernel (> 0 only for independent-sites programs: every force term reads
 *    one coordinate and constants) */
int fg_program_stream_records(const fg_program *p, int which);
/* The model's return value: the `A` of `Model<A>` that `pure(a)` closes a model with (src/core/model.rs:20-131, `pure`) and that
 * every driver hands back next to the trace, `Vec<(A, Trace)>` (src/inference/hmc.rs:566-583).  A result is one named postfix
 * expression over the token set of a parameter expression (FG_T_CONST .. FG_T_SELECT); it is compiled like the expression of a
 * `factor(..)` statement (same constant folding, same fused linear predictors) into an instruction list of its own and changes
 * nothing of the program's statements.  Before fg_program_finalize; returns the result index r >= 0 (registration order).
 * FG_E_STATE after finalize; FG_E_BAD_ARG for a malformed token stream, an unknown site handle, an empty or a duplicate name. */
int fg_program_result(fg_program *p, const char *name_utf8, const fg_tok *toks, int n);
int fg_program_n_results(const fg_program *p);    /* R: the scalar components of `A` (model.rs `pure`) */
/* name of result r (model.rs `pure`), like fg_program_site_name: returns bytes needed incl. NUL */
int fg_program_result_name(const fg_program *p, int r, char *buf, int buf_len);
/* after finalize: the sorted site indices some result reads (model.rs `pure`: the sampled values `A` is computed from), ascending;
 * writes the first min(count, cap) of them and returns the count */
int fg_program_result_sites(const fg_program *p, int32_t *h_sites, int cap);

const char *fg_last_error(void);
int         fg_abi_version(void);

/* Model-language front-end: the `prob!` subset of the reference's playground
 * (crates/fugue-wasm/src/dsl.rs:10-35 grammar, :1062-1120 CompiledModel::compile).  `data_json` is a JSON
 * object of number/boolean arrays, a bare array (bound to `data`), "null" or NULL.  Returns a FINALIZED
 * program, or NULL with the reference-worded message ("line N: expected .., found ..") in
 * fg_last_error().  Warnings (out-of-bounds data index -> NaN, dsl.rs:715-722) are kept on the program. */
fg_program *fg_dsl_compile(const char *source_utf8, const char *data_json_utf8);
int         fg_dsl_warning_count(const fg_program *p);
const char *fg_dsl_warning(const fg_program *p, int i);

/* ------------------------------------------------------------------ engine
 * One engine = one batch of `n_chains` independent chains (or particles) of one program
 * on one GPU, with its own HIP stream.  Chain c uses the counter-based RNG stream
 * (seed, chain_offset + c): results do not depend on how chains are sharded over GPUs. */
typedef struct fg_engine fg_engine;

fg_engine *fg_engine_new(const fg_program *p, int64_t n_chains, uint64_t seed,
                         uint32_t chain_offset, int device_ordinal);
void  fg_engine_free(fg_engine *e);
int   fg_engine_synchronize(fg_engine *e);
void *fg_engine_stream(fg_engine *e);                       /* hipStream_t */
/* run on a caller-owned hipStream_t (e.g. PyTorch's current stream) instead of the engine's own */
int   fg_engine_set_stream(fg_engine *e, void *hip_stream);
int64_t fg_engine_n_chains(const fg_engine *e);
/* current trace values, cells [S][C]; set_values re-scores the cached log-joint of a live HMC / MH session at the new values */
int fg_engine_set_values(fg_engine *e, const void *h_cells);
int fg_engine_get_values(fg_engine *e, void *h_cells);
void *fg_engine_values_device(fg_engine *e);                 /* d_cells [S][C] */

/* `run(PriorHandler, model)` per chain (src/runtime/interpreters.rs:88-104): draws every
 * site from its prior, scores it; h_acc (optional) gets [3][C] = log_prior,
 * log_likelihood, log_factors.  `iteration` selects the RNG sub-stream. */
int fg_prior_init(fg_engine *e, uint32_t iteration, double *h_acc);
/* `run(ScoreGivenTrace, model)` per chain (interpreters.rs:138-163) on the engine's current
 * values; h_acc [3][C]; h_logp (optional) [S][C] fresh per-site log-densities. */
int fg_log_joint(fg_engine *e, double *h_acc, double *h_logp);
/* The same scoring run evaluated over the SCORE STREAM (one 64-byte record per statement in program order) -- the
 * evaluator of the HMC endpoint score_full (src/inference/hmc.rs:283-299), of single_site_mh_step's model run
 * (src/inference/mh.rs:698-744) and of SMC rejuvenation (src/inference/smc.rs:662-675) for programs whose statements
 * all have a record form.  h_acc [3][C]; h_rec_lp (optional) [n_records][C], n_records =
 * fg_program_stream_records(p, 1): the log-density of every statement.  FG_E_UNSUPPORTED when the program has no
 * score stream. */
int fg_log_joint_stream(fg_engine *e, double *h_acc, double *h_rec_lp);
/* The same scoring run through the program's unit compiled at run time (k_log_joint_jit: what a sampler session re-scores its state
 * with after fg_engine_set_values), built here if it does not exist yet.  h_acc [3][C].  No fall-back: FG_E_UNSUPPORTED when the
 * program has no compiled unit (FG_JIT=0, no run-time compiler, no f64 site, the global-tile instantiations). */
int fg_log_joint_compiled(fg_engine *e, double *h_acc);
/* The model's return value `A` for every draw and chain -- the first half of each `(A, Trace)` pair hmc_chain / adaptive_mcmc_chain
 * return (src/inference/hmc.rs:566-583, mh.rs:921-944) and the value a Particle's trace gives (smc.rs) -- evaluated on the device:
 * d_draws [n][n_rows][C] 8-byte cells -> d_out [n][R][C] doubles, R = fg_program_n_results.  Row j of a draw holds sorted site
 * h_rows[j]; h_rows == NULL is the HMC draw layout (n_rows must be d: the f64 sites in coordinate order, as fg_hmc_step records them).
 * A site that a result reads and that is not among the rows is read from the engine's current values [S][C] (HMC moves only the f64
 * sites).  d_draws == NULL with n == 1 and n_rows == 0 evaluates at the current values alone (particles; HmcSession::result,
 * hmc.rs:761).  Integer sites enter as f64 like FG_T_SITE.  Asynchronous on the engine's stream; n == 0 is FG_OK without a launch.
 * FG_E_STATE: the program has no result; FG_E_BAD_ARG: a row index outside [0, S) or given twice, n_rows != d without h_rows. */
int fg_result_eval(fg_engine *e, const void *d_draws, int n, const int32_t *h_rows, int n_rows, double *d_out);
/* Posterior (or prior) predictive draws: for every draw and chain, replicated data sampled from the distributions of the observe
 * statements with the latent sites pinned to the draw -- what the reference's workflows do by hand after a run
 * (tests/inference_integration.rs:717-740, tests/end_to_end_workflows.rs:650-700) -- and, if asked, the log-likelihood of the OBSERVED
 * value per statement (`Choice.logp` of an observe site), the table WAIC / LOO start from.  d_draws, n, h_rows, n_rows as in
 * fg_result_eval (h_rows == NULL: the HMC draw layout; d_draws == NULL with n == 1 and n_rows == 0: the engine's current values --
 * after fg_prior_init the prior predictive, after fg_smc_run one replicate per particle).  Draw t of chain c draws from the stream
 * (seed, chain_offset + c, iter0 + t, purpose 9), consumed by the observe statements in program order; every observe statement is
 * drawn whether selected or not, so a selection holds the bits of the full table.  h_sel: the n_sel observe statements (program-order
 * indices) to store, NULL: all O of them (n_sel is ignored).  d_yrep [n][n_sel][C] 8-byte cells (f64, or i64 for discrete
 * distributions, as site cells are); d_loglik [n][n_sel][C] doubles: the term the scoring run adds to log_likelihood for that
 * statement.  Either may be NULL, not both.  Asynchronous on the engine's stream; n == 0 is FG_OK without a launch.  Reads engine
 * state and changes none (no sampler's stream moves).  FG_E_STATE: the program has no observe statement; FG_E_BAD_ARG: a bad row, a
 * selection index outside [0, O) or given twice, both outputs NULL. */
int fg_predict_eval(fg_engine *e, const void *d_draws, int n, const int32_t *h_rows, int n_rows, uint32_t iter0,
                    const int32_t *h_sel, int n_sel, void *d_yrep, double *d_loglik);

/* ------------------------------------------------------------------ approximate Bayesian computation
 * The device pieces of src/inference/abc.rs.  A simulator's output for a batch of B attempts is an f64 table [K][B] (attempt-fastest):
 * the selected observe statements drawn by fg_predict_eval at the current values (cells converted by fg_diag_cells_f64), or named
 * results evaluated by fg_result_eval. */
enum { FG_ABC_EUCLIDEAN = 0,      /* EuclideanDistance, abc.rs:132-145 */
       FG_ABC_MANHATTAN = 1,      /* ManhattanDistance, abc.rs:168-180 */
       FG_ABC_SUMMARY_STATS = 2   /* SummaryStatsDistance, abc.rs:183-226 */ };
/* DistanceFunction::distance (abc.rs:132-145, 168-180, 183-226) of every attempt's column of d_sim [K][B] against h_observed
 * [n_observed]: d_dist [B].  IEEE operations in the reference's order: bit-identical to a sequential evaluation.  Euclidean: the
 * in-order sum of (o - s)(o - s), then sqrt; Manhattan: the in-order sum of |o - s|; both +inf for every attempt when K != n_observed.
 * SummaryStats: sqrt(sum_i w_i (o_i - s_i)^2) over zip(stats, weights), stats = mean (in-order sum / K), population standard
 * deviation (a second in-order pass), median (exact selection, the even-K average included); fewer than three weights give fewer
 * terms, more than three are ignored; the observed vector's statistics are computed once on the host by the same arithmetic.  A
 * NaN among an attempt's simulated values gives a NaN distance, which no tolerance accepts (the reference panics in
 * `partial_cmp().unwrap()`, abc.rs:202); a NaN in the observed vector is FG_E_BAD_ARG for SummaryStats.  h_weights is read for
 * FG_ABC_SUMMARY_STATS only.  Asynchronous on the engine's stream for SummaryStats, synchronous otherwise; B == 0 is FG_OK without a
 * launch.  Reads no engine state and changes none. */
int fg_abc_distance(fg_engine *e, const double *d_sim, int K, int64_t B, const double *h_observed, int n_observed, int kind,
                    const double *h_weights, int n_weights, double *d_dist);
/* kernel_mixture_log_density (abc.rs:776-799) for m proposals at once, the denominator of the importance weight of weighted ABC-SMC
 * (abc.rs:612-616): d_out[i] = log sum_j h_weights[j] prod_c N(d_x[c][i]; d_centers[c][j], max(h_std[c], 1e-12)).  d_x [d][m],
 * d_centers [d][n], h_weights [n], h_std [d], d_out [m].  The per-center constant ln w_j - sum_c ln s_c - d ln(2 pi)/2 is hoisted and
 * the coordinates are pre-scaled by 1/s_c, so this is NOT the reference's rounding: it agrees to about 1e-12 relative.  w_j = 0
 * contributes nothing; when every term is -inf the result is -inf; d = 0 gives log sum_j w_j; a NaN coordinate gives NaN.  Any d.
 * Synchronous.  FG_E_BAD_ARG: m < 0, n < 1, d < 0.  Reads no engine state and changes none. */
int fg_abc_mixture(fg_engine *e, const double *d_x, int64_t m, const double *d_centers, int64_t n, int d, const double *h_weights,
                   const double *h_std, double *d_out);
/* An ABC run over the model's own simulator.  The reference loops one attempt at a time (abc_rejection, abc.rs:283-325; the stages
 * of abc_smc_weighted, abc.rs:520-650) and stops right after the n-th accept or at its attempt budget; the handle runs rounds of
 * B = the engine's n_chains attempts and gives the result the sequential loop would give, whatever B is: attempt a (from 0 within a
 * stage) uses the chain word chain_offset + a and the iteration word t = the stage (0: the prior stage), the accepted set is the
 * first n accepted attempts in order of a, attempts beyond the budget are masked.  Streams of attempt a: stage 0 draws the trace
 * as fg_prior_init does (purpose 1); stage t >= 1 draws its proposal from purpose 10 (one Uniform(0,1) for the base particle, then
 * one Normal(0,1) per f64 site in address order); every stage simulates as fg_predict_eval does (purpose 9, iter0 = t).  The engine's
 * values [S][B] are the rounds' workspace; with a live HMC / MH / SMC session on the engine they are saved and put back, and no
 * sampler's stream moves.
 * fg_abc_new binds an engine, the simulator (FG_ABC_SIM_OBSERVE: h_sel = n_sel observe statements, program-order indices, strictly
 * increasing, NULL = all of them; FG_ABC_SIM_RESULT: h_sel = n_sel result indices, NULL = all of them), the observed vector, the
 * distance (as fg_abc_distance) and the capacity n of a population.  FG_E_BAD_ARG: a bad selection or kind, capacity < 1, a NaN in
 * the observed vector of SummaryStats; FG_E_STATE: the program has no observe statement / no result.  The handle must be freed before
 * its engine. */
enum { FG_ABC_SIM_OBSERVE = 0, FG_ABC_SIM_RESULT = 1 };
typedef struct fg_abc fg_abc;
int  fg_abc_new(fg_engine *e, int sim_kind, const int32_t *h_sel, int n_sel, const double *h_observed, int n_observed, int kind,
                const double *h_weights, int n_weights, int64_t capacity, fg_abc **out);     /* abc.rs:283-291, 520-528 */
void fg_abc_free(fg_abc *a);                                                                  /* abc.rs:283-325 */
/* The prior stage (abc.rs:295-316, 534-547): rounds of prior draws until n are accepted (dist <= tol) or `budget` attempts are made;
 * the accepted particles (site cells, distance, attempt index, log-prior) become the current population with weights 1 / accepted
 * (abc.rs:555-558).  *accepted <= n; *attempts = index of the n-th accepted attempt + 1, or the budget.  At most ceil(budget / B)
 * rounds.  FG_E_BAD_ARG: budget < 0 or budget > 2^32 - chain_offset. */
int fg_abc_round_prior(fg_abc *a, double tol, int64_t budget, int64_t *accepted, int64_t *attempts);
/* Opens a stage on the current population (abc.rs:570-580): downloads its f64 coordinates and weights once, computes
 * kernel_bandwidths (abc.rs:751-773), the weight total and the in-order cumulative weights on the host in the reference's order and
 * uploads them; empties the stage's accepted set.  FG_E_STATE: no population, or a weight total <= 0. */
int fg_abc_stage_begin(fg_abc *a);
/* The attempts of stage `stage` >= 1 (abc.rs:582-621): base particle by sample_index (abc.rs:816-830: u total <= cum[i], first such i,
 * else the last), its cells copied, every f64 site moved by bandwidth x Normal(0,1), discrete sites unchanged; the scoring run at the
 * proposal (log_prior = its first accumulator); simulate; distance; accepted when isfinite(log_prior) && dist <= tol.  Outputs as
 * fg_abc_round_prior, for the stage's accepted set.  FG_E_STATE without fg_abc_stage_begin. */
int fg_abc_round_stage(fg_abc *a, uint32_t stage, double tol, int64_t budget, int64_t *accepted, int64_t *attempts);
/* Closes the stage (abc.rs:612-616, 632-643): log_denom of the accepted particles against the previous population (fg_abc_mixture),
 * log_w = log_prior - log_denom normalised by log_sum_exp (1 / n each when the normaliser is not finite), and the accepted set
 * becomes the current population.  FG_E_STATE: no open stage or nothing accepted. */
int fg_abc_stage_end(fg_abc *a);
/* What the last round of attempts decided, [B] each (any may be NULL): the base particle (-1 in the prior stage), the distance, the
 * log-prior, the accept flag (0 for attempts beyond the budget); abc.rs:586-610. */
int fg_abc_last_round(fg_abc *a, int64_t *h_index, double *h_dist, double *h_log_prior, int32_t *h_accept);
/* A population (ABCParticle, abc.rs:457-463, with the engine's bookkeeping): which = 0 the current one, 1 the open stage's accepted
 * set.  *out_n particles; h_cells [S][*out_n], the others [*out_n]; any output may be NULL (call once with all NULL for the size). */
int fg_abc_get_population(fg_abc *a, int which, int64_t *out_n, void *h_cells, double *h_weights, double *h_dist,
                          int64_t *h_attempt, double *h_log_prior, double *h_log_denom);
/* Replaces the current population (abc.rs:457-463): 1 <= n <= capacity; h_cells [S][n] and h_weights [n] are required, the others
 * may be NULL (zeros).  Closes an open stage without a result. */
int fg_abc_set_population(fg_abc *a, int64_t n, const void *h_cells, const double *h_weights, const double *h_dist,
                          const int64_t *h_attempt, const double *h_log_prior, const double *h_log_denom);

/* ------------------------------------------------------------------ HMC
 * Replaces hmc_chain / HmcSession (src/inference/hmc.rs:566-583, 643-920). */
enum { FG_GRAD_FD_DENSE = 0,   /* hmc.rs:304-329 verbatim: 2d full model runs per gradient */
       FG_GRAD_FD_SPARSE = 1,  /* same central difference, re-evaluating only the terms that
                                  depend on the perturbed coordinate */
       FG_GRAD_ANALYTIC = 2    /* the derivative itself.  Programs whose force terms are all Normals with constant
                                  sigma whose mean is a site, a constant or a linear predictor: the closed form
                                  d/dq_i sum of -(x - mu)^2 / (2 sigma^2).  Every other program: the forward-mode
                                  derivative of each coordinate's sub-program in the unit compiled at run time
                                  (all 17 log-densities in value and parameters).  NOT the reference's arithmetic
                                  (it has no analytic mode): agrees with the finite difference to its O(h^2) +
                                  rounding error; the step-size search still uses FG_GRAD_FD_SPARSE.  fg_hmc_init
                                  returns FG_E_UNSUPPORTED where neither applies (no run-time compiler, FG_JIT=0). */ };
typedef struct fg_hmc_config {      /* HMCConfig, hmc.rs:106-135 (same defaults) */
    int32_t n_leapfrog;             /* 16 */
    double  target_accept;          /* 0.8 */
    double  init_step_size;         /* NaN = None: Hoffman-Gelman Alg. 4 (hmc.rs:479-535) */
    double  finite_diff_eps;        /* 1e-5 */
    int32_t adapt_mass;             /* 0 */
    int32_t grad_mode;              /* FG_GRAD_* (engine extension): default FG_GRAD_FD_SPARSE; FG_GRAD_FD_DENSE = the reference verbatim */
} fg_hmc_config;
typedef struct fg_hmc_stats {
    double  accept_rate;            /* mean acceptance probability over chains x transitions */
    double  mean_step_size;         /* mean over chains of the step size in use */
    int64_t n_divergent;
    int64_t n_transitions;          /* chains x transitions executed so far */
} fg_hmc_stats;
void fg_hmc_config_default(fg_hmc_config *cfg);
/* HmcSession::new (hmc.rs:667-729): prior draw, positions, initial step size */
int fg_hmc_init(fg_engine *e, const fg_hmc_config *cfg, int n_warmup);
/* HmcSession::step x n (hmc.rs:819-919).  Post-warmup positions are appended to
 * d_draws [n][d][C] when non-NULL (rows of warmup transitions are left untouched). */
int fg_hmc_step(fg_engine *e, int n_transitions, double *d_draws);
/* HmcSession::step x n returning every transition's HmcStepInfo (hmc.rs:587-602,803-805):
 * d_positions [n][d][C] = position after each transition (warmup included), d_info [n][4][C] =
 * accepted (0/1), divergent (0/1), accept_prob, step_size.  Either may be NULL. */
int fg_hmc_step_info(fg_engine *e, int n_transitions, double *d_positions, double *d_info);
/* hmc_chain (hmc.rs:566-583): init + n_warmup + n_samples; d_draws [n_samples][d][C] */
int fg_hmc_run(fg_engine *e, const fg_hmc_config *cfg, int n_samples, int n_warmup,
               double *d_draws, fg_hmc_stats *h_stats);
int fg_hmc_get_stats(fg_engine *e, fg_hmc_stats *h_stats);
int fg_hmc_get_step_sizes(fg_engine *e, double *h_eps /*[C]*/);
int fg_hmc_get_log_joint(fg_engine *e, double *h_lj /*[C]*/);
/* current diagonal inverse mass (HmcSession::m_inv, hmc.rs:652): h_m_inv [d][C] (all 1 without adapt_mass) */
int fg_hmc_get_mass(fg_engine *e, double *h_m_inv);
/* set_step_size (hmc.rs:741-747) for every chain */
int fg_hmc_set_step_size(fg_engine *e, double eps);
/* HmcSession::set_n_leapfrog / is_warming_up / iterations (hmc.rs:751-753, 780-782, 785-787) */
int     fg_hmc_set_n_leapfrog(fg_engine *e, int n_leapfrog);
int     fg_hmc_is_warming_up(const fg_engine *e);
int64_t fg_hmc_iterations(const fg_engine *e);
/* 1 when the host proved, for this session's finite_diff_eps, that the quotient by 2h of the sparse register-resident
 * trajectories (k_hmc_sep_steps' folded loop) is exact in two instructions; 0 when the divisor was refused -- the kernels then
 * run without the folded loop -- or no HMC session is initialised.  Results are the same bits either way. */
int     fg_hmc_short_quotient(const fg_engine *e);
/* 1 when the host proved, for this session's program and finite_diff_eps, that no finite non-zero numerator of that quotient can
 * leave the window in which the two instructions are exact (fg_sep_range.h): the folded loop then runs without its range test;
 * 0 when the bound was refused -- the test stays -- or no HMC session is initialised.  Results are the same bits either way. */
int     fg_hmc_range_proved(const fg_engine *e);
/* Which kernel the engine's last fg_hmc_step / fg_hmc_run launch ran, with its waves per 64-chain tile, e.g.
 * "k_hmc_sep_steps W=8" (independent sites: whole trajectories in registers), "k_hmc_lin_steps W=8" (dense regressions:
 * observation-major gradient), "k_hmc_stream_steps W=4" (gradient / score streams), "k_hmc_steps W=1" (interpreter);
 * "" before the first launch.  The pointer is valid until the engine's next launch. */
const char *fg_hmc_last_kernel(const fg_engine *e);
/* The same for fg_mh_step / fg_mh_run: "k_mh_mw_steps W=4" (score-stream programs of plain Normal records), "k_mh_mw_jit_steps W=4 ..."
 * (the same pipelined kernel around statements compiled at run time: score-stream programs with general records, programs without a
 * record stream), "k_mh_jit_steps W=4 (compiled at run time)" (programs whose term rows do not fit LDS), "k_mh_interp_mw_steps W=2",
 * "k_mh_steps W=1".  Compilation at run time uses hiprtc or hipcc when present (FG_JIT=0 keeps every program on the hand-written and
 * interpreter kernels). */
const char *fg_mh_last_kernel(const fg_engine *e);
/* HmcSession::step_recorded (hmc.rs:811-817) for every chain: ONE transition, and for the n_recorded chains h_chain_ids
 * the leapfrog trajectory with the Hamiltonian at each integration point (LeapfrogPoint, hmc.rs:338-343):
 * h_traj [n_recorded][L+1][d] positions, h_ham [n_recorded][L+1], h_n_points [n_recorded] (L + 1, fewer when the
 * trajectory left the support: recording stops at the last finite point).  d_info (optional) [4][C] as fg_hmc_step_info.
 * Recording consumes no randomness: the chains advance exactly as under fg_hmc_step (hmc.rs:1058-1087). */
int fg_hmc_step_recorded(fg_engine *e, int n_recorded, const int64_t *h_chain_ids, double *h_traj, double *h_ham,
                         int32_t *h_n_points, double *d_info);
/* test / diagnostics hooks under injected randomness -------------------------------- */
/* grad_log_joint (hmc.rs:304-329) at the engine's current values; h_grad [d][C], h_ok [C] */
int fg_hmc_grad(fg_engine *e, double h, int grad_mode, double *h_grad, int32_t *h_ok);
/* hmc_transition (hmc.rs:419-473) with momentum h_p0 [d][C] and uniform h_u [C] injected
 * and one step size for all chains; outputs are host arrays [C] (any may be NULL).
 * The engine's values / log-joint advance exactly as a real transition would. */
int fg_hmc_transition_injected(fg_engine *e, const fg_hmc_config *cfg, double eps,
                               const double *h_p0, const double *h_u, int32_t *h_accepted,
                               double *h_alpha, int32_t *h_divergent, double *h_lj);
/* find_reasonable_epsilon (hmc.rs:479-535) with momentum injected; h_eps [C] */
int fg_hmc_find_eps_injected(fg_engine *e, const fg_hmc_config *cfg, const double *h_p0,
                             double *h_eps);

/* ------------------------------------------------------------------ adaptive single-site MH
 * Replaces adaptive_mcmc_chain[_with_overrides] (src/inference/mh.rs:921-1014). */
enum { FG_PROP_AUTO = 0,      /* support-based choice: Gaussian, or LogSpace for positive support (mh.rs:339-358) */
       FG_PROP_GAUSSIAN = 1, FG_PROP_LOGSPACE = 2, FG_PROP_REFLECT = 3, FG_PROP_PRIOR_RESAMPLE = 4 };
typedef struct fg_site_proposal {   /* SiteProposal, mh.rs:145-161 */
    int32_t kind; double lower, upper;
} fg_site_proposal;
typedef struct fg_mh_stats { double accept_rate; int64_t n_steps; } fg_mh_stats;
/* prior init + DiminishingAdaptation::new(0.44, 0.7) per chain (mh.rs:945-965).
 * overrides: [S] in site order (HashMap<Address, SiteProposal> flattened) or NULL. */
int fg_mh_init(fg_engine *e, int n_warmup, const fg_site_proposal *h_overrides);
/* n x single_site_mh_step (mh.rs:698-744); adapts while iteration < n_warmup.  After every
 * sampling-phase step the current values of h_rec_sites[0..n_rec) are appended to
 * d_draws [n_sampling_steps][n_rec][C] (8-byte cells).  n_rec = 0 records nothing. */
int fg_mh_step(fg_engine *e, int n_steps, const int32_t *h_rec_sites, int n_rec, void *d_draws);
/* Incremental drivers (the step(n) / values_since protocol of crates/fugue-wasm/src/mh.rs:92-168, whose chains adapt for ever
 * and keep every state): with during_adaptation != 0 fg_mh_step records after EVERY step, d_draws [n_steps][n_rec][C]. */
int fg_mh_set_recording(fg_engine *e, int during_adaptation);
int fg_mh_run(fg_engine *e, int n_samples, int n_warmup, const fg_site_proposal *h_overrides,
              const int32_t *h_rec_sites, int n_rec, void *d_draws, fg_mh_stats *h_stats);
int fg_mh_get_stats(fg_engine *e, fg_mh_stats *h_stats);
int fg_mh_get_scales(fg_engine *e, double *h_scales /*[S][C]*/);     /* DiminishingAdaptation::scales */
int fg_mh_get_log_weight(fg_engine *e, double *h_lw /*[C]*/);        /* total_log_weight of the current trace */

/* ------------------------------------------------------------------ likelihood-tempered SMC
 * Replaces adaptive_smc (src/inference/smc.rs:455-581).  Particles = the engine's n_chains. */
enum { FG_RESAMPLE_MULTINOMIAL = 0, FG_RESAMPLE_SYSTEMATIC = 1, FG_RESAMPLE_STRATIFIED = 2 };   /* ResamplingMethod, smc.rs:133-140 */
typedef struct fg_smc_config {      /* SMCConfig, smc.rs:172-189 (same defaults) */
    int32_t resampling_method;      /* systematic */
    double  ess_threshold;          /* 0.5 */
    int32_t rejuvenation_steps;     /* 0 */
    int32_t sequential_adaptation;  /* 0: every particle of a rejuvenation sweep uses the scales from the sweep's start and the shared
                                     * DiminishingAdaptation is updated once per sweep from per-site counts (the many-particle form);
                                     * 1: the reference's own order (smc.rs:482,544-553,698-713) -- particle-major, the one adaptation
                                     * updated after EVERY move -- walked by one wave, sequential by construction (a few us per move:
                                     * for checking parity with the reference's semantics, not for speed).  (Sits in what was padding:
                                     * the struct's size and the other fields' offsets are unchanged.) */
} fg_smc_config;
typedef struct fg_smc_result {      /* SMCResult minus the particles (smc.rs:361-366) */
    double  log_evidence;
    int32_t n_steps;                /* tempering steps taken */
    int64_t n_model_runs;
} fg_smc_result;
void fg_smc_config_default(fg_smc_config *cfg);
/* Runs the whole ladder.  On return the engine's values [S][N] hold the final particles;
 * h_log_w / h_weights (optional, [N]) get the normalised log-weights / weights;
 * h_betas (optional) the inverse-temperature ladder. */
int fg_smc_run(fg_engine *e, const fg_smc_config *cfg, double *h_log_w, double *h_weights,
               fg_smc_result *h_result, double *h_betas, int max_betas);
/* The reference's standalone SMC building blocks over the engine's particles (values [S][N] in the engine; log-weights,
 * weights and log-likelihoods in HBM beside them):
 *   fg_smc_prior_particles  smc_prior_particles (smc.rs:764-790): prior draws, log_weight = log_likelihood + log_factors, normalised
 *   fg_smc_normalize        normalize_particles (smc.rs:719-755): weight = exp(log_weight - lse) / sum; uniform if all -inf
 *   fg_smc_ess              effective_sample_size (smc.rs:230-233): 1 / sum w^2
 *   fg_smc_resample         resample_particles (smc.rs:326-349): ancestors (h_indices, optional), clones, weight = 1/N
 *   fg_smc_rejuvenate       rejuvenate_particles (smc.rs:698-713): pi_beta-invariant MH moves, weights untouched
 *   fg_smc_get_weights / fg_smc_set_log_weights: the population's log-weights and weights (a caller's own reweighting) */
int fg_smc_prior_particles(fg_engine *e, uint32_t iteration);
int fg_smc_normalize(fg_engine *e);
int fg_smc_ess(fg_engine *e, double *out_ess);
int fg_smc_resample(fg_engine *e, int method, uint32_t step, int64_t *h_indices /*[N] or NULL*/);
int fg_smc_rejuvenate(fg_engine *e, double beta, int steps, uint32_t first_move_id, double *h_accept_rate /*or NULL*/);
int fg_smc_get_weights(fg_engine *e, double *h_log_w, double *h_weights);
int fg_smc_set_log_weights(fg_engine *e, const double *h_log_w);
/* population-wide primitives on device `device_ordinal`, usable without a program:
 * log_sum_exp (src/core/numerical.rs:15-38), next_beta (smc.rs:588-622) and
 * {multinomial,systematic,stratified}_indices (smc.rs:255-314) with the uniforms injected
 * (h_u: 1 value for systematic, n otherwise). */
int fg_device_log_sum_exp(int device_ordinal, const double *h_x, int64_t n, double *out);
int fg_device_next_beta(int device_ordinal, double beta, const double *h_log_w, const double *h_loglik,
                        int64_t n, double target_ess, double *out_beta);
int fg_device_resample_indices(int device_ordinal, int method, const double *h_weights, int64_t n,
                               const double *h_u, int64_t *h_idx);
/* one tempering step of fg_smc_run (next_beta by the device's passes, reweight, log-normaliser) on the
 * log-likelihoods h_loglik[n] from uniform log-weights -ln n.  flags: 1 = plain passes only (no zoom
 * passes), 2 = force the separate-kernels reweight.  h_log_w / h_weights receive the reweighted
 * log-weights and weights (either may be NULL); *out_need_sum (or NULL) = 1 when the separate kernels
 * took the step (beta' = beta + 1e-9, or flag 2). */
int fg_device_smc_temper(int device_ordinal, double beta, const double *h_loglik, int64_t n, double target_ess,
                         int flags, double *out_beta, double *out_log_norm, double *h_log_w, double *h_weights,
                         int *out_need_sum);

/* ------------------------------------------------------------------ mean-field variational inference
 * Replaces src/inference/vi.rs:104-923 (MeanFieldGuide, elbo_with_guide, elbo_gradient_fd, optimize_meanfield_vi_with_config,
 * estimate_elbo).  The engine's n_chains is the number of Monte Carlo samples per ELBO evaluation (VIConfig::n_samples_per_iter);
 * sample n of an evaluation draws from the counter-based stream (seed, chain_offset + n, stream id of the evaluation), so two
 * evaluations with one stream id see common random numbers -- the whole mechanism of elbo_gradient_fd (vi.rs:687-725).
 * A guide is a row of factors in address-sorted order (MeanFieldGuide::sample_trace, vi.rs:609-630). */
typedef struct fg_vi_factor {       /* VariationalParam, vi.rs:210-232 */
    int32_t family;                 /* 0 Normal {mu, log_sigma}, 1 LogNormal {mu, log_sigma}, 2 Beta {log_alpha, log_beta} */
    int32_t site;                   /* sorted site index, or -1: the address is no model site (drawn, adds nothing to log q: vi.rs:659-664) */
    double  a, b;                   /* location coordinate, scale coordinate (ParamCoord, vi.rs:167-172) */
} fg_vi_factor;
typedef struct fg_vi_config {       /* VIConfig, vi.rs:729-759 (same defaults; n_samples_per_iter = the engine's n_chains) */
    int32_t n_iterations;           /* 1000 */
    int32_t convergence_window;     /* 20 */
    double  base_learning_rate, fd_eps, convergence_tol, step_decay_exponent;   /* 0.1, 0.01, 1e-4, 0.6 */
} fg_vi_config;
typedef struct fg_vi_result { int32_t converged; int32_t iterations; } fg_vi_result;   /* VIResult minus guide and history, vi.rs:763-772 */
void fg_vi_config_default(fg_vi_config *cfg);
/* n_eval ELBO estimates (elbo_with_guide, vi.rs:639-669) in one launch: h_factors [n_eval][n_factors], h_stream_ids [n_eval],
 * h_elbo [n_eval]; h_terms (optional) [n_eval][C] = every sample's log p(x, z) - log q(z); with h_terms the draws of evaluation 0
 * are left in the engine's values (fg_engine_get_values: the guide traces, for inspection), otherwise the values are untouched.  The ELBO is the sum of the terms in the
 * engine's fixed order (fg_vi.hip) over C.  Errors: FG_ERR_ADDRESS_NOT_FOUND when an f64 site has no factor (the panic of
 * ScoreGivenTrace) or the program has a discrete sample site (GuideError::UnsupportedDiscreteLatent, vi.rs:136-144); a non-finite
 * factor parameter is InvalidParameters with FG_ERR_INVALID_MEAN / _VARIANCE / _SHAPE; a family outside 0..2, a site out of range
 * or factors out of address order are FG_E_BAD_ARG. */
int fg_vi_elbo_batch(fg_engine *e, const fg_vi_factor *h_factors, int n_eval, int n_factors, const uint32_t *h_stream_ids,
                     double *h_elbo, double *h_terms);
/* optimize_meanfield_vi_with_config (vi.rs:784-864): h_factors [n_factors] is the initial guide and receives the optimized one,
 * h_elbo_history [n_iterations] the monitor of every iteration run.  Iteration t draws the monitor from stream id t (2 n_factors + 1)
 * and both signs of coordinate j = 2 factor + (0 location, 1 scale) from t (2 n_factors + 1) + 1 + j; FG_E_LIMIT when
 * n_iterations (2 n_factors + 1) reaches 2^32. */
int fg_vi_optimize(fg_engine *e, fg_vi_factor *h_factors, int n_factors, const fg_vi_config *cfg, double *h_elbo_history,
                   fg_vi_result *h_result);
/* estimate_elbo (vi.rs:905-923): the prior as the guide -- the mean over the engine's chains of log_likelihood + log_factors of a
 * prior run (the draws of fg_prior_init at `iteration`), summed in the same fixed order. */
int fg_vi_estimate_elbo(fg_engine *e, uint32_t iteration, double *h_elbo);

/* ------------------------------------------------------------------ cross-chain diagnostics
 * Per-chain statistics behind r_hat_f64 / effective_sample_size_multichain
 * (src/inference/diagnostics.rs:218-304, src/inference/mcmc_utils.rs:214-339).  Draws stay on the
 * GPU; only these small summaries are exchanged between GPUs (RCCL) and combined on the host. */
/* d_draws [n][d][C] -> d_moments [d][6][C] = mean, sum of squared deviations of the full chain,
 * of its first half and of its second half (half = n/2, middle draw dropped when n is odd). */
int fg_diag_chain_moments(fg_engine *e, const double *d_draws, int n, int d, double *d_moments);
/* h_sums [d][n_lags] = sum over this engine's chains of the biased lag-t autocovariances
 * (mcmc_utils.rs:231-244) for t in [lag0, lag0 + n_lags). */
int fg_diag_autocov_sums(fg_engine *e, const double *d_draws, int n, int d, const double *d_moments,
                         int lag0, int n_lags, double *h_sums);

/* ------------------------------------------------------------------ checkpoint / resume
 * The per-chain sampler state as one flat host blob: the fields of HmcSession (hmc.rs:643-661) for every chain, the MH
 * chain state (current trace, log-weight, DiminishingAdaptation per site, decided proposal kinds, overrides) and the
 * iteration counters that position the counter-based random streams (cf. the wasm samplers' step(n) protocol,
 * crates/fugue-wasm/src/mh.rs:92-168).  run(a); export; [new engine of the same program and chain count] import;
 * run(b) reproduces run(a + b) bit for bit. */
int64_t fg_state_size(fg_engine *e);
int     fg_state_export(fg_engine *e, void *h_buf, size_t capacity);
int     fg_state_import(fg_engine *e, const void *h_buf, size_t size);

/* geweke_diagnostic (src/inference/mcmc_utils.rs:354-421) of every (coordinate, chain): d_draws [n][d][C] -> d_z [d][C] */
int fg_diag_geweke(fg_engine *e, const double *d_draws, int n, int d, double *d_z);
/* r_hat_f64 (split R-hat, diagnostics.rs:218-224,240-304), effective_sample_size_multichain (mcmc_utils.rs:214-339) and the
 * pooled mean / sample std of summarize_f64_parameter (diagnostics.rs:331-352) for every coordinate of d_draws [n][d][C],
 * over the chains of EVERY rank of `rccl_comm` (an ncclComm_t; NULL = this engine's chains only).  With a communicator the
 * chain sums and the pooled lag sums are all-reduced over RCCL / xGMI inside the call (fg_diag_set_exchange); all ranks call
 * it with equal n, d and chain count and receive the same numbers.  h_* are [d]; any may be NULL. */
int fg_diag_rhat_ess(fg_engine *e, const double *d_draws, int n, int d, void *rccl_comm, double *h_rhat, double *h_ess,
                     double *h_mean, double *h_std, int64_t *out_total_chains);
/* How the ranks of `rccl_comm` exchange chain statistics inside fg_diag_rhat_ess.  FG_DIAG_REDUCE (default): chains enter split
 * R-hat (diagnostics.rs:262-304), the pooled mean / std and the multi-chain ESS (mcmc_utils.rs:253-339) only through sums over
 * chains, so every rank reduces its own chains on the device and the ranks all-reduce 6 d + 2 d doubles plus 32 d per chunk of
 * lags (+ d when h_std is asked for: the cross term sum_j (mean_j - mean) sum_t (x_t - mean_j) that keeps the pooled std exact
 * when the in-order chain means are rounded, in either mode) -- nothing proportional to the chain count leaves a GPU.  FG_DIAG_GATHER: all-gather of every chain's moments
 * ([d][6][C] per rank) and the combination in global chain order on every rank, as a single process would sum them.  The two
 * agree to rounding of the sums over chains (~1e-15 relative).  fg_diag_exchange_bytes: bytes this rank contributed to
 * collectives during the last fg_diag_rhat_ess (0 without a communicator). */
#define FG_DIAG_REDUCE 0
#define FG_DIAG_GATHER 1
int fg_diag_set_exchange(fg_engine *e, int mode);
int64_t fg_diag_exchange_bytes(const fg_engine *e);
/* The quantiles of summarize_f64_parameter (diagnostics.rs:355-371): for every coordinate of d_draws [n][d][C] and every
 * probability p, sorted[round((len - 1) p)] of ALL len = ranks x C x n draws of the coordinate (the reference's "2.5%", "25%",
 * "50%", "75%", "97.5%" are p = 0.025, 0.25, 0.5, 0.75, 0.975).  Radix select on the device (eight histogram passes over the
 * draws; the 256-bin counters are all-reduced over `rccl_comm` when the chains are sharded): exactly the element a sort would put
 * at that index.  n_probs <= 8; h_out [d][n_probs]. */
int fg_diag_quantiles(fg_engine *e, const double *d_draws, int n, int d, void *rccl_comm, const double *h_probs, int n_probs,
                      double *h_out);
/* The combination alone, on host buffers (no GPU needed): h_moments [d][6][m] of ALL chains in global chain order;
 * `acov` returns h_sums [d][n_lags] = sum over all chains of the biased lag-t autocovariances for t in
 * [lag0, lag0 + n_lags) (it is asked for 32 lags at a time, only as far as Geyer's sequence runs). */
typedef int (*fg_acov_fn)(void *user, int lag0, int n_lags, double *h_sums);
int fg_diag_combine(const double *h_moments, int64_t m, int n, int d, fg_acov_fn acov, void *user, double *h_rhat,
                    double *h_ess, double *h_mean, double *h_std);
/* The same combination from sums over chains (what FG_DIAG_REDUCE exchanges).  `reduce` returns sums over ALL chains of all ranks:
 * stage 1: h_out [d][6] = sums of the six moment rows; stage 2: h_in [d][2] = overall means {full chains, half chains},
 * h_out [d][2] = {sum_j (mean_j - in0)^2, sum_j (mean_h1_j - in1)^2 + (mean_h2_j - in1)^2} -- the reference's two-pass
 * between-chain sums of squares (diagnostics.rs:275-289, mcmc_utils.rs:296-304) with the pass over chains distributed. */
typedef int (*fg_reduce_fn)(void *user, int stage, const double *h_in, double *h_out);
int fg_diag_combine_reduced(int64_t m, int n, int d, fg_reduce_fn reduce, fg_acov_fn acov, void *user, double *h_rhat,
                            double *h_ess, double *h_mean, double *h_std);
/* ------------------------------------------------------------------ diagnostics without stored draws
 * The figures of fg_diag_rhat_ess -- r_hat_f64 (diagnostics.rs:218-224,240-304), effective_sample_size_multichain
 * (mcmc_utils.rs:214-339), the pooled mean / std of summarize_f64_parameter (diagnostics.rs:331-352) -- for a run that is handed
 * over one chunk of draws at a time and never stored.  Per (coordinate, chain) the stream keeps (3 K + 7) doubles, K = max_lag
 * rounded up to a multiple of 32 (at most 2 048, the reference's lag cap, mcmc_utils.rs:266): in-order sums about the column's
 * first draw, so the result does not depend on where the chunk boundaries fall.  Quantiles need the draws: fg_diag_qstream below selects
 * them from a run that is presented again, once per pass. */
typedef struct fg_diag_stream fg_diag_stream;
/* FG_E_BAD_ARG: n_total < 1, d outside [1, 65535], max_lag outside [1, 2048].  The stream must be freed before its engine. */
int  fg_diag_stream_new(fg_engine *e, int n_total, int d, int max_lag, fg_diag_stream **out);
/* The next n_chunk draws d_draws [n_chunk][d][C] (e.g. what fg_hmc_step / fg_mh_step just recorded); asynchronous on the engine's
 * stream.  FG_E_STATE when the chunk would pass n_total. */
int  fg_diag_stream_update(fg_diag_stream *s, const double *d_draws, int n_chunk);
int  fg_diag_stream_count(const fg_diag_stream *s);                       /* draws taken so far */
/* The read-outs below are FG_E_STATE before n_total draws have arrived.  d_moments [d][6][C] as fg_diag_chain_moments
 * (split_f64_chains, diagnostics.rs:240-253: the middle draw dropped when n_total is odd). */
int  fg_diag_stream_moments(fg_diag_stream *s, double *d_moments);
/* h_sums [d][n_lags] as fg_diag_autocov_sums (autocovariances, mcmc_utils.rs:231-244); lags >= n_total are 0, a lag >= K below
 * n_total is FG_E_LIMIT. */
int  fg_diag_stream_autocov_sums(fg_diag_stream *s, int lag0, int n_lags, double *h_sums);
/* fg_diag_rhat_ess over the stream: the same combination (ess_from_chains, mcmc_utils.rs:253-339; r_hat_from_f64_chains,
 * diagnostics.rs:262-304), exchange mode and communicator.  FG_E_LIMIT when Geyer's sequence asks for a lag >= K: a figure is never
 * computed from missing lags; with h_ess == NULL no lag is asked for.  K >= min(n_total - 1, 2048) never hits the limit. */
int  fg_diag_stream_rhat_ess(fg_diag_stream *s, void *rccl_comm, double *h_rhat, double *h_ess, double *h_mean,
                             double *h_std, int64_t *out_total_chains);
void fg_diag_stream_free(fg_diag_stream *s);
/* ------------------------------------------------------------------ quantiles without stored draws
 * The quantiles of summarize_f64_parameter (diagnostics.rs:355-371), sorted[round((len - 1) p)] over the len = n_total x C draws
 * of a coordinate, for a run that is never stored but can be presented again: the random streams are keyed by (seed, chain,
 * iteration), so fg_state_import of the blob taken after warmup followed by the same fg_hmc_step / fg_mh_step calls reproduces
 * every draw.  A pass is one presentation of all n_total draws, in any chunking.  Exact radix select on fg_diag_quantiles' key
 * (-0.0 below +0.0, positive NaN above +inf): a pass counts the next digit_bits bits of the elements that still match each
 * quantile's prefix; once at most `capacity` elements match, the next pass collects them (d x n_probs x capacity keys of device
 * memory) and the host picks the element.  The result is the element a sort would give.  Every pass must present the same draws:
 * the count of matching elements is checked against the previous pass at every end_pass (FG_E_STATE: a replay that diverged never
 * yields a quantile).  These entry points cover this engine's chains only and take no communicator; runs sharded over ranks keep
 * fg_diag_quantiles on stored draws. */
typedef struct fg_diag_qstream fg_diag_qstream;
/* diagnostics.rs:355-371.  FG_E_BAD_ARG: n_total < 1, d outside [1, 65535], n_probs outside [1, 8], a probability outside [0, 1],
 * digit_bits outside [1, 12], capacity < 0.  The stream must be freed before its engine. */
int  fg_diag_qstream_new(fg_engine *e, int n_total, int d, const double *h_probs, int n_probs,
                         int digit_bits, int64_t capacity, fg_diag_qstream **out);
/* diagnostics.rs:355-371: the next n_chunk draws d_draws [n_chunk][d][C] of the current pass; asynchronous on the engine's stream.
 * FG_E_STATE when the chunk would pass n_total, or once every quantile is selected. */
int  fg_diag_qstream_update(fg_diag_qstream *s, const double *d_draws, int n_chunk);
int  fg_diag_qstream_count(const fg_diag_qstream *s);          /* diagnostics.rs:355-371: draws taken in the current pass */
/* diagnostics.rs:355-371: ends the pass (FG_E_STATE before n_total draws, or when it did not reproduce the previous pass);
 * *out_done = 1 when every quantile is selected, else the next pass has begun. */
int  fg_diag_qstream_end_pass(fg_diag_qstream *s, int *out_done);
int  fg_diag_qstream_passes(const fg_diag_qstream *s);         /* diagnostics.rs:355-371: passes completed */
/* diagnostics.rs:355-371: h_out [d][n_probs]; h_slot_passes [d][n_probs] (or NULL) = the passes each quantile took part in.
 * FG_E_STATE before the stream is done. */
int  fg_diag_qstream_result(fg_diag_qstream *s, double *h_out, int32_t *h_slot_passes);
void fg_diag_qstream_free(fg_diag_qstream *s);                 /* diagnostics.rs:355-371 */
/* ------------------------------------------------------------------ discrete sites without stored draws
 * The reference extracts the values of a discrete site (extract_bool_values / extract_u64_values / extract_usize_values /
 * extract_i64_values, diagnostics.rs:76-98) and its callers tabulate them; fg_diag_cstream keeps those frequency tables for a run
 * that is handed over one chunk at a time and never stored.  A chunk is what fg_mh_step records: [n_chunk][n_rec][C] 8-byte cells,
 * f64 rows and integer rows mixed.  The stream watches n_watch of its rows.  Watched row k: its chunk row h_rows[k] (each at most
 * once), its ChoiceValue tag h_vtypes[k] (FG_U64 cells compare as unsigned, FG_BOOL / FG_USIZE / FG_I64 cells as signed; FG_F64 is
 * refused), a lower bound h_lo[k] and a bin count h_bins[k].  It keeps, as 64-bit integers, counts[bins] (bin j: the cells equal to
 * lo + j), `below` and `above` (the cells outside [lo, lo + bins): nothing is dropped silently) and the smallest and largest cell
 * seen.  Integer sums: the result does not depend on chunk boundaries or arrival order.  Rows of at most 8 bins are counted by
 * wave ballots, wider ones in an LDS histogram; FG_DIAG_CSTREAM_FORM=wide|narrow (read at fg_diag_cstream_new) forces a form where
 * it is legal.  This engine's chains only: counts of ranks add on the host. */
typedef struct fg_diag_cstream fg_diag_cstream;
/* diagnostics.rs:76-98.  FG_E_BAD_ARG: n_total < 1, n_rec < 1, n_watch outside [1, 65535], a row outside [0, n_rec) or given twice,
 * a tag that is FG_F64 or unknown, bins outside [1, 4096], lo + bins overflowing the row's integer type (lo < 0 on an FG_U64 row).
 * The stream must be freed before its engine. */
int  fg_diag_cstream_new(fg_engine *e, int n_total, int n_rec, const int32_t *h_rows, const int32_t *h_vtypes,
                         const int64_t *h_lo, const int32_t *h_bins, int n_watch, fg_diag_cstream **out);
/* diagnostics.rs:76-98: the next n_chunk draws d_cells [n_chunk][n_rec][C]; asynchronous on the engine's stream.  FG_E_STATE when
 * the chunk would pass n_total. */
int  fg_diag_cstream_update(fg_diag_cstream *s, const void *d_cells, int n_chunk);
int  fg_diag_cstream_count(const fg_diag_cstream *s);          /* diagnostics.rs:76-98: draws taken so far */
/* diagnostics.rs:76-98: h_counts = the rows' bins back to back, h_below / h_above / h_min / h_max [n_watch] (min / max of an FG_U64
 * row are the cell's 64 bits).  FG_E_STATE before n_total draws have arrived, or when a row's counts + below + above differ from
 * n_total x C (the stream's integrity check). */
int  fg_diag_cstream_result(fg_diag_cstream *s, uint64_t *h_counts, uint64_t *h_below, uint64_t *h_above,
                            int64_t *h_min, int64_t *h_max);
void fg_diag_cstream_free(fg_diag_cstream *s);                 /* diagnostics.rs:76-98 */
/* diagnostics.rs:153-191 (Diagnostics<u64>: `x as f64`): d_cells [n][n_rec][C] -> d_out [n][n_sel][C], output row k = chunk row
 * h_rows[k] (any order, repeats allowed) converted by its tag h_vtypes[k]: FG_F64 bits copied, FG_U64 (double)(uint64_t), FG_BOOL /
 * FG_USIZE / FG_I64 (double)(int64_t).  What fg_diag_stream / fg_diag_qstream take.  One streaming kernel, asynchronous on the
 * engine's stream; n = 0 is FG_OK without a launch.  FG_E_BAD_ARG: n < 0, n_rec < 1, n_sel < 1, a row outside [0, n_rec), an
 * unknown tag. */
int fg_diag_cells_f64(fg_engine *e, const void *d_cells, int n, int n_rec, const int32_t *h_rows,
                      const int32_t *h_vtypes, int n_sel, double *d_out);
/* ------------------------------------------------------------------ model comparison without a stored table
 * WAIC and importance-sampling LOO (BDA3 7.2; the reference has neither) from the pointwise log-likelihood fg_predict_eval writes,
 * d_loglik [n][n_sel][C], handed over one chunk at a time.  The stream keeps 10 words per (selected observe statement, chain) --
 * 80 x n_sel x C bytes, 5.4 GB at n_sel = 1 024 and C = 65 536: select the statements to compare with fg_predict_eval's h_sel --
 * updated in draw order by one thread, so the state does not depend on the chunking, bit for bit.  At read-out the chains of a
 * statement are pooled by a fixed binary tree on the chain index (a function of C alone) into FG_LL_POOLED finite words
 *   mx, sum exp(x - mx), mn, sum exp(mn - x), sum exp(mn - x)^2, the finite cells F, their mean, their sum of squared deviations
 * and three counters of the cells that are -inf, +inf, NaN.  Per statement, over the N = n_total x C pooled cells x, the
 * FG_LL_FIGURES figures are
 *   0 lppd = ln((1/N) sum exp x)            1 mean_ll = mean x              2 p_waic = the variance of x, divisor N - 1 (BDA3 eq. 7.12)
 *   3 elpd_waic = lppd - p_waic             4 elpd_loo = -ln((1/N) sum r), r = exp(-x) the raw importance ratios
 *   5 p_loo = lppd - elpd_loo               6 is_ess = (sum r)^2 / sum r^2  7 max_weight = max r / sum r
 * as the two-pass formulas give them in IEEE arithmetic: a NaN cell makes every figure of its statement NaN, a -inf cell is zero
 * mass in lppd and makes elpd_loo -inf, a +inf cell makes lppd +inf; both count in N.  No Pareto smoothing: is_ess and max_weight
 * are the diagnostic of the raw ratios.  This engine's chains only.  The stream reads engine state and changes none. */
#define FG_LL_POOLED 8
#define FG_LL_FIGURES 8
typedef struct fg_loglik_stream fg_loglik_stream;
/* FG_E_BAD_ARG: n_total < 1, n_sel < 1.  The stream must be freed before its engine. */
int  fg_loglik_stream_new(fg_engine *e, int n_total, int n_sel, fg_loglik_stream **out);
/* the next n_chunk draws d_loglik [n_chunk][n_sel][C]; asynchronous on the engine's stream; n_chunk == 0 is FG_OK without a
 * launch.  FG_E_STATE when the chunk would pass n_total. */
int  fg_loglik_stream_update(fg_loglik_stream *s, const double *d_loglik, int n_chunk);
int  fg_loglik_stream_count(const fg_loglik_stream *s);        /* draws taken so far */
/* the pooled words h_words [n_sel][FG_LL_POOLED] and counters h_counts [n_sel][3] (-inf, +inf, NaN).  FG_E_STATE before n_total
 * draws have arrived. */
int  fg_loglik_stream_pooled(fg_loglik_stream *s, double *h_words, int64_t *h_counts);
/* the figures h_figures [FG_LL_FIGURES][n_sel] and the counters as above.  FG_E_STATE before n_total draws have arrived. */
int  fg_loglik_stream_result(fg_loglik_stream *s, double *h_figures, int64_t *h_counts);
void fg_loglik_stream_free(fg_loglik_stream *s);
/* ------------------------------------------------------------------ posterior predictive checks without a stored table
 * What the reference's workflows do by hand after replicating the data (tests/end_to_end_workflows.rs:650-745,
 * tests/inference_integration.rs:717-740, examples/bayesian_coin_flip.rs:211-): the mean of every replicated data set, its variance
 * with divisor K - 1, or its number of heads, compared with the same statistic of the observed data and read as a p-value.  Here from
 * the replicate table fg_predict_eval writes, d_yrep [n][n_rows][C] raw cells, handed over one chunk at a time.
 * A CHECK is a group of K >= 1 rows of the table (members, in the order given; a row may belong to several checks) and an observed
 * vector y[K].  Cells become doubles as fg_diag_cells_f64 converts them (`x as f64` by the row's value type).  The statistics of a
 * data set, in member order, every operation rounded:
 *   FG_PPC_MEAN  the in-order sum onto +0.0 over (double)K (end_to_end_workflows.rs:700-703)
 *   FG_PPC_VAR   a second in-order pass of (x - mean)(x - mean) onto +0.0 over (double)(K - 1) (:720-726); K = 1: 0/0 = NaN
 *   FG_PPC_MIN / FG_PPC_MAX  from the first member by x < m ? x : m and x > m ? x : m
 *   FG_PPC_SUM   the in-order sum itself (the number of heads of Bernoulli rows, bayesian_coin_flip.rs:211-)
 * and a NaN cell anywhere in the group makes all five NaN.  A SLOT is a (check, statistic) pair asked for by the check's mask (bit
 * FG_PPC_x), numbered in check order, then in statistic order.  Per (slot, chain) the stream keeps 6 words -- 48 bytes; a model with
 * 1 024 observe statements selects the checks it needs -- updated in draw order by one thread, so the state does not depend on the
 * chunking, bit for bit: counters of draws whose statistic T is <, ==, > the observed one (-0.0 == +0.0, infinities as IEEE compares
 * them) and of draws where either is NaN (u32: n_total < 2^31), and the pivoted sums of the finite T.  At read-out the counters pool
 * over the chains by addition and the moments by the fixed tree on the chain index of the log-likelihood stream.  This engine's chains
 * only; unweighted draws only (not an SMC population).  The stream reads engine state and changes none. */
enum { FG_PPC_MEAN = 0, FG_PPC_VAR = 1, FG_PPC_MIN = 2, FG_PPC_MAX = 3, FG_PPC_SUM = 4, FG_PPC_N_STATS = 5 };
typedef struct fg_ppc_stream fg_ppc_stream;
/* h_vtypes [n_rows]: the value type of every table row (FG_F64 .. FG_I64); h_offsets [n_checks + 1] into h_members (rows in
 * [0, n_rows)) and h_observed (aligned with h_members); h_stat_mask [n_checks].  FG_E_BAD_ARG: n_total < 1, n_rows < 1, no check, an
 * empty check, an empty mask or a mask bit >= FG_PPC_N_STATS, a member outside the rows, an unknown value type, offsets that do not
 * start at 0 or decrease.  The stream must be freed before its engine. */
int  fg_ppc_stream_new(fg_engine *e, int n_total, int n_rows, const int32_t *h_vtypes, int n_checks, const int32_t *h_offsets,
                       const int32_t *h_members, const int32_t *h_stat_mask, const double *h_observed, fg_ppc_stream **out);
/* the next n_chunk draws d_yrep [n_chunk][n_rows][C]; asynchronous on the engine's stream; n_chunk == 0 is FG_OK without a launch.
 * FG_E_STATE when the chunk would pass n_total. */
int  fg_ppc_stream_update(fg_ppc_stream *s, const void *d_yrep, int n_chunk);
int  fg_ppc_stream_count(const fg_ppc_stream *s);              /* draws taken so far */
int  fg_ppc_stream_n_slots(const fg_ppc_stream *s);
/* h_t_obs [n_slots]: the statistic of the observed vector of every slot (the `obs_mean` / `obs_var` of the workflows) */
int  fg_ppc_stream_observed(const fg_ppc_stream *s, double *h_t_obs);
/* pooled over the chains: h_counts [n_slots][5] draws with T < / == / > T_obs, NaN draws, finite T; h_moments [n_slots][2] the mean of
 * the finite T and their sum of squared deviations (NaN without a finite draw; +0.0 deviations with one).  FG_E_STATE before n_total
 * draws have arrived. */
int  fg_ppc_stream_pooled(fg_ppc_stream *s, int64_t *h_counts, double *h_moments);
/* the same five counters of one slot per chain, h_counts [5][C]: the between-chain spread of a p-value.  FG_E_STATE as above;
 * FG_E_BAD_ARG: a slot outside [0, n_slots). */
int  fg_ppc_stream_chains(fg_ppc_stream *s, int slot, int64_t *h_counts);
void fg_ppc_stream_free(fg_ppc_stream *s);
/* ------------------------------------------------------------------ weighted populations on the device
 * The reference summarises a weighted population on the host: ABCSMCResult::weighted_mean (abc.rs:476) and the doc example that walks
 * the particles by hand (smc.rs:445-453).  fg_wpop does it where the population lies: rows d_x [d][N] of doubles (element i of a row
 * belongs to particle i) and normalised weights w [N], both in device memory.
 *   Units: q_i = (uint64) rint(w_i 2^52), half to even, for 0 <= w_i <= 1; any other weight (NaN, negative, infinite, above 1) is BAD,
 *   has no units and is counted in n_bad; n_zero counts the good weights of zero units; T = sum q_i (FG_E_BAD_ARG at 2^53 and above:
 *   such weights are not normalised).  Quantiles and tables are sums of units -- integers, whatever the order of the additions -- and a
 *   particle of zero units takes no part in them.
 *   Quantile of p: with t = min(T, max(1, ceil(p (double)T))), the smallest value v of the row with sum_{key(x_j) <= key(v)} q_j >= t,
 *   keys ordered as fg_diag_qstream orders them (-0.0 below +0.0, a positive-sign NaN above +inf): an inverse weighted CDF, NOT the
 *   sorted[round((len - 1) p)] of summarize_f64_parameter.  T == 0: NaN.  Found by radix select over digits of `digit_bits` bits,
 *   collecting a bucket once it holds at most `capacity` elements.
 *   Moments use the doubles w_i of the particles with a good weight above zero and a finite cell, merged over the fixed binary tree
 *   on the particle index of the chain-pooled streams: W = sum w, mean, var = ssd / W, std, mcse = sqrt(sum w_i^2 (x_i - mean)^2) / W
 *   and n_used, the number of such particles (as a double).  No such particle: W = 0, n_used = 0, the rest NaN.
 *   Tables: bin j of an integer row holds the units of the cells equal to lo + j, `below` / `above` the units outside the bins, min /
 *   max are taken over the cells of non-zero units (0 when T == 0).  Cells are read by their tag as fg_diag_cstream reads them.
 * The handle copies the weights at fg_wpop_new and reads no engine state afterwards; it changes none.  One device, one rank. */
#define FG_WPOP_MOMENTS 6
typedef struct fg_wpop fg_wpop;
/* abc.rs:476 / smc.rs:445-453: the weights d_w [n] in device memory (any n >= 1), or d_w == NULL for the engine's own population
 * (FG_E_STATE without one; FG_E_BAD_ARG unless n is the engine's number of chains).  Free the handle before its engine. */
int  fg_wpop_new(fg_engine *e, int64_t n, const double *d_w, fg_wpop **out);
/* abc.rs:476 / smc.rs:445-453: T, n_bad, n_zero (any may be NULL) */
int  fg_wpop_units(const fg_wpop *h, uint64_t *out_T, uint64_t *out_n_bad, uint64_t *out_n_zero);
/* abc.rs:476 / smc.rs:445-453: h_out [d][FG_WPOP_MOMENTS] = W, mean, var, std, mcse, n_used of rows d_x [d][n].  FG_E_BAD_ARG: d
 * outside [1, 65535]. */
int  fg_wpop_moments(fg_wpop *h, const double *d_x, int d, double *h_out);
/* abc.rs:476 / smc.rs:445-453: h_out [d][n_probs]; h_passes [d][n_probs] (or NULL) = the passes over its row each quantile took.
 * FG_E_BAD_ARG: d outside [1, 65535], n_probs outside [1, 8], a probability outside [0, 1], digit_bits outside [1, 12],
 * capacity < 0.  FG_E_STATE: a pass whose totals differ from what the previous pass left (never a quantile). */
int  fg_wpop_quantiles(fg_wpop *h, const double *d_x, int d, const double *h_probs, int n_probs, int digit_bits,
                       int64_t capacity, double *h_out, int32_t *h_passes);
/* abc.rs:476 / smc.rs:445-453: integer rows d_cells [n_rows][n] with tags h_vtypes, lower bounds h_lo and bin counts h_bins [n_rows];
 * h_units = the rows' bins back to back, h_below / h_above / h_min / h_max [n_rows].  FG_E_BAD_ARG: n_rows outside [1, 65535], a tag
 * that is FG_F64 or unknown, bins outside [1, 4096], lo + bins overflowing the row's integer type.  FG_E_STATE: a row whose units do
 * not add up to T. */
int  fg_wpop_counts(fg_wpop *h, const void *d_cells, int n_rows, const int32_t *h_vtypes, const int64_t *h_lo,
                    const int32_t *h_bins, uint64_t *h_units, uint64_t *h_below, uint64_t *h_above, int64_t *h_min, int64_t *h_max);
/* Predictive checks and WAIC / IS-LOO of the population (tests/end_to_end_workflows.rs:330-400 compares models and :650-745 checks
 * replicated data after every sampler, SMC included).  Rows [rows][n], particle-fastest, in device memory; nothing of size n goes to
 * the host; engine state is neither read nor changed.
 *   Checks: fg_ppc_stream's checks (CSR members, 5-bit masks, observed vectors, its statistics, cell conversion and slot numbering) of
 *   ONE replicate per particle.  Per slot, FG_WPOP_CATS categories: T_rep < / == / > T_obs by IEEE compare (-0.0 == +0.0), or either
 *   side NaN.  A particle adds its units to exactly one category and, with units above zero, 1 to that category's element count.
 *   The p-values are quotients of unit sums: p_ge = (U_gt + U_eq) / (U_lt + U_eq + U_gt), p_gt, p_mid = (2 U_gt + U_eq) / (2 (...)).
 *   The moments of T_rep are fg_wpop_moments' of a scratch table of the statistics.
 *   Log-likelihood: a particle takes part in a row iff its weight is good and above zero.  h_counts: participating cells that are
 *   finite, -inf, +inf, NaN.  h_words, FG_WLL_WORDS per row: W (the participating weights), W_fin, W2 = sum w^2, mean, ssd and n_used of
 *   the finite participating cells (the leaves of fg_wpop_moments), mx, mn (their exact max and min), sp = sum w exp(x - mx),
 *   sn = sum w exp(mn - x), sn2 = sum (w exp(mn - x))^2, tmax = the largest term of sn; every sum over the fixed tree on the
 *   particle index.  h_figures in fg_loglik_stream's order: lppd = mx + ln(sp / W), mean_ll, p_waic = ssd / (W_fin - W2 / W_fin)
 *   (reliability weights: the divisor N - 1 at equal weights; NaN when n_used < 2), elpd_waic, elpd_loo = mn - ln(sn / W), p_loo,
 *   is_ess = sn^2 / sn2 (Kish, in particles), max_weight = tmax / sn.  A NaN cell makes every figure NaN; a -inf cell is zero mass
 *   in lppd and makes elpd_loo -inf, is_ess and max_weight NaN; a +inf cell makes lppd +inf; both count in W; a row without a finite
 *   participating cell has NaN figures and its counters. */
#define FG_WPOP_CATS 4
#define FG_WLL_FIGURES 8
#define FG_WLL_WORDS 12
#define FG_WLL_COUNTS 4
/* abc.rs:476 / smc.rs:445-453, end_to_end_workflows.rs:650-745: the slots the masks ask for (at most 65535), or FG_E_BAD_ARG */
int  fg_wpop_checks_n_slots(int n_checks, const int32_t *h_stat_mask);
/* abc.rs:476 / smc.rs:445-453, end_to_end_workflows.rs:650-745: d_yrep [n_rows][n] raw cells; the check arguments of
 * fg_ppc_stream_new.  h_t_obs [n_slots], h_units [n_slots][FG_WPOP_CATS], h_counts [n_slots][FG_WPOP_CATS] (lt, eq, gt, nan),
 * h_moments [n_slots][FG_WPOP_MOMENTS].  FG_E_BAD_ARG: fg_ppc_stream_new's, n_rows or n_slots outside [1, 65535].  FG_E_STATE: a slot
 * whose units do not add up to T. */
int  fg_wpop_checks(fg_wpop *h, const void *d_yrep, int n_rows, const int32_t *h_vtypes, int n_checks, const int32_t *h_offsets,
                    const int32_t *h_members, const int32_t *h_stat_mask, const double *h_observed, double *h_t_obs, uint64_t *h_units,
                    int64_t *h_counts, double *h_moments);
/* abc.rs:476 / smc.rs:445-453, end_to_end_workflows.rs:330-400: d_ll [n_sel][n] doubles; h_figures [FG_WLL_FIGURES][n_sel], h_words
 * [n_sel][FG_WLL_WORDS], h_counts [n_sel][FG_WLL_COUNTS] (h_words and h_counts may be NULL).  FG_E_BAD_ARG: n_sel outside [1, 65535]. */
int  fg_wpop_loglik(fg_wpop *h, const double *d_ll, int n_sel, double *h_figures, double *h_words, int64_t *h_counts);
void fg_wpop_free(fg_wpop *h);                                 /* abc.rs:476 / smc.rs:445-453 */
/* ------------------------------------------------------------------ Pareto-smoothed LOO of a stored log-likelihood table
 * PSIS-LOO and k-hat per observe statement (Vehtari, Simpson, Gelman, Yao, Gabry; the generalised Pareto fit of Zhang and Stephens
 * 2009 with the weakly informative prior, as the R `loo` package's psis / gpdfit; r_eff = 1; the reference has none of it) from a
 * table d_ll [n][n_sel][C] that lies on the device (C the engine's chains): what fg_predict_eval writes and fg_loglik_stream_update
 * takes.  Nothing is replayed.  Per statement over its S = n C pooled cells x: lw = x_min - x; the tail is the M = min(ceil(S / 5),
 * ceil(3 sqrt S)) smallest x, the cutoff the (M + 1)-th smallest; the fit runs over t_j = exp(lw_(j)) - exp(lw_cut) in ascending
 * order; the smoothed tail replaces the M largest ratios, capped at the largest raw one.  The rule, the fixed summation orders and the
 * limits: fg_psis_plan.h and DESIGN 3.22.  A row of FG_PSIS_WORDS doubles per statement:
 *   0 elpd_loo_psis  1 p_loo_psis = lppd - elpd_loo_psis  2 khat  3 sigma  4 khat_threshold = min(1 - 1 / log10 S, 0.7)  5 lppd
 *   6 x_min  7 the cutoff x  8 exp(lw_cut)  9 t*  10 theta-hat  11 the body's sum of ratios  12 the tail's  13 the tail's numerator
 * and a row of FG_PSIS_COUNTS integers:
 *   0 tail_len = M  1 status (FG_PSIS_*)  2 n_capped  3 finite cells  4 -inf cells  5 +inf cells  6 NaN cells
 *   7 cells below the cutoff key  8 cells on it  9 cells collected (= word 7, or FG_E_STATE)
 * Without a fit (M < 5, a degenerate tail: t* <= 0) khat = +inf and elpd_loo_psis is the raw importance-sampling value by the same
 * formula.  A NaN cell makes every figure of its statement NaN; a -inf cell gives elpd_loo_psis = -inf and khat = +inf; +inf cells
 * have ratio 0 and lie in the body (a +inf cell that reaches the cutoff: no fit, status FG_PSIS_NONFINITE). */
#define FG_PSIS_WORDS 14
#define FG_PSIS_COUNTS 10
enum { FG_PSIS_FITTED = 0, FG_PSIS_TOO_FEW = 1, FG_PSIS_DEGENERATE = 2, FG_PSIS_NONFINITE = 3 };
int     fg_psis_words(void);                                   /* FG_PSIS_WORDS of this library */
/* M for S pooled draws; FG_E_BAD_ARG for S < 1, FG_E_LIMIT for S >= 2^31.  No device. */
int64_t fg_psis_tail_len(int64_t S);
/* h_figures [n_sel][FG_PSIS_WORDS], h_counts [n_sel][FG_PSIS_COUNTS]; d_tail_or_null, if given, receives the sorted raw tails
 * [n_sel][M] (ascending in the order of fg_diag_quantiles' keys: -0.0 below +0.0).  Every argument is checked before the device is
 * looked for.  FG_E_BAD_ARG: a null pointer, n < 1, n_sel < 1; FG_E_LIMIT: n C >= 2^31; FG_E_STATE: a statement whose collected
 * cells differ from the select's count (never a figure).  Synchronous; reads engine state and changes none. */
int     fg_psis_loo(fg_engine *e, const double *d_ll, int n, int n_sel, double *h_figures, int64_t *h_counts, double *d_tail_or_null);
/* ------------------------------------------------------------------ rank-normalised R-hat and bulk / tail ESS
 * Vehtari, Gelman, Simpson, Carpenter, Buerkner (2021), "Rank-normalization, folding, and localization: an improved R-hat for
 * assessing convergence of MCMC" -- what the R `posterior` package and Stan report; the reference has none of it -- of stored draws
 * d_draws [n][d][C] on the device (fg_diag_rank.hip; the rule, the sort and the limits: fg_diag_rank_plan.h and DESIGN 3.23).  Per
 * coordinate the S = n C pooled cells are sorted exactly (a stable radix sort of key and cell index; ties are ties of values: -0.0
 * and +0.0 tie, all NaN tie above +inf); a cell's doubled average rank r2 = lo + hi + 1 gives its normal score
 * z = ndtri((r2 / 2 - 3/8) / (S + 1/4)) (AS241 PPND16), the folded cells |x - median| are sorted again for z_folded, and
 * I_lo / I_hi = 1 where x <= sorted[floor((S - 1) p)].  The figures are the library's own combination -- r_hat_from_f64_chains
 * (diagnostics.rs:262-304) and ess_from_chains (mcmc_utils.rs:253-339), the code behind fg_diag_rhat_ess -- applied to those rows in
 * the original [n][.][C] layout: same transform as `posterior`, the project's own ESS estimator (no split chains, Geyer's sequence as
 * the reference truncates it).  A row of FG_RANK_WORDS doubles per coordinate:
 *   0 rhat_rank = max(1, 2)  1 rhat_bulk (of z)  2 rhat_folded (of z_folded)  3 ess_bulk (of z)  4 ess_tail = min(5, 6)
 *   5 ess_lower (of I_lo)  6 ess_upper (of I_hi)  7 median  8 x_lo = sorted[k_lo]  9 x_hi = sorted[k_hi]
 * and a row of FG_RANK_COUNTS integers:
 *   0 S  1 tie runs (distinct values)  2 the longest run  3 NaN cells  4 -inf cells  5 +inf cells  6 NaN folded cells
 *   7 radix passes run, both sorts together (a pass whose digit is equal in every cell is skipped)
 * +-inf cells are ordinary values.  A NaN cell makes every figure of its coordinate NaN; NaN folded cells (median = +-inf) make
 * rhat_folded and rhat_rank NaN only.  This engine's chains only, no communicator: ranks over the chains of several GPUs need a
 * distributed sort.  Both calls are synchronous, read engine state and change none; every argument is checked before the device is
 * looked for.  FG_E_BAD_ARG: a null pointer, n < 1, d outside [1, 65535], a block outside [0, d), a probability outside [0, 1],
 * p_lo > p_hi, max_out_bytes < 0; FG_E_LIMIT: n C >= 2^31. */
#define FG_RANK_ROWS 4      /* z, z_folded, I_lo, I_hi */
#define FG_RANK_WORDS 10    /* rhat_rank rhat_bulk rhat_folded ess_bulk ess_tail ess_lower ess_upper median x_lo x_hi */
#define FG_RANK_COUNTS 8    /* S, tie runs, longest run, NaN, -inf, +inf cells, NaN folded cells, radix passes run (both sorts) */
int     fg_diag_rank_words(void);                              /* FG_RANK_WORDS of this library */
/* The transform alone (Vehtari et al. 2021, section 4): coordinates [j0, j0 + n_j) of d_draws [n][d][C] -> d_out
 * [n][FG_RANK_ROWS n_j][C] (row 4 k + i: row i of coordinate j0 + k), ready for fg_diag_rhat_ess (diagnostics.rs:262-304,
 * mcmc_utils.rs:253-339); d_rank2_or_null [n][n_j][C] u32 doubled average ranks; h_median [n_j]; h_counts [n_j][FG_RANK_COUNTS]. */
int     fg_diag_rank_transform(fg_engine *e, const double *d_draws, int n, int d, int j0, int n_j, double p_lo, double p_hi,
                               double *d_out, uint32_t *d_rank2_or_null, double *h_median, int64_t *h_counts);
/* The transform block by block (a block: the coordinates whose d_out stays under max_out_bytes, at least one; 0 = 1 GiB), then the
 * combination of fg_diag_rhat_ess (r_hat_from_f64_chains, diagnostics.rs:262-304; ess_from_chains, mcmc_utils.rs:253-339) on each
 * block; h_figures [d][FG_RANK_WORDS], h_counts [d][FG_RANK_COUNTS].  The figures do not depend on the blocks. */
int     fg_diag_rank_rhat_ess(fg_engine *e, const double *d_draws, int n, int d, double p_lo, double p_hi, int64_t max_out_bytes,
                              double *h_figures, int64_t *h_counts);
/* ------------------------------------------------------------------ MCSE and ESS of the mean, the sd and quantiles
 * What `posterior::summarise_draws` reports next to a mean, a standard deviation and a quantile -- mcse_mean, mcse_sd, mcse_quantile,
 * ess_mean, ess_sd, ess_quantile (ess_median: p = 0.5) and mad; the reference has none of it -- of stored draws d_draws [n][d][C] on the
 * device (fg_diag_mcse.hip; the rule, the Beta inverse and the limits: fg_diag_mcse_plan.h and DESIGN 3.24).  Per coordinate: mean,
 * sd, rhat and ess_mean are fg_diag_rhat_ess's own figures of the raw draws; the S = n C pooled cells are sorted as fg_diag_rank_* sort
 * them (same key: -0.0 and +0.0 tie, all NaN tie above +inf); the rows |x - mean|, (x - mean)^2 and, per probability p, I_p = 1 where
 * x <= sorted[floor((S - 1) p)] go through the combination of fg_diag_rhat_ess (r_hat_from_f64_chains, diagnostics.rs:262-304;
 * ess_from_chains, mcmc_utils.rs:253-339) in the original [n][.][C] layout; mcse_sd is Kenney and Keeping's formula, mcse_quantile half
 * the distance of the order statistics at the 15.87 % and 84.13 % points of Beta(ess p + 1, ess (1 - p) + 1), as `posterior` has them.
 * The ESS is the project's estimator (no split chains, Geyer's sequence as the reference truncates it), not Stan's FFT estimator.
 * A row of FG_MCSE_FIXED_WORDS + FG_MCSE_PROB_WORDS n_probs doubles per coordinate:
 *   0 mean  1 sd  2 rhat  3 ess_mean  4 mcse_mean = sd / sqrt(ess_mean)  5 ess_sd (of |x - mean|)  6 ess_sq (of (x - mean)^2)  7 mcse_sd
 *   8 median  9 mad = 1.4826 median |x - median|;  then per probability, in the order given:
 *   q = sorted[k_p]  q7 (the interpolated type-7 quantile)  ess_quantile (of I_p)  mcse_quantile = (th_hi - th_lo) / 2
 *   th_lo = sorted[i_lo]  th_hi = sorted[i_hi]
 * and a row of FG_MCSE_FIXED_COUNTS + FG_MCSE_PROB_COUNTS n_probs integers:
 *   0 S  1 NaN cells  2 -inf cells  3 +inf cells  4 NaN folded cells  5 radix passes run (both sorts);  per probability: k_p  i_lo  i_hi
 * (i_lo = i_hi = -1 and th_lo, th_hi, mcse_quantile NaN where ess_quantile is not finite or not positive).  +-inf cells are ordinary
 * values of the sort; what passes through the mean follows IEEE.  A NaN cell makes every word of its coordinate NaN; NaN folded cells
 * (median = +-inf) make mad NaN.  This engine's chains only.  The calls are synchronous, read engine state and change none; every
 * argument is checked before the device is looked for.  FG_E_BAD_ARG: a null pointer, n < 1, d outside [1, 65535], a block outside
 * [0, d), n_probs outside [1, 8], a probability outside [0, 1], max_out_bytes < 0; FG_E_LIMIT: n C >= 2^31. */
#define FG_MCSE_MAX_PROBS 8
#define FG_MCSE_FIXED_WORDS 10   /* mean sd rhat ess_mean mcse_mean ess_sd ess_sq mcse_sd median mad */
#define FG_MCSE_PROB_WORDS 6     /* q q7 ess_quantile mcse_quantile th_lo th_hi */
#define FG_MCSE_FIXED_COUNTS 6   /* S, NaN, -inf, +inf cells, NaN folded cells, radix passes run (both sorts) */
#define FG_MCSE_PROB_COUNTS 3    /* k_p i_lo i_hi */
int     fg_diag_mcse_words(int n_probs);                       /* the figures' row length; FG_E_BAD_ARG outside [1, 8] */
/* The 0-based positions of mcse_quantile's two order statistics among S sorted cells: i_lo = max(floor(a1 S), 1) - 1 and
 * i_hi = min(ceil(a2 S), S) - 1 with a1, a2 the 0.15865525393145707 and 0.8413447460685429 points of Beta(ess p + 1, ess (1 - p) + 1).
 * Host only, no device.  FG_E_BAD_ARG: a null pointer, S < 1, p outside [0, 1], ess not finite or not positive. */
int     fg_mcse_quantile_ranks(int64_t S, double p, double ess, int64_t *i_lo, int64_t *i_hi);
/* The rows alone: coordinates [j0, j0 + n_j) of d_draws [n][d][C], centred at h_mean [n_j], -> d_out [n][(2 + n_probs) n_j][C] (row
 * (2 + n_probs) k + i: row i of coordinate j0 + k; rows |c|, c c, I_p ...), ready for fg_diag_rhat_ess; d_sorted_or_null [n_j][S] the
 * sorted cells as doubles; h_median [n_j]; h_mad [n_j]; h_counts [n_j][FG_MCSE_FIXED_COUNTS + FG_MCSE_PROB_COUNTS n_probs] (i_lo and
 * i_hi are -1 here: they need the figures). */
int     fg_diag_mcse_transform(fg_engine *e, const double *d_draws, int n, int d, int j0, int n_j, const double *h_mean, const double *h_probs,
                               int n_probs, double *d_out, double *d_sorted_or_null, double *h_median, double *h_mad, int64_t *h_counts);
/* Every figure, block by block (a block: the coordinates whose rows and sorted keys stay under max_out_bytes, at least one; 0 = 1 GiB);
 * h_figures [d][fg_diag_mcse_words(n_probs)], h_counts [d][FG_MCSE_FIXED_COUNTS + FG_MCSE_PROB_COUNTS n_probs].  The figures do not
 * depend on the blocks. */
int     fg_diag_mcse(fg_engine *e, const double *d_draws, int n, int d, const double *h_probs, int n_probs, int64_t max_out_bytes,
                     double *h_figures, int64_t *h_counts);
/* ------------------------------------------------------------------ bootstrap particle filter bank
 * WasmParticleFilter (crates/fugue-wasm/src/pf.rs): a 1-D bootstrap filter on the random-walk model x_0 ~ N(0, prior_sig),
 * x_t = x_{t-1} + N(0, sig_step), y_t ~ N(x_t, sig_obs), systematic resampling when ESS / n < ess_threshold, the running log-evidence.
 * A bank is B independent filters of n particles each, one workgroup per filter, T steps in one launch (fg_pf.hip).
 * No program and no engine: a device ordinal, as the fg_device_* calls.  Parameters are clamped as pf.rs:82-94 clamps them (each
 * sigma .max(1e-6), the threshold .clamp(0, 1)); n is NOT clamped here: below 2 is FG_E_BAD_ARG, above the cap of one workgroup's
 * LDS (at least the reference's 5000) FG_E_LIMIT.  Random numbers: the stream (seed, particle, time, FG_RNG_PF = 11), time 0 the
 * initial draw, time t the transition into t; the resampling uniform of step t is the first of (seed, 0, t, FG_RNG_PF_RESAMPLE = 12).
 * Every argument is checked before the device is touched: null handles and arrays, n_filters < 1, T < 0, per_filter outside {0, 1},
 * a non-finite parameter or observation are FG_E_BAD_ARG.  Synchronous.  fg_pf_t counts the steps whose launch was accepted; after
 * FG_E_HIP from a run or a step the state on the device is undefined and the handle is only good for fg_pf_free. */
typedef struct fg_pf fg_pf;
typedef struct fg_pf_params { double prior_sig, sig_step, sig_obs, ess_threshold; uint64_t seed; } fg_pf_params;
/* pf.rs:74-98: params [n_filters]; draws the initial populations */
int  fg_pf_new(int device_ordinal, int64_t n_particles, int64_t n_filters, const fg_pf_params *params, fg_pf **out);
/* pf.rs:101-103: filter in [0, n_filters), or -1 for every filter */
int  fg_pf_set_sig_obs(fg_pf *pf, int64_t filter, double sig_obs);
/* pf.rs:107-172, T times: h_obs [T] shared by the filters (per_filter 0) or [n_filters][T] (per_filter 1); the summaries of every
 * step, each [T][n_filters], any may be NULL: ess_frac, log_z_inc, resampled, and the weighted mean and variance of the propagated
 * particles under the normalised weights (before resampling). */
int  fg_pf_run(fg_pf *pf, const double *h_obs, int64_t T, int per_filter, double *h_ess_frac, double *h_log_z_inc, int32_t *h_resampled,
               double *h_mean, double *h_var);
/* pf.rs:107-172, one step: h_obs [1] or [n_filters]; the summaries [n_filters]; StepOut's arrays, each [n_filters][n], any may be NULL.
 * The same kernel as fg_pf_run and the same bits. */
int  fg_pf_step(fg_pf *pf, const double *h_obs, int per_filter, double *h_ess_frac, double *h_log_z_inc, int32_t *h_resampled, double *h_mean,
                double *h_var, double *h_prev, double *h_propagated, double *h_weights, int64_t *h_parents, double *h_posterior);
int  fg_pf_log_evidence(fg_pf *pf, double *h_out);             /* pf.rs:175-177: h_out [n_filters] */
int64_t fg_pf_t(const fg_pf *pf);                              /* pf.rs:180-182: steps taken (-1 for a null handle) */
int  fg_pf_positions(fg_pf *pf, double *h_x);                  /* pf.rs:169: h_x [n_filters][n] */
void fg_pf_free(fg_pf *pf);                                    /* pf.rs:60-68 */
/* ------------------------------------------------------------------ log-joint surfaces over one or two sites
 * log_joint_grid (crates/fugue-wasm/src/grid.rs): for two f64 sample sites and axes a_values [n_a], b_values [n_b], cell (j, i) is
 * the total log weight (prior + likelihood + factors, as lj_out of a scoring run) of a base trace with a := a_values[i] and then
 * b := b_values[j] (the same site twice: b wins), row-major out[j * n_a + i].  A base is an engine chain; the engine's values, its
 * log-joint and every other state word are read only.  Axis values are scored as given: a non-finite or out-of-support value gives
 * what ScoreGivenTrace gives, never an error.  Per base the handle keeps (n_a + n_b + 6 words on the host) log_marg_a[i] =
 * log_sum_exp of column i, log_marg_b[j] = log_sum_exp of row j, log_norm = log_sum_exp of the row marginals (numerical.rs:15-38,
 * rule for rule), the maximum and its flat index by the fold of wasm.rs:115-124 (strict > from -inf: the first maximum, NaN never
 * wins, -1 when no cell exceeds -inf) and the counts of NaN, -inf and +inf cells; over the bases that arrive it accumulates
 * mix[cell] += exp(lj[c][cell] - log_norm[c]) for the bases of finite log_norm, in arrival order.  Every sum's order is a function
 * of (n_a, n_b) alone (fg_grid_plan.h): a base gives the same bits alone or in a bank, under any base_chunk, in one
 * call or several, with or without d_out.  Synchronous on the engine's stream.  Free the handle before its engine. */
typedef struct fg_grid fg_grid;
/* grid.rs:22-46: site_a / site_b sorted site indices (site_b == -1: one axis, h_b and n_b ignored, n_b = 1); h_a [n_a], h_b [n_b];
 * base_chunk = bases per launch and chunk table (0: the largest that keeps the table under 256 MiB, at least 1).  FG_E_BAD_ARG: a
 * site that is not an f64 sample site (the reference's message), n_a or n_b < 1, base_chunk < 0, a null axis.  FG_E_LIMIT: 2^31
 * cells or more; a program whose tile lives in global memory. */
int  fg_grid_new(fg_engine *e, int site_a, int site_b, const double *h_a, int64_t n_a, const double *h_b, int64_t n_b, int64_t base_chunk,
                 fg_grid **out);
/* grid.rs:48-67 for the bases = engine chains [chain0, chain0 + n_bases) (FG_E_BAD_ARG unless 0 <= chain0, 1 <= n_bases and
 * chain0 + n_bases <= n_chains): d_out [n_bases][n_b][n_a] and d_acc [3][n_bases][n_b][n_a] (prior, likelihood, factors) are device
 * tables of the caller, either may be NULL. */
int  fg_grid_eval(fg_grid *g, int64_t chain0, int64_t n_bases, double *d_out, double *d_acc);
/* grid.rs:48-67, wasm.rs:115-124: per base that has arrived (n = fg_grid_count), any may be NULL: h_log_norm [n], h_max [n],
 * h_argmax [n], h_counts [n][3] = n_nan, n_neg_inf, n_pos_inf.  FG_E_STATE before any base has arrived (the three read-outs). */
int  fg_grid_summary(fg_grid *g, double *h_log_norm, double *h_max, int64_t *h_argmax, int64_t *h_counts);
int  fg_grid_marginals(fg_grid *g, double *h_log_marg_a, double *h_log_marg_b);   /* grid.rs:48-67: [n][n_a], [n][n_b]; either may be NULL */
/* grid.rs:48-67: h_log_mix [n_b][n_a] = ln(mix / n_mixed) (NaN when n_mixed is 0); the bases mixed and skipped; any may be NULL */
int  fg_grid_mixture(fg_grid *g, double *h_log_mix, int64_t *n_mixed, int64_t *n_skipped);
int64_t fg_grid_count(const fg_grid *g);                       /* grid.rs:48-67: bases that have arrived (-1 for a null handle) */
void fg_grid_free(fg_grid *g);                                 /* grid.rs:22-69 */
/* ------------------------------------------------------------------ exact Gibbs moves of the discrete sites
 * hmc.rs:68-71: HMC moves the f64 sites only and holds every discrete site at its prior draw ("compose with `mh` to also move
 * discrete sites").  A sweep is that composition with the exact conditional in place of a blind proposal: for every chain and every
 * listed site, in list order, the trace is scored (the run fg_log_joint does, bit for bit) at every value of the site's finite
 * support, the scores are normalised and the site's new value is drawn from them with the (i + 1)-th uniform of the stream (seed,
 * chain_offset + chain, sweep index, 13).  The rule, the summation orders and the refusals: fg_gibbs_plan.h, DESIGN 3.25.  Chain c's
 * sweep t gives the same bits alone or among any number of chains, under any cut of the chains into engines, in one call of several
 * sweeps or in several calls.  The conditional probabilities are summed per (cell, chain) -- cell = cell0 of the site + the value's
 * index -- and pooled over the chains on a fixed tree: the Rao-Blackwell estimate of P(site = value | data).  Asynchronous on the
 * engine's stream unless a host pointer is written.  Free the handle before its engine. */
#define FG_GIBBS_K_CAP 4096          /* values of one site's support */
#define FG_GIBBS_COUNTS 4            /* per site: moved, stuck, nan_cells, neg_inf_cells */
typedef struct fg_gibbs fg_gibbs;
/* hmc.rs:68-71: the support of sorted site `site` where constants alone state it: returns 1 and [*lo, *hi] for Bernoulli [0, 1],
 * Categorical of K probabilities [0, K - 1] (whatever their values), DiscreteUniform with constant bounds lo <= hi, Binomial with a
 * constant valid n [0, n]; 0 otherwise (Poisson, f64 sites, bounds that read a site; *lo and *hi are left alone).  FG_E_BAD_ARG: a
 * site outside [0, S), a null pointer. */
int  fg_program_site_support(const fg_program *p, int site, int64_t *lo, int64_t *hi);
/* hmc.rs:68-71: h_sites [n_sites] sorted site indices in visiting order; n_sites == 0: every site for which fg_program_site_support
 * returns 1 with at most FG_GIBBS_K_CAP values, in site order.  Arguments are checked before the device is looked for.  FG_E_BAD_ARG
 * (the message names the site): a site that is not discrete, a site without a finite constant support, a site listed twice,
 * n_sites < 0, a null pointer, an empty resulting list.  FG_E_LIMIT: a listed site with more than FG_GIBBS_K_CAP values; a program
 * whose tile lives in global memory. */
int  fg_gibbs_new(fg_engine *e, const int32_t *h_sites, int n_sites, fg_gibbs **out);
int  fg_gibbs_n_sites(const fg_gibbs *g);                      /* hmc.rs:68-71: listed sites G (FG_E_BAD_ARG for a null handle) */
int64_t fg_gibbs_n_cells(const fg_gibbs *g);                   /* hmc.rs:68-71: the sum of their K (-1 for a null handle) */
/* hmc.rs:68-71: per listed site, any may be NULL: h_site [G], h_lo [G], h_K [G], h_cell0 [G] */
int  fg_gibbs_layout(const fg_gibbs *g, int32_t *h_site, int64_t *h_lo, int32_t *h_K, int64_t *h_cell0);
/* hmc.rs:68-71: n_sweeps sweeps with the sweep indices count, count + 1, ...; one launch each.  d_rec (device, may be NULL)
 * [n_sweeps][n_rec][C]: the 8-byte cells of the sites h_rec_sites (any sites of the program) after each sweep.  d_scores and d_cond
 * (device, either may be NULL) [cells][C]: the scores and the conditional probabilities of the call's last sweep; the cells of a stuck
 * site hold NaN in d_cond.  After the last sweep the cached log-joint of a live HMC / MH session is re-scored as fg_engine_set_values
 * does.  FG_E_BAD_ARG: n_sweeps < 0, n_rec < 0, a recorded site outside [0, S), d_rec without sites; FG_E_LIMIT: the sweep index would
 * pass 2^32. */
int  fg_gibbs_sweep(fg_gibbs *g, int n_sweeps, const int32_t *h_rec_sites, int n_rec, int64_t *d_rec, double *d_scores, double *d_cond);
int64_t fg_gibbs_count(const fg_gibbs *g);                     /* hmc.rs:68-71: the sweep index of the next sweep (-1 for a null handle) */
int  fg_gibbs_seek(fg_gibbs *g, int64_t t);                    /* hmc.rs:68-71: sets it; FG_E_BAD_ARG outside [0, 2^32) */
/* hmc.rs:68-71: h_counts [G][FG_GIBBS_COUNTS] = moved, stuck, nan_cells, neg_inf_cells summed over the chains and the sweeps run */
int  fg_gibbs_stats(fg_gibbs *g, int64_t *h_counts);
/* hmc.rs:68-71: h_mean [cells] = the tree-pooled probability sums divided by the contributing (sweep, chain) pairs of the cell's site
 * (NaN when there is none), h_n [G] = those pairs (sweeps run x C - stuck); either may be NULL.  FG_E_STATE before any sweep has run. */
int  fg_gibbs_probs(fg_gibbs *g, double *h_mean, int64_t *h_n);
void fg_gibbs_free(fg_gibbs *g);                               /* hmc.rs:68-71 */
/* RCCL communicator of the ranks of one run (one process per GPU): rank 0 obtains a 128-byte id (ncclGetUniqueId), the
 * host distributes it by any means, every rank calls fg_comm_init.  RCCL is bound at run time (librccl.so). */
int fg_comm_unique_id(void *out_128_bytes);
int fg_comm_init(fg_engine *e, int world_size, int rank, const void *unique_id_128_bytes, void **out_comm);
int fg_comm_destroy(void *comm);

/* raw device memory helpers so a host without a HIP binding can own draw buffers */
void *fg_device_alloc(fg_engine *e, size_t bytes);
int   fg_device_free(fg_engine *e, void *d_ptr);
int   fg_device_download(fg_engine *e, void *h_dst, const void *d_src, size_t bytes);
int   fg_device_upload(fg_engine *e, void *d_dst, const void *h_src, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* FUGUE_AMD_H */
