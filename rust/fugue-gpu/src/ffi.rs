//! `extern "C"` view of `include/fugue_amd.h` (ABI version 1).  Every `c_int` result is 0, a reference `ErrorCode` value
//! (`src/error.rs:40-59`) or a negative `FG_E_*`; `fg_last_error()` carries the message.
//! UNVERIFIED SOURCE -- never compiled.
#![allow(non_camel_case_types, dead_code)]
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)] pub struct fg_program { _p: [u8; 0] }
#[repr(C)] pub struct fg_engine { _p: [u8; 0] }
#[repr(C)] pub struct fg_diag_stream { _p: [u8; 0] }
#[repr(C)] pub struct fg_diag_qstream { _p: [u8; 0] }
#[repr(C)] pub struct fg_diag_cstream { _p: [u8; 0] }
#[repr(C)] pub struct fg_loglik_stream { _p: [u8; 0] }
#[repr(C)] pub struct fg_ppc_stream { _p: [u8; 0] }
#[repr(C)] pub struct fg_wpop { _p: [u8; 0] }
#[repr(C)] pub struct fg_abc { _p: [u8; 0] }
#[repr(C)] pub struct fg_pf { _p: [u8; 0] }
#[repr(C)] pub struct fg_grid { _p: [u8; 0] }
#[repr(C)] pub struct fg_gibbs { _p: [u8; 0] }

pub const FG_E_NO_DEVICE: c_int = -1;
pub const FG_E_HIP: c_int = -2;
pub const FG_E_BAD_ARG: c_int = -3;
pub const FG_E_STATE: c_int = -5;
pub const FG_E_UNSUPPORTED: c_int = -6;
pub const FG_E_LIMIT: c_int = -7;

// expression tokens (postfix), include/fugue_amd.h FG_T_*
pub const FG_T_CONST: i32 = 0;
pub const FG_T_SITE: i32 = 1;
pub const FG_T_ADD: i32 = 12;
pub const FG_T_MUL: i32 = 14;
pub const FG_T_SELECT: i32 = 20;

// value types (ChoiceValue tags) and gradient modes
pub const FG_F64: c_int = 0;
pub const FG_BOOL: c_int = 1;
pub const FG_U64: c_int = 2;
pub const FG_USIZE: c_int = 3;
pub const FG_I64: c_int = 4;
pub const FG_GRAD_FD_DENSE: i32 = 0;
pub const FG_GRAD_FD_SPARSE: i32 = 1;

#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct fg_tok { pub op: i32, pub a: i32, pub b: i32, pub reserved: i32, pub imm: f64 }

#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct fg_hmc_config {
    pub n_leapfrog: i32, pub target_accept: f64, pub init_step_size: f64 /* NaN = None */,
    pub finite_diff_eps: f64, pub adapt_mass: i32, pub grad_mode: i32,
}
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct fg_hmc_stats { pub accept_rate: f64, pub mean_step_size: f64, pub n_divergent: i64, pub n_transitions: i64 }
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct fg_site_proposal { pub kind: i32, pub lower: f64, pub upper: f64 }
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct fg_mh_stats { pub accept_rate: f64, pub n_steps: i64 }
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct fg_smc_config { pub resampling_method: i32, pub ess_threshold: f64, pub rejuvenation_steps: i32, pub sequential_adaptation: i32 }
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct fg_smc_result { pub log_evidence: f64, pub n_steps: i32, pub n_model_runs: i64 }
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct fg_vi_factor { pub family: i32, pub site: i32, pub a: f64, pub b: f64 }
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct fg_vi_config { pub n_iterations: i32, pub convergence_window: i32, pub base_learning_rate: f64, pub fd_eps: f64, pub convergence_tol: f64, pub step_decay_exponent: f64 }
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct fg_vi_result { pub converged: i32, pub iterations: i32 }
#[repr(C)] #[derive(Clone, Copy, Debug)]
pub struct fg_pf_params { pub prior_sig: f64, pub sig_step: f64, pub sig_obs: f64, pub ess_threshold: f64, pub seed: u64 }

pub type fg_acov_fn = Option<unsafe extern "C" fn(user: *mut c_void, lag0: c_int, n_lags: c_int, h_sums: *mut f64) -> c_int>;
pub type fg_reduce_fn = Option<unsafe extern "C" fn(user: *mut c_void, stage: c_int, h_in: *const f64, h_out: *mut f64) -> c_int>;
pub const FG_DIAG_REDUCE: c_int = 0;
pub const FG_DIAG_GATHER: c_int = 1;

#[link(name = "fugue_amd")]
extern "C" {
    pub fn fg_last_error() -> *const c_char;
    pub fn fg_abi_version() -> c_int;
    // ---- site programs (replaces Model<A> + Handler + run: model.rs:20-131, handler.rs:29-209)
    pub fn fg_program_new() -> *mut fg_program;
    pub fn fg_program_free(p: *mut fg_program);
    pub fn fg_program_data(p: *mut fg_program, name: *const c_char, v: *const f64, n: i64) -> c_int;
    pub fn fg_program_sample(p: *mut fg_program, addr: *const c_char, dist: c_int, toks: *const fg_tok, param_len: *const i32, n_params: c_int) -> c_int;
    pub fn fg_program_sample_discrete_uniform(p: *mut fg_program, addr: *const c_char, lo: i64, hi: i64) -> c_int;
    pub fn fg_program_observe(p: *mut fg_program, addr: *const c_char, dist: c_int, toks: *const fg_tok, param_len: *const i32, n_params: c_int,
                              value: *const fg_tok, n_value: c_int) -> c_int;
    pub fn fg_program_factor(p: *mut fg_program, toks: *const fg_tok, n: c_int) -> c_int;
    pub fn fg_program_finalize(p: *mut fg_program) -> c_int;
    pub fn fg_program_n_sites(p: *const fg_program) -> c_int;
    pub fn fg_program_n_f64(p: *const fg_program) -> c_int;
    pub fn fg_program_n_observe(p: *const fg_program) -> c_int;
    pub fn fg_program_site_name(p: *const fg_program, j: c_int, buf: *mut c_char, len: c_int) -> c_int;
    pub fn fg_program_site_vtype(p: *const fg_program, j: c_int) -> c_int;
    pub fn fg_program_site_of_handle(p: *const fg_program, h: c_int) -> c_int;
    pub fn fg_program_f64_site(p: *const fg_program, k: c_int) -> c_int;
    pub fn fg_program_stream_records(p: *const fg_program, which: c_int) -> c_int;
    // observe statements in program order (the rows of fg_predict_eval)
    pub fn fg_program_observe_name(p: *const fg_program, k: c_int, buf: *mut c_char, buf_len: c_int) -> c_int;
    pub fn fg_program_observe_vtype(p: *const fg_program, k: c_int) -> c_int;
    pub fn fg_program_observe_dist(p: *const fg_program, k: c_int) -> c_int;
    pub fn fg_program_observe_value(p: *const fg_program, k: c_int, out: *mut f64) -> c_int;
    // the model's return value, `A` of Model<A> (model.rs `pure`; hmc.rs:566-583 returns it with every trace)
    pub fn fg_program_result(p: *mut fg_program, name_utf8: *const c_char, toks: *const fg_tok, n: c_int) -> c_int;
    pub fn fg_program_n_results(p: *const fg_program) -> c_int;
    pub fn fg_program_result_name(p: *const fg_program, r: c_int, buf: *mut c_char, buf_len: c_int) -> c_int;
    pub fn fg_program_result_sites(p: *const fg_program, h_sites: *mut i32, cap: c_int) -> c_int;
    pub fn fg_dsl_compile(source_utf8: *const c_char, data_json_utf8: *const c_char) -> *mut fg_program;
    // ---- engine
    pub fn fg_engine_new(p: *const fg_program, n_chains: i64, seed: u64, chain_offset: u32, device: c_int) -> *mut fg_engine;
    pub fn fg_engine_free(e: *mut fg_engine);
    pub fn fg_engine_synchronize(e: *mut fg_engine) -> c_int;
    pub fn fg_engine_set_values(e: *mut fg_engine, h_cells: *const c_void) -> c_int;
    pub fn fg_engine_get_values(e: *mut fg_engine, h_cells: *mut c_void) -> c_int;
    pub fn fg_prior_init(e: *mut fg_engine, iteration: u32, h_acc: *mut f64) -> c_int;
    pub fn fg_log_joint(e: *mut fg_engine, h_acc: *mut f64, h_logp: *mut f64) -> c_int;
    pub fn fg_result_eval(e: *mut fg_engine, d_draws: *const c_void, n: c_int, h_rows: *const i32, n_rows: c_int, d_out: *mut f64) -> c_int;
    // posterior / prior predictive draws of the observe statements and their pointwise log-likelihood (inference_integration.rs:717-740)
    pub fn fg_predict_eval(e: *mut fg_engine, d_draws: *const c_void, n: c_int, h_rows: *const i32, n_rows: c_int, iter0: u32,
                           h_sel: *const i32, n_sel: c_int, d_yrep: *mut c_void, d_loglik: *mut f64) -> c_int;
    // ---- ABC (abc.rs:132-226 the distances, :776-799 the kernel mixture of weighted ABC-SMC)
    pub fn fg_abc_distance(e: *mut fg_engine, d_sim: *const f64, k: c_int, b: i64, h_observed: *const f64, n_observed: c_int, kind: c_int,
                           h_weights: *const f64, n_weights: c_int, d_dist: *mut f64) -> c_int;
    pub fn fg_abc_mixture(e: *mut fg_engine, d_x: *const f64, m: i64, d_centers: *const f64, n: i64, d: c_int, h_weights: *const f64,
                          h_std: *const f64, d_out: *mut f64) -> c_int;
    // rounds of attempts and the stages of abc_smc_weighted (abc.rs:283-325, 520-650)
    pub fn fg_abc_new(e: *mut fg_engine, sim_kind: c_int, h_sel: *const i32, n_sel: c_int, h_observed: *const f64, n_observed: c_int, kind: c_int,
                      h_weights: *const f64, n_weights: c_int, capacity: i64, out: *mut *mut fg_abc) -> c_int;
    pub fn fg_abc_free(a: *mut fg_abc);
    pub fn fg_abc_round_prior(a: *mut fg_abc, tol: f64, budget: i64, accepted: *mut i64, attempts: *mut i64) -> c_int;
    pub fn fg_abc_stage_begin(a: *mut fg_abc) -> c_int;
    pub fn fg_abc_round_stage(a: *mut fg_abc, stage: u32, tol: f64, budget: i64, accepted: *mut i64, attempts: *mut i64) -> c_int;
    pub fn fg_abc_stage_end(a: *mut fg_abc) -> c_int;
    pub fn fg_abc_last_round(a: *mut fg_abc, h_index: *mut i64, h_dist: *mut f64, h_log_prior: *mut f64, h_accept: *mut i32) -> c_int;
    pub fn fg_abc_get_population(a: *mut fg_abc, which: c_int, out_n: *mut i64, h_cells: *mut c_void, h_weights: *mut f64, h_dist: *mut f64,
                                 h_attempt: *mut i64, h_log_prior: *mut f64, h_log_denom: *mut f64) -> c_int;
    pub fn fg_abc_set_population(a: *mut fg_abc, n: i64, h_cells: *const c_void, h_weights: *const f64, h_dist: *const f64, h_attempt: *const i64,
                                 h_log_prior: *const f64, h_log_denom: *const f64) -> c_int;
    // ---- HMC (hmc.rs:566-583, 643-920)
    pub fn fg_hmc_config_default(cfg: *mut fg_hmc_config);
    pub fn fg_hmc_init(e: *mut fg_engine, cfg: *const fg_hmc_config, n_warmup: c_int) -> c_int;
    pub fn fg_hmc_step(e: *mut fg_engine, n: c_int, d_draws: *mut f64) -> c_int;
    pub fn fg_hmc_step_info(e: *mut fg_engine, n: c_int, d_positions: *mut f64, d_info: *mut f64) -> c_int;
    pub fn fg_hmc_step_recorded(e: *mut fg_engine, n_recorded: c_int, h_chain_ids: *const i64, h_traj: *mut f64, h_ham: *mut f64,
                                h_n_points: *mut i32, d_info: *mut f64) -> c_int;
    pub fn fg_hmc_run(e: *mut fg_engine, cfg: *const fg_hmc_config, n_samples: c_int, n_warmup: c_int, d_draws: *mut f64, stats: *mut fg_hmc_stats) -> c_int;
    pub fn fg_hmc_get_stats(e: *mut fg_engine, stats: *mut fg_hmc_stats) -> c_int;
    pub fn fg_hmc_get_step_sizes(e: *mut fg_engine, h_eps: *mut f64) -> c_int;
    pub fn fg_hmc_set_step_size(e: *mut fg_engine, eps: f64) -> c_int;
    pub fn fg_hmc_set_n_leapfrog(e: *mut fg_engine, n_leapfrog: c_int) -> c_int;
    pub fn fg_hmc_is_warming_up(e: *const fg_engine) -> c_int;
    pub fn fg_hmc_iterations(e: *const fg_engine) -> i64;
    pub fn fg_hmc_short_quotient(e: *const fg_engine) -> c_int;
    pub fn fg_hmc_range_proved(e: *const fg_engine) -> c_int;
    pub fn fg_hmc_last_kernel(e: *const fg_engine) -> *const c_char;
    pub fn fg_mh_last_kernel(e: *const fg_engine) -> *const c_char;
    // ---- single-site MH (mh.rs:921-1014)
    pub fn fg_mh_init(e: *mut fg_engine, n_warmup: c_int, overrides: *const fg_site_proposal) -> c_int;
    pub fn fg_mh_step(e: *mut fg_engine, n: c_int, rec_sites: *const i32, n_rec: c_int, d_draws: *mut c_void) -> c_int;
    pub fn fg_mh_set_recording(e: *mut fg_engine, during_adaptation: c_int) -> c_int;
    pub fn fg_mh_run(e: *mut fg_engine, n_samples: c_int, n_warmup: c_int, overrides: *const fg_site_proposal, rec_sites: *const i32, n_rec: c_int,
                     d_draws: *mut c_void, stats: *mut fg_mh_stats) -> c_int;
    // ---- SMC (smc.rs:230-349, 455-790)
    pub fn fg_smc_config_default(cfg: *mut fg_smc_config);
    pub fn fg_smc_run(e: *mut fg_engine, cfg: *const fg_smc_config, h_log_w: *mut f64, h_weights: *mut f64, res: *mut fg_smc_result,
                      h_betas: *mut f64, max_betas: c_int) -> c_int;
    pub fn fg_smc_prior_particles(e: *mut fg_engine, iteration: u32) -> c_int;
    pub fn fg_smc_normalize(e: *mut fg_engine) -> c_int;
    pub fn fg_smc_ess(e: *mut fg_engine, out: *mut f64) -> c_int;
    pub fn fg_smc_resample(e: *mut fg_engine, method: c_int, step: u32, h_indices: *mut i64) -> c_int;
    pub fn fg_smc_rejuvenate(e: *mut fg_engine, beta: f64, steps: c_int, first_move_id: u32, h_accept_rate: *mut f64) -> c_int;
    pub fn fg_smc_get_weights(e: *mut fg_engine, h_log_w: *mut f64, h_w: *mut f64) -> c_int;
    pub fn fg_smc_set_log_weights(e: *mut fg_engine, h_log_w: *const f64) -> c_int;
    // ---- cross-chain diagnostics (diagnostics.rs:218-304, mcmc_utils.rs:214-421)
    pub fn fg_diag_rhat_ess(e: *mut fg_engine, d_draws: *const f64, n: c_int, d: c_int, rccl_comm: *mut c_void, h_rhat: *mut f64, h_ess: *mut f64,
                            h_mean: *mut f64, h_std: *mut f64, total_chains: *mut i64) -> c_int;
    pub fn fg_diag_geweke(e: *mut fg_engine, d_draws: *const f64, n: c_int, d: c_int, d_z: *mut f64) -> c_int;
    pub fn fg_diag_combine(h_moments: *const f64, m: i64, n: c_int, d: c_int, acov: fg_acov_fn, user: *mut c_void, h_rhat: *mut f64, h_ess: *mut f64,
                           h_mean: *mut f64, h_std: *mut f64) -> c_int;
    pub fn fg_diag_combine_reduced(m: i64, n: c_int, d: c_int, reduce: fg_reduce_fn, acov: fg_acov_fn, user: *mut c_void, h_rhat: *mut f64, h_ess: *mut f64,
                                   h_mean: *mut f64, h_std: *mut f64) -> c_int;
    pub fn fg_diag_quantiles(e: *mut fg_engine, d_draws: *const f64, n: c_int, d: c_int, rccl_comm: *mut c_void, h_probs: *const f64, n_probs: c_int,
                             h_out: *mut f64) -> c_int;
    pub fn fg_diag_set_exchange(e: *mut fg_engine, mode: c_int) -> c_int;
    // ---- the same figures without stored draws, one chunk at a time (fg_diag_stream.hip)
    pub fn fg_diag_stream_new(e: *mut fg_engine, n_total: c_int, d: c_int, max_lag: c_int, out: *mut *mut fg_diag_stream) -> c_int;
    pub fn fg_diag_stream_update(s: *mut fg_diag_stream, d_draws: *const f64, n_chunk: c_int) -> c_int;
    pub fn fg_diag_stream_count(s: *const fg_diag_stream) -> c_int;
    pub fn fg_diag_stream_moments(s: *mut fg_diag_stream, d_moments: *mut f64) -> c_int;
    pub fn fg_diag_stream_autocov_sums(s: *mut fg_diag_stream, lag0: c_int, n_lags: c_int, h_sums: *mut f64) -> c_int;
    pub fn fg_diag_stream_rhat_ess(s: *mut fg_diag_stream, rccl_comm: *mut c_void, h_rhat: *mut f64, h_ess: *mut f64, h_mean: *mut f64,
                                   h_std: *mut f64, out_total_chains: *mut i64) -> c_int;
    pub fn fg_diag_stream_free(s: *mut fg_diag_stream);
    // ---- quantiles without stored draws: exact radix select over replayed passes (fg_diag_qstream.hip)
    pub fn fg_diag_qstream_new(e: *mut fg_engine, n_total: c_int, d: c_int, h_probs: *const f64, n_probs: c_int, digit_bits: c_int, capacity: i64,
                               out: *mut *mut fg_diag_qstream) -> c_int;
    pub fn fg_diag_qstream_update(s: *mut fg_diag_qstream, d_draws: *const f64, n_chunk: c_int) -> c_int;
    pub fn fg_diag_qstream_count(s: *const fg_diag_qstream) -> c_int;
    pub fn fg_diag_qstream_end_pass(s: *mut fg_diag_qstream, out_done: *mut c_int) -> c_int;
    pub fn fg_diag_qstream_passes(s: *const fg_diag_qstream) -> c_int;
    pub fn fg_diag_qstream_result(s: *mut fg_diag_qstream, h_out: *mut f64, h_slot_passes: *mut i32) -> c_int;
    pub fn fg_diag_qstream_free(s: *mut fg_diag_qstream);
    // ---- discrete sites without stored draws: exact frequency tables and the gather into f64 rows (fg_diag_cstream.hip)
    pub fn fg_diag_cstream_new(e: *mut fg_engine, n_total: c_int, n_rec: c_int, h_rows: *const i32, h_vtypes: *const i32, h_lo: *const i64,
                               h_bins: *const i32, n_watch: c_int, out: *mut *mut fg_diag_cstream) -> c_int;
    pub fn fg_diag_cstream_update(s: *mut fg_diag_cstream, d_cells: *const c_void, n_chunk: c_int) -> c_int;
    pub fn fg_diag_cstream_count(s: *const fg_diag_cstream) -> c_int;
    pub fn fg_diag_cstream_result(s: *mut fg_diag_cstream, h_counts: *mut u64, h_below: *mut u64, h_above: *mut u64, h_min: *mut i64,
                                  h_max: *mut i64) -> c_int;
    pub fn fg_diag_cstream_free(s: *mut fg_diag_cstream);
    pub fn fg_diag_cells_f64(e: *mut fg_engine, d_cells: *const c_void, n: c_int, n_rec: c_int, h_rows: *const i32, h_vtypes: *const i32,
                             n_sel: c_int, d_out: *mut f64) -> c_int;
    // ---- WAIC / importance-sampling LOO from a streamed pointwise log-likelihood table (fg_loglik_stream.hip)
    pub fn fg_loglik_stream_new(e: *mut fg_engine, n_total: c_int, n_sel: c_int, out: *mut *mut fg_loglik_stream) -> c_int;
    pub fn fg_loglik_stream_update(s: *mut fg_loglik_stream, d_loglik: *const f64, n_chunk: c_int) -> c_int;
    pub fn fg_loglik_stream_count(s: *const fg_loglik_stream) -> c_int;
    pub fn fg_loglik_stream_pooled(s: *mut fg_loglik_stream, h_words: *mut f64, h_counts: *mut i64) -> c_int;
    pub fn fg_loglik_stream_result(s: *mut fg_loglik_stream, h_figures: *mut f64, h_counts: *mut i64) -> c_int;
    pub fn fg_loglik_stream_free(s: *mut fg_loglik_stream);
    // ---- posterior predictive checks from a streamed replicate table (fg_ppc_stream.hip)
    pub fn fg_ppc_stream_new(e: *mut fg_engine, n_total: c_int, n_rows: c_int, h_vtypes: *const i32, n_checks: c_int, h_offsets: *const i32,
                             h_members: *const i32, h_stat_mask: *const i32, h_observed: *const f64, out: *mut *mut fg_ppc_stream) -> c_int;
    pub fn fg_ppc_stream_update(s: *mut fg_ppc_stream, d_yrep: *const c_void, n_chunk: c_int) -> c_int;
    pub fn fg_ppc_stream_count(s: *const fg_ppc_stream) -> c_int;
    pub fn fg_ppc_stream_n_slots(s: *const fg_ppc_stream) -> c_int;
    pub fn fg_ppc_stream_observed(s: *const fg_ppc_stream, h_t_obs: *mut f64) -> c_int;
    pub fn fg_ppc_stream_pooled(s: *mut fg_ppc_stream, h_counts: *mut i64, h_moments: *mut f64) -> c_int;
    pub fn fg_ppc_stream_chains(s: *mut fg_ppc_stream, slot: c_int, h_counts: *mut i64) -> c_int;
    pub fn fg_ppc_stream_free(s: *mut fg_ppc_stream);
    // ---- weighted populations on the device (fg_wpop.hip): what abc.rs:476 / smc.rs:445-453 do on the host
    pub fn fg_wpop_new(e: *mut fg_engine, n: i64, d_w: *const f64, out: *mut *mut fg_wpop) -> c_int;
    pub fn fg_wpop_units(h: *const fg_wpop, out_t: *mut u64, out_n_bad: *mut u64, out_n_zero: *mut u64) -> c_int;
    pub fn fg_wpop_moments(h: *mut fg_wpop, d_x: *const f64, d: c_int, h_out: *mut f64) -> c_int;
    pub fn fg_wpop_quantiles(h: *mut fg_wpop, d_x: *const f64, d: c_int, h_probs: *const f64, n_probs: c_int, digit_bits: c_int, capacity: i64,
                             h_out: *mut f64, h_passes: *mut i32) -> c_int;
    pub fn fg_wpop_counts(h: *mut fg_wpop, d_cells: *const c_void, n_rows: c_int, h_vtypes: *const i32, h_lo: *const i64, h_bins: *const i32,
                          h_units: *mut u64, h_below: *mut u64, h_above: *mut u64, h_min: *mut i64, h_max: *mut i64) -> c_int;
    // predictive checks and WAIC / IS-LOO of the population (fg_wpop_eval.hip): tests/end_to_end_workflows.rs:330-400, :650-745
    pub fn fg_wpop_checks_n_slots(n_checks: c_int, h_stat_mask: *const i32) -> c_int;
    pub fn fg_wpop_checks(h: *mut fg_wpop, d_yrep: *const c_void, n_rows: c_int, h_vtypes: *const i32, n_checks: c_int, h_offsets: *const i32,
                          h_members: *const i32, h_stat_mask: *const i32, h_observed: *const f64, h_t_obs: *mut f64, h_units: *mut u64,
                          h_counts: *mut i64, h_moments: *mut f64) -> c_int;
    pub fn fg_wpop_loglik(h: *mut fg_wpop, d_ll: *const f64, n_sel: c_int, h_figures: *mut f64, h_words: *mut f64, h_counts: *mut i64) -> c_int;
    pub fn fg_wpop_free(h: *mut fg_wpop);
    // ---- Pareto-smoothed LOO and k-hat of a stored log-likelihood table (fg_psis.hip)
    pub fn fg_psis_words() -> c_int;
    pub fn fg_psis_tail_len(S: i64) -> i64;
    pub fn fg_psis_loo(e: *mut fg_engine, d_ll: *const f64, n: c_int, n_sel: c_int, h_figures: *mut f64, h_counts: *mut i64, d_tail_or_null: *mut f64) -> c_int;
    // ---- rank-normalised R-hat, bulk / tail ESS of stored draws (fg_diag_rank.hip)
    pub fn fg_diag_rank_words() -> c_int;
    pub fn fg_diag_rank_transform(e: *mut fg_engine, d_draws: *const f64, n: c_int, d: c_int, j0: c_int, n_j: c_int, p_lo: f64, p_hi: f64,
                                  d_out: *mut f64, d_rank2_or_null: *mut u32, h_median: *mut f64, h_counts: *mut i64) -> c_int;
    pub fn fg_diag_rank_rhat_ess(e: *mut fg_engine, d_draws: *const f64, n: c_int, d: c_int, p_lo: f64, p_hi: f64, max_out_bytes: i64,
                                 h_figures: *mut f64, h_counts: *mut i64) -> c_int;
    // ---- MCSE and ESS of the mean, the sd and quantiles of stored draws, and the mad (fg_diag_mcse.hip)
    pub fn fg_diag_mcse_words(n_probs: c_int) -> c_int;
    pub fn fg_mcse_quantile_ranks(S: i64, p: f64, ess: f64, i_lo: *mut i64, i_hi: *mut i64) -> c_int;
    pub fn fg_diag_mcse_transform(e: *mut fg_engine, d_draws: *const f64, n: c_int, d: c_int, j0: c_int, n_j: c_int, h_mean: *const f64, h_probs: *const f64,
                                  n_probs: c_int, d_out: *mut f64, d_sorted_or_null: *mut f64, h_median: *mut f64, h_mad: *mut f64, h_counts: *mut i64) -> c_int;
    pub fn fg_diag_mcse(e: *mut fg_engine, d_draws: *const f64, n: c_int, d: c_int, h_probs: *const f64, n_probs: c_int, max_out_bytes: i64,
                        h_figures: *mut f64, h_counts: *mut i64) -> c_int;
    // ---- bootstrap particle filter bank (fg_pf.hip): crates/fugue-wasm/src/pf.rs, B filters at once
    pub fn fg_pf_new(device_ordinal: c_int, n_particles: i64, n_filters: i64, params: *const fg_pf_params, out: *mut *mut fg_pf) -> c_int;
    pub fn fg_pf_set_sig_obs(pf: *mut fg_pf, filter: i64, sig_obs: f64) -> c_int;
    pub fn fg_pf_run(pf: *mut fg_pf, h_obs: *const f64, t: i64, per_filter: c_int, h_ess_frac: *mut f64, h_log_z_inc: *mut f64, h_resampled: *mut i32,
                     h_mean: *mut f64, h_var: *mut f64) -> c_int;
    pub fn fg_pf_step(pf: *mut fg_pf, h_obs: *const f64, per_filter: c_int, h_ess_frac: *mut f64, h_log_z_inc: *mut f64, h_resampled: *mut i32, h_mean: *mut f64,
                      h_var: *mut f64, h_prev: *mut f64, h_propagated: *mut f64, h_weights: *mut f64, h_parents: *mut i64, h_posterior: *mut f64) -> c_int;
    pub fn fg_pf_log_evidence(pf: *mut fg_pf, h_out: *mut f64) -> c_int;
    pub fn fg_pf_t(pf: *const fg_pf) -> i64;
    pub fn fg_pf_positions(pf: *mut fg_pf, h_x: *mut f64) -> c_int;
    pub fn fg_pf_free(pf: *mut fg_pf);
    // ---- log-joint surfaces over one or two sites (fg_grid.hip): crates/fugue-wasm/src/grid.rs, a bank of bases at once
    pub fn fg_grid_new(e: *mut fg_engine, site_a: c_int, site_b: c_int, h_a: *const f64, n_a: i64, h_b: *const f64, n_b: i64, base_chunk: i64,
                       out: *mut *mut fg_grid) -> c_int;
    pub fn fg_grid_eval(g: *mut fg_grid, chain0: i64, n_bases: i64, d_out: *mut f64, d_acc: *mut f64) -> c_int;
    pub fn fg_grid_summary(g: *mut fg_grid, h_log_norm: *mut f64, h_max: *mut f64, h_argmax: *mut i64, h_counts: *mut i64) -> c_int;
    pub fn fg_grid_marginals(g: *mut fg_grid, h_log_marg_a: *mut f64, h_log_marg_b: *mut f64) -> c_int;
    pub fn fg_grid_mixture(g: *mut fg_grid, h_log_mix: *mut f64, n_mixed: *mut i64, n_skipped: *mut i64) -> c_int;
    pub fn fg_grid_count(g: *const fg_grid) -> i64;
    pub fn fg_grid_free(g: *mut fg_grid);
    // ---- exact Gibbs moves of the discrete sites (fg_gibbs.hip): src/inference/hmc.rs:68-71, "compose with `mh` to also move discrete sites"
    pub fn fg_program_site_support(p: *const fg_program, site: c_int, lo: *mut i64, hi: *mut i64) -> c_int;
    pub fn fg_gibbs_new(e: *mut fg_engine, h_sites: *const i32, n_sites: c_int, out: *mut *mut fg_gibbs) -> c_int;
    pub fn fg_gibbs_n_sites(g: *const fg_gibbs) -> c_int;
    pub fn fg_gibbs_n_cells(g: *const fg_gibbs) -> i64;
    pub fn fg_gibbs_layout(g: *const fg_gibbs, h_site: *mut i32, h_lo: *mut i64, h_K: *mut i32, h_cell0: *mut i64) -> c_int;
    pub fn fg_gibbs_sweep(g: *mut fg_gibbs, n_sweeps: c_int, h_rec_sites: *const i32, n_rec: c_int, d_rec: *mut i64, d_scores: *mut f64, d_cond: *mut f64) -> c_int;
    pub fn fg_gibbs_count(g: *const fg_gibbs) -> i64;
    pub fn fg_gibbs_seek(g: *mut fg_gibbs, t: i64) -> c_int;
    pub fn fg_gibbs_stats(g: *mut fg_gibbs, h_counts: *mut i64) -> c_int;
    pub fn fg_gibbs_probs(g: *mut fg_gibbs, h_mean: *mut f64, h_n: *mut i64) -> c_int;
    pub fn fg_gibbs_free(g: *mut fg_gibbs);
    pub fn fg_diag_exchange_bytes(e: *const fg_engine) -> i64;
    pub fn fg_comm_unique_id(out_128_bytes: *mut c_void) -> c_int;
    pub fn fg_comm_init(e: *mut fg_engine, world: c_int, rank: c_int, id_128_bytes: *const c_void, out_comm: *mut *mut c_void) -> c_int;
    pub fn fg_comm_destroy(comm: *mut c_void) -> c_int;
    // ---- mean-field VI (vi.rs:104-923)
    pub fn fg_vi_config_default(cfg: *mut fg_vi_config);
    pub fn fg_vi_elbo_batch(e: *mut fg_engine, h_factors: *const fg_vi_factor, n_eval: c_int, n_factors: c_int, h_stream_ids: *const u32,
                            h_elbo: *mut f64, h_terms: *mut f64) -> c_int;
    pub fn fg_vi_optimize(e: *mut fg_engine, h_factors: *mut fg_vi_factor, n_factors: c_int, cfg: *const fg_vi_config, h_elbo_history: *mut f64,
                          h_result: *mut fg_vi_result) -> c_int;
    pub fn fg_vi_estimate_elbo(e: *mut fg_engine, iteration: u32, h_elbo: *mut f64) -> c_int;
    // ---- checkpoint / resume (HmcSession fields hmc.rs:643-661)
    pub fn fg_state_size(e: *mut fg_engine) -> i64;
    pub fn fg_state_export(e: *mut fg_engine, h_buf: *mut c_void, capacity: usize) -> c_int;
    pub fn fg_state_import(e: *mut fg_engine, h_buf: *const c_void, size: usize) -> c_int;
    // ---- raw device memory
    pub fn fg_device_alloc(e: *mut fg_engine, bytes: usize) -> *mut c_void;
    pub fn fg_device_free(e: *mut fg_engine, p: *mut c_void) -> c_int;
    pub fn fg_device_download(e: *mut fg_engine, h: *mut c_void, d: *const c_void, bytes: usize) -> c_int;
    pub fn fg_device_upload(e: *mut fg_engine, d_dst: *mut c_void, h_src: *const c_void, bytes: usize) -> c_int;
    // ---- introspection of programs and engines
    pub fn fg_program_n_instructions(p: *const fg_program) -> c_int;
    pub fn fg_program_n_slots(p: *const fg_program) -> c_int;
    pub fn fg_program_dep_count(p: *const fg_program, k: c_int) -> c_int;
    pub fn fg_dsl_warning_count(p: *const fg_program) -> c_int;
    pub fn fg_dsl_warning(p: *const fg_program, i: c_int) -> *const c_char;
    pub fn fg_engine_stream(e: *mut fg_engine) -> *mut c_void;                       // hipStream_t
    pub fn fg_engine_set_stream(e: *mut fg_engine, hip_stream: *mut c_void) -> c_int;
    pub fn fg_engine_n_chains(e: *const fg_engine) -> i64;
    pub fn fg_engine_values_device(e: *mut fg_engine) -> *mut c_void;                // d_cells [S][C]
    pub fn fg_log_joint_stream(e: *mut fg_engine, h_acc: *mut f64, h_rec_lp: *mut f64) -> c_int;
    pub fn fg_log_joint_compiled(e: *mut fg_engine, h_acc: *mut f64) -> c_int;      // k_log_joint_jit, no fall-back
    // ---- pieces of the samplers with their randomness injected (what the reference's unit tests drive: hmc.rs:304-329, 419-535)
    pub fn fg_hmc_get_log_joint(e: *mut fg_engine, h_lj: *mut f64) -> c_int;
    pub fn fg_hmc_get_mass(e: *mut fg_engine, h_m_inv: *mut f64) -> c_int;
    pub fn fg_hmc_grad(e: *mut fg_engine, h: f64, grad_mode: c_int, h_grad: *mut f64, h_ok: *mut i32) -> c_int;
    pub fn fg_hmc_transition_injected(e: *mut fg_engine, cfg: *const fg_hmc_config, eps: f64, h_p0: *const f64, h_u: *const f64,
                                      h_accepted: *mut i32, h_alpha: *mut f64, h_divergent: *mut i32, h_lj: *mut f64) -> c_int;
    pub fn fg_hmc_find_eps_injected(e: *mut fg_engine, cfg: *const fg_hmc_config, h_p0: *const f64, h_eps: *mut f64) -> c_int;
    pub fn fg_mh_get_stats(e: *mut fg_engine, h_stats: *mut fg_mh_stats) -> c_int;
    pub fn fg_mh_get_scales(e: *mut fg_engine, h_scales: *mut f64) -> c_int;
    pub fn fg_mh_get_log_weight(e: *mut fg_engine, h_lw: *mut f64) -> c_int;
    // ---- population primitives on host arrays (numerical.rs:15-38, smc.rs:255-314, 588-622)
    pub fn fg_device_log_sum_exp(device_ordinal: c_int, h_x: *const f64, n: i64, out: *mut f64) -> c_int;
    pub fn fg_device_next_beta(device_ordinal: c_int, beta: f64, h_log_w: *const f64, h_loglik: *const f64, n: i64, target_ess: f64, out_beta: *mut f64) -> c_int;
    pub fn fg_device_resample_indices(device_ordinal: c_int, method: c_int, h_weights: *const f64, n: i64, h_u: *const f64, h_idx: *mut i64) -> c_int;
    pub fn fg_device_smc_temper(device_ordinal: c_int, beta: f64, h_loglik: *const f64, n: i64, target_ess: f64, flags: c_int, out_beta: *mut f64,
                                out_log_norm: *mut f64, h_log_w: *mut f64, h_weights: *mut f64, out_need_sum: *mut c_int) -> c_int;
    pub fn fg_diag_chain_moments(e: *mut fg_engine, d_draws: *const f64, n: c_int, d: c_int, d_moments: *mut f64) -> c_int;
    pub fn fg_diag_autocov_sums(e: *mut fg_engine, d_draws: *const f64, n: c_int, d: c_int, d_moments: *const f64, lag0: c_int, n_lags: c_int, h_sums: *mut f64) -> c_int;
}

/// The message of the last failed call on this thread.
pub fn last_error() -> String {
    unsafe {
        let p = fg_last_error();
        if p.is_null() { String::new() } else { std::ffi::CStr::from_ptr(p).to_string_lossy().into_owned() }
    }
}
