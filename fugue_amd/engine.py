"""ctypes binding of the C ABI (include/fugue_amd.h) + lowering of a `model.Program`
description onto it.  This is host plumbing only: every density, gradient and transition is
computed by the HIP kernels in fugue_amd/lib/libfugue_amd.so.  There is no CPU fallback --
loading fails loudly when the library is missing, and engine creation fails loudly when no
gfx950 device is present.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

from . import model as M

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FG_LIB_PATH") or os.path.join(_HERE, "lib", "libfugue_amd.so")   # FG_LIB_PATH: an experiment build (tools/)


class fg_tok(C.Structure):
    _fields_ = [("op", C.c_int32), ("a", C.c_int32), ("b", C.c_int32), ("reserved", C.c_int32), ("imm", C.c_double)]


class fg_hmc_config(C.Structure):
    _fields_ = [("n_leapfrog", C.c_int32), ("target_accept", C.c_double), ("init_step_size", C.c_double),
                ("finite_diff_eps", C.c_double), ("adapt_mass", C.c_int32), ("grad_mode", C.c_int32)]


class fg_hmc_stats(C.Structure):
    _fields_ = [("accept_rate", C.c_double), ("mean_step_size", C.c_double), ("n_divergent", C.c_int64),
                ("n_transitions", C.c_int64)]


class fg_site_proposal(C.Structure):
    _fields_ = [("kind", C.c_int32), ("lower", C.c_double), ("upper", C.c_double)]


class fg_mh_stats(C.Structure):
    _fields_ = [("accept_rate", C.c_double), ("n_steps", C.c_int64)]


class fg_smc_config(C.Structure):
    _fields_ = [("resampling_method", C.c_int32), ("ess_threshold", C.c_double), ("rejuvenation_steps", C.c_int32), ("sequential_adaptation", C.c_int32)]


class fg_smc_result(C.Structure):
    _fields_ = [("log_evidence", C.c_double), ("n_steps", C.c_int32), ("n_model_runs", C.c_int64)]


class fg_vi_factor(C.Structure):
    _fields_ = [("family", C.c_int32), ("site", C.c_int32), ("a", C.c_double), ("b", C.c_double)]


class fg_vi_config(C.Structure):
    _fields_ = [("n_iterations", C.c_int32), ("convergence_window", C.c_int32), ("base_learning_rate", C.c_double), ("fd_eps", C.c_double),
                ("convergence_tol", C.c_double), ("step_decay_exponent", C.c_double)]


class fg_vi_result(C.Structure):
    _fields_ = [("converged", C.c_int32), ("iterations", C.c_int32)]


class fg_pf_params(C.Structure):
    _fields_ = [("prior_sig", C.c_double), ("sig_step", C.c_double), ("sig_obs", C.c_double), ("ess_threshold", C.c_double), ("seed", C.c_uint64)]


RESAMPLE_MULTINOMIAL, RESAMPLE_SYSTEMATIC, RESAMPLE_STRATIFIED = range(3)
PROP_AUTO, PROP_GAUSSIAN, PROP_LOGSPACE, PROP_REFLECT, PROP_PRIOR_RESAMPLE = range(5)

TOK = {"const": 0, "site": 1, "data": 2, "neg": 3, "exp": 4, "ln": 5, "sqrt": 6, "abs": 7, "floor": 8, "sin": 9,
       "cos": 10, "tanh": 11, "add": 12, "sub": 13, "mul": 14, "div": 15, "pow": 16, "min": 17, "max": 18,
       "clamp": 19, "select": 20}
GRAD_FD_DENSE, GRAD_FD_SPARSE, GRAD_ANALYTIC = 0, 1, 2
# engine error codes (include/fugue_amd.h)
FG_E_NO_DEVICE, FG_E_HIP, FG_E_BAD_ARG, FG_E_NOT_FINALIZED, FG_E_STATE, FG_E_UNSUPPORTED, FG_E_LIMIT = -1, -2, -3, -4, -5, -6, -7
# fg_psis_loo's rows (include/fugue_amd.h): FG_PSIS_WORDS doubles and FG_PSIS_COUNTS integers per statement, the status words
PSIS_WORD_NAMES = ("elpd_loo_psis", "p_loo_psis", "khat", "sigma", "khat_threshold", "lppd", "x_min", "x_cut", "exp_cutoff", "t_star", "theta_hat",
                   "body_sum", "tail_sum", "tail_num")
PSIS_COUNT_NAMES = ("tail_len", "status", "n_capped", "n_fin", "n_neg_inf", "n_pos_inf", "n_nan", "n_below", "n_equal", "n_collected")
PSIS_COUNTS = len(PSIS_COUNT_NAMES)
PSIS_STATUS = ("fitted", "too few draws", "degenerate tail", "non-finite cells")
# fg_diag_rank_rhat_ess's rows (include/fugue_amd.h): FG_RANK_WORDS doubles and FG_RANK_COUNTS integers per coordinate; fg_diag_rank_transform's rows
RANK_WORD_NAMES = ("rhat_rank", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "ess_lower", "ess_upper", "median", "x_lo", "x_hi")
RANK_COUNT_NAMES = ("n_cells", "n_runs", "longest_run", "n_nan", "n_neg_inf", "n_pos_inf", "n_nan_folded", "n_passes")
RANK_COUNTS = len(RANK_COUNT_NAMES)
RANK_ROWS = 4
# fg_diag_mcse's rows (include/fugue_amd.h): FG_MCSE_FIXED_WORDS doubles, then FG_MCSE_PROB_WORDS per probability; the counts likewise
MCSE_WORD_NAMES = ("mean", "sd", "rhat", "ess_mean", "mcse_mean", "ess_sd", "ess_sq", "mcse_sd", "median", "mad")
MCSE_PROB_WORD_NAMES = ("q", "q7", "ess_quantile", "mcse_quantile", "th_lo", "th_hi")
MCSE_COUNT_NAMES = ("n_cells", "n_nan", "n_neg_inf", "n_pos_inf", "n_nan_folded", "n_passes")
MCSE_PROB_COUNT_NAMES = ("k_p", "i_lo", "i_hi")
MCSE_MAX_PROBS = 8

# every symbol include/fugue_amd.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [
    "fg_program_new", "fg_program_free", "fg_program_data", "fg_program_sample", "fg_program_observe",
    "fg_program_factor", "fg_program_finalize", "fg_program_n_sites", "fg_program_n_f64", "fg_program_n_observe",
    "fg_program_n_instructions", "fg_program_n_slots", "fg_program_site_name", "fg_program_site_vtype",
    "fg_program_site_of_handle", "fg_program_f64_site", "fg_program_dep_count", "fg_program_stream_records", "fg_last_error", "fg_abi_version",
    "fg_engine_new", "fg_engine_free", "fg_engine_synchronize", "fg_engine_stream", "fg_engine_set_stream", "fg_engine_n_chains",
    "fg_engine_set_values", "fg_engine_get_values", "fg_engine_values_device", "fg_prior_init", "fg_log_joint", "fg_log_joint_stream", "fg_log_joint_compiled",
    "fg_program_sample_discrete_uniform",
    "fg_hmc_config_default", "fg_hmc_init", "fg_hmc_step", "fg_hmc_step_info", "fg_hmc_get_mass", "fg_hmc_run", "fg_hmc_get_stats", "fg_hmc_get_step_sizes",
    "fg_hmc_get_log_joint", "fg_hmc_set_step_size", "fg_hmc_set_n_leapfrog", "fg_hmc_is_warming_up", "fg_hmc_iterations", "fg_hmc_short_quotient", "fg_hmc_range_proved", "fg_hmc_step_recorded",
    "fg_state_size", "fg_state_export", "fg_state_import", "fg_hmc_grad", "fg_hmc_transition_injected",
    "fg_hmc_find_eps_injected", "fg_mh_init", "fg_mh_step", "fg_mh_set_recording", "fg_mh_run", "fg_mh_get_stats", "fg_mh_get_scales",
    "fg_mh_get_log_weight", "fg_smc_config_default", "fg_smc_run", "fg_smc_prior_particles", "fg_smc_normalize", "fg_smc_ess", "fg_smc_resample", "fg_smc_rejuvenate",
    "fg_smc_get_weights", "fg_smc_set_log_weights", "fg_device_log_sum_exp", "fg_device_next_beta", "fg_device_smc_temper",
    "fg_device_resample_indices", "fg_diag_chain_moments", "fg_diag_autocov_sums", "fg_diag_rhat_ess", "fg_diag_combine", "fg_diag_geweke",
    "fg_diag_combine_reduced", "fg_diag_set_exchange", "fg_diag_exchange_bytes", "fg_hmc_last_kernel", "fg_mh_last_kernel", "fg_diag_quantiles",
    "fg_comm_unique_id", "fg_comm_init", "fg_comm_destroy", "fg_device_alloc", "fg_device_free", "fg_device_download", "fg_device_upload",
    "fg_dsl_compile", "fg_dsl_warning_count", "fg_dsl_warning",
    "fg_vi_config_default", "fg_vi_elbo_batch", "fg_vi_optimize", "fg_vi_estimate_elbo",
    "fg_diag_stream_new", "fg_diag_stream_update", "fg_diag_stream_count", "fg_diag_stream_moments", "fg_diag_stream_autocov_sums",
    "fg_diag_stream_rhat_ess", "fg_diag_stream_free",
    "fg_diag_qstream_new", "fg_diag_qstream_update", "fg_diag_qstream_count", "fg_diag_qstream_end_pass", "fg_diag_qstream_passes",
    "fg_diag_qstream_result", "fg_diag_qstream_free",
    "fg_diag_cstream_new", "fg_diag_cstream_update", "fg_diag_cstream_count", "fg_diag_cstream_result", "fg_diag_cstream_free",
    "fg_diag_cells_f64",
    "fg_loglik_stream_new", "fg_loglik_stream_update", "fg_loglik_stream_count", "fg_loglik_stream_pooled", "fg_loglik_stream_result", "fg_loglik_stream_free",
    "fg_ppc_stream_new", "fg_ppc_stream_update", "fg_ppc_stream_count", "fg_ppc_stream_n_slots", "fg_ppc_stream_observed", "fg_ppc_stream_pooled",
    "fg_ppc_stream_chains", "fg_ppc_stream_free", "fg_program_observe_value",
    "fg_wpop_new", "fg_wpop_units", "fg_wpop_moments", "fg_wpop_quantiles", "fg_wpop_counts", "fg_wpop_free", "fg_wpop_checks_n_slots", "fg_wpop_checks", "fg_wpop_loglik",
    "fg_psis_words", "fg_psis_tail_len", "fg_psis_loo",
    "fg_diag_rank_words", "fg_diag_rank_transform", "fg_diag_rank_rhat_ess",
    "fg_diag_mcse_words", "fg_mcse_quantile_ranks", "fg_diag_mcse_transform", "fg_diag_mcse",
    "fg_program_result", "fg_program_n_results", "fg_program_result_name", "fg_program_result_sites", "fg_result_eval",
    "fg_program_observe_name", "fg_program_observe_vtype", "fg_program_observe_dist", "fg_predict_eval",
    "fg_abc_distance", "fg_abc_mixture", "fg_abc_new", "fg_abc_free", "fg_abc_round_prior", "fg_abc_stage_begin", "fg_abc_round_stage",
    "fg_abc_stage_end", "fg_abc_last_round", "fg_abc_get_population", "fg_abc_set_population",
    "fg_pf_new", "fg_pf_set_sig_obs", "fg_pf_run", "fg_pf_step", "fg_pf_log_evidence", "fg_pf_t", "fg_pf_positions", "fg_pf_free",
    "fg_grid_new", "fg_grid_eval", "fg_grid_summary", "fg_grid_marginals", "fg_grid_mixture", "fg_grid_count", "fg_grid_free",
    "fg_program_site_support", "fg_gibbs_new", "fg_gibbs_n_sites", "fg_gibbs_n_cells", "fg_gibbs_layout", "fg_gibbs_sweep", "fg_gibbs_count", "fg_gibbs_seek",
    "fg_gibbs_stats", "fg_gibbs_probs", "fg_gibbs_free",
]

_lib = None
ACOV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_double))     # fg_acov_fn
REDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double))     # fg_reduce_fn
DIAG_REDUCE, DIAG_GATHER = 0, 1


class DslError(ValueError):
    """Static error of the model DSL (syntax, unknown name, arity); message as the reference words it."""


class EngineError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"fugue_amd error {code}: {message}")
        self.code = code


def lib():
    """Loads libfugue_amd.so (building it in-tree first if hipcc is available and it is stale)."""
    global _lib
    if _lib is not None:
        return _lib
    from . import build as _b
    try:                                  # a no-op when the library is fresh; rebuilds a stale one where hipcc exists
        if not (os.environ.get("FG_LIB_PATH") and os.path.exists(LIB_PATH)):   # an experiment library is taken as it is
            _b.build()
    except Exception:
        if not os.path.exists(LIB_PATH):
            raise
    L = C.CDLL(LIB_PATH)
    vp, dp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32)
    tp = C.POINTER(fg_tok)
    L.fg_last_error.restype = C.c_char_p
    L.fg_program_new.restype = vp
    L.fg_program_free.argtypes = [vp]
    L.fg_program_data.argtypes = [vp, C.c_char_p, dp, C.c_int64]
    L.fg_program_sample.argtypes = [vp, C.c_char_p, C.c_int, tp, ip, C.c_int]
    L.fg_program_observe.argtypes = [vp, C.c_char_p, C.c_int, tp, ip, C.c_int, tp, C.c_int]
    L.fg_program_factor.argtypes = [vp, tp, C.c_int]
    L.fg_program_sample_discrete_uniform.argtypes = [vp, C.c_char_p, C.c_int64, C.c_int64]
    for f in ("fg_program_finalize", "fg_program_n_sites", "fg_program_n_f64", "fg_program_n_observe",
              "fg_program_n_instructions", "fg_program_n_slots"):
        getattr(L, f).argtypes = [vp]
    L.fg_program_site_name.argtypes = [vp, C.c_int, C.c_char_p, C.c_int]
    for f in ("fg_program_site_vtype", "fg_program_site_of_handle", "fg_program_f64_site", "fg_program_dep_count", "fg_program_stream_records"):
        getattr(L, f).argtypes = [vp, C.c_int]
    L.fg_program_result.argtypes = [vp, C.c_char_p, tp, C.c_int]
    L.fg_program_n_results.argtypes = [vp]
    L.fg_program_result_name.argtypes = [vp, C.c_int, C.c_char_p, C.c_int]
    L.fg_program_result_sites.argtypes = [vp, ip, C.c_int]
    L.fg_result_eval.argtypes = [vp, vp, C.c_int, ip, C.c_int, vp]
    L.fg_program_observe_name.argtypes = [vp, C.c_int, C.c_char_p, C.c_int]
    L.fg_program_observe_vtype.argtypes = [vp, C.c_int]
    L.fg_program_observe_dist.argtypes = [vp, C.c_int]
    L.fg_predict_eval.argtypes = [vp, vp, C.c_int, ip, C.c_int, C.c_uint32, ip, C.c_int, vp, vp]
    L.fg_abc_distance.argtypes = [vp, vp, C.c_int, C.c_int64, dp, C.c_int, C.c_int, dp, C.c_int, vp]
    L.fg_abc_mixture.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, C.c_int, dp, dp, vp]
    i64p = C.POINTER(C.c_int64)
    L.fg_abc_new.argtypes = [vp, C.c_int, ip, C.c_int, dp, C.c_int, C.c_int, dp, C.c_int, C.c_int64, C.POINTER(vp)]
    L.fg_abc_free.argtypes = [vp]
    L.fg_abc_free.restype = None
    L.fg_abc_round_prior.argtypes = [vp, C.c_double, C.c_int64, i64p, i64p]
    L.fg_abc_stage_begin.argtypes = [vp]
    L.fg_abc_round_stage.argtypes = [vp, C.c_uint32, C.c_double, C.c_int64, i64p, i64p]
    L.fg_abc_stage_end.argtypes = [vp]
    L.fg_abc_last_round.argtypes = [vp, i64p, dp, dp, ip]
    L.fg_abc_get_population.argtypes = [vp, C.c_int, i64p, vp, dp, dp, i64p, dp, dp]
    L.fg_abc_set_population.argtypes = [vp, C.c_int64, vp, dp, dp, i64p, dp, dp]
    L.fg_engine_new.restype = vp
    L.fg_engine_new.argtypes = [vp, C.c_int64, C.c_uint64, C.c_uint32, C.c_int]
    L.fg_engine_free.argtypes = [vp]
    L.fg_engine_synchronize.argtypes = [vp]
    L.fg_engine_stream.restype = vp
    L.fg_engine_stream.argtypes = [vp]
    L.fg_engine_set_stream.argtypes = [vp, vp]
    L.fg_engine_n_chains.restype = C.c_int64
    L.fg_engine_n_chains.argtypes = [vp]
    L.fg_engine_set_values.argtypes = [vp, vp]
    L.fg_engine_get_values.argtypes = [vp, vp]
    L.fg_engine_values_device.restype = vp
    L.fg_engine_values_device.argtypes = [vp]
    L.fg_prior_init.argtypes = [vp, C.c_uint32, dp]
    L.fg_log_joint.argtypes = [vp, dp, dp]
    L.fg_log_joint_stream.argtypes = [vp, dp, dp]
    L.fg_log_joint_compiled.argtypes = [vp, dp]
    L.fg_hmc_config_default.argtypes = [C.POINTER(fg_hmc_config)]
    L.fg_hmc_init.argtypes = [vp, C.POINTER(fg_hmc_config), C.c_int]
    L.fg_hmc_step.argtypes = [vp, C.c_int, vp]
    L.fg_hmc_step_info.argtypes = [vp, C.c_int, vp, vp]
    L.fg_hmc_get_mass.argtypes = [vp, dp]
    L.fg_hmc_run.argtypes = [vp, C.POINTER(fg_hmc_config), C.c_int, C.c_int, vp, C.POINTER(fg_hmc_stats)]
    L.fg_hmc_get_stats.argtypes = [vp, C.POINTER(fg_hmc_stats)]
    L.fg_hmc_get_step_sizes.argtypes = [vp, dp]
    L.fg_hmc_get_log_joint.argtypes = [vp, dp]
    L.fg_hmc_set_step_size.argtypes = [vp, C.c_double]
    L.fg_hmc_set_n_leapfrog.argtypes = [vp, C.c_int]
    L.fg_hmc_is_warming_up.argtypes = [vp]
    L.fg_hmc_iterations.restype = C.c_int64
    L.fg_hmc_iterations.argtypes = [vp]
    L.fg_hmc_short_quotient.argtypes = [vp]
    L.fg_hmc_range_proved.argtypes = [vp]
    L.fg_hmc_step_recorded.argtypes = [vp, C.c_int, C.POINTER(C.c_int64), dp, dp, ip, vp]
    L.fg_state_size.restype = C.c_int64
    L.fg_state_size.argtypes = [vp]
    L.fg_state_export.argtypes = [vp, vp, C.c_size_t]
    L.fg_state_import.argtypes = [vp, vp, C.c_size_t]
    L.fg_hmc_grad.argtypes = [vp, C.c_double, C.c_int, dp, ip]
    L.fg_hmc_transition_injected.argtypes = [vp, C.POINTER(fg_hmc_config), C.c_double, dp, dp, ip, dp, ip, dp]
    L.fg_hmc_find_eps_injected.argtypes = [vp, C.POINTER(fg_hmc_config), dp, dp]
    L.fg_mh_init.argtypes = [vp, C.c_int, C.POINTER(fg_site_proposal)]
    L.fg_mh_step.argtypes = [vp, C.c_int, ip, C.c_int, vp]
    L.fg_mh_set_recording.argtypes = [vp, C.c_int]
    L.fg_mh_run.argtypes = [vp, C.c_int, C.c_int, C.POINTER(fg_site_proposal), ip, C.c_int, vp, C.POINTER(fg_mh_stats)]
    L.fg_mh_get_stats.argtypes = [vp, C.POINTER(fg_mh_stats)]
    L.fg_mh_get_scales.argtypes = [vp, dp]
    L.fg_mh_get_log_weight.argtypes = [vp, dp]
    L.fg_smc_config_default.argtypes = [C.POINTER(fg_smc_config)]
    L.fg_smc_run.argtypes = [vp, C.POINTER(fg_smc_config), dp, dp, C.POINTER(fg_smc_result), dp, C.c_int]
    L.fg_smc_prior_particles.argtypes = [vp, C.c_uint32]
    L.fg_smc_normalize.argtypes = [vp]
    L.fg_smc_ess.argtypes = [vp, dp]
    L.fg_smc_resample.argtypes = [vp, C.c_int, C.c_uint32, C.POINTER(C.c_int64)]
    L.fg_smc_rejuvenate.argtypes = [vp, C.c_double, C.c_int, C.c_uint32, dp]
    L.fg_smc_get_weights.argtypes = [vp, dp, dp]
    L.fg_smc_set_log_weights.argtypes = [vp, dp]
    L.fg_device_log_sum_exp.argtypes = [C.c_int, dp, C.c_int64, dp]
    L.fg_device_next_beta.argtypes = [C.c_int, C.c_double, dp, dp, C.c_int64, C.c_double, dp]
    L.fg_device_smc_temper.argtypes = [C.c_int, C.c_double, dp, C.c_int64, C.c_double, C.c_int, dp, dp, dp, dp, ip]
    L.fg_device_resample_indices.argtypes = [C.c_int, C.c_int, dp, C.c_int64, dp, C.POINTER(C.c_int64)]
    L.fg_diag_chain_moments.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    L.fg_diag_autocov_sums.argtypes = [vp, vp, C.c_int, C.c_int, vp, C.c_int, C.c_int, dp]
    L.fg_diag_geweke.argtypes = [vp, vp, C.c_int, C.c_int, vp]
    L.fg_diag_rhat_ess.argtypes = [vp, vp, C.c_int, C.c_int, vp, dp, dp, dp, dp, C.POINTER(C.c_int64)]
    L.fg_diag_combine.argtypes = [dp, C.c_int64, C.c_int, C.c_int, ACOV_FN, vp, dp, dp, dp, dp]
    L.fg_diag_combine_reduced.argtypes = [C.c_int64, C.c_int, C.c_int, REDUCE_FN, ACOV_FN, vp, dp, dp, dp, dp]
    L.fg_diag_quantiles.argtypes = [vp, vp, C.c_int, C.c_int, vp, dp, C.c_int, dp]
    L.fg_diag_set_exchange.argtypes = [vp, C.c_int]
    L.fg_diag_exchange_bytes.restype = C.c_int64
    L.fg_diag_exchange_bytes.argtypes = [vp]
    L.fg_diag_stream_new.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.fg_diag_stream_update.argtypes = [vp, vp, C.c_int]
    L.fg_diag_stream_count.argtypes = [vp]
    L.fg_diag_stream_moments.argtypes = [vp, vp]
    L.fg_diag_stream_autocov_sums.argtypes = [vp, C.c_int, C.c_int, dp]
    L.fg_diag_stream_rhat_ess.argtypes = [vp, vp, dp, dp, dp, dp, C.POINTER(C.c_int64)]
    L.fg_diag_stream_free.restype = None
    L.fg_diag_stream_free.argtypes = [vp]
    L.fg_diag_qstream_new.argtypes = [vp, C.c_int, C.c_int, dp, C.c_int, C.c_int, C.c_int64, C.POINTER(vp)]
    L.fg_diag_qstream_update.argtypes = [vp, vp, C.c_int]
    L.fg_diag_qstream_count.argtypes = [vp]
    L.fg_diag_qstream_end_pass.argtypes = [vp, C.POINTER(C.c_int)]
    L.fg_diag_qstream_passes.argtypes = [vp]
    L.fg_diag_qstream_result.argtypes = [vp, dp, C.POINTER(C.c_int32)]
    L.fg_diag_qstream_free.restype = None
    L.fg_diag_qstream_free.argtypes = [vp]
    L.fg_diag_cstream_new.argtypes = [vp, C.c_int, C.c_int, ip, ip, C.POINTER(C.c_int64), ip, C.c_int, C.POINTER(vp)]
    L.fg_diag_cstream_update.argtypes = [vp, vp, C.c_int]
    L.fg_diag_cstream_count.argtypes = [vp]
    L.fg_diag_cstream_result.argtypes = [vp, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.fg_diag_cstream_free.restype = None
    L.fg_diag_cstream_free.argtypes = [vp]
    L.fg_loglik_stream_new.argtypes = [vp, C.c_int, C.c_int, C.POINTER(vp)]
    L.fg_loglik_stream_update.argtypes = [vp, vp, C.c_int]
    L.fg_loglik_stream_count.argtypes = [vp]
    L.fg_loglik_stream_pooled.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.fg_loglik_stream_result.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
    L.fg_loglik_stream_free.restype = None
    L.fg_loglik_stream_free.argtypes = [vp]
    L.fg_ppc_stream_new.argtypes = [vp, C.c_int, C.c_int, ip, C.c_int, ip, ip, ip, C.POINTER(C.c_double), C.POINTER(vp)]
    L.fg_ppc_stream_update.argtypes = [vp, vp, C.c_int]
    L.fg_ppc_stream_count.argtypes = [vp]
    L.fg_ppc_stream_n_slots.argtypes = [vp]
    L.fg_ppc_stream_observed.argtypes = [vp, C.POINTER(C.c_double)]
    L.fg_ppc_stream_pooled.argtypes = [vp, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    L.fg_ppc_stream_chains.argtypes = [vp, C.c_int, C.POINTER(C.c_int64)]
    L.fg_ppc_stream_free.restype = None
    L.fg_ppc_stream_free.argtypes = [vp]
    L.fg_program_observe_value.argtypes = [vp, C.c_int, C.POINTER(C.c_double)]
    u64p = C.POINTER(C.c_uint64)
    L.fg_wpop_new.argtypes = [vp, C.c_int64, vp, C.POINTER(vp)]
    L.fg_wpop_units.argtypes = [vp, u64p, u64p, u64p]
    L.fg_wpop_moments.argtypes = [vp, vp, C.c_int, dp]
    L.fg_wpop_quantiles.argtypes = [vp, vp, C.c_int, dp, C.c_int, C.c_int, C.c_int64, dp, ip]
    L.fg_wpop_counts.argtypes = [vp, vp, C.c_int, ip, i64p, ip, u64p, u64p, u64p, i64p, i64p]
    L.fg_wpop_checks_n_slots.argtypes = [C.c_int, ip]
    L.fg_wpop_checks.argtypes = [vp, vp, C.c_int, ip, C.c_int, ip, ip, ip, dp, dp, u64p, i64p, dp]
    L.fg_wpop_loglik.argtypes = [vp, vp, C.c_int, dp, dp, i64p]
    L.fg_wpop_free.restype = None
    L.fg_wpop_free.argtypes = [vp]
    L.fg_psis_words.argtypes = []
    L.fg_psis_tail_len.restype = C.c_int64
    L.fg_psis_tail_len.argtypes = [C.c_int64]
    L.fg_psis_loo.argtypes = [vp, vp, C.c_int, C.c_int, dp, i64p, vp]
    L.fg_diag_rank_words.argtypes = []
    L.fg_diag_rank_transform.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, vp, vp, dp, i64p]
    L.fg_diag_rank_rhat_ess.argtypes = [vp, vp, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int64, dp, i64p]
    L.fg_diag_mcse_words.argtypes = [C.c_int]
    L.fg_mcse_quantile_ranks.argtypes = [C.c_int64, C.c_double, C.c_double, i64p, i64p]
    L.fg_diag_mcse_transform.argtypes = [vp, vp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, C.c_int, vp, vp, dp, dp, i64p]
    L.fg_diag_mcse.argtypes = [vp, vp, C.c_int, C.c_int, dp, C.c_int, C.c_int64, dp, i64p]
    L.fg_pf_new.argtypes = [C.c_int, C.c_int64, C.c_int64, C.POINTER(fg_pf_params), C.POINTER(vp)]
    L.fg_pf_set_sig_obs.argtypes = [vp, C.c_int64, C.c_double]
    L.fg_pf_run.argtypes = [vp, dp, C.c_int64, C.c_int, dp, dp, ip, dp, dp]
    L.fg_pf_step.argtypes = [vp, dp, C.c_int, dp, dp, ip, dp, dp, dp, dp, dp, i64p, dp]
    L.fg_pf_log_evidence.argtypes = [vp, dp]
    L.fg_pf_t.restype = C.c_int64
    L.fg_pf_t.argtypes = [vp]
    L.fg_pf_positions.argtypes = [vp, dp]
    L.fg_pf_free.restype = None
    L.fg_pf_free.argtypes = [vp]
    L.fg_grid_new.argtypes = [vp, C.c_int, C.c_int, dp, C.c_int64, dp, C.c_int64, C.c_int64, C.POINTER(vp)]
    L.fg_grid_eval.argtypes = [vp, C.c_int64, C.c_int64, vp, vp]
    L.fg_grid_summary.argtypes = [vp, dp, dp, i64p, i64p]
    L.fg_grid_marginals.argtypes = [vp, dp, dp]
    L.fg_grid_mixture.argtypes = [vp, dp, i64p, i64p]
    L.fg_grid_count.restype = C.c_int64
    L.fg_grid_count.argtypes = [vp]
    L.fg_grid_free.restype = None
    L.fg_grid_free.argtypes = [vp]
    L.fg_program_site_support.argtypes = [vp, C.c_int, i64p, i64p]
    L.fg_gibbs_new.argtypes = [vp, ip, C.c_int, C.POINTER(vp)]
    L.fg_gibbs_n_sites.argtypes = [vp]
    L.fg_gibbs_n_cells.restype = C.c_int64
    L.fg_gibbs_n_cells.argtypes = [vp]
    L.fg_gibbs_layout.argtypes = [vp, ip, i64p, ip, i64p]
    L.fg_gibbs_sweep.argtypes = [vp, C.c_int, ip, C.c_int, vp, vp, vp]
    L.fg_gibbs_count.restype = C.c_int64
    L.fg_gibbs_count.argtypes = [vp]
    L.fg_gibbs_seek.argtypes = [vp, C.c_int64]
    L.fg_gibbs_stats.argtypes = [vp, i64p]
    L.fg_gibbs_probs.argtypes = [vp, dp, i64p]
    L.fg_gibbs_free.restype = None
    L.fg_gibbs_free.argtypes = [vp]
    L.fg_diag_cells_f64.argtypes = [vp, vp, C.c_int, C.c_int, ip, ip, C.c_int, vp]
    L.fg_hmc_last_kernel.restype = C.c_char_p
    L.fg_hmc_last_kernel.argtypes = [vp]
    L.fg_mh_last_kernel.restype = C.c_char_p
    L.fg_mh_last_kernel.argtypes = [vp]
    L.fg_comm_unique_id.argtypes = [vp]
    L.fg_comm_init.argtypes = [vp, C.c_int, C.c_int, vp, C.POINTER(vp)]
    L.fg_comm_destroy.argtypes = [vp]
    L.fg_device_alloc.restype = vp
    L.fg_device_alloc.argtypes = [vp, C.c_size_t]
    L.fg_device_free.argtypes = [vp, vp]
    L.fg_device_download.argtypes = [vp, vp, vp, C.c_size_t]
    L.fg_device_upload.argtypes = [vp, vp, vp, C.c_size_t]
    L.fg_vi_config_default.argtypes = [C.POINTER(fg_vi_config)]
    L.fg_vi_elbo_batch.argtypes = [vp, C.POINTER(fg_vi_factor), C.c_int, C.c_int, C.POINTER(C.c_uint32), dp, dp]
    L.fg_vi_optimize.argtypes = [vp, C.POINTER(fg_vi_factor), C.c_int, C.POINTER(fg_vi_config), dp, C.POINTER(fg_vi_result)]
    L.fg_vi_estimate_elbo.argtypes = [vp, C.c_uint32, dp]
    L.fg_dsl_compile.restype = vp
    L.fg_dsl_compile.argtypes = [C.c_char_p, C.c_char_p]
    L.fg_dsl_warning_count.argtypes = [vp]
    L.fg_dsl_warning.restype = C.c_char_p
    L.fg_dsl_warning.argtypes = [vp, C.c_int]
    _lib = L
    return L


def last_error() -> str:
    return lib().fg_last_error().decode("utf-8", "replace")


def _check(rc: int):
    if rc != 0:
        raise EngineError(rc, last_error())


def _dp(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def mcse_quantile_ranks(S: int, p: float, ess: float):
    """`fg_mcse_quantile_ranks`: the 0-based positions (i_lo, i_hi) of mcse_quantile's two order statistics among S sorted cells, from the
    15.87 % and 84.13 % points of Beta(ess p + 1, ess (1 - p) + 1).  Host only: no device and no engine."""
    lo, hi = C.c_int64(-1), C.c_int64(-1)
    _check(lib().fg_mcse_quantile_ranks(int(S), float(p), float(ess), C.byref(lo), C.byref(hi)))
    return int(lo.value), int(hi.value)


def hmc_config(n_leapfrog=16, target_accept=0.8, init_step_size=None, finite_diff_eps=1e-5, adapt_mass=False,
               grad_mode=GRAD_FD_SPARSE) -> fg_hmc_config:
    """`HMCConfig` (/root/reference/src/inference/hmc.rs:106-135), same defaults; grad_mode: the engine's one default is
    FG_GRAD_FD_SPARSE (C ABI, Python, bench) -- GRAD_FD_DENSE is the reference's arithmetic verbatim."""
    return fg_hmc_config(int(n_leapfrog), float(target_accept),
                         float("nan") if init_step_size is None else float(init_step_size),
                         float(finite_diff_eps), int(bool(adapt_mass)), int(grad_mode))


# --------------------------------------------------------------------------------------
def _postfix(e: M.Expr, out: List[fg_tok]):
    if e.op == "const":
        out.append(fg_tok(TOK["const"], 0, 0, 0, e.value))
    elif e.op == "site":
        out.append(fg_tok(TOK["site"], e.a, 0, 0, 0.0))
    elif e.op == "data":
        out.append(fg_tok(TOK["data"], e.a, e.b, 0, 0.0))
    elif e.op == "select":
        for a in e.args:
            _postfix(a, out)
        out.append(fg_tok(TOK["select"], len(e.args) - 1, 0, 0, 0.0))
    else:
        for a in e.args:
            _postfix(a, out)
        out.append(fg_tok(TOK[e.op], 0, 0, 0, 0.0))


def _tok_array(toks: List[fg_tok]):
    arr = (fg_tok * max(1, len(toks)))()
    for i, t in enumerate(toks):
        arr[i] = t
    return arr


class CompiledProgram:
    """A finalized `fg_program` (site program) built from a `model.Program` description."""

    def __init__(self, program: Optional[M.Program], _handle=None):
        L = lib()
        self.program = program
        self.warnings: List[str] = []
        self.result_skipped: List[str] = []      # leaves of the model's return value that are no expression (or that the builder refused)
        if _handle is not None:           # already finalized by a native front-end (fg_dsl_compile)
            self.h = _handle
            self._describe()
            return
        self.h = L.fg_program_new()
        for name, arr in zip(program.data_names, program.data):
            a = np.ascontiguousarray(arr, dtype=np.float64)
            rc = L.fg_program_data(self.h, name.encode(), _dp(a), a.size)
            if rc < 0:
                raise EngineError(rc, last_error())
        for st in program.stmts:
            if st.kind == M.FACTOR:
                toks: List[fg_tok] = []
                _postfix(st.value, toks)
                _check(L.fg_program_factor(self.h, _tok_array(toks), len(toks)))
                continue
            toks, lens = [], []
            for p in st.dist.params:
                n0 = len(toks)
                _postfix(p, toks)
                lens.append(len(toks) - n0)
            plen = (C.c_int32 * max(1, len(lens)))(*lens)
            if st.kind == M.SAMPLE and st.dist.i64_bounds is not None:
                rc = L.fg_program_sample_discrete_uniform(self.h, st.addr.encode("utf-8"), *st.dist.i64_bounds)
                if rc < 0 or rc != st.handle:
                    raise EngineError(rc, last_error())
            elif st.kind == M.SAMPLE:
                rc = L.fg_program_sample(self.h, st.addr.encode("utf-8"), st.dist.kind, _tok_array(toks), plen, len(lens))
                if rc < 0 or rc != st.handle:
                    raise EngineError(rc, last_error())
            else:
                vt: List[fg_tok] = []
                _postfix(st.value, vt)
                _check(L.fg_program_observe(self.h, st.addr.encode("utf-8"), st.dist.kind, _tok_array(toks), plen,
                                            len(lens), _tok_array(vt), len(vt)))
        # the model's return value (`pure(..)`, model.rs; hmc.rs:566-583 hands it back per draw): one result per scalar leaf
        names, exprs, self.result_skipped = M.flatten_result(program.result)
        for name, ex in zip(names, exprs):
            rt: List[fg_tok] = []
            try:
                _postfix(ex, rt)
                rc = L.fg_program_result(self.h, name.encode("utf-8"), _tok_array(rt), len(rt))
            except (KeyError, RecursionError):
                rc = FG_E_BAD_ARG
            if rc < 0:
                self.result_skipped.append(name)
        rc = L.fg_program_finalize(self.h)
        if rc != 0:
            msg = last_error()
            L.fg_program_free(self.h)
            self.h = None
            raise M.FugueError(msg, rc) if rc > 0 else EngineError(rc, msg)
        self._describe()

    @classmethod
    def from_dsl(cls, source: str, data=None) -> "CompiledProgram":
        """`CompiledModel::compile(source, data_json)` of the playground DSL (crates/fugue-wasm/src/dsl.rs:1062-1120):
        `data` is a JSON string, a dict of arrays, a bare list (bound to `data`) or None."""
        import json
        L = lib()
        dj = data if isinstance(data, str) else ("" if data is None else json.dumps(data))
        h = L.fg_dsl_compile(source.encode("utf-8"), dj.encode("utf-8"))
        if not h:
            raise DslError(last_error())
        cp = cls(None, _handle=h)
        cp.warnings = [L.fg_dsl_warning(h, i).decode("utf-8") for i in range(L.fg_dsl_warning_count(h))]
        return cp

    def _describe(self):
        L = lib()
        self.S = L.fg_program_n_sites(self.h)
        self.d = L.fg_program_n_f64(self.h)
        self.O = L.fg_program_n_observe(self.h)
        self.n_instructions = L.fg_program_n_instructions(self.h)
        self.n_slots = L.fg_program_n_slots(self.h)
        buf = C.create_string_buffer(4096)
        self.site_names = []
        for j in range(self.S):
            L.fg_program_site_name(self.h, j, buf, 4096)
            self.site_names.append(buf.value.decode("utf-8"))
        self.site_vtypes = [L.fg_program_site_vtype(self.h, j) for j in range(self.S)]
        self.f64_sites = [L.fg_program_f64_site(self.h, k) for k in range(self.d)]
        self.dep_counts = [L.fg_program_dep_count(self.h, k) for k in range(self.d)]
        self.stream_records = tuple(L.fg_program_stream_records(self.h, w) for w in range(3))   # (gradient, score, kinds)
        self.R = L.fg_program_n_results(self.h)
        self.result_names = []
        for r in range(self.R):
            L.fg_program_result_name(self.h, r, buf, 4096)
            self.result_names.append(buf.value.decode("utf-8"))
        self.observe_names = []
        for k in range(self.O):
            L.fg_program_observe_name(self.h, k, buf, 4096)
            self.observe_names.append(buf.value.decode("utf-8"))
        self.observe_vtypes = [L.fg_program_observe_vtype(self.h, k) for k in range(self.O)]     # program order, as the names
        self.observe_dists = [L.fg_program_observe_dist(self.h, k) for k in range(self.O)]
        self.observe_values = []                      # the observed value where the model states it (a literal or a data element), else None
        v = C.c_double()
        for k in range(self.O):
            rc = L.fg_program_observe_value(self.h, k, C.byref(v))
            if rc < 0:
                _check(rc)
            self.observe_values.append(float(v.value) if rc == 1 else None)
        rs = (C.c_int32 * max(1, self.S))()
        self.result_sites = list(rs[:L.fg_program_result_sites(self.h, rs, self.S)])   # sorted site indices some result reads

    def site_of_handle(self, h: int) -> int:
        return lib().fg_program_site_of_handle(self.h, h)

    def __del__(self):
        try:
            if self.h:
                lib().fg_program_free(self.h)
        except Exception:
            pass

    # cells helpers (same convention as the oracle wrapper: int64 raw view) ---------------
    def cells(self, values: Sequence) -> np.ndarray:
        out = np.zeros(self.S, dtype=np.int64)
        for j, v in enumerate(values):
            out[j] = np.array([v], dtype=np.float64).view(np.int64)[0] if self.site_vtypes[j] == 0 else int(v)
        return out


def compile_model(model_or_fn) -> CompiledProgram:
    prog = model_or_fn if isinstance(model_or_fn, M.Program) else M.trace_model(model_or_fn)
    return CompiledProgram(prog)


class Engine:
    """`fg_engine`: n_chains chains of one program on one MI355X."""

    def __init__(self, compiled: CompiledProgram, n_chains: int, seed: int, chain_offset: int = 0, device: int = 0):
        L = lib()
        self.cp = compiled
        self.C = int(n_chains)
        self.h = L.fg_engine_new(compiled.h, self.C, int(seed) & 0xFFFFFFFFFFFFFFFF, int(chain_offset), int(device))
        if not self.h:
            raise EngineError(-1, last_error())

    def close(self):
        if getattr(self, "h", None):
            lib().fg_engine_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def S(self): return self.cp.S
    @property
    def d(self): return self.cp.d

    def set_stream(self, hip_stream: int):
        _check(lib().fg_engine_set_stream(self.h, hip_stream))

    def synchronize(self):
        _check(lib().fg_engine_synchronize(self.h))

    def set_values(self, cells: np.ndarray):
        a = np.ascontiguousarray(cells, dtype=np.int64)
        assert a.shape == (self.S, self.C), a.shape
        _check(lib().fg_engine_set_values(self.h, a.ctypes.data))

    def get_values(self) -> np.ndarray:
        a = np.zeros((max(1, self.S), self.C), dtype=np.int64)
        _check(lib().fg_engine_get_values(self.h, a.ctypes.data))
        return a[:self.S]

    def prior_init(self, iteration: int = 0) -> np.ndarray:
        acc = np.zeros((3, self.C))
        _check(lib().fg_prior_init(self.h, iteration, _dp(acc)))
        return acc

    def log_joint(self, want_logp: bool = False):
        acc = np.zeros((3, self.C))
        logp = np.zeros((max(1, self.S), self.C)) if want_logp else None
        _check(lib().fg_log_joint(self.h, _dp(acc), _dp(logp) if want_logp else None))
        return (acc, logp[:self.S]) if want_logp else acc

    def grid(self, site_a, a_values, site_b=None, b_values=None, base_chunk: int = 0):
        """`fg_grid_new`: the log-joint surfaces of this engine's chains over the axes of one or two f64 sites (fugue_amd/grid.py:
        `LogJointGrid`), sites by address or sorted index.  Close it before the engine."""
        from .grid import LogJointGrid
        return LogJointGrid(self, site_a, a_values, site_b, b_values, base_chunk)

    def gibbs(self, sites=None):
        """`fg_gibbs_new`: the exact Gibbs transition of this engine's chains over the discrete sites `sites` (addresses or sorted
        indices, in visiting order; None: every discrete site whose finite support constants state) -- fugue_amd/gibbs.py:
        `GibbsSweep`.  Close it before the engine."""
        from .gibbs import GibbsSweep
        return GibbsSweep(self, sites)

    def result_eval(self, d_draws: Optional[int], n: int, rows: Optional[Sequence[int]] = None, out: Optional[int] = None) -> int:
        """`fg_result_eval`: the model's return value for every draw and chain of the device buffer d_draws [n][n_rows][C] (row j =
        sorted site rows[j]; rows=None: the HMC draw layout, the d f64 sites) into the device buffer `out` [n][R][C] (allocated here
        when None: the caller frees it), asynchronously.  d_draws=None with n=1 evaluates at the engine's current values."""
        n = int(n)
        if out is None:
            out = self.device_alloc(max(1, n * self.cp.R * self.C) * 8)
        if d_draws is None:
            rp, n_rows = None, 0
        elif rows is None:
            rp, n_rows = None, self.d
        else:
            rows = list(rows)
            rp, n_rows = (C.c_int32 * max(1, len(rows)))(*rows), len(rows)
        _check(lib().fg_result_eval(self.h, d_draws, n, rp, n_rows, out))
        return out

    def predict_eval(self, d_draws: Optional[int], n: int, rows: Optional[Sequence[int]] = None, iter0: int = 0, sel: Optional[Sequence[int]] = None,
                     out=None, loglik=None):
        """`fg_predict_eval`: replicated data of the observe statements for every draw and chain of the device buffer d_draws
        [n][n_rows][C] (rows as in `result_eval`; d_draws=None with n=1: the engine's current values), drawn from the stream
        (seed, chain, iter0 + t, 9).  `sel`: program-order indices of the observe statements to keep (None: all O).  `out` / `loglik`:
        device buffers [n][n_sel][C] of cells / doubles; None allocates one (the caller frees it), False leaves that table out.
        Returns (out, loglik) with None for a table left out.  Asynchronous."""
        n = int(n)
        n_sel = self.cp.O if sel is None else len(list(sel))
        words = max(1, n * n_sel * self.C) * 8
        mine = []
        try:
            if out is None:
                out = self.device_alloc(words); mine.append(out)
            if loglik is None:
                loglik = self.device_alloc(words); mine.append(loglik)
            out, loglik = (None if out is False else out), (None if loglik is False else loglik)
            if d_draws is None:
                rp, n_rows = None, 0
            elif rows is None:
                rp, n_rows = None, self.d
            else:
                rows = list(rows)
                rp, n_rows = (C.c_int32 * max(1, len(rows)))(*rows), len(rows)
            sp = None if sel is None else (C.c_int32 * max(1, n_sel))(*[int(k) for k in sel])
            _check(lib().fg_predict_eval(self.h, d_draws, n, rp, n_rows, int(iter0) & 0xFFFFFFFF, sp, n_sel, out, loglik))
        except Exception:
            for b in mine:
                self.device_free(b)
            raise
        return out, loglik

    def result_values(self) -> np.ndarray:
        """The model's return value at the engine's current values, [R][C] (a particle's `A`; HmcSession::result, hmc.rs:761)."""
        out = self.result_eval(None, 1)
        try:
            return self.download(out, (self.cp.R, self.C))
        finally:
            self.device_free(out)

    def log_joint_stream(self, want_records: bool = False):
        """ScoreGivenTrace over the score stream: acc [3][C] (and every statement's log-density [n_records][C])."""
        acc = np.zeros((3, self.C))
        rec = np.zeros((max(1, self.cp.stream_records[1]), self.C)) if want_records else None
        _check(lib().fg_log_joint_stream(self.h, _dp(acc), _dp(rec) if want_records else None))
        return (acc, rec[:self.cp.stream_records[1]]) if want_records else acc

    def log_joint_compiled(self) -> np.ndarray:
        """ScoreGivenTrace through the unit compiled at run time (k_log_joint_jit), acc [3][C]; EngineError where the program has none."""
        acc = np.zeros((3, self.C))
        _check(lib().fg_log_joint_compiled(self.h, _dp(acc)))
        return acc

    # ---- HMC ----------------------------------------------------------------------------
    def hmc_init(self, cfg: fg_hmc_config, n_warmup: int):
        _check(lib().fg_hmc_init(self.h, C.byref(cfg), int(n_warmup)))

    def hmc_step(self, n: int, d_draws: Optional[int] = None):
        _check(lib().fg_hmc_step(self.h, int(n), d_draws))

    def hmc_step_info(self, n: int):
        """n transitions with HmcStepInfo: returns positions [n][d][C] and a dict of [n][C] arrays."""
        n = int(n)
        d_pos = self.device_alloc(max(1, n * self.d * self.C) * 8)
        d_info = self.device_alloc(max(1, n * 4 * self.C) * 8)
        try:
            _check(lib().fg_hmc_step_info(self.h, n, d_pos, d_info))
            pos = self.download(d_pos, (n, self.d, self.C))
            info = self.download(d_info, (n, 4, self.C))
        finally:
            self.device_free(d_pos)
            self.device_free(d_info)
        return pos, dict(accepted=info[:, 0] != 0, divergent=info[:, 1] != 0, accept_prob=info[:, 2], step_size=info[:, 3])

    def hmc_mass(self) -> np.ndarray:
        a = np.zeros((max(1, self.d), self.C))
        _check(lib().fg_hmc_get_mass(self.h, _dp(a)))
        return a[:self.d]

    def hmc_run(self, cfg: fg_hmc_config, n_samples: int, n_warmup: int, d_draws: Optional[int] = None) -> fg_hmc_stats:
        st = fg_hmc_stats()
        _check(lib().fg_hmc_run(self.h, C.byref(cfg), int(n_samples), int(n_warmup), d_draws, C.byref(st)))
        return st

    def hmc_stats(self) -> fg_hmc_stats:
        st = fg_hmc_stats()
        _check(lib().fg_hmc_get_stats(self.h, C.byref(st)))
        return st

    def hmc_step_sizes(self) -> np.ndarray:
        a = np.zeros(self.C)
        _check(lib().fg_hmc_get_step_sizes(self.h, _dp(a)))
        return a

    def hmc_log_joint(self) -> np.ndarray:
        a = np.zeros(self.C)
        _check(lib().fg_hmc_get_log_joint(self.h, _dp(a)))
        return a

    def hmc_set_step_size(self, eps: float):
        _check(lib().fg_hmc_set_step_size(self.h, float(eps)))

    def hmc_set_n_leapfrog(self, n: int):
        _check(lib().fg_hmc_set_n_leapfrog(self.h, int(n)))

    def hmc_is_warming_up(self) -> bool:
        return bool(lib().fg_hmc_is_warming_up(self.h))

    def hmc_iterations(self) -> int:
        return int(lib().fg_hmc_iterations(self.h))

    def hmc_short_quotient(self) -> bool:
        """Whether k_hmc_sep_steps's sparse trajectories divide by 2h in two instructions (the host proved it exact for this h)."""
        return bool(lib().fg_hmc_short_quotient(self.h))

    def hmc_range_proved(self) -> bool:
        """Whether the folded loop of those trajectories runs without its range test (the host bounded every numerator for this program and h)."""
        return bool(lib().fg_hmc_range_proved(self.h))

    def hmc_step_recorded(self, chain_ids: Sequence[int], n_leapfrog: int):
        """`HmcSession::step_recorded` for every chain; returns (trajectories [K][L+1][d], Hamiltonians [K][L+1],
        points recorded [K]) of the chosen chains."""
        ids = np.ascontiguousarray(chain_ids, dtype=np.int64)
        K, L = ids.size, int(n_leapfrog)
        traj, ham = np.zeros((max(1, K), L + 1, max(1, self.d))), np.zeros((max(1, K), L + 1))
        npts = np.zeros(max(1, K), dtype=np.int32)
        _check(lib().fg_hmc_step_recorded(self.h, K, ids.ctypes.data_as(C.POINTER(C.c_int64)), _dp(traj), _dp(ham),
                                          npts.ctypes.data_as(C.POINTER(C.c_int32)), None))
        return traj[:K, :, :self.d], ham[:K], npts[:K]

    def state_export(self) -> bytes:
        n = lib().fg_state_size(self.h)
        buf = C.create_string_buffer(n)
        _check(lib().fg_state_export(self.h, buf, n))
        return buf.raw

    def state_import(self, blob: bytes):
        _check(lib().fg_state_import(self.h, blob, len(blob)))

    def hmc_grad(self, h: float = 1e-5, grad_mode: int = GRAD_FD_DENSE):
        g = np.zeros((max(1, self.d), self.C))
        ok = np.zeros(self.C, dtype=np.int32)
        _check(lib().fg_hmc_grad(self.h, float(h), int(grad_mode), _dp(g), ok.ctypes.data_as(C.POINTER(C.c_int32))))
        return g[:self.d], ok.astype(bool)

    def hmc_transition_injected(self, cfg: fg_hmc_config, eps: float, p0: np.ndarray, u: np.ndarray):
        p0 = np.ascontiguousarray(p0, dtype=np.float64)
        u = np.ascontiguousarray(u, dtype=np.float64)
        assert p0.shape == (self.d, self.C) and u.shape == (self.C,)
        acc = np.zeros(self.C, dtype=np.int32)
        div = np.zeros(self.C, dtype=np.int32)
        alpha, lj = np.zeros(self.C), np.zeros(self.C)
        ip = C.POINTER(C.c_int32)
        _check(lib().fg_hmc_transition_injected(self.h, C.byref(cfg), float(eps), _dp(p0), _dp(u), acc.ctypes.data_as(ip),
                                                _dp(alpha), div.ctypes.data_as(ip), _dp(lj)))
        return acc.astype(bool), alpha, div.astype(bool), lj

    def hmc_find_eps_injected(self, cfg: fg_hmc_config, p0: np.ndarray) -> np.ndarray:
        p0 = np.ascontiguousarray(p0, dtype=np.float64)
        eps = np.zeros(self.C)
        _check(lib().fg_hmc_find_eps_injected(self.h, C.byref(cfg), _dp(p0), _dp(eps)))
        return eps

    # ---- MH -----------------------------------------------------------------------------
    def _overrides(self, overrides):
        if overrides is None:
            return None
        arr = (fg_site_proposal * max(1, self.S))()
        for j, o in enumerate(overrides):
            arr[j] = fg_site_proposal(*o) if o is not None else fg_site_proposal(0, 0.0, 0.0)
        return arr

    def mh_init(self, n_warmup: int, overrides=None):
        _check(lib().fg_mh_init(self.h, int(n_warmup), self._overrides(overrides)))

    def mh_step(self, n: int, rec_sites: Sequence[int] = (), d_draws: Optional[int] = None):
        rec = (C.c_int32 * max(1, len(rec_sites)))(*rec_sites)
        _check(lib().fg_mh_step(self.h, int(n), rec, len(rec_sites), d_draws))

    def mh_set_recording(self, during_adaptation: bool):
        """Record after every step, adapting or not (incremental sessions: fugue_amd.session)."""
        _check(lib().fg_mh_set_recording(self.h, 1 if during_adaptation else 0))

    def mh_run(self, n_samples: int, n_warmup: int, overrides=None, rec_sites: Sequence[int] = (), d_draws=None) -> fg_mh_stats:
        rec = (C.c_int32 * max(1, len(rec_sites)))(*rec_sites)
        st = fg_mh_stats()
        _check(lib().fg_mh_run(self.h, int(n_samples), int(n_warmup), self._overrides(overrides), rec, len(rec_sites),
                               d_draws, C.byref(st)))
        return st

    def mh_stats(self) -> fg_mh_stats:
        st = fg_mh_stats()
        _check(lib().fg_mh_get_stats(self.h, C.byref(st)))
        return st

    def mh_scales(self) -> np.ndarray:
        a = np.zeros((max(1, self.S), self.C))
        _check(lib().fg_mh_get_scales(self.h, _dp(a)))
        return a[:self.S]

    def mh_log_weight(self) -> np.ndarray:
        a = np.zeros(self.C)
        _check(lib().fg_mh_get_log_weight(self.h, _dp(a)))
        return a

    # ---- SMC ----------------------------------------------------------------------------
    def smc_run(self, resampling_method=RESAMPLE_SYSTEMATIC, ess_threshold=0.5, rejuvenation_steps=0, max_betas=10000, download=True, sequential_adaptation=False):
        """`adaptive_smc` (/root/reference/src/inference/smc.rs:455-581) over this engine's chains as particles.
        download=False leaves particles and weights in HBM (engine values / fg_smc_run's device state): only the
        evidence, the ladder and the counters come back."""
        cfg = fg_smc_config(int(resampling_method), float(ess_threshold), int(rejuvenation_steps), 1 if sequential_adaptation else 0)
        res = fg_smc_result()
        betas = np.zeros(max_betas)
        log_w, w = (np.zeros(self.C), np.zeros(self.C)) if download else (None, None)
        _check(lib().fg_smc_run(self.h, C.byref(cfg), _dp(log_w) if download else None, _dp(w) if download else None, C.byref(res), _dp(betas), max_betas))
        return dict(values=self.get_values() if download else None, log_w=log_w, weights=w, log_evidence=res.log_evidence,
                    betas=betas[:res.n_steps], n_model_runs=res.n_model_runs)

    # standalone building blocks (smc.rs:230-349, 698-790) over the engine's particle population
    def smc_prior_particles(self, iteration: int = 0):
        _check(lib().fg_smc_prior_particles(self.h, int(iteration)))

    def smc_normalize(self):
        _check(lib().fg_smc_normalize(self.h))

    def smc_ess(self) -> float:
        out = C.c_double()
        _check(lib().fg_smc_ess(self.h, C.byref(out)))
        return out.value

    def smc_resample(self, method: int = RESAMPLE_SYSTEMATIC, step: int = 1) -> np.ndarray:
        idx = np.zeros(self.C, dtype=np.int64)
        _check(lib().fg_smc_resample(self.h, int(method), int(step), idx.ctypes.data_as(C.POINTER(C.c_int64))))
        return idx

    def smc_rejuvenate(self, beta: float, steps: int, first_move_id: int = 0) -> float:
        out = C.c_double()
        _check(lib().fg_smc_rejuvenate(self.h, float(beta), int(steps), int(first_move_id), C.byref(out)))
        return out.value

    def smc_weights(self):
        lw, w = np.zeros(self.C), np.zeros(self.C)
        _check(lib().fg_smc_get_weights(self.h, _dp(lw), _dp(w)))
        return lw, w

    def smc_set_log_weights(self, log_w):
        a = np.ascontiguousarray(log_w, dtype=np.float64)
        assert a.shape == (self.C,)
        _check(lib().fg_smc_set_log_weights(self.h, _dp(a)))

    # ---- mean-field VI (fg_vi.hip) ------------------------------------------------------------
    @staticmethod
    def _vi_factors(rows):
        """rows: [n_eval][n_factors] of (family, site, a, b) -> a flat fg_vi_factor array."""
        flat = [q for row in rows for q in row]
        arr = (fg_vi_factor * max(1, len(flat)))()
        for i, (fam, site, a, b) in enumerate(flat):
            arr[i] = fg_vi_factor(int(fam), int(site), float(a), float(b))
        return arr

    def vi_elbo_batch(self, rows, stream_ids, want_terms: bool = False):
        """`elbo_with_guide` of every guide in `rows` ([n_eval][n_factors] of (family, site, a, b), address-sorted) over this
        engine's chains as samples: ELBOs [n_eval] (and every sample's term [n_eval][C])."""
        n_eval, n_factors = len(rows), (len(rows[0]) if rows else 0)
        assert all(len(r) == n_factors for r in rows) and len(stream_ids) == n_eval
        sid = np.ascontiguousarray(stream_ids, dtype=np.uint32)
        elbo = np.zeros(max(1, n_eval))
        terms = np.zeros((max(1, n_eval), self.C)) if want_terms else None
        _check(lib().fg_vi_elbo_batch(self.h, self._vi_factors(rows), n_eval, n_factors, sid.ctypes.data_as(C.POINTER(C.c_uint32)), _dp(elbo),
                                      _dp(terms) if want_terms else None))
        return (elbo[:n_eval], terms[:n_eval]) if want_terms else elbo[:n_eval]

    def vi_optimize(self, factors, cfg: fg_vi_config):
        """`optimize_meanfield_vi_with_config`: -> (optimized factors [(family, site, a, b)], elbo_history, converged, iterations)."""
        arr = self._vi_factors([factors])
        hist = np.zeros(max(1, cfg.n_iterations))
        res = fg_vi_result()
        _check(lib().fg_vi_optimize(self.h, arr, len(factors), C.byref(cfg), _dp(hist), C.byref(res)))
        out = [(arr[i].family, arr[i].site, arr[i].a, arr[i].b) for i in range(len(factors))]
        return out, hist[:res.iterations], bool(res.converged), int(res.iterations)

    def vi_estimate_elbo(self, iteration: int = 0) -> float:
        out = C.c_double()
        _check(lib().fg_vi_estimate_elbo(self.h, int(iteration), C.byref(out)))
        return out.value

    # ---- diagnostics kernels -----------------------------------------------------------------
    def diag_chain_moments(self, d_draws: int, n: int, d: int, d_moments: int):
        _check(lib().fg_diag_chain_moments(self.h, d_draws, int(n), int(d), d_moments))

    def diag_autocov_sums(self, d_draws: int, n: int, d: int, d_moments: int, lag0: int, n_lags: int) -> np.ndarray:
        out = np.zeros((d, n_lags))
        _check(lib().fg_diag_autocov_sums(self.h, d_draws, int(n), int(d), d_moments, int(lag0), int(n_lags), _dp(out)))
        return out

    def diag_geweke(self, d_draws: int, n: int, d: int) -> np.ndarray:
        """`geweke_diagnostic` of every (coordinate, chain) on the device: [d][C]."""
        d_z = self.device_alloc(max(1, d * self.C) * 8)
        try:
            _check(lib().fg_diag_geweke(self.h, d_draws, int(n), int(d), d_z))
            return self.download(d_z, (d, self.C))
        finally:
            self.device_free(d_z)

    def diag_rhat_ess(self, d_draws: int, n: int, d: int, comm: Optional[int] = None, exchange: Optional[int] = None):
        """Split R-hat, multi-chain ESS, pooled mean / std of d_draws [n][d][C] over the chains of every rank of `comm`
        (an RCCL communicator from `comm_init`; None = this engine's chains): computed inside the library.  `exchange`:
        DIAG_REDUCE (default: all-reduces of O(d) chain sums) or DIAG_GATHER (all-gather of every chain's moments)."""
        rhat, ess, mean, std = (np.zeros(d) for _ in range(4))
        tot = C.c_int64()
        if exchange is not None:
            _check(lib().fg_diag_set_exchange(self.h, int(exchange)))
        _check(lib().fg_diag_rhat_ess(self.h, d_draws, int(n), int(d), comm, _dp(rhat), _dp(ess), _dp(mean), _dp(std), C.byref(tot)))
        return dict(r_hat=rhat, ess=ess, mean=mean, std=std, chains=tot.value, exchange_bytes=int(lib().fg_diag_exchange_bytes(self.h)))

    def diag_quantiles(self, d_draws: int, n: int, d: int, probs=(0.025, 0.25, 0.5, 0.75, 0.975), comm: Optional[int] = None) -> np.ndarray:
        """summarize_f64_parameter's quantiles (diagnostics.rs:355-371) of every coordinate of d_draws [n][d][C], selected on the
        device over the draws of every rank of `comm`: [d][len(probs)]."""
        pr = np.ascontiguousarray(probs, dtype=np.float64)
        out = np.zeros((d, len(pr)))
        _check(lib().fg_diag_quantiles(self.h, d_draws, int(n), int(d), comm, _dp(pr), len(pr), _dp(out)))
        return out

    def diag_stream(self, n_total: int, d: int, max_lag: int = 64) -> "DiagStream":
        """A `fg_diag_stream`: the figures of `diag_rhat_ess` for `n_total` draws of `d` coordinates that arrive one chunk at a time
        and are never stored; `max_lag` (rounded up to a multiple of 32, at most 2 048) is the deepest lag Geyer's sequence may reach."""
        return DiagStream(self, n_total, d, max_lag)

    def diag_qstream(self, n_total: int, d: int, probs=(0.025, 0.25, 0.5, 0.75, 0.975), digit_bits: int = 12, capacity: int = 65536) -> "DiagQuantileStream":
        """A `fg_diag_qstream`: the quantiles of `diag_quantiles` for `n_total` draws of `d` coordinates that are never stored but
        presented once per pass (the sampling phase replayed from `state_export`'s blob), until `end_pass()` returns True."""
        return DiagQuantileStream(self, n_total, d, probs, digit_bits, capacity)

    def diag_cstream(self, n_total: int, n_rec: int, rows: Sequence[int], vtypes: Sequence[int], lo: Sequence[int], bins: Sequence[int]) -> "DiagCountStream":
        """A `fg_diag_cstream`: exact frequency tables of the integer rows `rows` of chunks [n_chunk][n_rec][C] of cells (what
        `mh_step` records) for a run of `n_total` draws that is never stored.  Row k has the ChoiceValue tag vtypes[k] and counts the
        cells equal to lo[k] + j in bin j of bins[k]; whatever lies outside is counted in `below` / `above`."""
        return DiagCountStream(self, n_total, n_rec, rows, vtypes, lo, bins)

    def loglik_stream(self, n_total: int, n_sel: int) -> "LoglikStream":
        """A `fg_loglik_stream`: WAIC and importance-sampling LOO of `n_sel` observe statements from chunks [n_chunk][n_sel][C] of the
        pointwise log-likelihood (`predict_eval`'s `loglik` table) of a run of `n_total` draws that is never stored."""
        return LoglikStream(self, n_total, n_sel)

    def psis_loo(self, d_ll: int, n: int, n_sel: int, tail: bool = False) -> dict:
        """`fg_psis_loo` (fg_psis.hip): Pareto-smoothed LOO and k-hat per observe statement of the stored table `d_ll` [n][n_sel][C] on
        the device (C this engine's chains).  -> the figures by name (PSIS_WORD_NAMES, [n_sel] doubles each), the counts by name
        (PSIS_COUNT_NAMES, [n_sel] int64 each), `words` [n_sel][14], `counts` [n_sel][10]; with `tail` also `tail` [n_sel][M], the sorted
        M smallest cells of every statement.  Reads engine state and changes none."""
        for name, v in (("n", n), ("n_sel", n_sel)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"psis_loo: {name} must be an integer, not {type(v).__name__}")
        L = lib()
        nw = int(L.fg_psis_words())
        n_sel_buf = max(int(n_sel), 1)
        words = np.zeros((n_sel_buf, nw), dtype=np.float64)
        counts = np.zeros((n_sel_buf, PSIS_COUNTS), dtype=np.int64)
        M = int(L.fg_psis_tail_len(int(n) * self.C)) if n >= 1 else 0
        d_tail = self.device_alloc(8 * n_sel_buf * M) if tail and M > 0 else None
        try:
            _check(L.fg_psis_loo(self.h, d_ll, int(n), int(n_sel), _dp(words), counts.ctypes.data_as(C.POINTER(C.c_int64)), d_tail))
            out = {name: words[:, j].copy() for j, name in enumerate(PSIS_WORD_NAMES)}
            out.update({name: counts[:, j].copy() for j, name in enumerate(PSIS_COUNT_NAMES)})
            out["words"], out["counts"] = words, counts
            if d_tail is not None:
                out["tail"] = self.download(d_tail, (int(n_sel), M))
            return out
        finally:
            if d_tail is not None:
                self.device_free(d_tail)

    def diag_rank_transform(self, d_draws: int, n: int, d: int, j0: int = 0, n_j: Optional[int] = None, probs=(0.05, 0.95), d_out: Optional[int] = None,
                            rank2: bool = False) -> dict:
        """`fg_diag_rank_transform` (fg_diag_rank.hip): the rank-normalised rows of coordinates [j0, j0 + n_j) of the stored draws
        `d_draws` [n][d][C] on the device.  -> `out` [n][4 n_j][C] (rows z, z_folded, I_lo, I_hi per coordinate; downloaded, or None when
        the caller's device buffer `d_out` received them), `median` [n_j], `counts` [n_j][8] and the counts by name (RANK_COUNT_NAMES);
        with `rank2` also `rank2` [n][n_j][C], the doubled average ranks (uint32).  Reads engine state and changes none."""
        n_j = int(d) - int(j0) if n_j is None else n_j
        for name, v in (("n", n), ("d", d), ("j0", j0), ("n_j", n_j)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"diag_rank_transform: {name} must be an integer, not {type(v).__name__}")
        p_lo, p_hi = (float(p) for p in probs)
        nb = max(int(n_j), 1)
        cells = max(int(n), 1) * nb * self.C
        median = np.zeros(nb)
        counts = np.zeros((nb, RANK_COUNTS), dtype=np.int64)
        own = self.device_alloc(8 * RANK_ROWS * cells) if d_out is None else None
        d_r2 = self.device_alloc(4 * cells) if rank2 else None
        try:
            _check(lib().fg_diag_rank_transform(self.h, d_draws, int(n), int(d), int(j0), int(n_j), p_lo, p_hi, own if d_out is None else d_out, d_r2, _dp(median),
                                                counts.ctypes.data_as(C.POINTER(C.c_int64))))
            out = {name: counts[:, j].copy() for j, name in enumerate(RANK_COUNT_NAMES)}
            out.update(out=self.download(own, (int(n), RANK_ROWS * int(n_j), self.C)) if own is not None else None, median=median, counts=counts)
            if d_r2 is not None:
                out["rank2"] = self.download(d_r2, (int(n), int(n_j), self.C), dtype=np.uint32)
            return out
        finally:
            for b in (own, d_r2):
                if b is not None:
                    self.device_free(b)

    def diag_rank(self, d_draws: int, n: int, d: int, probs=(0.05, 0.95), max_out_bytes: int = 0) -> dict:
        """`fg_diag_rank_rhat_ess` (fg_diag_rank.hip): rank-normalised split R-hat, folded R-hat, bulk and tail ESS of every coordinate of
        the stored draws `d_draws` [n][d][C] on the device (C this engine's chains).  -> the figures by name (RANK_WORD_NAMES, [d] doubles
        each), the counts by name (RANK_COUNT_NAMES, [d] int64 each), `words` [d][10], `counts` [d][8].  `max_out_bytes` bounds the
        transformed rows held at a time (0: 1 GiB); the figures do not depend on it.  Reads engine state and changes none."""
        for name, v in (("n", n), ("d", d), ("max_out_bytes", max_out_bytes)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"diag_rank: {name} must be an integer, not {type(v).__name__}")
        p_lo, p_hi = (float(p) for p in probs)
        L = lib()
        db = max(int(d), 1)
        words = np.zeros((db, int(L.fg_diag_rank_words())), dtype=np.float64)
        counts = np.zeros((db, RANK_COUNTS), dtype=np.int64)
        _check(L.fg_diag_rank_rhat_ess(self.h, d_draws, int(n), int(d), p_lo, p_hi, int(max_out_bytes), _dp(words), counts.ctypes.data_as(C.POINTER(C.c_int64))))
        out = {name: words[:, j].copy() for j, name in enumerate(RANK_WORD_NAMES)}
        out.update({name: counts[:, j].copy() for j, name in enumerate(RANK_COUNT_NAMES)})
        out["words"], out["counts"] = words, counts
        return out

    def diag_mcse_transform(self, d_draws: int, n: int, d: int, mean, j0: int = 0, n_j: Optional[int] = None, probs=(0.05, 0.5, 0.95), d_out: Optional[int] = None,
                            sorted_cells: bool = False) -> dict:
        """`fg_diag_mcse_transform` (fg_diag_mcse.hip): the rows |x - mean|, (x - mean)^2 and I_p per probability of coordinates
        [j0, j0 + n_j) of the stored draws `d_draws` [n][d][C] on the device, centred at `mean` [n_j].  -> `out` [n][(2 + len(probs)) n_j][C]
        (downloaded, or None when the caller's device buffer `d_out` received them), `median` [n_j], `mad` [n_j], `counts`
        [n_j][6 + 3 len(probs)] and the counts by name (MCSE_COUNT_NAMES; `k_p` [n_j][len(probs)]); with `sorted_cells` also `sorted`
        [n_j][n C], the sorted cells.  Reads engine state and changes none."""
        n_j = int(d) - int(j0) if n_j is None else n_j
        for name, v in (("n", n), ("d", d), ("j0", j0), ("n_j", n_j)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"diag_mcse_transform: {name} must be an integer, not {type(v).__name__}")
        pr = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        mean = np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)
        nb, npb = max(int(n_j), 1), len(pr)
        if mean.size != nb:
            raise ValueError(f"diag_mcse_transform: {mean.size} means for {nb} coordinates")
        rows = 2 + npb
        cells = max(int(n), 1) * nb * self.C
        median, mad = np.zeros(nb), np.zeros(nb)
        counts = np.zeros((nb, len(MCSE_COUNT_NAMES) + len(MCSE_PROB_COUNT_NAMES) * npb), dtype=np.int64)
        own = self.device_alloc(8 * rows * cells) if d_out is None else None
        d_sorted = self.device_alloc(8 * cells) if sorted_cells else None
        try:
            _check(lib().fg_diag_mcse_transform(self.h, d_draws, int(n), int(d), int(j0), int(n_j), _dp(mean), _dp(pr), npb, own if d_out is None else d_out, d_sorted,
                                                _dp(median), _dp(mad), counts.ctypes.data_as(C.POINTER(C.c_int64))))
            out = {name: counts[:, j].copy() for j, name in enumerate(MCSE_COUNT_NAMES)}
            out["k_p"] = counts[:, len(MCSE_COUNT_NAMES)::len(MCSE_PROB_COUNT_NAMES)].copy()
            out.update(out=self.download(own, (int(n), rows * int(n_j), self.C)) if own is not None else None, median=median, mad=mad, counts=counts, probs=pr)
            if d_sorted is not None:
                out["sorted"] = self.download(d_sorted, (int(n_j), int(n) * self.C))
            return out
        finally:
            for b in (own, d_sorted):
                if b is not None:
                    self.device_free(b)

    def diag_mcse(self, d_draws: int, n: int, d: int, probs=(0.05, 0.5, 0.95), max_out_bytes: int = 0) -> dict:
        """`fg_diag_mcse` (fg_diag_mcse.hip): the Monte Carlo standard errors and effective sample sizes of the mean, the standard deviation
        and the quantiles `probs` (at most 8), the median and the mad of every coordinate of the stored draws `d_draws` [n][d][C] on the
        device (C this engine's chains).  -> the fixed figures by name (MCSE_WORD_NAMES, [d] doubles each), the figures per probability by
        name (MCSE_PROB_WORD_NAMES, [d][len(probs)] each), the counts by name (MCSE_COUNT_NAMES [d], MCSE_PROB_COUNT_NAMES
        [d][len(probs)]), `words`, `counts`, `probs`.  `max_out_bytes` bounds the rows and sorted keys held at a time (0: 1 GiB); the
        figures do not depend on it.  Reads engine state and changes none."""
        for name, v in (("n", n), ("d", d), ("max_out_bytes", max_out_bytes)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"diag_mcse: {name} must be an integer, not {type(v).__name__}")
        pr = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        npb, nf, ncf = len(pr), len(MCSE_WORD_NAMES), len(MCSE_COUNT_NAMES)
        npw, npc = len(MCSE_PROB_WORD_NAMES), len(MCSE_PROB_COUNT_NAMES)
        L = lib()
        db = max(int(d), 1)
        words = np.zeros((db, nf + npw * max(npb, 1)), dtype=np.float64)
        counts = np.zeros((db, ncf + npc * max(npb, 1)), dtype=np.int64)
        _check(L.fg_diag_mcse(self.h, d_draws, int(n), int(d), _dp(pr), npb, int(max_out_bytes), _dp(words), counts.ctypes.data_as(C.POINTER(C.c_int64))))
        assert words.shape[1] == int(L.fg_diag_mcse_words(npb))
        out = {name: words[:, j].copy() for j, name in enumerate(MCSE_WORD_NAMES)}
        out.update({name: words[:, nf + j::npw].copy() for j, name in enumerate(MCSE_PROB_WORD_NAMES)})
        out.update({name: counts[:, j].copy() for j, name in enumerate(MCSE_COUNT_NAMES)})
        out.update({name: counts[:, ncf + j::npc].copy() for j, name in enumerate(MCSE_PROB_COUNT_NAMES)})
        out["words"], out["counts"], out["probs"] = words, counts, pr
        return out

    def ppc_stream(self, n_total: int, vtypes: Sequence[int], checks: Sequence) -> "PpcStream":
        """A `fg_ppc_stream`: posterior predictive checks from chunks [n_chunk][len(vtypes)][C] of replicated data (`predict_eval`'s cell
        table; `vtypes` the value type of every row) of a run of `n_total` draws that is never stored.  `checks`: one (member rows,
        statistics, observed values) per check -- statistics as indices or names of PPC_STATS, observed aligned with the members."""
        return PpcStream(self, n_total, vtypes, checks)

    def wpop(self, n: Optional[int] = None, d_w: Optional[int] = None) -> "WeightedPopulation":
        """A `fg_wpop`: weighted moments, exact weighted quantiles and exact weighted frequency tables of rows that stay on the
        device.  Without arguments the population is the engine's own (after `smc_run` / `smc_prior_particles`; EngineError
        FG_E_STATE without one); `d_w` is a device buffer of `n` normalised weights of the caller's."""
        return WeightedPopulation(self, n, d_w)

    def cells_f64(self, d_cells: int, n: int, n_rec: int, rows: Sequence[int], vtypes: Sequence[int], out: Optional[int] = None) -> int:
        """`fg_diag_cells_f64`: rows `rows` of the device cells [n][n_rec][C] as doubles [n][len(rows)][C] in the device buffer `out`
        (allocated here when None: the caller frees it), asynchronously: an f64 row is copied, a u64 row converted as unsigned
        (`x as f64`), bool / usize / i64 rows as signed.  The layout `diag_stream` and `diag_qstream` take."""
        rows, vtypes = [int(r) for r in rows], [int(v) for v in vtypes]
        if len(rows) != len(vtypes) or not rows:
            raise ValueError("rows and vtypes must have one entry per selected row, at least one")
        n = int(n)
        if out is None:
            out = self.device_alloc(max(1, n * len(rows) * self.C) * 8)
        _check(lib().fg_diag_cells_f64(self.h, d_cells, n, int(n_rec), (C.c_int32 * len(rows))(*rows), (C.c_int32 * len(rows))(*vtypes), len(rows), out))
        return out

    def hmc_last_kernel(self) -> str:
        """Kernel (and waves per tile) the engine's last HMC launch ran."""
        return (lib().fg_hmc_last_kernel(self.h) or b"").decode()

    def mh_last_kernel(self) -> str:
        """Kernel the engine's last MH launch ran."""
        return (lib().fg_mh_last_kernel(self.h) or b"").decode()

    def comm_init(self, world_size: int, rank: int, unique_id: bytes) -> int:
        out = C.c_void_p()
        _check(lib().fg_comm_init(self.h, int(world_size), int(rank), unique_id, C.byref(out)))
        return out.value

    # ---- raw device buffers ---------------------------------------------------------------
    def device_alloc(self, nbytes: int) -> int:
        p = lib().fg_device_alloc(self.h, int(nbytes))
        if not p:
            raise EngineError(-2, last_error())
        return p

    def device_free(self, ptr: int):
        _check(lib().fg_device_free(self.h, ptr))

    def download(self, ptr: int, shape, dtype=np.float64) -> np.ndarray:
        out = np.zeros(shape, dtype=dtype)
        _check(lib().fg_device_download(self.h, out.ctypes.data, ptr, out.nbytes))
        return out

    def upload(self, array: np.ndarray, ptr: Optional[int] = None) -> int:
        """Copy a host array into device memory (`ptr`, or a fresh `device_alloc` of its size); returns the device pointer."""
        a = np.ascontiguousarray(array)
        if ptr is None:
            ptr = self.device_alloc(max(1, a.nbytes))
        _check(lib().fg_device_upload(self.h, ptr, a.ctypes.data, a.nbytes))
        return ptr


class _Stream:
    """What the stream classes share: the engine, the handle `h` of the C object (None before it exists and once it is closed), its
    release through the entry the subclass names in `_free`, and the check of the integer arguments."""

    _free = None                     # "fg_..._free"
    engine, h = None, None

    @staticmethod
    def _integers(**named):
        for name, v in named.items():
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"{name} must be an integer, not {type(v).__name__}")

    def _handle(self):
        if not self.h:
            raise ValueError("the stream is closed")
        return self.h

    def close(self):
        if self.h:
            if getattr(self.engine, "h", None):          # the state lives in the engine's device context
                getattr(lib(), self._free)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DiagStream(_Stream):
    """`fg_diag_stream` (fg_diag_stream.hip): split R-hat, multi-chain ESS and the pooled mean / std of a run handed over in chunks.
    Constant memory per (coordinate, chain): (3 K + 7) doubles, K = `max_lag` rounded up to a multiple of 32.  Close it before its
    engine."""

    _free = "fg_diag_stream_free"

    def __init__(self, engine: Engine, n_total: int, d: int, max_lag: int = 64):
        self._integers(n_total=n_total, d=d, max_lag=max_lag)
        if n_total < 1:
            raise ValueError("n_total must be at least 1")
        if not 1 <= d <= 65535:
            raise ValueError("d must lie in [1, 65535]")
        if not 1 <= max_lag <= 2048:
            raise ValueError("max_lag must lie in [1, 2048]")
        self.engine, self.n, self.d = engine, int(n_total), int(d)
        self.K = (int(max_lag) + 31) // 32 * 32
        self.h = None
        out = C.c_void_p()
        _check(lib().fg_diag_stream_new(engine.h, self.n, self.d, int(max_lag), C.byref(out)))
        self.h = out.value

    def update(self, d_draws: int, n_chunk: int):
        """The next `n_chunk` draws, a device buffer [n_chunk][d][C]."""
        _check(lib().fg_diag_stream_update(self._handle(), d_draws, int(n_chunk)))

    @property
    def count(self) -> int:
        return int(lib().fg_diag_stream_count(self._handle()))

    def moments(self) -> np.ndarray:
        """[d][6][C] as `Engine.diag_chain_moments` gives for a stored buffer."""
        eng = self.engine
        d_mom = eng.device_alloc(max(1, self.d * 6 * eng.C) * 8)
        try:
            _check(lib().fg_diag_stream_moments(self._handle(), d_mom))
            return eng.download(d_mom, (self.d, 6, eng.C))
        finally:
            eng.device_free(d_mom)

    def autocov_sums(self, lag0: int, n_lags: int) -> np.ndarray:
        out = np.zeros((self.d, int(n_lags)))
        _check(lib().fg_diag_stream_autocov_sums(self._handle(), int(lag0), int(n_lags), _dp(out)))
        return out

    def rhat_ess(self, comm: Optional[int] = None, exchange: Optional[int] = None, want_ess: bool = True):
        """As `Engine.diag_rhat_ess`.  An ESS whose Geyer sequence runs past the stream's K lags raises EngineError (FG_E_LIMIT);
        `want_ess=False` asks for no lag and returns R-hat / mean / std alone (ess = None)."""
        d = self.d
        rhat, ess, mean, std = (np.zeros(d) for _ in range(4))
        tot = C.c_int64()
        if exchange is not None:
            _check(lib().fg_diag_set_exchange(self.engine.h, int(exchange)))
        _check(lib().fg_diag_stream_rhat_ess(self._handle(), comm, _dp(rhat), _dp(ess) if want_ess else None, _dp(mean), _dp(std), C.byref(tot)))
        return dict(r_hat=rhat, ess=ess if want_ess else None, mean=mean, std=std, chains=tot.value,
                    exchange_bytes=int(lib().fg_diag_exchange_bytes(self.engine.h)))



class DiagQuantileStream(_Stream):
    """`fg_diag_qstream` (fg_diag_qstream.hip): summarize_f64_parameter's quantiles (diagnostics.rs:355-371) by exact radix select
    over a run that is presented once per pass.  A pass is `n_total` draws through `update`, then `end_pass()`; while that returns
    False the same draws must be presented again (in any chunking).  A pass that does not reproduce the previous one raises
    EngineError (FG_E_STATE).  Device memory: d x len(probs) x (2^digit_bits counters + capacity keys).  Close it before its engine."""

    _free = "fg_diag_qstream_free"

    def __init__(self, engine: Engine, n_total: int, d: int, probs=(0.025, 0.25, 0.5, 0.75, 0.975), digit_bits: int = 12, capacity: int = 65536):
        self._integers(n_total=n_total, d=d, digit_bits=digit_bits, capacity=capacity)
        pr = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        if n_total < 1:
            raise ValueError("n_total must be at least 1")
        if not 1 <= d <= 65535:
            raise ValueError("d must lie in [1, 65535]")
        if not 1 <= pr.size <= 8:
            raise ValueError("between 1 and 8 probabilities")
        if not np.all((pr >= 0.0) & (pr <= 1.0)):
            raise ValueError("probabilities must lie in [0, 1]")
        if not 1 <= digit_bits <= 12:
            raise ValueError("digit_bits must lie in [1, 12]")
        if capacity < 0:
            raise ValueError("capacity must not be negative")
        self.engine, self.n, self.d, self.probs = engine, int(n_total), int(d), pr
        self.h = None
        out = C.c_void_p()
        _check(lib().fg_diag_qstream_new(engine.h, self.n, self.d, _dp(pr), pr.size, int(digit_bits), int(capacity), C.byref(out)))
        self.h = out.value

    def update(self, d_draws: int, n_chunk: int):
        """The next `n_chunk` draws of the current pass, a device buffer [n_chunk][d][C]."""
        _check(lib().fg_diag_qstream_update(self._handle(), d_draws, int(n_chunk)))

    @property
    def count(self) -> int:
        """Draws taken in the current pass."""
        return int(lib().fg_diag_qstream_count(self._handle()))

    def end_pass(self) -> bool:
        """Ends the pass; True when every quantile is selected, False when the run must be presented again."""
        done = C.c_int()
        _check(lib().fg_diag_qstream_end_pass(self._handle(), C.byref(done)))
        return bool(done.value)

    @property
    def passes(self) -> int:
        """Passes completed."""
        return int(lib().fg_diag_qstream_passes(self._handle()))

    def result(self):
        """(values [d][len(probs)], slot_passes [d][len(probs)]: the passes each quantile took part in)."""
        out = np.zeros((self.d, self.probs.size))
        sp = np.zeros((self.d, self.probs.size), dtype=np.int32)
        _check(lib().fg_diag_qstream_result(self._handle(), _dp(out), sp.ctypes.data_as(C.POINTER(C.c_int32))))
        return out, sp



class DiagCountStream(_Stream):
    """`fg_diag_cstream` (fg_diag_cstream.hip): exact posterior frequency tables of integer rows (the tabulation of the reference's
    extract_bool_values / extract_u64_values / extract_usize_values / extract_i64_values, diagnostics.rs:76-98) of a run handed over
    in chunks of cells [n_chunk][n_rec][C].  Integer sums: the result does not depend on the chunking.  Close it before its engine."""

    _free = "fg_diag_cstream_free"

    def __init__(self, engine: Engine, n_total: int, n_rec: int, rows: Sequence[int], vtypes: Sequence[int], lo: Sequence[int], bins: Sequence[int]):
        self._integers(n_total=n_total, n_rec=n_rec)
        self.rows, self.vtypes = [int(r) for r in rows], [int(v) for v in vtypes]
        self.lo, self.bins = [int(v) for v in lo], [int(b) for b in bins]
        nw = len(self.rows)
        if not (nw == len(self.vtypes) == len(self.lo) == len(self.bins)):
            raise ValueError("rows, vtypes, lo and bins must have one entry per watched row")
        if not 1 <= nw <= 65535:
            raise ValueError("between 1 and 65535 watched rows")
        if any(not -2 ** 63 <= v < 2 ** 63 for v in self.lo):
            raise ValueError("lo must fit 64 signed bits")
        self.engine, self.n, self.n_rec = engine, int(n_total), int(n_rec)
        self.h = None
        out = C.c_void_p()
        i32 = lambda v: (C.c_int32 * nw)(*v)
        _check(lib().fg_diag_cstream_new(engine.h, self.n, self.n_rec, i32(self.rows), i32(self.vtypes), (C.c_int64 * nw)(*self.lo), i32(self.bins), nw, C.byref(out)))
        self.h = out.value

    def update(self, d_cells: int, n_chunk: int):
        """The next `n_chunk` draws, a device buffer of cells [n_chunk][n_rec][C]."""
        _check(lib().fg_diag_cstream_update(self._handle(), d_cells, int(n_chunk)))

    @property
    def count(self) -> int:
        return int(lib().fg_diag_cstream_count(self._handle()))

    def result(self) -> dict:
        """counts: a list of uint64 arrays [bins[k]]; below / above: uint64 [n_watch]; min / max: lists of Python ints [n_watch]
        (a u64 row's are unsigned, so they may pass 2^63).  Raises EngineError (FG_E_STATE) before
        `n_total` draws have arrived or when a row's total is not n_total x C."""
        nw = len(self.rows)
        flat = np.zeros(max(1, sum(self.bins)), dtype=np.uint64)
        below, above = np.zeros(nw, dtype=np.uint64), np.zeros(nw, dtype=np.uint64)
        mn, mx = np.zeros(nw, dtype=np.int64), np.zeros(nw, dtype=np.int64)
        u64p, i64p = C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
        _check(lib().fg_diag_cstream_result(self._handle(), flat.ctypes.data_as(u64p), below.ctypes.data_as(u64p), above.ctypes.data_as(u64p),
                                            mn.ctypes.data_as(i64p), mx.ctypes.data_as(i64p)))
        at = np.concatenate([[0], np.cumsum(self.bins)])
        counts = [flat[at[k]:at[k + 1]].copy() for k in range(nw)]
        unsigned = lambda a: [int(v) & (2 ** 64 - 1) if self.vtypes[k] == M.U64 else int(v) for k, v in enumerate(a)]
        return dict(counts=counts, below=below, above=above, min=unsigned(mn), max=unsigned(mx))



LL_POOLED, LL_FIGURES = 8, 8                # FG_LL_POOLED, FG_LL_FIGURES
LL_POOLED_WORDS = ("mx", "sp", "mn", "sn", "sn2", "n_fin", "mean", "ssd")
LL_FIGURE_NAMES = ("lppd", "mean_ll", "p_waic", "elpd_waic", "elpd_loo", "p_loo", "is_ess", "max_weight")


class LoglikStream(_Stream):
    """`fg_loglik_stream` (fg_loglik_stream.hip): WAIC and importance-sampling LOO per observe statement from the pointwise
    log-likelihood of a run handed over in chunks [n_chunk][n_sel][C] of doubles (`Engine.predict_eval`'s `loglik` table).  Every
    (statement, chain) column is updated in draw order by one thread and the chains are pooled by a fixed tree on the chain index, so
    the result does not depend on the chunking, bit for bit.  Device memory: 80 x n_sel x C bytes (5.4 GB at n_sel = 1 024 and
    C = 65 536; select the statements to compare with `predict_eval`'s `sel`).  Close it before its engine."""

    _free = "fg_loglik_stream_free"

    def __init__(self, engine: Engine, n_total: int, n_sel: int):
        self._integers(n_total=n_total, n_sel=n_sel)
        self.engine, self.n, self.n_sel = engine, int(n_total), int(n_sel)
        self.h = None
        out = C.c_void_p()
        _check(lib().fg_loglik_stream_new(engine.h, self.n, self.n_sel, C.byref(out)))
        self.h = out.value

    def update(self, d_loglik: int, n_chunk: int):
        """The next `n_chunk` draws, a device buffer of doubles [n_chunk][n_sel][C]; asynchronous.  n_chunk = 0 does nothing."""
        _check(lib().fg_loglik_stream_update(self._handle(), d_loglik, int(n_chunk)))

    def count(self) -> int:
        return int(lib().fg_loglik_stream_count(self._handle()))

    def pooled(self) -> dict:
        """The pooled words of every statement: `words` float64 [n_sel][8] in the order LL_POOLED_WORDS, `counts` int64 [n_sel][3]
        (cells that are -inf, +inf, NaN).  Raises EngineError (FG_E_STATE) before `n_total` draws have arrived."""
        words, counts = np.zeros((self.n_sel, LL_POOLED)), np.zeros((self.n_sel, 3), dtype=np.int64)
        _check(lib().fg_loglik_stream_pooled(self._handle(), _dp(words), counts.ctypes.data_as(C.POINTER(C.c_int64))))
        return dict(words=words, counts=counts)

    def result(self) -> dict:
        """The figures of every statement, each float64 [n_sel]: lppd, mean_ll, p_waic (divisor N - 1), elpd_waic, elpd_loo, p_loo,
        is_ess, max_weight; and n_neg_inf, n_pos_inf, n_nan int64 [n_sel].  Raises EngineError (FG_E_STATE) before `n_total` draws."""
        figs, counts = np.zeros((LL_FIGURES, self.n_sel)), np.zeros((self.n_sel, 3), dtype=np.int64)
        _check(lib().fg_loglik_stream_result(self._handle(), _dp(figs), counts.ctypes.data_as(C.POINTER(C.c_int64))))
        out = {name: figs[i].copy() for i, name in enumerate(LL_FIGURE_NAMES)}
        out.update(n_neg_inf=counts[:, 0].copy(), n_pos_inf=counts[:, 1].copy(), n_nan=counts[:, 2].copy())
        return out

    free = _Stream.close


PPC_STATS = ("mean", "var", "min", "max", "sum")          # FG_PPC_MEAN .. FG_PPC_SUM
PPC_COUNTS = ("n_lt", "n_eq", "n_gt", "n_nan", "n_fin")
PPC_SCRATCH_DRAWS = 16                                    # FG_PPC_SCRATCH_DRAWS (fg_ppc_stream_plan.h): an update walks its chunk in pieces of that many draws


def _ppc_csr(checks):
    """checks [(rows, statistics, observed)] -> (offsets, members, masks, observed, slots): the CSR form of the C entry points, and the
    (check, statistic) pair of every slot."""
    offsets, members, masks, observed, slots = [0], [], [], [], []
    for q, (rows, stats, obs) in enumerate(checks):
        rows, obs = [int(r) for r in rows], [float(v) for v in obs]
        if len(rows) != len(obs):
            raise ValueError(f"check {q}: {len(rows)} members and {len(obs)} observed values")
        ids = sorted({PPC_STATS.index(st) if isinstance(st, str) else int(st) for st in stats})
        mask = 0
        for st in ids:
            mask |= 1 << st
        members += rows
        observed += obs
        offsets.append(len(members))
        masks.append(mask)
        slots += [(q, st) for st in ids if 0 <= st < len(PPC_STATS)]
    return offsets, members, masks, observed, slots


class PpcStream(_Stream):
    """`fg_ppc_stream` (fg_ppc_stream.hip): test statistics of every replicated data set of a run handed over in chunks
    [n_chunk][n_rows][C] of raw cells (`Engine.predict_eval`'s cell table), compared with the observed ones -- what the reference's
    workflows do on the host after replicating the data (tests/end_to_end_workflows.rs:650-745).  A slot is a (check, statistic)
    pair, in check order, then in the order of PPC_STATS; `slots` lists them.  Every (slot, chain) column is updated in draw order by
    one thread and the chains are pooled by a fixed tree on the chain index, so the result does not depend on the chunking, bit for
    bit.  Device memory: 48 x n_slots x C bytes of state and a scratch table of 16 draws' statistics.  Close it before its engine."""

    _free = "fg_ppc_stream_free"

    def __init__(self, engine: Engine, n_total: int, vtypes: Sequence[int], checks):
        self._integers(n_total=n_total)
        self.engine, self.n, self.h = engine, int(n_total), None
        vt = [int(v) for v in vtypes]
        offsets, members, masks, observed, self.slots = _ppc_csr(checks)
        i32 = lambda v: (C.c_int32 * max(1, len(v)))(*v)
        out = C.c_void_p()
        _check(lib().fg_ppc_stream_new(engine.h, self.n, len(vt), i32(vt), len(masks), i32(offsets), i32(members), i32(masks),
                                       (C.c_double * max(1, len(observed)))(*observed), C.byref(out)))
        self.h = out.value
        self.n_slots = int(lib().fg_ppc_stream_n_slots(self.h))

    def update(self, d_yrep: int, n_chunk: int):
        """The next `n_chunk` draws, a device buffer of cells [n_chunk][n_rows][C]; asynchronous.  n_chunk = 0 does nothing."""
        _check(lib().fg_ppc_stream_update(self._handle(), d_yrep, int(n_chunk)))

    def count(self) -> int:
        return int(lib().fg_ppc_stream_count(self._handle()))

    def observed(self) -> np.ndarray:
        """T_obs float64 [n_slots]: the statistic of every slot's observed vector."""
        t = np.zeros(self.n_slots)
        _check(lib().fg_ppc_stream_observed(self._handle(), _dp(t)))
        return t

    def pooled(self) -> dict:
        """Pooled over the chains, per slot: n_lt, n_eq, n_gt, n_nan, n_fin int64 [n_slots] (draws whose statistic is below / equal to /
        above the observed one, NaN draws, finite statistics) and `mean`, `ssd` float64 [n_slots] of the finite statistics.  Raises
        EngineError (FG_E_STATE) before `n_total` draws have arrived."""
        counts, mom = np.zeros((self.n_slots, 5), dtype=np.int64), np.zeros((self.n_slots, 2))
        _check(lib().fg_ppc_stream_pooled(self._handle(), counts.ctypes.data_as(C.POINTER(C.c_int64)), _dp(mom)))
        out = {name: counts[:, i].copy() for i, name in enumerate(PPC_COUNTS)}
        out.update(mean=mom[:, 0].copy(), ssd=mom[:, 1].copy())
        return out

    def chains(self, slot: int) -> dict:
        """The five counters of one slot per chain, each int64 [C]."""
        counts = np.zeros((5, self.engine.C), dtype=np.int64)
        _check(lib().fg_ppc_stream_chains(self._handle(), int(slot), counts.ctypes.data_as(C.POINTER(C.c_int64))))
        return {name: counts[i].copy() for i, name in enumerate(PPC_COUNTS)}

    free = _Stream.close


WPOP_MOMENTS = ("W", "mean", "var", "std", "mcse", "n_used")      # FG_WPOP_MOMENTS words per row
WPOP_CATS = ("lt", "eq", "gt", "nan")                             # FG_WPOP_CATS categories per slot
WLL_WORDS = ("W", "W_fin", "W2", "mean", "ssd", "n_used", "mx", "mn", "sp", "sn", "sn2", "tmax")      # FG_WLL_WORDS words per row
WLL_COUNTS = ("n_fin", "n_neg_inf", "n_pos_inf", "n_nan")         # FG_WLL_COUNTS counters per row


class WeightedPopulation(_Stream):
    """`fg_wpop` (fg_wpop.hip): the summary of a weighted population that stays on the device -- what the reference does on the host
    with ABCSMCResult::weighted_mean (abc.rs:476) and the doc example's walk over the particles (smc.rs:445-453).  Rows are device
    buffers [d][n] of doubles (cells [n_rows][n] for `counts`), element i of a row belonging to particle i.  The handle keeps a copy
    of the weights as they were when it was made, and their units q_i = rint(w_i 2^52): quantiles and tables are exact sums of units,
    moments use the doubles over a fixed tree on the particle index.  Close it before its engine."""

    _free = "fg_wpop_free"

    def __init__(self, engine: "Engine", n: Optional[int] = None, d_w: Optional[int] = None):
        if n is None:
            n = engine.C
        self._integers(n=n)
        if n < 1:
            raise ValueError("n must be at least 1")
        self.engine, self.n = engine, int(n)
        self.h = None
        out = C.c_void_p()
        _check(lib().fg_wpop_new(engine.h, self.n, d_w, C.byref(out)))
        self.h = out.value

    def units(self) -> dict:
        """T (the units of the population), n_bad (weights that are NaN, negative, infinite or above 1), n_zero (good weights of zero units)."""
        T, bad, zero = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _check(lib().fg_wpop_units(self._handle(), C.byref(T), C.byref(bad), C.byref(zero)))
        return dict(T=T.value, n_bad=bad.value, n_zero=zero.value)

    def moments(self, d_x: int, d: int) -> dict:
        """W, mean, var, std, mcse, n_used of every row, each float64 [d] (n_used int64)."""
        self._integers(d=d)
        if not 1 <= d <= 65535:
            raise ValueError("d must lie in [1, 65535]")
        out = np.zeros((int(d), len(WPOP_MOMENTS)))
        _check(lib().fg_wpop_moments(self._handle(), d_x, int(d), _dp(out)))
        res = {name: out[:, j].copy() for j, name in enumerate(WPOP_MOMENTS)}
        res["n_used"] = res["n_used"].astype(np.int64)
        return res

    def quantiles(self, d_x: int, d: int, probs=(0.025, 0.25, 0.5, 0.75, 0.975), digit_bits: int = 12, capacity: int = 65536):
        """(values [d][len(probs)], passes [d][len(probs)]): the inverse weighted CDF at every probability, and the passes over its
        row each one took."""
        self._integers(d=d, digit_bits=digit_bits, capacity=capacity)
        pr = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
        if not 1 <= d <= 65535:
            raise ValueError("d must lie in [1, 65535]")
        if not 1 <= pr.size <= 8:
            raise ValueError("between 1 and 8 probabilities")
        if not np.all((pr >= 0.0) & (pr <= 1.0)):
            raise ValueError("probabilities must lie in [0, 1]")
        if not 1 <= digit_bits <= 12:
            raise ValueError("digit_bits must lie in [1, 12]")
        if capacity < 0:
            raise ValueError("capacity must not be negative")
        out = np.zeros((int(d), pr.size))
        passes = np.zeros((int(d), pr.size), dtype=np.int32)
        _check(lib().fg_wpop_quantiles(self._handle(), d_x, int(d), _dp(pr), pr.size, int(digit_bits), int(capacity), _dp(out),
                                       passes.ctypes.data_as(C.POINTER(C.c_int32))))
        return out, passes

    def counts(self, d_cells: int, vtypes: Sequence[int], lo: Sequence[int], bins: Sequence[int]) -> dict:
        """Weighted frequency tables of integer rows d_cells [len(vtypes)][n].  units: a list of uint64 arrays [bins[k]]; below /
        above: uint64 [n_rows]; min / max: lists of Python ints over the cells of non-zero units (None when T == 0; a u64 row's are
        unsigned); T: the units of the population, so units / T are the probabilities."""
        vt, lo, bins = [int(v) for v in vtypes], [int(v) for v in lo], [int(b) for b in bins]
        nr = len(vt)
        if not (nr == len(lo) == len(bins)):
            raise ValueError("vtypes, lo and bins must have one entry per row")
        if not 1 <= nr <= 65535:
            raise ValueError("between 1 and 65535 rows")
        if any(not -2 ** 63 <= v < 2 ** 63 for v in lo):
            raise ValueError("lo must fit 64 signed bits")
        flat = np.zeros(max(1, sum(b for b in bins if b > 0)), dtype=np.uint64)
        below, above = np.zeros(nr, dtype=np.uint64), np.zeros(nr, dtype=np.uint64)
        mn, mx = np.zeros(nr, dtype=np.int64), np.zeros(nr, dtype=np.int64)
        u64p, i64p = C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
        i32 = lambda v: (C.c_int32 * nr)(*v)
        _check(lib().fg_wpop_counts(self._handle(), d_cells, nr, i32(vt), (C.c_int64 * nr)(*lo), i32(bins), flat.ctypes.data_as(u64p), below.ctypes.data_as(u64p),
                                    above.ctypes.data_as(u64p), mn.ctypes.data_as(i64p), mx.ctypes.data_as(i64p)))
        at = np.concatenate([[0], np.cumsum(bins)])
        T = self.units()["T"]
        ints = lambda a: [None if T == 0 else (int(v) & (2 ** 64 - 1) if vt[k] == M.U64 else int(v)) for k, v in enumerate(a)]
        return dict(units=[flat[at[k]:at[k + 1]].copy() for k in range(nr)], below=below, above=above, min=ints(mn), max=ints(mx), T=T)

    def checks(self, d_yrep: int, vtypes: Sequence[int], checks, observed=None) -> dict:
        """Weighted predictive checks of ONE replicate per particle, d_yrep a device buffer of cells [len(vtypes)][n]: `checks` as
        `PpcStream` takes them, [(rows, statistics, observed values)], or [(rows, statistics)] with `observed` the vectors.  Per slot
        (`slots`: (check, statistic)): t_obs; units uint64 [n_slots][4] and counts int64 [n_slots][4], the units and the particles of
        non-zero units whose replicated statistic is below / equal to / above the observed one, or where either is NaN; p_ge, p_gt,
        p_mid, quotients of unit sums (NaN for a denominator of 0); W, mean, var, std, mcse, n_used of the replicated statistic."""
        if observed is not None:
            checks = [(c[0], c[1], o) for c, o in zip(checks, observed)]
        vt = [int(v) for v in vtypes]
        offsets, members, masks, obs, slots = _ppc_csr(checks)
        if not 1 <= len(vt) <= 65535:
            raise ValueError("between 1 and 65535 rows")
        i32 = lambda v: (C.c_int32 * max(1, len(v)))(*v)
        n_slots = int(lib().fg_wpop_checks_n_slots(len(masks), i32(masks)))
        if n_slots < 0:
            _check(n_slots)
        t_obs, units, counts = np.zeros(n_slots), np.zeros((n_slots, len(WPOP_CATS)), dtype=np.uint64), np.zeros((n_slots, len(WPOP_CATS)), dtype=np.int64)
        mom = np.zeros((n_slots, len(WPOP_MOMENTS)))
        _check(lib().fg_wpop_checks(self._handle(), d_yrep, len(vt), i32(vt), len(masks), i32(offsets), i32(members), i32(masks), (C.c_double * max(1, len(obs)))(*obs),
                                    _dp(t_obs), units.ctypes.data_as(C.POINTER(C.c_uint64)), counts.ctypes.data_as(C.POINTER(C.c_int64)), _dp(mom)))
        res = dict(slots=slots, t_obs=t_obs, units=units, counts=counts)
        res.update(wpop_p_values(units))
        res.update({name: mom[:, j].copy() for j, name in enumerate(WPOP_MOMENTS)})
        res["n_used"] = res["n_used"].astype(np.int64)
        return res

    def loglik(self, d_ll: int, n_sel: int) -> dict:
        """Weighted WAIC / IS-LOO of rows d_ll [n_sel][n] of doubles: the figures of `LoglikStream.result` (lppd, mean_ll, p_waic in
        its reliability-weights form, elpd_waic, elpd_loo, p_loo, is_ess, max_weight), each float64 [n_sel]; `words` float64
        [n_sel][12] in the order WLL_WORDS; n_fin, n_neg_inf, n_pos_inf, n_nan int64 [n_sel], over the cells of the particles that take
        part (a good weight above zero)."""
        self._integers(n_sel=n_sel)
        if not 1 <= n_sel <= 65535:
            raise ValueError("n_sel must lie in [1, 65535]")
        figs, words, counts = np.zeros((LL_FIGURES, int(n_sel))), np.zeros((int(n_sel), len(WLL_WORDS))), np.zeros((int(n_sel), len(WLL_COUNTS)), dtype=np.int64)
        _check(lib().fg_wpop_loglik(self._handle(), d_ll, int(n_sel), _dp(figs), _dp(words), counts.ctypes.data_as(C.POINTER(C.c_int64))))
        out = {name: figs[i].copy() for i, name in enumerate(LL_FIGURE_NAMES)}
        out.update({name: counts[:, i].copy() for i, name in enumerate(WLL_COUNTS)})
        out["words"] = words
        return out

    free = _Stream.close


_HOLDER_PROGRAM = None


@contextlib.contextmanager
def stored_population(weights: np.ndarray, table: np.ndarray, device: int = 0):
    """A stored weighted population on the device: uploads `weights` [N] and `table` [rows][N] and yields (WeightedPopulation, device
    pointer of the table); everything is freed on exit.  The handle needs an engine only for its device and stream: one chain of a
    one-site model, compiled once per process."""
    global _HOLDER_PROGRAM
    if _HOLDER_PROGRAM is None:
        from . import workloads as _W
        _HOLDER_PROGRAM = compile_model(_W.normal_sites(1))
    eng = Engine(_HOLDER_PROGRAM, 1, seed=0, device=device)
    bufs, wp = [], None
    try:
        bufs.append(eng.upload(np.ascontiguousarray(weights, dtype=np.float64)))
        wp = eng.wpop(int(np.size(weights)), bufs[0])
        bufs.append(eng.upload(np.ascontiguousarray(table)))
        yield wp, bufs[1]
    finally:
        if wp is not None:
            wp.close()
        for b in bufs:
            eng.device_free(b)
        eng.close()


def wpop_p_values(units) -> dict:
    """p_ge, p_gt, p_mid [n_slots] from unit sums [n_slots][4] (lt, eq, gt, nan): integers first, one division each (fg_wpe_p_values)."""
    out = {k: [] for k in ("p_ge", "p_gt", "p_mid")}
    for lt, eq, gt, _ in ([int(v) for v in row] for row in np.asarray(units).reshape(-1, 4)):
        den = lt + eq + gt
        out["p_ge"].append(float(gt + eq) / float(den) if den else float("nan"))
        out["p_gt"].append(float(gt) / float(den) if den else float("nan"))
        out["p_mid"].append(float(2 * gt + eq) / float(2 * den) if den else float("nan"))
    return {k: np.array(v, dtype=np.float64) for k, v in out.items()}


# ---- population-wide device primitives (no program needed) -----------------------------------
def device_log_sum_exp(x, device: int = 0) -> float:
    a = np.ascontiguousarray(x, dtype=np.float64)
    out = C.c_double()
    _check(lib().fg_device_log_sum_exp(device, _dp(a), a.size, C.byref(out)))
    return out.value


def device_next_beta(beta, log_w, ll, target_ess, device: int = 0) -> float:
    lw = np.ascontiguousarray(log_w, dtype=np.float64)
    l2 = np.ascontiguousarray(ll, dtype=np.float64)
    out = C.c_double()
    _check(lib().fg_device_next_beta(device, float(beta), _dp(lw), _dp(l2), lw.size, float(target_ess), C.byref(out)))
    return out.value


def device_smc_temper(beta, ll, target_ess, zoom: bool = True, force_sum: bool = False, device: int = 0) -> dict:
    """One tempering step of smc_run's ladder on `ll` from uniform log-weights -ln n: beta' (next_beta), the reweight's log-normaliser,
    the reweighted log_w / w, and need_sum (the separate-kernels path took the step)."""
    l2 = np.ascontiguousarray(ll, dtype=np.float64)
    n = l2.size
    lw, w = np.empty(n), np.empty(n)
    b, ln, ns = C.c_double(), C.c_double(), C.c_int32()
    flags = (0 if zoom else 1) | (2 if force_sum else 0)
    _check(lib().fg_device_smc_temper(device, float(beta), _dp(l2), n, float(target_ess), flags, C.byref(b), C.byref(ln), _dp(lw), _dp(w), C.byref(ns)))
    return {"beta": b.value, "log_norm": ln.value, "log_w": lw, "w": w, "need_sum": bool(ns.value)}


def device_resample_indices(method: int, weights, u, device: int = 0) -> np.ndarray:
    w = np.ascontiguousarray(weights, dtype=np.float64)
    uu = np.ascontiguousarray(np.atleast_1d(u), dtype=np.float64)
    idx = np.zeros(w.size, dtype=np.int64)
    _check(lib().fg_device_resample_indices(device, int(method), _dp(w), w.size, _dp(uu), idx.ctypes.data_as(C.POINTER(C.c_int64))))
    return idx


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the library (rank 0 calls it; the host distributes the 128 bytes)."""
    buf = C.create_string_buffer(128)
    _check(lib().fg_comm_unique_id(buf))
    return buf.raw


def comm_destroy(comm: int):
    _check(lib().fg_comm_destroy(comm))


def diag_combine(moments: np.ndarray, n: int, acov_sums):
    """`fg_diag_combine`: the C++ R-hat / ESS combination over host moments [d][6][m] of all chains; `acov_sums(lag0, n_lags)`
    returns the pooled lag sums [d][n_lags] (e.g. all-reduced over gloo)."""
    mom = np.ascontiguousarray(moments, dtype=np.float64)
    d, _, m = mom.shape
    err = []

    def cb(_user, lag0, n_lags, out):
        try:
            a = np.ascontiguousarray(acov_sums(int(lag0), int(n_lags)), dtype=np.float64)
            C.memmove(out, a.ctypes.data, d * n_lags * 8)
            return 0
        except Exception as ex:      # pragma: no cover
            err.append(ex)
            return FG_E_BAD_ARG
    fn = ACOV_FN(cb)
    rhat, ess, mean, std = (np.zeros(d) for _ in range(4))
    rc = lib().fg_diag_combine(_dp(mom), m, int(n), d, fn, None, _dp(rhat), _dp(ess), _dp(mean), _dp(std))
    if err:
        raise err[0]
    _check(rc)
    return dict(r_hat=rhat, ess=ess, mean=mean, std=std)


def diag_combine_reduced(m: int, n: int, d: int, reduce, acov_sums):
    """`fg_diag_combine_reduced`: the same combination from sums over chains.  `reduce(stage, overall)` returns the sums over
    ALL chains of all ranks ([d][6] for stage 1, [d][2] for stage 2 given the overall means [d][2]); `acov_sums(lag0, n_lags)`
    the pooled lag sums [d][n_lags]."""
    err = []

    def rcb(_user, stage, h_in, h_out):
        try:
            ov = np.ctypeslib.as_array(h_in, shape=(d, 2)).copy() if stage == 2 else None
            a = np.ascontiguousarray(reduce(int(stage), ov), dtype=np.float64)
            C.memmove(h_out, a.ctypes.data, d * (6 if stage == 1 else 2) * 8)
            return 0
        except Exception as ex:      # pragma: no cover
            err.append(ex)
            return FG_E_BAD_ARG

    def acb(_user, lag0, n_lags, out):
        try:
            a = np.ascontiguousarray(acov_sums(int(lag0), int(n_lags)), dtype=np.float64)
            C.memmove(out, a.ctypes.data, d * n_lags * 8)
            return 0
        except Exception as ex:      # pragma: no cover
            err.append(ex)
            return FG_E_BAD_ARG
    rfn, afn = REDUCE_FN(rcb), ACOV_FN(acb)
    rhat, ess, mean, std = (np.zeros(d) for _ in range(4))
    rc = lib().fg_diag_combine_reduced(int(m), int(n), int(d), rfn, afn, None, _dp(rhat), _dp(ess), _dp(mean), _dp(std))
    if err:
        raise err[0]
    _check(rc)
    return dict(r_hat=rhat, ess=ess, mean=mean, std=std)
