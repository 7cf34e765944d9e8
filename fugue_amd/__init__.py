"""fugue_amd: the MI355X-native many-chain engine for Fugue's `src/inference` hot path.

    from fugue_amd import sample, observe, factor, pure, addr, Normal, hmc_chain, HMCConfig
    model = lambda: sample(addr("mu"), Normal(0.0, 1.0)).bind(lambda mu: observe(addr("y"), Normal(mu, 0.5), 1.2).map(lambda _: mu))
    chains = hmc_chain(42, model, 1000, 500, HMCConfig(), n_chains=65536)
    chains.get_f64(addr("mu")).mean()          # 0.96
"""
from .model import (Bernoulli, Beta, Binomial, Categorical, Cauchy, ChiSquared, DiscreteUniform, Exponential, FugueError, Gamma,  # noqa: F401
                    InverseGamma, Laplace, LogNormal, Model, Normal, Poisson, Program, StudentT, Uniform, Weibull, addr, factor, guard,
                    observe, plate, pure, sample, sequence_vec, traverse_vec, zip_models)
from .inference import (ChainBatch, ChainSummary, HMCConfig, PopulationSummary, PriorPredictive, ResamplingMethod, SMCConfig, SMCResult,  # noqa: F401
                        SiteProposal, WeightedTables, adaptive_mcmc_chain, adaptive_mcmc_chain_summary, adaptive_mcmc_chain_with_overrides,
                        adaptive_smc, adaptive_smc_summary, hmc_chain, hmc_chain_summary, population_summary, prior_predictive)
from .diagnostics import (ParameterSummary, RankDiagnostics, StreamMoments, classic_r_hat_f64, effective_sample_size,  # noqa: F401
                          effective_sample_size_multichain, ess_bulk, ess_tail, geweke_diagnostic, r_hat_f64, rank_diagnostics, rank_r_hat_f64,
                          summarize_f64_parameter)
from .diagnostics import (McseDiagnostics, ess_mean, ess_median, ess_quantile, ess_sd, mad, mcse_diagnostics, mcse_mean, mcse_median,  # noqa: F401
                          mcse_quantile, mcse_sd, summarise_draws)
from .comparison import PointwiseComparison, PsisLoo, WeightedComparison, compare_models, model_comparison, psis_loo, weighted_model_comparison  # noqa: F401
from .checks import CheckSpec, PredictiveCheck, WeightedPredictiveCheck, marginal_checks, posterior_predictive_check, weighted_predictive_check  # noqa: F401
from .validation import effective_sample_size_mcmc  # noqa: F401
from .abc import (ABC_SMC_DEFAULT_ATTEMPT_FACTOR, ABCError, ABCSMCConfig, ABCSMCResult, EuclideanDistance, ManhattanDistance,  # noqa: F401
                  SummaryStatsDistance, abc_rejection, abc_scalar_summary, abc_smc, abc_smc_weighted)
from .pf import BankStep, PFRun, ParticleFilter, ParticleFilterBank, StepOut  # noqa: F401
from .grid import GridSurface, LogJointGrid, log_joint_grid, log_joint_surface  # noqa: F401
from .gibbs import GibbsSweep, SweepOutput, gibbs_chain, hmc_gibbs_chain, site_support  # noqa: F401
from .vi import (GuideError, MeanFieldGuide, ParamCoord, Support, VIConfig, VIResult, VariationalParam, elbo_gradient_fd,  # noqa: F401
                 elbo_with_guide, estimate_elbo, optimize_meanfield_vi, optimize_meanfield_vi_with_config)
