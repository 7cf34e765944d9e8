"""One table of the free-running parity runs whose chains are compared with the oracle draw for draw: model, seed, chain count, warmup and
recorded steps, chain offset, overrides, leapfrog count and step size.  The GPU tests (tests/test_gpu_mh.py, test_gpu_parity.py,
test_gpu_sampler_branches.py, test_gpu_fullsize.py) and their CPU twin (tests/test_knife_margins_cpu.py) both read it, so the condition the
twin proves -- no decision of the oracle's run within the band of its boundary -- is a condition on the very runs the device is judged by.
A row that is changed here has to pass the twin again: pick another seed if it does not, the band stays.  Data and small helpers only."""
from typing import Callable, NamedTuple, Optional

import numpy as np

from fugue_amd import model as M
from fugue_amd import workloads as W
from tests.mh_edge_cases import MARGIN, PROP_GAUSSIAN, PROP_PRIOR_RESAMPLE, PROP_REFLECT
from tests.models import ZOO, f64_values_for
from tests.random_models import random_program

MH_BAND = MARGIN                                        # |ln u - log_alpha|
HMC_BAND = 1e-6                                         # |u - alpha|, and |log-ratio - threshold| of the step-size search


class MhCase(NamedTuple):
    id: str
    make: Callable[[], M.Program]
    seed: int
    C: int
    nw: int
    ns: int
    chain0: int = 0
    overrides: Optional[dict] = None                    # {site name: (kind, lower, upper)}

    def overrides_for(self, site_names):
        """Per sorted site: None or (kind, lower, upper); None where the row has no overrides."""
        if self.overrides is None: return None
        ov = [None] * len(site_names)
        for name, o in self.overrides.items(): ov[site_names.index(name)] = o
        return ov


class HmcCase(NamedTuple):
    id: str
    make: Callable[[], M.Program]
    seed: int
    C: int
    nw: int
    ns: int
    chain0: int
    n_leapfrog: int
    step_size: Optional[float]                          # None: the step-size search and dual averaging


class EpsCase(NamedTuple):
    id: str
    make: Callable[[], M.Program]
    C: int
    rng_seed: int


def overrides_model() -> M.Program:
    """adaptive_mcmc_chain_with_overrides (mh.rs:938-944): Reflect, a forced Gaussian walk on a positive-support site, PriorResample."""
    P = M.Program()
    a = P.sample(M.addr("a"), M.Uniform(0.0, 2.0))
    g = P.sample(M.addr("g"), M.Gamma(2.0, 1.0))
    t = P.sample(M.addr("t"), M.Normal(0.0, 2.0))
    P.observe(M.addr("y"), M.Normal(a + t, 0.5 + g), 1.0)
    return P


def boosted_gamma_model() -> M.Program:
    """g ~ Gamma(0.3, 2) (a boosted Marsaglia-Tsang draw) with observations whose mean is an expression of g: no score stream."""
    P = M.Program()
    g = P.sample(M.addr("g"), M.Gamma(0.3, 2.0))
    for i, y in enumerate([0.4, 0.1, 0.9]):                 # (four statements: shorter programs stay on the one-wave kernel)
        P.observe(M.addr("y", i), M.Normal(g * 1.5 + 0.1, 1.0), y)
    return P


MH_ZOO = ["readme", "coin", "refmodel8", "mixture", "alldists", "normal32", "hier_scale", "ridge7", "linreg", "logistic", "poisson_glm", "hier_logsigma"]
MH_RANDOM_SEEDS = list(range(12))


def _random(seed):
    return lambda: random_program(1000 + seed)


MH_CASES = {c.id: c for c in (
    [MhCase(f"zoo-{name}", ZOO[name], seed=13, C=96, nw=150, ns=60, chain0=3) for name in MH_ZOO]
    + [MhCase(f"random-{s}", _random(s), seed=21 + s, C=64, nw=80, ns=40, chain0=s) for s in MH_RANDOM_SEEDS]
    + [MhCase("gamma-log-walk", W.gamma_scale_model, seed=2, C=512, nw=300, ns=300),
       MhCase("overrides", overrides_model, seed=4, C=128, nw=100, ns=100,
              overrides={"a": (PROP_REFLECT, 0.0, 2.0), "g": (PROP_GAUSSIAN, 0.0, 0.0), "t": (PROP_PRIOR_RESAMPLE, 0.0, 0.0)}),
       MhCase("boosted-gamma", boosted_gamma_model, seed=19, C=256, nw=50, ns=150, overrides={"g": (PROP_PRIOR_RESAMPLE, 0.0, 0.0)}),
       MhCase("c5-mixture-64", lambda: W.mixture(W.mixture_data(64)[0]), seed=3, C=64, nw=400, ns=40, chain0=5)])}

HMC_FIXED = ["readme", "normal32"]
HMC_CASES = {c.id: c for c in (
    [HmcCase(f"fixed-{name}", ZOO[name], seed=11, C=64, nw=0, ns=60, chain0=0, n_leapfrog=8, step_size=0.15) for name in HMC_FIXED]
    + [HmcCase("adaptive-normal32", ZOO["normal32"], seed=5, C=96, nw=3, ns=3, chain0=7, n_leapfrog=8, step_size=None)])}

EPS_MODELS = ["readme", "normal32", "refmodel8", "alldists"]
EPS_CASES = {c.id: c for c in [EpsCase(name, ZOO[name], C=80, rng_seed=31) for name in EPS_MODELS]}


def eps_inputs(om, case: EpsCase):
    """(cells [S][C], p0 [d][C]) of a step-size search under injected momentum: in-support cells and standard-normal momenta."""
    rng = np.random.default_rng(case.rng_seed)
    cells = f64_values_for(om, rng, case.C)
    p0 = rng.standard_normal((om.d, case.C))
    return cells, p0
