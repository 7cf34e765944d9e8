"""One table of sampler cases, shared by tests/test_sampler_law_cpu.py (the oracle alone) and tests/test_gpu_sampler_branches.py (the
device): every branch of the rejection samplers behind fg_sample_dist (fugue_amd/csrc/fg_math.h) -- Marsaglia-Tsang Gamma with and without
the shape < 1 boost, Knuth / PTRS Poisson on both sides of lambda = 30, BINV / BTRS Binomial on both sides of n q = 10 and of the p > 0.5
flip -- each with the scipy frozen distribution that judges its law.  The oracle restates the same algorithms, so it cannot judge a
constant of PTRS or BTRS; the analytic cdf / pmf can.

Draws come from a one-site model on chains 0 .. N-1, iteration 0, purpose 1 (the prior stream), N = 16384; alpha = 0.001 per check, the
standing level of tests/test_gpu_sampler_validation.py.  The law helpers:
  ks_one_sample / ks_critical   the reference test's one-sample Kolmogorov-Smirnov statistic and its asymptotic critical value;
  chi_square_pooled             Pearson's chi-square over ppf(1e-9) .. ppf(1 - 1e-9) with neighbouring bins pooled until each expects at
                                least 5; a draw outside that range (probability 2e-9 per draw) is a failure;
  mean_z                        the 5-standard-error check of the mean, where the standard error is finite;
  pit_mixed                     the probability integral transform of every site of the mixed model given its parent, randomised for the
                                discrete sites (F(k-1) + V pmf(k), V from a fixed numpy generator), KS-tested against the uniform.
Every helper returns its figures; check_case / check_mixed assert on them and put them into the message."""
import math
from collections import namedtuple

import numpy as np
from scipy import stats

import fugue_amd as F
from fugue_amd import model as M

N, ALPHA = 16384, 0.001
SEED_DISCRETE, SEED_CONTINUOUS, SEED_MIXED = 77, 78, 91

Case = namedtuple("Case", "name family params branch path ref seed")   # branch: what the case is for; path: the code path it takes


def _d(name, family, params, branch, path, ref):
    return Case(name, family, params, branch, path, ref, SEED_DISCRETE)


def _c(name, family, params, branch, path, ref):
    return Case(name, family, params, branch, path, ref, SEED_CONTINUOUS)


LAM_KNUTH = math.nextafter(30.0, 0.0)
P_FLIP = math.nextafter(0.5, 1.0)

DISCRETE = [
    _d("pois_30", "Poisson", [30.0], "first PTRS value", "PTRS", stats.poisson(30.0)),
    _d("pois_30_pred", "Poisson", [LAM_KNUTH], "last Knuth value", "Knuth", stats.poisson(LAM_KNUTH)),
    _d("pois_100.5", "Poisson", [100.5], "PTRS", "PTRS", stats.poisson(100.5)),
    _d("pois_5000", "Poisson", [5000.0], "PTRS", "PTRS", stats.poisson(5000.0)),
    _d("binom_40_0.3", "Binomial", [40, 0.3], "BTRS", "BTRS", stats.binom(40, 0.3)),
    _d("binom_40_0.7", "Binomial", [40, 0.7], "BTRS + flip", "BTRS + flip", stats.binom(40, 0.7)),
    _d("binom_1000_0.5", "Binomial", [1000, 0.5], "BTRS", "BTRS", stats.binom(1000, 0.5)),
    _d("binom_30_0.9", "Binomial", [30, 0.9], "BINV + flip", "BINV + flip", stats.binom(30, 0.9)),
    _d("binom_1e5_5e-5", "Binomial", [100000, 5e-5], "BINV, huge n", "BINV", stats.binom(100000, 5e-5)),
    _d("binom_25_0.4", "Binomial", [25, 0.4], "n q rounds to exactly 10: BTRS", "BTRS", stats.binom(25, 0.4)),
    _d("binom_20_0.5", "Binomial", [20, 0.5], "n q rounds to exactly 10: BTRS", "BTRS", stats.binom(20, 0.5)),
    _d("binom_20_0.5_succ", "Binomial", [20, P_FLIP], "flip at its threshold (q = 0.5 - 2^-53: n q < 10)", "BINV + flip", stats.binom(20, P_FLIP)),
    _d("binom_1e6_0.37", "Binomial", [1000000, 0.37], "BTRS", "BTRS", stats.binom(1000000, 0.37)),
]
CONTINUOUS = [
    _c("gamma_0.3_2", "Gamma", [0.3, 2.0], "boost", "boost", stats.gamma(0.3, scale=0.5)),                         # RATE parameterisation
    _c("gamma_1_1", "Gamma", [1.0, 1.0], "first value without the boost", "no boost", stats.gamma(1.0)),
    _c("gamma_0.05_1", "Gamma", [0.05, 1.0], "boost, tiny shape", "boost", stats.gamma(0.05)),
    _c("beta_0.5_0.5", "Beta", [0.5, 0.5], "two boosted Gammas", "boost, boost", stats.beta(0.5, 0.5)),
    _c("beta_0.2_3", "Beta", [0.2, 3.0], "one boosted Gamma", "boost, no boost", stats.beta(0.2, 3.0)),
    _c("chisq_1", "ChiSquared", [1.0], "shape 0.5", "boost", stats.chi2(1.0)),
    _c("studt_1.5", "StudentT", [1.5, 0.0, 1.0], "shape 0.75", "boost", stats.t(1.5, 0.0, 1.0)),
    _c("invgamma_0.7_2", "InverseGamma", [0.7, 2.0], "boost", "boost", stats.invgamma(0.7, scale=2.0)),
]
CASES = DISCRETE + CONTINUOUS
# The transformed-rejection cases are judged a second time on 2^20 draws: their squeeze constants (PTRS vr, BTRS alpha) only decide which
# candidates skip the exact acceptance test, so at small means a constant 5 % off leaves the law unchanged to within what 16384 draws
# -- or 4 million -- can see; Poisson(5000), Binomial(1000, 0.5) and Binomial(10^6, 0.37) show it at 2^20.
N_LARGE = 1 << 20
LARGE = [c for c in DISCRETE if c.path.startswith(("PTRS", "BTRS"))]
BY_NAME = {c.name: c for c in CASES}
INT_FAMILIES = {"Poisson", "Binomial"}


def is_discrete(case):
    return case.family in INT_FAMILIES


def dist_of(case):
    """The model distribution of a case (constructor-validated: every table case has valid parameters)."""
    return getattr(F, case.family)(*case.params)


def one_site_model(case):
    return lambda: F.sample(F.addr("x"), dist_of(case))


def branch_reached(case):
    """The branch the sampler code takes at the case's parameters, worked out as fg_smp_* work it out (in f64)."""
    if case.family == "Poisson":
        return "Knuth" if case.params[0] < 30.0 else "PTRS"
    if case.family == "Binomial":
        n, p = case.params
        flip = p > 0.5
        q = 1.0 - p if flip else p
        return ("BINV" if float(n) * q < 10.0 else "BTRS") + (" + flip" if flip else "")
    shapes = {"Gamma": lambda p: [p[0]], "Beta": lambda p: [p[0], p[1]], "ChiSquared": lambda p: [p[0] / 2.0],
              "StudentT": lambda p: [p[0] / 2.0], "InverseGamma": lambda p: [p[0]]}[case.family](case.params)
    return ", ".join("boost" if s < 1.0 else "no boost" for s in shapes)


def oracle_draws(oracle, case, n=N, chain0=0):
    """oracle.sample_dist on the stream (seed, chain, 0, 1) of chains chain0 .. chain0 + n - 1 -> (draws, blocks consumed per chain)."""
    return oracle.sample_dist_many(case.family, case.params, case.seed, n, chain0=chain0)


# ---- the law helpers ------------------------------------------------------------------------------------------------------------------
def ks_critical(alpha, n):
    return math.sqrt(-0.5 * math.log(alpha / 2.0)) / math.sqrt(n)


def ks_one_sample(x, cdf):
    x = np.sort(np.asarray(x, dtype=np.float64))
    n = len(x)
    f = cdf(x)
    i = np.arange(n)
    return float(max(((i + 1.0) / n - f).max(), (f - i / n).max()))


def chi_square_pooled(x, ref):
    """-> (statistic, degrees of freedom, p-value, draws outside ppf(1e-9) .. ppf(1 - 1e-9))."""
    x = np.asarray(x, dtype=np.int64)
    lo, hi = int(ref.ppf(1e-9)), int(ref.ppf(1.0 - 1e-9))
    ks = np.arange(lo, hi + 1)
    e = ref.pmf(ks) * len(x)
    inside = (x >= lo) & (x <= hi)
    cnt = np.bincount(x[inside] - lo, minlength=len(ks)).astype(np.float64)
    E, O, ce, co = [], [], 0.0, 0.0
    for ei, oi in zip(e, cnt):
        ce += ei
        co += oi
        if ce >= 5.0:
            E.append(ce), O.append(co)
            ce = co = 0.0
    if ce > 0.0:                                           # the upper tail's remainder joins the last bin
        E[-1] += ce
        O[-1] += co
    E, O = np.array(E), np.array(O)
    stat = float(((O - E) ** 2 / E).sum())
    df = len(E) - 1
    return stat, df, float(stats.chi2.sf(stat, df)), int((~inside).sum())


def mean_z(x, ref):
    """|mean - mu| in standard errors, or None where the standard error is not finite (no mean, or an infinite variance)."""
    mu, sd = float(ref.mean()), float(ref.std())
    if not (math.isfinite(mu) and math.isfinite(sd)):
        return None
    return abs(float(np.mean(np.asarray(x, dtype=np.float64))) - mu) / (sd / math.sqrt(len(x)))


def law_figures(case, x):
    """Every figure of the law checks of one case over the draws x."""
    fig = dict(n=len(x), mean_z=mean_z(x, case.ref))
    if is_discrete(case):
        fig["chi2"], fig["df"], fig["p"], fig["outside"] = chi_square_pooled(x, case.ref)
    else:
        fig["finite"] = bool(np.isfinite(x).all())
        fig["ks"] = ks_one_sample(x, case.ref.cdf) if fig["finite"] else float("nan")
        fig["ks_crit"] = ks_critical(ALPHA, len(x))
    return fig


def describe(case, fig):
    z = "none (no finite standard error)" if fig["mean_z"] is None else f"{fig['mean_z']:.2f}"
    if is_discrete(case):
        return (f"{case.name} [{case.branch}] n = {fig['n']}: chi-square {fig['chi2']:.1f} on {fig['df']} df, p = {fig['p']:.4f} (alpha {ALPHA}), "
                f"{fig['outside']} draws outside the range, mean z {z}")
    return f"{case.name} [{case.branch}] n = {fig['n']}: KS D {fig['ks']:.5f} (critical {fig['ks_crit']:.5f}), finite {fig['finite']}, mean z {z}"


def check_case(case, x):
    """Assert every law check of the case on the draws x; returns the figures."""
    fig = law_figures(case, x)
    msg = describe(case, fig)
    print(msg)
    if is_discrete(case):
        assert fig["outside"] == 0, msg
        assert fig["p"] >= ALPHA, msg
    else:
        assert fig["finite"], msg
        assert fig["ks"] < fig["ks_crit"], msg
    assert fig["mean_z"] is None or fig["mean_z"] < 5.0, msg
    return fig


# ---- the mixed model ------------------------------------------------------------------------------------------------------------------
MIXED_SITES = ["a_u", "b_pois", "c_bin", "d_gam", "e_z"]       # sorted: the engine's and the oracle's site order


def mixed_program():
    """Site-fed parameters that put both branches of every sampler into one wave: about half the lanes of every wave take each Poisson
    branch and each Gamma branch, about 40 % take BTRS; e_z sits behind three samplers with lane-dependent block counts."""
    P = M.Program()
    u = P.sample(M.addr("a_u"), M.Uniform(0.0, 1.0))
    P.sample(M.addr("b_pois"), M.Poisson(20.0 + u * 20.0))
    P.sample(M.addr("c_bin"), M.Binomial(30, 0.1 + u * 0.8))
    P.sample(M.addr("d_gam"), M.Gamma(0.25 + u * 1.5, 2.0))
    P.sample(M.addr("e_z"), M.Normal(0.0, 1.0))
    return P


def mixed_params(u):
    """The parameters as the interpreter computes them: one rounding per operation."""
    u = np.asarray(u, dtype=np.float64)
    return dict(lam=20.0 + u * 20.0, p=0.1 + u * 0.8, shape=0.25 + u * 1.5)


def mixed_decode(cells):
    """cells int64 [5][n] -> (u, k, b, g, z)."""
    cells = np.ascontiguousarray(cells, dtype=np.int64)
    f = lambda j: cells[j].copy().view(np.float64)
    return f(0), cells[1].copy(), cells[2].copy(), f(3), f(4)


def mixed_branch_shares(u):
    par = mixed_params(u)
    q = np.minimum(par["p"], 1.0 - par["p"])
    return dict(ptrs=float((par["lam"] >= 30.0).mean()), btrs=float((30.0 * q >= 10.0).mean()), flip=float((par["p"] > 0.5).mean()),
                boost=float((par["shape"] < 1.0).mean()))


def pit_mixed(cells):
    """KS D of the (randomised) probability integral transform of every site given its parent -> dict site -> D."""
    u, k, b, g, z = mixed_decode(cells)
    n = len(u)
    par = mixed_params(u)
    v = np.random.default_rng(1).uniform(size=n)
    unif = stats.uniform(0.0, 1.0).cdf
    pit_k = stats.poisson.cdf(k - 1, par["lam"]) + v * stats.poisson.pmf(k, par["lam"])
    pit_b = stats.binom.cdf(b - 1, 30, par["p"]) + v * stats.binom.pmf(b, 30, par["p"])
    return dict(a_u=ks_one_sample(u, unif), b_pois=ks_one_sample(pit_k, unif), c_bin=ks_one_sample(pit_b, unif),
                d_gam=ks_one_sample(stats.gamma.cdf(g, par["shape"], scale=0.5), unif), e_z=ks_one_sample(z, stats.norm.cdf))


def check_mixed(cells):
    u, k, b, g, z = mixed_decode(cells)
    n = len(u)
    crit = ks_critical(ALPHA, n)
    shares = mixed_branch_shares(u)
    d = pit_mixed(cells)
    msg = (f"mixed model n = {n}: PIT KS D " + ", ".join(f"{s} {d[s]:.5f}" for s in MIXED_SITES) + f" (critical {crit:.5f}); lanes on PTRS "
           f"{shares['ptrs']:.3f}, BTRS {shares['btrs']:.3f}, flip {shares['flip']:.3f}, boost {shares['boost']:.3f}")
    print(msg)
    assert np.isfinite(g).all() and np.isfinite(z).all() and (k >= 0).all() and (b >= 0).all() and (b <= 30).all(), msg
    assert 0.4 < shares["ptrs"] < 0.6 and 0.4 < shares["boost"] < 0.6 and 0.3 < shares["btrs"] < 0.5, msg
    for s in MIXED_SITES:
        assert d[s] < crit, msg
    return d


# ---- edge parameters ------------------------------------------------------------------------------------------------------------------
I64_MAX = 9223372036854775807
# (name, family, parameters, the cell, Philox blocks consumed or None where only device == oracle is pinned)
EDGES = [
    ("binom_n0", "Binomial", [0, 0.3], 0, 0),
    ("binom_p0", "Binomial", [7, 0.0], 0, 0),
    ("binom_p1", "Binomial", [7, 1.0], 7, 0),
    ("pois_inf", "Poisson", [math.inf], 0, 0),
    ("pois_tiny", "Poisson", [1e-300], 0, 1),
    ("binom_nan", "Binomial", [10, math.nan], 0, 0),          # a non-finite p draws nothing, as Bernoulli
    ("pois_1e19", "Poisson", [1e19], I64_MAX, None),          # every PTRS candidate lies above 2^63: the cast saturates (Rust `as`)
]
