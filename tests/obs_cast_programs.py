"""The programs of the observed-count tests (tests/test_obs_cast_cpu.py on the oracle, tests/test_gpu_obs_cast.py on the device) and what
the reference computes for them.  Every statement is described once (`Stmt`: family, parameters as a Python function of the sites, observed
value as one, and how to build it) and becomes a `Program` and an expectation (tests/obs_cast_restatement.py + the oracle's integer
densities) from that one description.

An accumulator is a SUM: one -inf term hides every other statement of its chain, and one term of -3.8e20 (a Poisson at i64::MAX) hides every
ordinary one behind the relative tolerance.  So the programs whose accumulators are compared are laid out for that:

  RUNTIME  every value-observing statement has an f64 site of its own (v0, v1, ..) for its observed value.  A chain is one CASE: one
           statement observes one fixture value (specials included), every other statement observes 2 (finite for all of them) under n = 8;
           or every statement observes 2 and `w` carries one Binomial-n row.  At most one statement per chain can leave its support, and
           a huge term stands beside ordinary ones only.  More cases than chains: several value tables are scored one after the other.
  SMALL / BIG   literal observed values (the conversion is the host's or the compiler's: hoisted ln k! / ln C(n, k), stream-record
           constants, constant folding in the generated unit): the statements of ALL whose expectation is finite on every chain, split at
           |term| = 1e9.
  ALL      the families x every FINITE fixture value as a literal, with constant parameters and with parameters reading a site.  Most
           chains' sums are -inf here: it is compared PER STATEMENT only (predict_eval's loglik table).
  STREAM / STREAM_SMALL   the statements of ALL / SMALL that the compiler turns into score-stream records (a DiscreteUniform, a
           literal-valued Categorical or a Binomial with three hoisted constants has no record form, and one such statement leaves the
           whole program without a stream): per record, and per accumulator for STREAM_SMALL."""
import json
import math
import os
from dataclasses import dataclass
from typing import Callable

import numpy as np

from fugue_amd import model as M
from tests import obs_cast_restatement as R

with open(os.path.join(os.path.dirname(__file__), "golden", "observed_casts.json")) as _f:
    FIX = json.load(_f)
VALUES = [R.from_bits(r["value"]) for r in FIX["observed"] if r["vtype"] == "u64"]          # the same 21 values for every value type
assert all([r["value"] for r in FIX["observed"] if r["vtype"] == t] == [r["value"] for r in FIX["observed"] if r["vtype"] == "u64"] for t in ("usize", "i64", "bool"))
FINITE = [v for v in VALUES if math.isfinite(v)]
BINOMIAL_N = [R.from_bits(r["value"]) for r in FIX["binomial_n"]]
XS = [-0.7, 0.0, 0.4, 1.3]                     # `x`: ordinary values (it drives exp(x) * 3 and clamp(0.5 + 0.1 x, ..))
RATES = [0.6, 1.9, 3.2, 7.5]                   # `lam`: a Poisson rate read straight from a site
PROBS = [0.1, 0.35, 0.5, 0.9]                  # `q`: a probability read straight from a site
C = 130                                        # two 64-chain tiles and a tail of 2
BIG = 1e9                                      # a term beyond this is compared in a program of its own
P52, TOP, P63 = 4503599627370497.0, 9223372036854774784.0, 9223372036854775808.0            # 2^52 + 1, 2^63 - 1024, 2^63 (as i64: i64::MAX)


@dataclass(frozen=True)
class Stmt:
    address: str
    family: str
    params: Callable      # {site: float} -> the distribution's parameters as numbers
    observed: Callable    # {site: float} -> the observed expression's value
    make: Callable        # {site: Expr} -> (Dist, observed expression)


def _p_of_x(x):
    return min(max(0.5 + 0.1 * x, 0.05), 0.95)


# (address, family, parameters, distribution): the value-observing statements of RUNTIME.  Statement i observes site "v<i>".
_RUNTIME_DISTS = [
    ("pois_x", "Poisson", lambda s: [math.exp(s["x"]) * 3.0], lambda e: M.Poisson(M.exp(e["x"]) * 3.0)),
    ("pois_c", "Poisson", lambda s: [3.0], lambda e: M.Poisson(3.0)),
    ("binom", "Binomial", lambda s: [8.0, _p_of_x(s["x"])], lambda e: M.Binomial(8, M.clamp(0.5 + 0.1 * e["x"], 0.05, 0.95))),
    ("cat", "Categorical", lambda s: [0.2, 0.5, 0.3], lambda e: M.Categorical([0.2, 0.5, 0.3])),
    ("du", "DiscreteUniform", lambda s: [1, 9], lambda e: M.DiscreteUniform(1, 9)),                 # 0 is outside: truncation and the reference part ways at 2.5
    ("du_neg", "DiscreteUniform", lambda s: [-2, 2], lambda e: M.DiscreteUniform(-2, 2)),           # i64 keeps -2 where a count clamps it; -1e300 is i64::MIN, outside
    ("du_52", "DiscreteUniform", lambda s: [2.0, P52], lambda e: M.DiscreteUniform(2.0, P52)),      # 2^52 + 1 is the last value inside: an integer kept exact
    ("du_top", "DiscreteUniform", lambda s: [2.0, TOP], lambda e: M.DiscreteUniform(2.0, TOP)),     # 2^63 - 1024 inside, 2^63 (-> i64::MAX) outside
    ("du_max", "DiscreteUniform", lambda s: [2.0, P63], lambda e: M.DiscreteUniform(2.0, P63)),     # the bound saturates too: i64::MAX inside, nothing outside above
    ("bern", "Bernoulli", lambda s: [0.3], lambda e: M.Bernoulli(0.3)),
]
N_V = len(_RUNTIME_DISTS)
BENIGN = 2.0                                   # inside every support above, and a valid k of Binomial(8, .)


def runtime_statements():
    out = []
    for i, (name, fam, par, dist) in enumerate(_RUNTIME_DISTS):
        site = f"v{i}"
        if name == "pois_c":                   # an expression of the site, not the site: the value comes out of the accumulator
            out.append(Stmt(name, fam, par, (lambda s, site=site: s[site] * 1.0), (lambda e, dist=dist, site=site: (dist(e), e[site] * 1.0))))
        else:
            out.append(Stmt(name, fam, par, (lambda s, site=site: s[site]), (lambda e, dist=dist, site=site: (dist(e), e[site]))))
    out.append(Stmt("binom_n", "Binomial", lambda s: [s["w"], 0.25], lambda s: 2.0, lambda e: (M.Binomial(e["w"], 0.25), 2.0)))
    return out


RUNTIME_SITES = [("x", M.Normal(0.0, 1.0))] + [(f"v{i}", M.Normal(0.0, 1.0)) for i in range(N_V)] + [("w", M.Normal(0.0, 1.0))]
CONST_SITES = [("lam", M.Gamma(2.0, 1.0)), ("q", M.Beta(2.0, 2.0))]
N_CASES = N_V * len(VALUES) + len(BINOMIAL_N)


def runtime_case(n):
    """case n -> the site values of one chain: statement n // 21 observes fixture value n % 21, or (the last 11 cases) w = a Binomial-n row"""
    s = {"x": XS[n % len(XS)], "w": 8.0}
    s.update({f"v{i}": BENIGN for i in range(N_V)})
    if n < N_V * len(VALUES):
        s[f"v{n // len(VALUES)}"] = VALUES[n % len(VALUES)]
    else:
        s["w"] = BINOMIAL_N[n - N_V * len(VALUES)]
    return s


def runtime_tables(n_chains=C):
    """value tables [table][chain] that together hold every case (the last table wraps round to the first cases)"""
    n_tables = -(-N_CASES // n_chains)
    return [[runtime_case((t * n_chains + k) % N_CASES) for k in range(n_chains)] for t in range(n_tables)]


_CONST_DISTS = [
    ("pois_c", "Poisson", lambda s: [3.0], lambda e: M.Poisson(3.0)),
    ("pois_s", "Poisson", lambda s: [s["lam"]], lambda e: M.Poisson(e["lam"])),                                   # FG_F_XHOIST: ln k!
    ("binom_c", "Binomial", lambda s: [8.0, 0.25], lambda e: M.Binomial(8, 0.25)),
    ("binom_s", "Binomial", lambda s: [8.0, s["q"]], lambda e: M.Binomial(8, e["q"])),                            # FG_F_XHOIST: ln C(n, k)
    ("cat_c", "Categorical", lambda s: [0.2, 0.5, 0.3], lambda e: M.Categorical([0.2, 0.5, 0.3])),
    ("cat_s", "Categorical", lambda s: [s["q"], 1.0 - s["q"]], lambda e: M.Categorical([e["q"], 1.0 - e["q"]])),
    ("du_c", "DiscreteUniform", lambda s: [1, 9], lambda e: M.DiscreteUniform(1, 9)),
    ("du_s", "DiscreteUniform", lambda s: [1.0, s["lam"] + 7.0], lambda e: M.DiscreteUniform(1.0, e["lam"] + 7.0)),    # bounds `as i64`
    ("du_neg", "DiscreteUniform", lambda s: [-2, 2], lambda e: M.DiscreteUniform(-2, 2)),
    ("du_52", "DiscreteUniform", lambda s: [2.0, P52], lambda e: M.DiscreteUniform(2.0, P52)),
    ("du_top", "DiscreteUniform", lambda s: [2.0, TOP], lambda e: M.DiscreteUniform(2.0, TOP)),
    ("du_max", "DiscreteUniform", lambda s: [2.0, P63], lambda e: M.DiscreteUniform(2.0, P63)),
    ("bern_c", "Bernoulli", lambda s: [0.3], lambda e: M.Bernoulli(0.3)),
    ("bern_s", "Bernoulli", lambda s: [s["q"]], lambda e: M.Bernoulli(e["q"])),
]
STREAMABLE = ("pois_c", "pois_s", "binom_s", "bern_c", "bern_s")


def all_statements():
    return [Stmt(f"{tag}#{i}", fam, par, (lambda s, v=val: v), (lambda e, dist=dist, v=val: (dist(e), v)))
            for i, val in enumerate(FINITE) for tag, fam, par, dist in _CONST_DISTS]


def const_site_values(n_chains=C):
    return [{"lam": RATES[k % len(RATES)], "q": PROBS[(k // len(RATES)) % len(PROBS)]} for k in range(n_chains)]


def split_statements(oracle):
    """ALL -> (small, big, rest) by the expectation alone: finite on every parameter combination and below / beyond BIG, or not finite somewhere"""
    stm = all_statements()
    exp = expected_table(oracle, stm, const_site_values(len(RATES) * len(PROBS)))
    small = [st for st, row in zip(stm, exp) if np.isfinite(row).all() and np.abs(row).max() < BIG]
    big = [st for st, row in zip(stm, exp) if np.isfinite(row).all() and np.abs(row).max() >= BIG]
    rest = [st for st, row in zip(stm, exp) if not np.isfinite(row).all()]
    return small, big, rest


def streamable(statements):
    return [st for st in statements if st.address.split("#")[0] in STREAMABLE]


def build(statements, sites):
    """sites: [(name, Dist)] sampled first, in this order -> Program"""
    P = M.Program()
    e = {name: P.sample(M.addr(name), dist) for name, dist in sites}
    for st in statements:
        dist, value = st.make(e)
        P.observe(st.address, dist, value)
    return P


def cells_of(site_names, site_values):
    """[S][C] int64 cells (every site here is f64: the double's bits, NaN payloads and the sign of zero as the fixture gives them)"""
    cells = np.zeros((len(site_names), len(site_values)), dtype=np.int64)
    for j, name in enumerate(site_names):
        for k, s in enumerate(site_values):
            cells[j, k] = R.to_bits(s[name])
    return cells


def prior_of(sites, s):
    """log-density of the latent sites (all continuous, constant parameters), by the formulas of distribution.rs:189-208, 897-956, 1039-1068"""
    total = 0.0
    for name, dist in sites:
        x, p = s[name], [q.value for q in dist.params]
        if dist.name == "Normal":
            lp = -math.inf if not math.isfinite(x) else -0.5 * ((x - p[0]) / p[1]) * ((x - p[0]) / p[1]) - math.log(p[1]) - 0.5 * 1.8378770664093456
        elif dist.name == "Gamma":
            lp = p[0] * math.log(p[1]) + (p[0] - 1.0) * math.log(x) - p[1] * x - math.lgamma(p[0])
        elif dist.name == "Beta":
            lp = (p[0] - 1.0) * math.log(x) + (p[1] - 1.0) * math.log(1.0 - x) - (math.lgamma(p[0]) + math.lgamma(p[1]) - math.lgamma(p[0] + p[1]))
        else:
            raise KeyError(dist.name)
        total += lp
    return total


def expected_table(oracle, statements, site_values):
    """[n statements][n chains]: the reference's log-weight of every observe statement at every chain's site values"""
    out = np.zeros((len(statements), len(site_values)))
    memo = {}
    for i, st in enumerate(statements):
        for k, s in enumerate(site_values):
            p, x = st.params(s), st.observed(s)
            key = (st.family, tuple(R.to_bits(float(q)) for q in p), R.to_bits(float(x)))
            if key not in memo:
                memo[key] = R.expected_logpdf(oracle, st.family, float(x), p)
            out[i, k] = memo[key]
    return out


def in_order_sum(column):
    """the likelihood accumulator: the statements' terms added in program order, starting from 0.0 (interpreters.rs:76-83)"""
    acc = 0.0
    for t in column:
        acc += float(t)
    return acc


def check(got, exp, what):
    """exact for a non-finite expectation, 1e-12 max(1, |exp|) otherwise: the project's log-joint tolerance"""
    got, exp = float(got), float(exp)
    if not math.isfinite(exp):
        assert got == exp or (math.isnan(exp) and math.isnan(got)), (what, got, exp)
    else:
        assert math.isfinite(got) and abs(got - exp) <= 1e-12 * max(1.0, abs(exp)), (what, got, exp, abs(got - exp))
