"""Posterior predictive checks: test statistics of every replicated data set compared with the same statistic of the observed data
-- the step the reference's workflows do by hand after replicating the data (tests/end_to_end_workflows.rs:650-745: the mean and
the variance with divisor K - 1; examples/bayesian_coin_flip.rs:211-: the number of heads, read as a p-value) -- computed on the
device by the check stream (`Engine.ppc_stream`, fg_ppc_stream.hip), for f64 and discrete observe sites alike.

The drivers `hmc_chain_summary(checks=...)` / `adaptive_mcmc_chain_summary(checks=...)` feed the stream chunk by chunk and never
hold the replicates (`ChainSummary.checks`); `posterior_predictive_check` takes the stored replicates of a `ChainBatch` or a
`PriorPredictive` and feeds them as one chunk -- the same figures bit for bit, since the stream does not depend on the chunking.

A check is a group of observe addresses (`CheckSpec`); a slot is one statistic of one check.  The draws of an SMC population are
weighted and the counts here are not: an `SMCResult` is refused.

A weighted population has `weighted_predictive_check` (a stored `SMCResult`) and `adaptive_smc_summary(checks=...)` (on the device,
`PopulationSummary.checks`): the same statistics of one replicate per particle, the p-values as quotients of the units
rint(w 2^52) of the weights -- exact integers (`WeightedPredictiveCheck`; `WeightedPopulation.checks`, fg_wpop_eval.hip)."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import engine as E
from . import workloads as W

STATISTICS = E.PPC_STATS
P_VALUES = ("p_ge", "p_gt", "p_mid")


@dataclass
class CheckSpec:
    """One check: the observe `addresses` whose replicates form a data set (in this order), and the `statistics` of it to compare."""
    name: str
    addresses: Sequence[str]
    statistics: Sequence[str] = STATISTICS

    def __post_init__(self):
        self.addresses = [self.addresses] if isinstance(self.addresses, str) else [str(a) for a in self.addresses]
        self.statistics = [self.statistics] if isinstance(self.statistics, str) else list(self.statistics)
        if not self.addresses:
            raise ValueError(f"check {self.name!r} names no address")
        if not self.statistics:
            raise ValueError(f"check {self.name!r} names no statistic")
        for st in self.statistics:
            if st not in STATISTICS:
                raise ValueError(f"check {self.name!r}: {st!r} is no statistic {STATISTICS}")
        if len(set(self.statistics)) != len(self.statistics):
            raise ValueError(f"check {self.name!r} names a statistic twice")


def marginal_checks(addresses: Sequence[str]) -> List[CheckSpec]:
    """One check per address with the statistic "mean": K = 1, so the statistic is the replicated value itself and `p_mid` is the
    PIT value of that observation."""
    return [CheckSpec(str(a), [str(a)], ("mean",)) for a in addresses]


def _ratio(num: np.ndarray, den: np.ndarray) -> np.ndarray:
    out = np.full(len(den), np.nan)
    ok = den > 0
    out[ok] = num[ok].astype(np.float64) / den[ok].astype(np.float64)
    return out


def _p_values(n_lt, n_eq, n_gt) -> Dict[str, np.ndarray]:
    n_lt, n_eq, n_gt = (np.asarray(a, dtype=np.int64) for a in (n_lt, n_eq, n_gt))
    N = n_lt + n_eq + n_gt
    return dict(p_ge=_ratio(n_gt + n_eq, N), p_gt=_ratio(n_gt, N), p_mid=_ratio(2 * n_gt + n_eq, 2 * N))


@dataclass
class PredictiveCheck:
    """Per slot (`names[k]`, `statistics[k]`: one statistic of one check; [n_slots] each) over `n_draws` pooled draws of `n_chains`
    chains: `t_obs`, the statistic of the observed data; `n_lt`, `n_eq`, `n_gt`, the draws whose replicated statistic is below, equal
    to, above it; `n_nan`, the draws where either side is NaN (they enter no p-value); `n_fin`, `t_rep_mean`, `t_rep_ssd`, the count,
    mean and sum of squared deviations of the finite replicated statistics."""
    names: List[str]
    statistics: List[str]
    n_draws: int
    n_chains: int
    t_obs: np.ndarray
    n_lt: np.ndarray
    n_eq: np.ndarray
    n_gt: np.ndarray
    n_nan: np.ndarray
    n_fin: np.ndarray
    t_rep_mean: np.ndarray
    t_rep_ssd: np.ndarray
    chain_sd: np.ndarray = field(default_factory=lambda: np.zeros((0, 3)))    # [n_slots][3]: between-chain sd of p_ge, p_gt, p_mid

    @classmethod
    def from_stream(cls, specs: Sequence[CheckSpec], stream: "E.PpcStream", n_draws: int, n_chains: int) -> "PredictiveCheck":
        """From a complete `PpcStream` whose checks are `specs`, in that order.  The between-chain spreads are taken here, while the
        stream is alive: one download of 5 C counters and one standard deviation per slot (the result outlives the stream, so they
        cannot be fetched on demand later)."""
        pooled = stream.pooled()
        names = [specs[q].name for q, _ in stream.slots]
        stats = [STATISTICS[st] for _, st in stream.slots]
        sd = np.full((stream.n_slots, 3), np.nan)
        for k in range(stream.n_slots):
            ch = stream.chains(k)
            p = _p_values(ch["n_lt"], ch["n_eq"], ch["n_gt"])
            for i, which in enumerate(P_VALUES):
                v = p[which][np.isfinite(p[which])]
                if v.size >= 2:
                    sd[k, i] = float(np.std(v, ddof=1))
        return cls(names, stats, int(n_draws), int(n_chains), stream.observed(), pooled["n_lt"], pooled["n_eq"], pooled["n_gt"], pooled["n_nan"],
                   pooled["n_fin"], pooled["mean"], pooled["ssd"], sd)

    @property
    def n_slots(self) -> int:
        return len(self.names)

    def slot(self, name: str, statistic: str) -> int:
        for k, (a, st) in enumerate(zip(self.names, self.statistics)):
            if a == name and st == statistic:
                return k
        raise KeyError(f"no slot ({name!r}, {statistic!r})")

    @property
    def p_ge(self) -> np.ndarray:
        """(n_gt + n_eq) / N, N = n_lt + n_eq + n_gt: the share of replicated data sets at least as extreme as the data -- the p-value of
        the coin-flip tutorial ("extreme p-values (< 0.05 or > 0.95) suggest potential model issues")."""
        return _p_values(self.n_lt, self.n_eq, self.n_gt)["p_ge"]

    @property
    def p_gt(self) -> np.ndarray:
        return _p_values(self.n_lt, self.n_eq, self.n_gt)["p_gt"]

    @property
    def p_mid(self) -> np.ndarray:
        """(n_gt + n_eq / 2) / N: the mid p-value; for a marginal check the PIT value of the observation, correct for discrete data."""
        return _p_values(self.n_lt, self.n_eq, self.n_gt)["p_mid"]

    @property
    def t_rep_sd(self) -> np.ndarray:
        """The standard deviation (ddof = 1) of the finite replicated statistics; NaN below two of them."""
        out = np.full(self.n_slots, np.nan)
        ok = np.asarray(self.n_fin) >= 2
        with np.errstate(invalid="ignore"):
            out[ok] = np.sqrt(np.asarray(self.t_rep_ssd)[ok] / (np.asarray(self.n_fin)[ok] - 1).astype(np.float64))
        return out

    def between_chain_sd(self, slot: int, which: str = "p_mid") -> float:
        """The standard deviation (ddof = 1) over the chains of a slot's p-value computed per chain: how far the pooled figure rests on
        single chains.  NaN below two chains with a draw that counts."""
        if which not in P_VALUES:
            raise ValueError(f"between_chain_sd: {which!r} is none of {P_VALUES}")
        return float(self.chain_sd[int(slot), P_VALUES.index(which)])


def resolve_checks(checks, names: Sequence[str], stated: Sequence[Optional[float]], observed: Optional[Dict[str, float]], who: str
                   ) -> Tuple[List[CheckSpec], List[Tuple[List[int], List[str], List[float]]]]:
    """`checks` (None / True: one check "all" over every address of `names` with all five statistics; else CheckSpecs) against the
    addresses `names` with the observed values `stated` the model gives (None where the value reads a site) and the overrides
    `observed`: -> (specs, [(indices into names, statistics, observed values)])."""
    names = list(names)
    specs = [CheckSpec("all", names)] if checks is None or checks is True else [checks] if isinstance(checks, CheckSpec) else list(checks)
    if not specs:
        raise ValueError(f"{who}: checks is an empty list")
    observed = dict(observed or {})
    for a in observed:
        if a not in names:
            raise ValueError(f"{who}: observed names {a!r}, which is no observe address at hand")
    seen, out = set(), []
    for sp in specs:
        if not isinstance(sp, CheckSpec):
            raise TypeError(f"{who}: checks holds a {type(sp).__name__}, not a CheckSpec")
        if sp.name in seen:
            raise ValueError(f"{who}: two checks are named {sp.name!r}")
        seen.add(sp.name)
        rows, obs = [], []
        for a in sp.addresses:
            if a not in names:
                raise ValueError(f"{who}: check {sp.name!r} names {a!r}, which is no observe address at hand")
            k = names.index(a)
            v = observed.get(a, stated[k] if k < len(stated) else None)
            if v is None:
                raise ValueError(f"{who}: the observed value of {a!r} reads a site, so the model states no number for it; pass observed={{{a!r}: value}}")
            rows.append(k)
            obs.append(float(v))
        out.append((rows, list(sp.statistics), obs))
    return specs, out


def posterior_predictive_check(x, checks: Optional[Sequence[CheckSpec]] = None, observed: Optional[Dict[str, float]] = None, device: int = 0) -> PredictiveCheck:
    """The checks of stored replicates: `x` is a `ChainBatch` of a chain driver run with `predictive=` or a `PriorPredictive`.  The
    cells are uploaded and run through the check stream as one chunk (value types from `predictive_vtypes`, nothing is converted on
    the host).  `checks=None`: one check "all" over every stored observe row with all five statistics.  The observed value of a
    member is the one the model states (`fg_program_observe_value`); `observed={address: value}` overrides it, and is needed where the
    model's value reads a site (ValueError naming the address otherwise).  An `SMCResult` raises ValueError: its particles are
    weighted."""
    who = "posterior_predictive_check"
    from .inference import SMCResult                     # late: inference imports this module's names lazily
    if isinstance(x, SMCResult) or hasattr(x, "weights"):
        raise ValueError(f"{who}: an SMCResult holds a weighted population; the counts of a check are unweighted (resample it, or run a chain driver)")
    cells = getattr(x, "predictive", None)
    if cells is None or not hasattr(x, "predictive_vtypes"):
        raise ValueError(f"{who}: no stored replicates (run the driver with predictive=True)")
    cells = np.ascontiguousarray(cells, dtype=np.int64)
    if cells.ndim == 2:
        cells = cells[None]
    if cells.ndim != 3 or min(cells.shape) < 1:
        raise ValueError(f"{who}: the replicates must be [n][n_sel][C] with every extent at least 1, not {cells.shape}")
    n, n_rows, C_ = cells.shape
    names, vtypes = list(x.predictive_names), [int(v) for v in x.predictive_vtypes]
    stated = [(getattr(x, "observe_values", None) or {}).get(a) for a in names]
    specs, tuples = resolve_checks(checks, names, stated, observed, who)
    eng = E.Engine(E.compile_model(W.normal_sites(1)), C_, seed=0, device=device)       # the stream wants the engine's chain count only
    buf = stream = None
    try:
        buf = eng.upload(cells)
        stream = eng.ppc_stream(n, vtypes, tuples)
        stream.update(buf, n)
        return PredictiveCheck.from_stream(specs, stream, n * C_, C_)
    finally:
        if stream is not None:
            stream.free()
        if buf is not None:
            eng.device_free(buf)
        eng.close()


@dataclass
class WeightedPredictiveCheck:
    """Per slot (`names[k]`, `statistics[k]`; [n_slots] each) over the `n_particles` particles of a weighted population of `T` units
    (rint(w 2^52) each): `t_obs`; `units` uint64 [n_slots][4], the units of the particles whose replicated statistic is below / equal
    to / above the observed one, or where either side is NaN (they enter no p-value); `counts` int64 [n_slots][4], the particles of
    non-zero units behind them; `p_ge`, `p_gt`, `p_mid`, quotients of unit sums (NaN for a denominator of 0); `t_rep_mean`,
    `t_rep_sd`, `t_rep_mcse`, `n_used`: the weighted moments of the finite replicated statistics (`WeightedPopulation.moments`)."""
    names: List[str]
    statistics: List[str]
    n_particles: int
    T: int
    t_obs: np.ndarray
    units: np.ndarray
    counts: np.ndarray
    p_ge: np.ndarray
    p_gt: np.ndarray
    p_mid: np.ndarray
    t_rep_mean: np.ndarray
    t_rep_sd: np.ndarray
    t_rep_mcse: np.ndarray
    n_used: np.ndarray

    @classmethod
    def from_parts(cls, specs: Sequence[CheckSpec], parts: Sequence[Tuple[int, dict]], n_particles: int, T: int) -> "WeightedPredictiveCheck":
        """From the results of `WeightedPopulation.checks` over consecutive groups of `specs`: [(index of the group's first check, result)]."""
        names = [specs[q0 + q].name for q0, r in parts for q, _ in r["slots"]]
        stats = [STATISTICS[st] for _, r in parts for _, st in r["slots"]]
        cat = lambda key: np.concatenate([np.asarray(r[key]) for _, r in parts])
        return cls(names, stats, int(n_particles), int(T), cat("t_obs"), cat("units"), cat("counts"), cat("p_ge"), cat("p_gt"), cat("p_mid"), cat("mean"), cat("std"),
                   cat("mcse"), cat("n_used"))

    @property
    def n_slots(self) -> int:
        return len(self.names)

    def slot(self, name: str, statistic: str) -> int:
        for k, (a, st) in enumerate(zip(self.names, self.statistics)):
            if a == name and st == statistic:
                return k
        raise KeyError(f"no slot ({name!r}, {statistic!r})")


def check_groups(tuples, N: int, budget_words: int = 1 << 24):
    """Consecutive checks whose member rows together stay within `budget_words` cells of N each (a single check that does not is a
    group of its own): [(first check, rows of the group, the group's checks over those rows)]."""
    cap = max(1, budget_words // max(int(N), 1))
    out, q = [], 0
    while q < len(tuples):
        rows, q1 = set(tuples[q][0]), q + 1
        while q1 < len(tuples) and len(rows | set(tuples[q1][0])) <= cap:
            rows |= set(tuples[q1][0])
            q1 += 1
        sel = sorted(rows)
        out.append((q, sel, [([sel.index(k) for k in r], st, ob) for r, st, ob in tuples[q:q1]]))
        q = q1
    return out


def weighted_predictive_check(smc, checks: Optional[Sequence[CheckSpec]] = None, observed: Optional[Dict[str, float]] = None, device: int = 0) -> WeightedPredictiveCheck:
    """The checks of the stored replicates of an `SMCResult` (`adaptive_smc(predictive=True)`: one replicate per particle) under its
    weights: cells and weights are uploaded and run through `WeightedPopulation.checks`, the entry `adaptive_smc_summary(checks=...)`
    runs where the population lies -- the same bytes.  `checks` / `observed` as `posterior_predictive_check` takes them.  Weights that
    are not all in [0, 1] raise ValueError (n_bad > 0), as the summary does."""
    who = "weighted_predictive_check"
    cells, w = getattr(smc, "predictive", None), getattr(smc, "weights", None)
    if w is None:
        raise ValueError(f"{who}: no weights (an unweighted batch goes to posterior_predictive_check)")
    if cells is None or not hasattr(smc, "predictive_vtypes"):
        raise ValueError(f"{who}: no stored replicates (run adaptive_smc with predictive=True)")
    cells, w = np.ascontiguousarray(cells, dtype=np.int64), np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
    if cells.ndim != 2 or min(cells.shape) < 1 or cells.shape[1] != w.size:
        raise ValueError(f"{who}: the replicates must be [n_sel][N] with N = {w.size} weights, not {cells.shape}")
    n_bad = int(np.count_nonzero(~((w >= 0.0) & (w <= 1.0))))
    if n_bad > 0:
        raise ValueError(f"{who}: n_bad = {n_bad} of {w.size} weights are NaN, negative, infinite or above 1: the population is not normalised")
    names, vtypes = list(smc.predictive_names), [int(v) for v in smc.predictive_vtypes]
    stated = [(getattr(smc, "observe_values", None) or {}).get(a) for a in names]
    specs, tuples = resolve_checks(checks, names, stated, observed, who)
    with E.stored_population(w, cells, device) as (wp, d_cells):
        return WeightedPredictiveCheck.from_parts(specs, [(0, wp.checks(d_cells, vtypes, tuples))], w.size, wp.units()["T"])
