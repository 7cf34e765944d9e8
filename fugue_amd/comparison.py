"""Model comparison from the pointwise log-likelihood: WAIC and importance-sampling LOO per observe statement (BDA3 7.2; the
reference has neither), computed on the device by the log-likelihood stream (`Engine.loglik_stream`, fg_loglik_stream.hip).

The drivers `hmc_chain_summary(pointwise=...)` / `adaptive_mcmc_chain_summary(pointwise=...)` feed the stream chunk by chunk and never
hold the table (`ChainSummary.comparison`); `model_comparison` takes a stored table ([n][n_sel][C], or a `ChainBatch` of
`hmc_chain(pointwise=True)`) and feeds it as one chunk -- the same figures bit for bit, since the stream does not depend on the
chunking.

`p_waic` is the UNBIASED variance of the pointwise log-likelihood over the N = n_draws x n_chains pooled draws (divisor N - 1: BDA3
eq. 7.12 and the R `loo` package; ArviZ divides by N).  `elpd_loo` is plain importance-sampling LOO with the raw ratios
r = exp(-log-likelihood).  `is_ess` = (sum r)^2 / sum r^2 and `max_weight` = max r / sum r are the honest diagnostic of those raw
ratios: an `is_ess` of a few, or a `max_weight` near 1, says the estimate of that statement rests on a handful of draws.

A STORED table also has the Pareto-smoothed estimate with its k-hat (`psis_loo`, `model_comparison(..., psis=True)` -> `PsisLoo`;
`Engine.psis_loo`, fg_psis.hip): the R `loo` package's psis / gpdfit with r_eff = 1, on the device, nothing replayed.
The chunked summaries (`ChainSummary.comparison`) and weighted populations still give the raw estimate only: they never hold the
table, and the tail would have to be carried across chunks.

A weighted population has `weighted_model_comparison` (a stored `SMCResult`) and `adaptive_smc_summary(pointwise=...)` (on the device,
`PopulationSummary.comparison`): the same figures under the particles' weights (`WeightedComparison`; `WeightedPopulation.loglik`,
fg_wpop_eval.hip), `p_waic` in its reliability-weights form ssd / (W - sum w^2 / W), which is the divisor N - 1 at equal weights."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import engine as E
from . import workloads as W

POINTWISE = ("lppd", "mean_ll", "p_waic", "elpd_waic", "elpd_loo", "p_loo", "is_ess", "max_weight")


def _total(a: np.ndarray) -> float:
    t = 0.0
    for v in np.asarray(a, dtype=np.float64).tolist():      # a plain sum in index order
        t += v
    return t


@dataclass
class PointwiseComparison:
    """Per selected observe statement (`names`, [n_sel] each) over `n_draws` = N pooled draws: `lppd` = ln((1/N) sum exp x),
    `mean_ll`, `p_waic` (variance, divisor N - 1), `elpd_waic` = lppd - p_waic, `elpd_loo` = -ln((1/N) sum exp(-x)), `p_loo` = lppd -
    elpd_loo, `is_ess`, `max_weight`, and the counts of cells that are -inf / +inf / NaN.  A NaN cell makes every figure of its
    statement NaN; a -inf cell makes elpd_loo -inf; a +inf cell makes lppd +inf."""
    names: List[str]
    n_draws: int
    lppd: np.ndarray
    mean_ll: np.ndarray
    p_waic: np.ndarray
    elpd_waic: np.ndarray
    elpd_loo: np.ndarray
    p_loo: np.ndarray
    is_ess: np.ndarray
    max_weight: np.ndarray
    n_neg_inf: np.ndarray
    n_pos_inf: np.ndarray
    n_nan: np.ndarray
    psis: Optional["PsisLoo"] = None            # `model_comparison(..., psis=True)`: the Pareto-smoothed LOO of the same table

    @classmethod
    def from_result(cls, names: Sequence[str], n_draws: int, res: dict) -> "PointwiseComparison":
        """From `LoglikStream.result()`."""
        return cls(names=list(names), n_draws=int(n_draws), **{k: res[k] for k in POINTWISE + ("n_neg_inf", "n_pos_inf", "n_nan")})

    @property
    def n_sel(self) -> int:
        return len(self.names)

    @property
    def elpd_waic_total(self) -> float:
        return _total(self.elpd_waic)

    @property
    def elpd_loo_total(self) -> float:
        return _total(self.elpd_loo)

    @property
    def p_waic_total(self) -> float:
        return _total(self.p_waic)

    @property
    def p_loo_total(self) -> float:
        return _total(self.p_loo)

    @property
    def lppd_total(self) -> float:
        return _total(self.lppd)

    def se(self, name: str = "elpd_loo") -> float:
        """The standard error of the total of a pointwise figure: sqrt(O var(pointwise, ddof=1)), O statements (NaN for O = 1)."""
        if name not in POINTWISE:
            raise ValueError(f"se: {name!r} is no pointwise figure {POINTWISE}")
        return _se(getattr(self, name))


def _se(a: np.ndarray) -> float:
    a = np.asarray(a, dtype=np.float64)
    if a.size < 2:
        return float("nan")
    with np.errstate(invalid="ignore"):
        return float(math.sqrt(a.size * float(np.var(a, ddof=1)))) if np.isfinite(a).all() else float("nan")


PSIS_POINTWISE = ("elpd_loo_psis", "p_loo_psis", "khat", "sigma", "khat_threshold", "lppd")


@dataclass
class PsisLoo:
    """Pareto-smoothed importance-sampling LOO per selected observe statement (`names`, [n_sel] each) over `n_draws` = S pooled draws
    (`Engine.psis_loo`, fg_psis.hip): `elpd_loo_psis`, `p_loo_psis` = lppd - elpd_loo_psis, `khat` and `sigma` of the
    generalised Pareto fit to the `tail_len` = M largest ratios, `khat_threshold` = min(1 - 1 / log10 S, 0.7), `n_capped` smoothed
    ratios cut at the largest raw one, `status` (an index into `engine.PSIS_STATUS`: fitted, too few draws, degenerate tail,
    non-finite cells) and the counts of cells that are -inf / +inf / NaN.  Without a fit `khat` = +inf and `elpd_loo_psis` is the raw
    importance-sampling value; a NaN cell makes every figure of its statement NaN; a -inf cell makes elpd_loo_psis -inf."""
    names: List[str]
    n_draws: int
    elpd_loo_psis: np.ndarray
    p_loo_psis: np.ndarray
    khat: np.ndarray
    sigma: np.ndarray
    khat_threshold: np.ndarray
    lppd: np.ndarray
    tail_len: np.ndarray
    status: np.ndarray
    n_capped: np.ndarray
    n_neg_inf: np.ndarray
    n_pos_inf: np.ndarray
    n_nan: np.ndarray

    @classmethod
    def from_result(cls, names: Sequence[str], n_draws: int, res: dict) -> "PsisLoo":
        """From `Engine.psis_loo`."""
        return cls(names=list(names), n_draws=int(n_draws), **{k: res[k] for k in PSIS_POINTWISE + ("tail_len", "status", "n_capped", "n_neg_inf", "n_pos_inf", "n_nan")})

    @property
    def n_sel(self) -> int:
        return len(self.names)

    @property
    def elpd_loo_psis_total(self) -> float:
        return _total(self.elpd_loo_psis)

    @property
    def p_loo_psis_total(self) -> float:
        return _total(self.p_loo_psis)

    def se(self, name: str = "elpd_loo_psis") -> float:
        """The standard error of the total of a pointwise figure: sqrt(O var(pointwise, ddof=1)), O statements (NaN for O = 1)."""
        if name not in PSIS_POINTWISE:
            raise ValueError(f"se: {name!r} is no pointwise figure {PSIS_POINTWISE}")
        return _se(getattr(self, name))

    def n_bad_k(self) -> int:
        """the statements whose khat lies above khat_threshold (a NaN khat counts: nothing vouches for that statement)"""
        k, t = np.asarray(self.khat, dtype=np.float64), np.asarray(self.khat_threshold, dtype=np.float64)
        with np.errstate(invalid="ignore"):
            return int(np.count_nonzero(~(k <= t)))

    def status_words(self) -> List[str]:
        return [E.PSIS_STATUS[int(s)] for s in self.status]


def _table_and_names(who: str, x, names):
    ll = getattr(x, "log_likelihood", x)
    if ll is None:
        raise ValueError(f"{who}: the ChainBatch has no log_likelihood (run the driver with pointwise=True)")
    if names is None:
        names = getattr(x, "predictive_names", None) if ll is not x else None
    table = np.ascontiguousarray(ll, dtype=np.float64)
    if table.ndim != 3 or min(table.shape) < 1:
        raise ValueError(f"{who}: the table must be [n][n_sel][C] with every extent at least 1, not {table.shape}")
    n_sel = table.shape[1]
    names = [f"observe#{k}" for k in range(n_sel)] if names is None else [str(a) for a in names]
    if len(names) != n_sel:
        raise ValueError(f"{who}: {len(names)} names for {n_sel} statements")
    return table, names


def psis_loo(x, names: Optional[Sequence[str]] = None, device: int = 0) -> PsisLoo:
    """Pareto-smoothed LOO and khat of a stored pointwise log-likelihood table: `x` as `model_comparison` takes it.  The table is
    uploaded and `Engine.psis_loo` runs on it; nothing is replayed.  n x C must stay below 2^31."""
    table, names = _table_and_names("psis_loo", x, names)
    n, n_sel, C_ = table.shape
    eng = E.Engine(E.compile_model(W.normal_sites(1)), C_, seed=0, device=device)
    buf = None
    try:
        buf = eng.upload(table)
        return PsisLoo.from_result(names, n * C_, eng.psis_loo(buf, n, n_sel))
    finally:
        if buf is not None:
            eng.device_free(buf)
        eng.close()


def model_comparison(x, names: Optional[Sequence[str]] = None, device: int = 0, psis: bool = False) -> PointwiseComparison:
    """WAIC / IS-LOO of a stored pointwise log-likelihood table: `x` is a `ChainBatch` with `log_likelihood` (names default to its
    `predictive_names`) or an array [n][n_sel][C].  The table is uploaded and run through the log-likelihood stream as one chunk;
    device memory is the table plus 80 x n_sel x C bytes.  `psis=True` also runs `Engine.psis_loo` on the uploaded table: the result
    carries it as `.psis` (a `PsisLoo`; None otherwise)."""
    ll = getattr(x, "log_likelihood", x)
    if ll is None:
        raise ValueError("model_comparison: the ChainBatch has no log_likelihood (run the driver with pointwise=True)")
    if names is None:
        names = getattr(x, "predictive_names", None) if ll is not x else None
    table = np.ascontiguousarray(ll, dtype=np.float64)
    if table.ndim != 3 or min(table.shape) < 1:
        raise ValueError(f"model_comparison: the table must be [n][n_sel][C] with every extent at least 1, not {table.shape}")
    n, n_sel, C_ = table.shape
    names = [f"observe#{k}" for k in range(n_sel)] if names is None else [str(a) for a in names]
    if len(names) != n_sel:
        raise ValueError(f"model_comparison: {len(names)} names for {n_sel} statements")
    eng = E.Engine(E.compile_model(W.normal_sites(1)), C_, seed=0, device=device)       # the stream wants the engine's chain count only
    buf = stream = None
    try:
        buf = eng.upload(table)
        stream = eng.loglik_stream(n, n_sel)
        stream.update(buf, n)
        out = PointwiseComparison.from_result(names, n * C_, stream.result())
        if psis:
            out.psis = PsisLoo.from_result(names, n * C_, eng.psis_loo(buf, n, n_sel))
        return out
    finally:
        if stream is not None:
            stream.free()
        if buf is not None:
            eng.device_free(buf)
        eng.close()


def compare_models(a: PointwiseComparison, b: PointwiseComparison, which: str = "elpd_loo") -> Tuple[float, float]:
    """(total of a - total of b, the standard error of the pointwise difference sqrt(O var(a_k - b_k, ddof=1))) for `which` =
    "elpd_loo" | "elpd_waic" | "elpd_loo_psis" (both sides must carry `.psis`: `model_comparison(..., psis=True)`).  Both must hold the
    same observe statements in the same order (the same data): ValueError otherwise."""
    if which not in ("elpd_loo", "elpd_waic", "elpd_loo_psis"):
        raise ValueError(f"compare_models: which must be 'elpd_loo', 'elpd_waic' or 'elpd_loo_psis', not {which!r}")
    if a.n_sel != b.n_sel:
        raise ValueError(f"compare_models: {a.n_sel} statements against {b.n_sel}")
    if list(a.names) != list(b.names):
        raise ValueError("compare_models: the two comparisons name different observe statements")
    if which == "elpd_loo_psis":
        if getattr(a, "psis", None) is None or getattr(b, "psis", None) is None:
            raise ValueError("compare_models: 'elpd_loo_psis' needs both comparisons to carry .psis (model_comparison(..., psis=True))")
        a, b = a.psis, b.psis
    pa, pb = np.asarray(getattr(a, which), dtype=np.float64), np.asarray(getattr(b, which), dtype=np.float64)
    return _total(pa) - _total(pb), _se(pa - pb)


@dataclass
class WeightedComparison(PointwiseComparison):
    """`PointwiseComparison` under the weights of a population of `n_draws` particles (so `compare_models` takes it as it stands):
    lppd = ln(sum w exp x / W), elpd_loo = -ln(sum w exp(-x) / W), p_waic = ssd / (W_fin - sum w^2 / W_fin), is_ess = the Kish
    effective size of the weights w exp(-x), in particles.  The counters count the cells of the particles that take part (a good
    weight above zero): `n_fin` finite ones beside -inf / +inf / NaN; `words` [n_sel][12] in the order `engine.WLL_WORDS`.  A statement
    without a finite participating cell has NaN figures."""
    n_fin: np.ndarray = None
    words: np.ndarray = None

    @classmethod
    def from_parts(cls, names: Sequence[str], n_particles: int, parts: Sequence[dict]) -> "WeightedComparison":
        """From the results of `WeightedPopulation.loglik` over consecutive slices of the statements."""
        cat = lambda key: np.concatenate([np.asarray(r[key]) for r in parts])
        return cls(names=list(names), n_draws=int(n_particles), **{k: cat(k) for k in POINTWISE + ("n_neg_inf", "n_pos_inf", "n_nan", "n_fin", "words")})


def weighted_model_comparison(smc, names: Optional[Sequence[str]] = None, device: int = 0) -> WeightedComparison:
    """WAIC / IS-LOO of the stored pointwise log-likelihood of an `SMCResult` (`adaptive_smc(pointwise=True)`: [n_sel][N]) under its
    weights: table and weights are uploaded and run through `WeightedPopulation.loglik`, the entry `adaptive_smc_summary(pointwise=...)`
    runs where the population lies -- the same bytes.  Weights that are not all in [0, 1] raise ValueError (n_bad > 0)."""
    who = "weighted_model_comparison"
    ll, w = getattr(smc, "log_likelihood", None), getattr(smc, "weights", None)
    if w is None:
        raise ValueError(f"{who}: no weights (an unweighted table goes to model_comparison)")
    if ll is None:
        raise ValueError(f"{who}: the SMCResult has no log_likelihood (run adaptive_smc with pointwise=True)")
    table, w = np.ascontiguousarray(ll, dtype=np.float64), np.ascontiguousarray(w, dtype=np.float64).reshape(-1)
    if table.ndim != 2 or min(table.shape) < 1 or table.shape[1] != w.size:
        raise ValueError(f"{who}: the table must be [n_sel][N] with N = {w.size} weights, not {table.shape}")
    n_bad = int(np.count_nonzero(~((w >= 0.0) & (w <= 1.0))))
    if n_bad > 0:
        raise ValueError(f"{who}: n_bad = {n_bad} of {w.size} weights are NaN, negative, infinite or above 1: the population is not normalised")
    names = list(getattr(smc, "predictive_names", None) or [f"observe#{k}" for k in range(table.shape[0])]) if names is None else [str(a) for a in names]
    if len(names) != table.shape[0]:
        raise ValueError(f"{who}: {len(names)} names for {table.shape[0]} statements")
    with E.stored_population(w, table, device) as (wp, d_table):
        return WeightedComparison.from_parts(names, w.size, [wp.loglik(d_table, table.shape[0])])
