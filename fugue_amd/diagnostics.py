"""Cross-chain diagnostics over many chains on one or several GPUs.

Mirrors `r_hat_f64` / `classic_r_hat_f64` / `summarize_f64_parameter`
(/root/reference/src/inference/diagnostics.rs:218-391) and `effective_sample_size_multichain`
(/root/reference/src/inference/mcmc_utils.rs:214-339) for draws laid out [n][d][C] in HBM.

This is the ONLY place chains interact, hence the only collective of the engine:
every rank reduces its own draws to per-chain moments (`fg_diag_chain_moments`, [d][6][C_local])
and pooled per-lag autocovariance sums (`fg_diag_autocov_sums`, [d][lags]) on its GPU.  Chains
enter split R-hat, the pooled moments and the ESS only through SUMS over chains, so the ranks
exchange `all_reduce`s of 6 d + 2 d doubles (+ 32 d per chunk of lags) -- over RCCL/xGMI
(`backend="nccl"`), or gloo in the CPU tests; `exchange="gather"` keeps the older `all_gather` of
every chain's moments (a single process's summation order).  The final formulas run in the
library in float64 and follow the reference line by line.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Protocol

import numpy as np


class MomentProvider(Protocol):
    n: int          # draws per chain
    d: int          # coordinates
    def moments(self) -> np.ndarray: ...                       # [d][6][C_local]
    def autocov_sums(self, lag0: int, n_lags: int) -> np.ndarray: ...   # [d][n_lags]


class EngineMoments:
    """MomentProvider backed by the HIP kernels of an `engine.Engine` and a device draw buffer."""

    def __init__(self, engine, d_draws: int, n: int, d: int):
        self.engine, self.d_draws, self.n, self.d = engine, d_draws, int(n), int(d)
        self._d_mom = engine.device_alloc(max(1, d * 6 * engine.C) * 8)
        engine.diag_chain_moments(d_draws, n, d, self._d_mom)
        self._mom: Optional[np.ndarray] = None

    def moments(self) -> np.ndarray:
        if self._mom is None:
            self._mom = self.engine.download(self._d_mom, (self.d, 6, self.engine.C))
        return self._mom

    def autocov_sums(self, lag0: int, n_lags: int) -> np.ndarray:
        return self.engine.diag_autocov_sums(self.d_draws, self.n, self.d, self._d_mom, lag0, n_lags)

    def close(self):
        if self._d_mom:
            self.engine.device_free(self._d_mom)
            self._d_mom = 0


class StreamMoments:
    """MomentProvider over an `engine.DiagStream` that has taken all its draws: the run was handed to the stream one chunk at a
    time and is stored nowhere.  `ChainDiagnostics(StreamMoments(stream), group, device, exchange)` works as with any other
    provider; a lag beyond the stream's K surfaces as `EngineError` (FG_E_LIMIT), never as a figure."""

    def __init__(self, stream):
        self.stream, self.n, self.d = stream, int(stream.n), int(stream.d)
        self._mom: Optional[np.ndarray] = None

    def moments(self) -> np.ndarray:
        if self._mom is None:
            self._mom = self.stream.moments()
        return self._mom

    def autocov_sums(self, lag0: int, n_lags: int) -> np.ndarray:
        return self.stream.autocov_sums(lag0, n_lags)


class HostMoments:
    """MomentProvider over host draws [n][d][C] (numpy): the same statistics the GPU kernels produce, for callers that
    already hold the draws on the host (fugue_amd.validation) and for CPU tests of the combination logic."""

    def __init__(self, draws: np.ndarray):
        self.x = np.asarray(draws, dtype=np.float64)
        self.n, self.d, self.C = self.x.shape

    def moments(self) -> np.ndarray:
        n, half = self.n, self.n // 2
        out = np.zeros((self.d, 6, self.C))
        for k, (a, b) in enumerate(((0, n), (0, half), (half, 2 * half))):
            seg = self.x[a:b]
            mean = seg.sum(axis=0) / max(1, b - a)
            out[:, 2 * k] = mean
            out[:, 2 * k + 1] = ((seg - mean) ** 2).sum(axis=0)
        return out

    def autocov_sums(self, lag0: int, n_lags: int) -> np.ndarray:
        c = self.x - self.x.mean(axis=0, keepdims=True)
        out = np.zeros((self.d, n_lags))
        for k in range(n_lags):
            lag = lag0 + k
            if lag < self.n:
                out[:, k] = ((c[:self.n - lag] * c[lag:]).sum(axis=0) / self.n).sum(axis=1)
        return out


# ---- collectives (identity when not distributed) ------------------------------------------
def _dist(group):
    import torch.distributed as dist
    return dist if (dist.is_available() and dist.is_initialized()) else None


def _all_gather_concat(x: np.ndarray, group=None, device=None) -> np.ndarray:
    """Concatenate `x` ([..., C_local]) of every rank along the last axis, in rank order."""
    dist = _dist(group)
    if dist is None or dist.get_world_size(group) == 1:
        return x
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x))
    if device is not None:
        t = t.to(device)
    outs = [torch.empty_like(t) for _ in range(dist.get_world_size(group))]
    dist.all_gather(outs, t, group=group)          # equal C_local on every rank (chains are sharded evenly)
    return np.concatenate([o.cpu().numpy() for o in outs], axis=-1)


def _all_reduce_sum(x: np.ndarray, group=None, device=None) -> np.ndarray:
    dist = _dist(group)
    if dist is None or dist.get_world_size(group) == 1:
        return x
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x))
    if device is not None:
        t = t.to(device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t.cpu().numpy()


# ---- the combination: C++ (fg_diag_combine, fugue_amd/csrc/fg_diag_host.cpp) ------------------------------------------
class ChainDiagnostics:
    """Diagnostics of `C_total` chains x `n` draws x `d` coordinates, sharded over the ranks of `group`: every rank's
    moments are all-gathered, pooled lag sums all-reduced (torch.distributed: RCCL on GPUs, gloo in the CPU tests), and the
    R-hat / Geyer-ESS formulas run in the library.  (A process that owns an RCCL communicator can skip this class and call
    `Engine.diag_rhat_ess(..., comm)`: the same computation with the collectives inside the library.)"""

    def __init__(self, provider: MomentProvider, group=None, device=None, exchange: str = "reduce"):
        from . import engine as E
        assert exchange in ("reduce", "gather")
        self.p, self.group, self.device, self.exchange = provider, group, device, exchange
        self.n, self.d = provider.n, provider.d
        self.exchange_bytes = 0                          # bytes this rank contributed to collectives
        if exchange == "gather":
            local = provider.moments()
            self._mom = _all_gather_concat(local, group, device)        # [d][6][C_total]
            self.m = self._mom.shape[2]
            if self.m != local.shape[2]:
                self.exchange_bytes += local.nbytes
        else:
            self._local = np.ascontiguousarray(provider.moments())      # [d][6][C_local]
            dist = _dist(group)
            world = dist.get_world_size(group) if dist is not None else 1
            self.m = self._local.shape[2] * world                       # chains are sharded evenly
            self._world = world
            self._sums = None
        self._res = None
        self._E = E

    def _acov(self, lag0: int, n_lags: int) -> np.ndarray:
        a = self.p.autocov_sums(lag0, n_lags)
        if _dist(self.group) is not None and _dist(self.group).get_world_size(self.group) > 1:
            self.exchange_bytes += a.nbytes
        return _all_reduce_sum(a, self.group, self.device)

    def _reduce(self, stage: int, overall):
        """Sums over this rank's chains, all-reduced: the chain sums of fg_diag_combine_reduced."""
        mom = self._local
        if stage == 1:
            a = mom.sum(axis=2)                                          # [d][6]
        else:
            a = np.stack([((mom[:, 0] - overall[:, 0:1]) ** 2).sum(axis=1),
                          ((mom[:, 2] - overall[:, 1:2]) ** 2 + (mom[:, 4] - overall[:, 1:2]) ** 2).sum(axis=1)], axis=1)    # [d][2]
        if self._world > 1:
            self.exchange_bytes += a.nbytes
        out = _all_reduce_sum(np.ascontiguousarray(a), self.group, self.device)
        if stage == 1:
            self._sums = [out, None]
        else:
            self._sums[1] = out
        return out

    def _combine(self):
        if self._res is None:
            if self.exchange == "gather":
                self._res = self._E.diag_combine(self._mom, self.n, self._acov)
            else:
                self._res = self._E.diag_combine_reduced(self.m, self.n, self.d, self._reduce, self._acov)
        return self._res

    def split_rhat(self) -> np.ndarray:                 # r_hat_f64 (diagnostics.rs:218-224, 240-260)
        return self._combine()["r_hat"]

    def classic_rhat(self) -> np.ndarray:               # classic_r_hat_f64 (diagnostics.rs:226-238): whole chains, no split
        m, n = self.m, float(self.n)
        out = np.empty(self.d)
        if self.exchange == "reduce":                   # from the chain sums the combination already exchanged
            self._combine()
            s1, s2 = self._sums
        for i in range(self.d):
            if m < 2:
                out[i] = 1.0
                continue
            if self.exchange == "gather":
                means, ssds = self._mom[i, 0], self._mom[i, 1]
                overall = means.sum() / m
                between, ssd = ((means - overall) ** 2).sum(), (ssds / (n - 1.0)).sum()
            else:
                between, ssd = s2[i, 0], s1[i, 1] / (n - 1.0)
            b = n / (m - 1.0) * between
            w = ssd / m
            out[i] = math.sqrt((((n - 1.0) / n) * w + b / n) / w) if w > 0 else float("nan")
        return out

    def pooled_mean(self) -> np.ndarray:
        return self._combine()["mean"]

    def pooled_std(self) -> np.ndarray:
        return self._combine()["std"]

    def ess(self) -> np.ndarray:                        # effective_sample_size_multichain (mcmc_utils.rs:214-339)
        return self._combine()["ess"]

    def summary(self) -> dict:
        r = self._combine()
        return dict(mean=r["mean"], std=r["std"], r_hat=r["r_hat"], ess=r["ess"])


def quantiles_f64(values: np.ndarray, ps=(0.025, 0.25, 0.5, 0.75, 0.975)) -> dict:
    """summarize_f64_parameter's quantile rule: sorted[round((len-1) * p)] (diagnostics.rs:355-371)."""
    v = np.sort(np.asarray(values, dtype=np.float64).ravel())
    names = {0.025: "2.5%", 0.25: "25%", 0.5: "50%", 0.75: "75%", 0.975: "97.5%"}
    out = {}
    for p in ps:
        idx = int(math.floor((len(v) - 1) * p + 0.5))          # f64::round: half away from zero
        out[names.get(p, f"{100 * p:g}%")] = float(v[idx])
    return out


def geweke_diagnostic(chain: np.ndarray) -> float:
    """geweke_diagnostic (mcmc_utils.rs:354-421): single chain, host-side."""
    x = np.asarray(chain, dtype=np.float64)
    n = len(x)
    if n < 20:
        return float("nan")
    a, b = x[:n // 10], x[n // 2:]
    if len(a) < 2 or len(b) < 2:
        return float("nan")

    def spec_var_mean(seg):
        k = len(seg)
        mean = seg.sum() / k
        s2 = ((seg - mean) ** 2).sum() / (k - 1.0)
        if s2 == 0.0:
            return 0.0
        c = seg - mean
        max_lag = min(k - 1, 1024)
        var0 = (c * c).sum() / k
        if var0 <= 0.0:
            return 0.0
        tau = 1.0
        for lag in range(1, max_lag + 1):
            r = (c[:k - lag] * c[lag:]).sum() / k / var0
            if r <= 0.0:
                break
            tau += 2.0 * r
        return s2 * tau / k

    se = math.sqrt(spec_var_mean(a) + spec_var_mean(b))
    if se == 0.0:
        return 0.0
    return float((a.sum() / len(a) - b.sum() / len(b)) / se)


# ---- the reference's per-parameter entry points over a many-chain result (fugue_amd.inference.ChainBatch) -----------------
@dataclass
class ParameterSummary:                 # diagnostics.rs:306-318
    mean: float
    std: float
    quantiles: dict
    r_hat: float
    ess: float


def _site_draws(chains, address: str) -> np.ndarray:
    """[n_samples][1][n_chains] f64 draws of one site (extract_f64_values, diagnostics.rs:206-216)."""
    return np.ascontiguousarray(chains.get_f64(address))[:, None, :]


def r_hat_f64(chains, address: str) -> float:
    """Split R-hat of one f64 site over the chains of a ChainBatch (r_hat_f64, diagnostics.rs:218-224, 240-260)."""
    return float(ChainDiagnostics(HostMoments(_site_draws(chains, address))).split_rhat()[0])


def classic_r_hat_f64(chains, address: str) -> float:
    """classic_r_hat_f64 (diagnostics.rs:226-238): whole chains, no split."""
    return float(ChainDiagnostics(HostMoments(_site_draws(chains, address))).classic_rhat()[0])


def effective_sample_size_multichain(values: np.ndarray) -> float:
    """effective_sample_size_multichain (mcmc_utils.rs:214-229) of draws [n_samples][n_chains]."""
    x = np.asarray(values, dtype=np.float64)
    return float(ChainDiagnostics(HostMoments(x[:, None, :])).ess()[0])


def summarize_f64_parameter(chains, address: str) -> ParameterSummary:
    """summarize_f64_parameter (diagnostics.rs:320-392): pooled mean / std (n - 1) / quantiles, split R-hat, multi-chain ESS."""
    x = _site_draws(chains, address)
    allv = x.ravel()
    if allv.size == 0:
        return ParameterSummary(float("nan"), float("nan"), {}, float("nan"), 0.0)
    cd = ChainDiagnostics(HostMoments(x))
    mean = float(allv.sum() / allv.size)
    std = float(np.sqrt(((allv - mean) ** 2).sum() / (allv.size - 1))) if allv.size > 1 else float("nan")
    return ParameterSummary(mean, std, quantiles_f64(allv), float(cd.split_rhat()[0]), float(cd.ess()[0]))


def effective_sample_size(particles) -> float:
    """effective_sample_size (smc.rs:230-233) of a weighted population (SMCResult): 1 / sum w_i^2."""
    w = np.asarray(particles.weights, dtype=np.float64)
    return float(1.0 / (w * w).sum()) if w.size else 0.0


# ---- rank-normalised split R-hat, bulk and tail ESS (Vehtari, Gelman, Simpson, Carpenter, Buerkner 2021; fg_diag_rank.hip) ----
RANK_FIGURES = ("rhat_rank", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "ess_lower", "ess_upper", "median", "x_lo", "x_hi")


@dataclass
class RankDiagnostics:
    """The rank-normalised figures of `d` coordinates, one array entry per coordinate: `rhat_rank` = max(`rhat_bulk`, `rhat_folded`),
    `ess_bulk`, `ess_tail` = min(`ess_lower`, `ess_upper`), the `median` and the order statistics `x_lo` / `x_hi` the tail indicators
    cut at; `counts` by name (engine.RANK_COUNT_NAMES).  The ESS is the project's estimator (the reference's Geyer sequence over whole
    chains) applied to the rank-normalised draws, not `posterior`'s split-chain estimate."""
    names: list
    n_draws: int
    rhat_rank: np.ndarray
    rhat_bulk: np.ndarray
    rhat_folded: np.ndarray
    ess_bulk: np.ndarray
    ess_tail: np.ndarray
    ess_lower: np.ndarray
    ess_upper: np.ndarray
    median: np.ndarray
    x_lo: np.ndarray
    x_hi: np.ndarray
    counts: dict

    @property
    def d(self) -> int:
        return len(self.names)

    def of(self, name: str) -> dict:
        """the ten figures of one coordinate"""
        if name not in self.names:
            raise KeyError(name)
        k = self.names.index(name)
        return {f: float(getattr(self, f)[k]) for f in RANK_FIGURES}

    @classmethod
    def from_result(cls, names, n_draws: int, res: dict) -> "RankDiagnostics":
        from . import engine as E
        return cls(names=list(names), n_draws=int(n_draws), counts={k: np.asarray(res[k]) for k in E.RANK_COUNT_NAMES}, **{f: np.asarray(res[f]) for f in RANK_FIGURES})


def _rank_table(x, addresses):
    """a ChainBatch (its f64 sites, or the named ones) or an array [n][d][C] -> the table and the coordinates' names"""
    if hasattr(x, "get_f64") and hasattr(x, "sites"):
        names = [a for a, v in zip(x.sites, x.vtypes) if v == 0] if addresses is None else [str(a) for a in addresses]
        if not names:
            raise ValueError("rank_diagnostics: the ChainBatch has no f64 site")
        return np.ascontiguousarray(np.stack([np.asarray(x.get_f64(a)) for a in names], axis=1), dtype=np.float64), names
    table = np.ascontiguousarray(x, dtype=np.float64)
    if table.ndim != 3 or min(table.shape) < 1:
        raise ValueError(f"rank_diagnostics: the draws must be [n][d][C] with every extent at least 1, not {table.shape}")
    names = [f"x[{j}]" for j in range(table.shape[1])] if addresses is None else [str(a) for a in addresses]
    if len(names) != table.shape[1]:
        raise ValueError(f"rank_diagnostics: {len(names)} names for {table.shape[1]} coordinates")
    return table, names


def rank_diagnostics(x, addresses=None, probs=(0.05, 0.95), device: int = 0) -> RankDiagnostics:
    """Rank-normalised split R-hat, folded R-hat, bulk and tail ESS of stored draws: `x` is a `ChainBatch` (its f64 sites, or the sites
    `addresses`) or an array [n][d][C].  The draws are uploaded and `Engine.diag_rank` runs on them on a throw-away engine; n x C must
    stay below 2^31."""
    from . import engine as E, workloads as W
    table, names = _rank_table(x, addresses)
    n, d, C_ = table.shape
    eng = E.Engine(E.compile_model(W.normal_sites(1)), C_, seed=0, device=device)        # the call wants the engine's chain count only
    buf = None
    try:
        buf = eng.upload(table)
        return RankDiagnostics.from_result(names, n * C_, eng.diag_rank(buf, n, d, probs=probs))
    finally:
        if buf is not None:
            eng.device_free(buf)
        eng.close()


def rank_r_hat_f64(chains, address: str) -> float:
    """`rhat_rank` of one f64 site of a ChainBatch: the larger of the rank-normalised and the folded split R-hat."""
    return float(rank_diagnostics(chains, [address]).rhat_rank[0])


def ess_bulk(chains, address: str) -> float:
    """Bulk ESS of one f64 site of a ChainBatch: the multi-chain ESS of its rank-normalised draws."""
    return float(rank_diagnostics(chains, [address]).ess_bulk[0])


def ess_tail(chains, address: str) -> float:
    """Tail ESS of one f64 site of a ChainBatch: the smaller ESS of the 5 % and 95 % tail indicators."""
    return float(rank_diagnostics(chains, [address]).ess_tail[0])


# ---- MCSE and ESS of the mean, the sd and quantiles, and the mad (`posterior::summarise_draws`; fg_diag_mcse.hip) ----
MCSE_FIGURES = ("mean", "sd", "rhat", "ess_mean", "mcse_mean", "ess_sd", "ess_sq", "mcse_sd", "median", "mad")
MCSE_PROB_FIGURES = ("q", "q7", "ess_quantile", "mcse_quantile", "th_lo", "th_hi")
SUMMARY_COLUMNS = ("mean", "median", "sd", "mad", "q5", "q95", "rhat", "ess_bulk", "ess_tail", "mcse_mean", "mcse_sd", "mcse_q5", "mcse_median", "mcse_q95")


@dataclass
class McseDiagnostics:
    """The Monte Carlo standard errors and effective sample sizes of `d` coordinates: the fixed figures (MCSE_FIGURES) one array entry
    per coordinate, the figures per probability (MCSE_PROB_FIGURES) [d][len(probs)]; `counts` by name (engine.MCSE_COUNT_NAMES and
    engine.MCSE_PROB_COUNT_NAMES).  The ESS is the project's estimator (the reference's Geyer sequence over whole chains) applied to the
    rows `posterior` uses, not Stan's split-chain FFT estimate."""
    names: list
    n_draws: int
    probs: np.ndarray
    mean: np.ndarray
    sd: np.ndarray
    rhat: np.ndarray
    ess_mean: np.ndarray
    mcse_mean: np.ndarray
    ess_sd: np.ndarray
    ess_sq: np.ndarray
    mcse_sd: np.ndarray
    median: np.ndarray
    mad: np.ndarray
    q: np.ndarray
    q7: np.ndarray
    ess_quantile: np.ndarray
    mcse_quantile: np.ndarray
    th_lo: np.ndarray
    th_hi: np.ndarray
    counts: dict

    @property
    def d(self) -> int:
        return len(self.names)

    def _prob(self, p: float) -> int:
        hit = np.flatnonzero(self.probs == float(p))
        if hit.size == 0:
            raise KeyError(p)
        return int(hit[0])

    def of(self, name: str) -> dict:
        """the figures of one coordinate: the fixed ones as floats, those per probability as arrays [len(probs)]"""
        if name not in self.names:
            raise KeyError(name)
        k = self.names.index(name)
        out = {f: float(getattr(self, f)[k]) for f in MCSE_FIGURES}
        out.update({f: np.asarray(getattr(self, f)[k]).copy() for f in MCSE_PROB_FIGURES})
        return out

    def at(self, figure: str, p: float) -> np.ndarray:
        """one figure per probability (MCSE_PROB_FIGURES) at the probability `p` of the call: [d]"""
        if figure not in MCSE_PROB_FIGURES:
            raise KeyError(figure)
        return np.asarray(getattr(self, figure))[:, self._prob(p)]

    @classmethod
    def from_result(cls, names, n_draws: int, res: dict) -> "McseDiagnostics":
        from . import engine as E
        return cls(names=list(names), n_draws=int(n_draws), probs=np.asarray(res["probs"], dtype=np.float64),
                   counts={k: np.asarray(res[k]) for k in E.MCSE_COUNT_NAMES + E.MCSE_PROB_COUNT_NAMES},
                   **{f: np.asarray(res[f]) for f in MCSE_FIGURES + MCSE_PROB_FIGURES})


def _with_uploaded(x, addresses, device, call):
    """upload the table of `x` to a throw-away engine of its chain count and run call(engine, buffer, n, d, names, n C) on it"""
    from . import engine as E, workloads as W
    table, names = _rank_table(x, addresses)
    n, d, C_ = table.shape
    eng = E.Engine(E.compile_model(W.normal_sites(1)), C_, seed=0, device=device)        # the calls want the engine's chain count only
    buf = None
    try:
        buf = eng.upload(table)
        return call(eng, buf, n, d, names, n * C_)
    finally:
        if buf is not None:
            eng.device_free(buf)
        eng.close()


def mcse_diagnostics(x, addresses=None, probs=(0.05, 0.5, 0.95), device: int = 0) -> McseDiagnostics:
    """MCSE and ESS of the mean, the standard deviation and the quantiles `probs` (at most 8), the median and the mad of stored draws:
    `x` is a `ChainBatch` (its f64 sites, or the sites `addresses`) or an array [n][d][C].  The draws are uploaded and `Engine.diag_mcse`
    runs on them on a throw-away engine; n x C must stay below 2^31."""
    return _with_uploaded(x, addresses, device, lambda eng, buf, n, d, names, S: McseDiagnostics.from_result(names, S, eng.diag_mcse(buf, n, d, probs=probs)))


def mcse_mean(chains, address: str) -> float:
    """`posterior::mcse_mean` of one f64 site of a ChainBatch: sd / sqrt(ess_mean)."""
    return float(mcse_diagnostics(chains, [address], probs=(0.5,)).mcse_mean[0])


def mcse_sd(chains, address: str) -> float:
    """`posterior::mcse_sd` of one f64 site of a ChainBatch (Kenney and Keeping's formula on the ESS of the squared centred draws)."""
    return float(mcse_diagnostics(chains, [address], probs=(0.5,)).mcse_sd[0])


def mcse_quantile(chains, address: str, prob: float) -> float:
    """`posterior::mcse_quantile` of one f64 site of a ChainBatch at the probability `prob`."""
    return float(mcse_diagnostics(chains, [address], probs=(float(prob),)).mcse_quantile[0, 0])


def mcse_median(chains, address: str) -> float:
    """`posterior::mcse_median`: `mcse_quantile` at 0.5."""
    return mcse_quantile(chains, address, 0.5)


def ess_mean(chains, address: str) -> float:
    """`posterior::ess_mean` of one f64 site of a ChainBatch: the multi-chain ESS of its raw draws."""
    return float(mcse_diagnostics(chains, [address], probs=(0.5,)).ess_mean[0])


def ess_sd(chains, address: str) -> float:
    """`posterior::ess_sd` of one f64 site of a ChainBatch: the ESS of |x - mean|."""
    return float(mcse_diagnostics(chains, [address], probs=(0.5,)).ess_sd[0])


def ess_quantile(chains, address: str, prob: float) -> float:
    """`posterior::ess_quantile` of one f64 site of a ChainBatch: the ESS of the indicator x <= the order statistic at `prob`."""
    return float(mcse_diagnostics(chains, [address], probs=(float(prob),)).ess_quantile[0, 0])


def ess_median(chains, address: str) -> float:
    """`posterior::ess_median`: `ess_quantile` at 0.5."""
    return ess_quantile(chains, address, 0.5)


def mad(chains, address: str) -> float:
    """R's `mad` of one f64 site of a ChainBatch: 1.4826 times the median of |x - median| over all its draws."""
    return float(mcse_diagnostics(chains, [address], probs=(0.5,)).mad[0])


def summarise_draws(x, addresses=None, device: int = 0) -> dict:
    """`posterior::summarise_draws`' default table of stored draws (`x` as for `mcse_diagnostics`): one row per site, a dict of the columns
    SUMMARY_COLUMNS -- mean, median, sd, mad, q5, q95 (the interpolated type-7 quantiles), rhat (= rhat_rank), ess_bulk, ess_tail, then
    mcse_mean, mcse_sd, mcse_q5, mcse_median, mcse_q95 -- from one `Engine.diag_rank` and one `Engine.diag_mcse` call on one upload."""
    def call(eng, buf, n, d, names, S):
        return names, RankDiagnostics.from_result(names, S, eng.diag_rank(buf, n, d, probs=(0.05, 0.95))), \
            McseDiagnostics.from_result(names, S, eng.diag_mcse(buf, n, d, probs=(0.05, 0.5, 0.95)))
    names, rk, mc = _with_uploaded(x, addresses, device, call)
    out = {}
    for k, name in enumerate(names):
        out[name] = dict(mean=float(mc.mean[k]), median=float(mc.median[k]), sd=float(mc.sd[k]), mad=float(mc.mad[k]), q5=float(mc.q7[k, 0]), q95=float(mc.q7[k, 2]),
                         rhat=float(rk.rhat_rank[k]), ess_bulk=float(rk.ess_bulk[k]), ess_tail=float(rk.ess_tail[k]), mcse_mean=float(mc.mcse_mean[k]),
                         mcse_sd=float(mc.mcse_sd[k]), mcse_q5=float(mc.mcse_quantile[k, 0]), mcse_median=float(mc.mcse_quantile[k, 1]), mcse_q95=float(mc.mcse_quantile[k, 2]))
    return out
