"""The three drivers of the reference's `src/inference` under their own names, over many chains:

    hmc_chain(seed, model_fn, n_samples, n_warmup, config, n_chains)          hmc.rs:566-583
    adaptive_mcmc_chain(seed, model_fn, n_samples, n_warmup, n_chains)        mh.rs:921-944
    adaptive_mcmc_chain_with_overrides(..., overrides)                        mh.rs:946-1014
    adaptive_smc(seed, num_particles, model_fn, config)                       smc.rs:455-581
    hmc_chain_summary / adaptive_mcmc_chain_summary                           the same runs, summarised in chunks (ChainSummary)
    prior_predictive(seed, model_fn, n_chains)                                PriorHandler, then replicated data of the observe sites

Every driver takes `predictive=` / `pointwise=`: replicated data drawn on the device from the observe statements at every draw (the
posterior predictive the reference's workflows sample by hand, tests/inference_integration.rs:717-740) and the per-observation
log-likelihood (`Choice.logp` of the observe sites).

`model_fn` is what the reference passes (`Fn() -> Model<A>`): here a zero-argument callable returning a
`fugue_amd.model.Model`, or an already traced `Program`.  The reference threads `&mut R`; the engine's RNG is
counter-based, so a `seed` replaces it (results do not depend on how chains are sharded).  Results come back as
`ChainBatch` / `SMCResult`, the many-chain form of `Vec<(A, Trace)>` / `Vec<Particle>`: `get_f64(addr)` etc. return
every chain's values of a site."""
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import engine as E
from . import model as M


@dataclass
class HMCConfig:                      # hmc.rs:106-135, same defaults
    n_leapfrog: int = 16
    target_accept: float = 0.8
    init_step_size: Optional[float] = None
    finite_diff_eps: float = 1e-5
    adapt_mass: bool = False
    grad_mode: int = E.GRAD_FD_SPARSE  # engine extension: FD_DENSE is the reference's arithmetic verbatim

    def raw(self):
        return E.hmc_config(self.n_leapfrog, self.target_accept, self.init_step_size, self.finite_diff_eps, self.adapt_mass, self.grad_mode)


class ResamplingMethod:               # smc.rs:236-241
    Multinomial, Systematic, Stratified = E.RESAMPLE_MULTINOMIAL, E.RESAMPLE_SYSTEMATIC, E.RESAMPLE_STRATIFIED


@dataclass
class SMCConfig:                      # smc.rs:316-337
    resampling_method: int = ResamplingMethod.Systematic
    ess_threshold: float = 0.5
    rejuvenation_steps: int = 0


@dataclass
class SiteProposal:                   # mh.rs:145-161
    kind: int = E.PROP_AUTO
    lower: float = 0.0
    upper: float = 0.0

    @staticmethod
    def Gaussian(): return SiteProposal(E.PROP_GAUSSIAN)
    @staticmethod
    def LogSpace(): return SiteProposal(E.PROP_LOGSPACE)
    @staticmethod
    def Reflect(lower, upper): return SiteProposal(E.PROP_REFLECT, float(lower), float(upper))
    @staticmethod
    def PriorResample(): return SiteProposal(E.PROP_PRIOR_RESAMPLE)


@dataclass
class ChainBatch:
    """`n_samples` post-warmup states of `n_chains` chains: the many-chain `Vec<(A, Trace)>`."""
    sites: List[str]
    vtypes: List[int]
    cells: np.ndarray                 # [n_samples][n_sites][n_chains] int64 cells (f64 bits or integers)
    accept_rate: float = 0.0
    mean_step_size: float = float("nan")
    n_divergent: int = 0
    result_names: List[str] = field(default_factory=list)    # the scalars of the model's return value `A` (CompiledProgram.result_names)
    results: Optional[np.ndarray] = None                      # [n_samples][R][n_chains] float64, evaluated on the device; None when R = 0
    predictive_names: List[str] = field(default_factory=list)   # predictive= / pointwise=: the selected observe addresses, program order as selected
    predictive_vtypes: List[int] = field(default_factory=list)
    predictive: Optional[np.ndarray] = None                   # [n_samples][n_sel][n_chains] int64 cells like `cells`: replicated data, draw t from stream (seed, chain, t, 9)
    log_likelihood: Optional[np.ndarray] = None               # pointwise=True: [n_samples][n_sel][n_chains] float64, log p(observed value | draw) per observe statement
    observe_values: Dict[str, Optional[float]] = field(default_factory=dict)   # every observe address -> the observed value the model states (a literal or a data element), None where it reads a site; filled whatever `predictive` is
    gibbs_probs: Optional[Dict[str, np.ndarray]] = None       # hmc_gibbs_chain / gibbs_chain: address of a swept site -> [K], the Rao-Blackwell estimate of P(site = lo + k | data) over the sampling sweeps
    gibbs_stats: Optional[Dict[str, np.ndarray]] = None       # ... and lo, K, n, moved, stuck, nan_cells, neg_inf_cells per swept site (`sites`: their addresses)

    def get_predictive(self, address: str) -> np.ndarray:     # [n_samples][n_chains]: float64 for an f64 observe site, int64 otherwise
        if self.predictive is None or address not in self.predictive_names:
            raise M.FugueError(f"address not found: {address}", M.ErrorCode.TraceAddressNotFound)
        k = self.predictive_names.index(address)
        col = np.ascontiguousarray(self.predictive[:, k, :])
        return col.view(np.float64) if self.predictive_vtypes[k] == 0 else col

    def get_result(self, name: str) -> np.ndarray:            # the `A` half of every (A, Trace): [n_samples][n_chains]
        if name not in self.result_names:
            raise M.FugueError(f"result not found: {name}", M.ErrorCode.TraceAddressNotFound)
        return self.results[:, self.result_names.index(name), :]

    def _row(self, address: str) -> int:
        if address not in self.sites:
            raise M.FugueError(f"address not found: {address}", M.ErrorCode.TraceAddressNotFound)
        return self.sites.index(address)

    def get_f64(self, address: str) -> np.ndarray:            # Trace::get_f64 for every draw and chain: [n_samples][n_chains]
        j = self._row(address)
        if self.vtypes[j] != 0:
            raise M.FugueError(f"site {address} is not f64", M.ErrorCode.TypeMismatch)
        return np.ascontiguousarray(self.cells[:, j, :]).view(np.float64)

    def get_int(self, address: str) -> np.ndarray:            # get_bool / get_u64 / get_usize / get_i64
        j = self._row(address)
        if self.vtypes[j] == 0:
            raise M.FugueError(f"site {address} is f64", M.ErrorCode.TypeMismatch)
        return self.cells[:, j, :]


@dataclass
class SMCResult:
    sites: List[str]
    vtypes: List[int]
    cells: np.ndarray                 # [n_sites][n_particles]
    weights: np.ndarray
    log_weights: np.ndarray
    log_evidence: float
    betas: np.ndarray = field(default_factory=lambda: np.zeros(0))
    result_names: List[str] = field(default_factory=list)    # the scalars of the model's return value `A`
    results: Optional[np.ndarray] = None                      # [R][n_particles] float64: every particle's `A`; None when R = 0
    predictive_names: List[str] = field(default_factory=list)   # predictive= / pointwise=: the selected observe addresses
    predictive_vtypes: List[int] = field(default_factory=list)
    predictive: Optional[np.ndarray] = None                   # [n_sel][n_particles] int64 cells: one replicate per particle
    log_likelihood: Optional[np.ndarray] = None               # pointwise=True: [n_sel][n_particles] float64
    observe_values: Dict[str, Optional[float]] = field(default_factory=dict)   # as ChainBatch.observe_values

    def get_f64(self, address: str) -> np.ndarray:
        return np.ascontiguousarray(self.cells[self.sites.index(address)]).view(np.float64)

    def get_predictive(self, address: str) -> np.ndarray:     # [n_particles]: float64 for an f64 observe site, int64 otherwise
        if self.predictive is None or address not in self.predictive_names:
            raise M.FugueError(f"address not found: {address}", M.ErrorCode.TraceAddressNotFound)
        k = self.predictive_names.index(address)
        col = np.ascontiguousarray(self.predictive[k])
        return col.view(np.float64) if self.predictive_vtypes[k] == 0 else col

    def get_result(self, name: str) -> np.ndarray:
        if name not in self.result_names:
            raise M.FugueError(f"result not found: {name}", M.ErrorCode.TraceAddressNotFound)
        return self.results[self.result_names.index(name)]

    def weighted_mean(self, address: str) -> Optional[float]:
        """ABCSMCResult::weighted_mean's rule (abc.rs:476-489) for an SMC population: sum w x / sum w in particle order, None for an
        address that is no f64 site or a population without weight."""
        if address not in self.sites or self.vtypes[self.sites.index(address)] != M.F64:
            return None
        num = den = 0.0
        for v, w in zip(self.get_f64(address).tolist(), self.weights.tolist()):
            num += w * v
            den += w
        return num / den if den > 0.0 else None


def _compile(model_fn) -> E.CompiledProgram:
    return model_fn if isinstance(model_fn, E.CompiledProgram) else E.compile_model(model_fn)


def _predictive_sel(cp, predictive, pointwise: bool, who: str):
    """The observe statements `predictive=` / `pointwise=` select, as program-order indices: None when neither is asked for, every
    statement for True (or for pointwise=True alone), else the addresses given, in the order given."""
    if predictive is False or predictive is None:
        if not pointwise:
            return None
        predictive = True
    if cp.O == 0:
        raise ValueError(f"{who}: predictive / pointwise asked for, but the model has no observe statement")
    if predictive is True:
        return list(range(cp.O))
    addrs = [predictive] if isinstance(predictive, str) else list(predictive)
    sel = []
    for a in addrs:
        a = str(a)
        if a not in cp.observe_names:
            raise ValueError(f"{who}: predictive names {a!r}, which is no observe address of the model")
        k = cp.observe_names.index(a)
        if k in sel:
            raise ValueError(f"{who}: predictive names {a!r} twice")
        sel.append(k)
    if not sel:
        raise ValueError(f"{who}: predictive is an empty list")
    return sel


def _predict(eng, sel, want_y: bool, pointwise: bool, d_draws, n: int, rows=None, iter0: int = 0):
    """One fg_predict_eval over n draws, downloaded: (cells [n][n_sel][C] or None, log-likelihood [n][n_sel][C] or None)."""
    shape = (n, len(sel), eng.C)
    if n == 0:
        return (np.zeros(shape, dtype=np.int64) if want_y else None), (np.zeros(shape) if pointwise else None)
    yb, lb = eng.predict_eval(d_draws, n, rows=rows, iter0=iter0, sel=sel, out=None if want_y else False, loglik=None if pointwise else False)
    try:
        y = eng.download(yb, shape, dtype=np.int64) if want_y else None
        ll = eng.download(lb, shape) if pointwise else None
    finally:
        for b in (yb, lb):
            if b:
                eng.device_free(b)
    return y, ll


def _predictive_fields(cp, sel, y, ll):
    return dict(predictive_names=[cp.observe_names[k] for k in sel], predictive_vtypes=[cp.observe_vtypes[k] for k in sel], predictive=y, log_likelihood=ll)


def _observe_values(cp) -> Dict[str, Optional[float]]:
    return dict(zip(cp.observe_names, cp.observe_values))


def hmc_chain(seed: int, model_fn, n_samples: int, n_warmup: int, config: Optional[HMCConfig] = None, n_chains: int = 1,
              device: int = 0, predictive=False, pointwise: bool = False) -> ChainBatch:
    """`predictive=True | [addresses]`: `ChainBatch.predictive`, replicated data of the (selected) observe sites at every draw, sampled
    on the device (draw t from the stream (seed, chain, t, 9)); `pointwise=True`: `ChainBatch.log_likelihood`, the log-likelihood of
    the observed value per selected observe statement (all of them when `predictive` is False)."""
    cp = _compile(model_fn)
    cfg = config or HMCConfig()
    sel = _predictive_sel(cp, predictive, pointwise, "hmc_chain")
    want_y = sel is not None and predictive is not False and predictive is not None
    pred_y = pred_ll = None
    eng = E.Engine(cp, n_chains, seed=seed, device=device)
    cells = np.zeros((n_samples, cp.S, n_chains), dtype=np.int64)
    results = np.zeros((n_samples, cp.R, n_chains)) if cp.R > 0 else None
    if cp.d == 0:                                               # no continuous site: every step is a fresh prior draw (hmc.rs:826-845)
        eng.hmc_init(cfg.raw(), n_warmup)
        eng.hmc_step(n_warmup)
        for t in range(n_samples):
            eng.hmc_step(1)
            cells[t] = eng.get_values()
            if cp.R > 0:
                results[t] = eng.result_values()
            if sel is not None:
                y1, l1 = _predict(eng, sel, want_y, pointwise, None, 1, iter0=t)
                if t == 0:
                    pred_y = np.zeros((n_samples, len(sel), n_chains), dtype=np.int64) if want_y else None
                    pred_ll = np.zeros((n_samples, len(sel), n_chains)) if pointwise else None
                if want_y:
                    pred_y[t] = y1[0]
                if pointwise:
                    pred_ll[t] = l1[0]
        if sel is not None and n_samples == 0:
            pred_y, pred_ll = _predict(eng, sel, want_y, pointwise, None, 0)
        st = eng.hmc_stats()
    else:
        buf = eng.device_alloc(max(1, n_samples * cp.d * n_chains) * 8)
        st = eng.hmc_run(cfg.raw(), n_samples, n_warmup, buf)
        draws = eng.download(buf, (n_samples, cp.d, n_chains), dtype=np.int64)
        if cp.R > 0 and n_samples > 0:                          # the `A` of every draw, from the draws where they lie (discrete sites: the engine's values)
            rbuf = eng.result_eval(buf, n_samples)
            results = eng.download(rbuf, (n_samples, cp.R, n_chains))
            eng.device_free(rbuf)
        if sel is not None:                                     # discrete sites: the engine's values, as for the results
            pred_y, pred_ll = _predict(eng, sel, want_y, pointwise, buf, n_samples)
        eng.device_free(buf)
        cells[:] = eng.get_values()[None]                       # HMC moves the f64 sites; discrete sites keep their prior draw (hmc.rs:238-260)
        cells[:, cp.f64_sites, :] = draws
    out = ChainBatch(list(cp.site_names), list(cp.site_vtypes), cells, st.accept_rate, st.mean_step_size, int(st.n_divergent), list(cp.result_names), results,
                     observe_values=_observe_values(cp))
    if sel is not None:
        for k, v in _predictive_fields(cp, sel, pred_y, pred_ll).items():
            setattr(out, k, v)
    eng.close()
    return out


def _override_rows(cp, overrides):
    ov = None
    if overrides:
        ov = [None] * cp.S
        for a, p in overrides:
            if a not in cp.site_names:
                raise M.FugueError(f"address not found: {a}", M.ErrorCode.TraceAddressNotFound)
            ov[cp.site_names.index(a)] = (p.kind, p.lower, p.upper)
    return ov


def adaptive_mcmc_chain_with_overrides(seed: int, model_fn, n_samples: int, n_warmup: int, overrides: Sequence[Tuple[str, SiteProposal]],
                                       n_chains: int = 1, device: int = 0, predictive=False, pointwise: bool = False) -> ChainBatch:
    """`predictive=` / `pointwise=`: as `hmc_chain` (every site is recorded, so every parameter is the draw's own)."""
    cp = _compile(model_fn)
    sel = _predictive_sel(cp, predictive, pointwise, "adaptive_mcmc_chain")
    want_y = sel is not None and predictive is not False and predictive is not None
    ov = _override_rows(cp, overrides)
    eng = E.Engine(cp, n_chains, seed=seed, device=device)
    rec = list(range(cp.S))
    buf = eng.device_alloc(max(1, n_samples * cp.S * n_chains) * 8)
    st = eng.mh_run(n_samples, n_warmup, ov, rec, buf)
    cells = eng.download(buf, (n_samples, cp.S, n_chains), dtype=np.int64)
    results = None
    if cp.R > 0:
        results = np.zeros((n_samples, cp.R, n_chains))
        if n_samples > 0 and cp.S > 0:
            rbuf = eng.result_eval(buf, n_samples, rows=rec)
            results = eng.download(rbuf, (n_samples, cp.R, n_chains))
            eng.device_free(rbuf)
        elif n_samples > 0:
            results[:] = eng.result_values()[None]
    pred = {}
    if sel is not None:
        if cp.S > 0 or n_samples == 0:
            y, ll = _predict(eng, sel, want_y, pointwise, buf, n_samples, rows=rec)
        else:                                                   # a model without sites: every draw is the (empty) current state
            parts = [_predict(eng, sel, want_y, pointwise, None, 1, iter0=t) for t in range(n_samples)]
            y = np.concatenate([q[0] for q in parts]) if want_y else None
            ll = np.concatenate([q[1] for q in parts]) if pointwise else None
        pred = _predictive_fields(cp, sel, y, ll)
    eng.device_free(buf)
    out = ChainBatch(list(cp.site_names), list(cp.site_vtypes), cells, st.accept_rate, result_names=list(cp.result_names), results=results, observe_values=_observe_values(cp), **pred)
    eng.close()
    return out


def adaptive_mcmc_chain(seed: int, model_fn, n_samples: int, n_warmup: int, n_chains: int = 1, device: int = 0, predictive=False,
                        pointwise: bool = False) -> ChainBatch:
    return adaptive_mcmc_chain_with_overrides(seed, model_fn, n_samples, n_warmup, (), n_chains, device, predictive, pointwise)


QUANTILE_PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)      # summarize_f64_parameter's "2.5%", "25%", "50%", "75%", "97.5%"


@dataclass
class ChainSummary:
    """What `summarize_f64_parameter` (diagnostics.rs:320-392) reports for every f64 site of a run whose draws were never stored:
    pooled mean / std, split R-hat, multi-chain ESS, each [n_sites] in the order of `sites`.  With `quantiles=True` the drivers
    also select `quantiles` [n_sites][5] at `quantile_probs` (diagnostics.rs:355-371: "2.5%" ... "97.5%"), exactly the elements a
    sort of all draws would give, by replaying the sampling phase: `passes` counts how often it ran (1 without quantiles)."""
    sites: List[str]
    mean: np.ndarray
    std: np.ndarray
    r_hat: np.ndarray
    ess: np.ndarray
    n_samples: int
    n_chains: int
    accept_rate: float = 0.0
    mean_step_size: float = float("nan")
    n_divergent: int = 0
    quantiles: Optional[np.ndarray] = None
    quantile_probs: Tuple[float, ...] = QUANTILE_PROBS
    passes: int = 1
    results: Optional["ChainSummary"] = None      # results=True: the same figures of the model's return value, `sites` = the result names
    discrete: Optional["DiscreteSummary"] = None  # adaptive_mcmc_chain_summary(discrete=True): the frequency tables of the discrete sites
    predictive: Optional["ChainSummary"] = None   # predictive=: the same figures of the replicated data, `sites` = the selected observe addresses
    comparison: Optional["PointwiseComparison"] = None   # pointwise=: WAIC / IS-LOO per selected observe statement (fugue_amd.comparison)
    checks: Optional["PredictiveCheck"] = None    # checks=: posterior predictive checks of the replicated data (fugue_amd.checks)


@dataclass
class DiscreteSummary:
    """The discrete sites of a run whose draws were never stored (`adaptive_mcmc_chain_summary(discrete=True)`): what a caller of
    the reference tabulates from extract_bool_values / extract_u64_values / extract_usize_values / extract_i64_values
    (diagnostics.rs:76-98).  Per site of `sites` (tags `vtypes`): `counts[k][j]` draws equal to `lo[k] + j`, `below[k]` / `above[k]`
    draws outside the bins, the smallest and largest value seen (`min`, `max`: Python ints), all exact.  `numeric` holds what
    Diagnostics<u64> (diagnostics.rs:153-191) gives the u64 sites through `x as f64`: mean / std / split R-hat / ESS (and the
    quantiles when asked); bool, usize and i64 sites get tables only, as in the reference."""
    sites: List[str]
    vtypes: List[int]
    lo: List[int]
    counts: List[np.ndarray]
    below: np.ndarray
    above: np.ndarray
    min: List[int]
    max: List[int]
    n_samples: int
    n_chains: int
    numeric: Optional[ChainSummary] = None

    def probs(self) -> List[np.ndarray]:
        """counts / (n_samples x n_chains): the posterior frequency of every bin (below / above are not in it)."""
        return [c.astype(np.float64) / float(self.n_samples * self.n_chains) for c in self.counts]


def _summary_args(n_samples: int, chunk: int, max_lag: int):
    if n_samples < 1:
        raise ValueError("n_samples must be at least 1")
    if chunk < 1:
        raise ValueError("chunk must be at least 1")
    if not 1 <= max_lag <= 2048:
        raise ValueError("max_lag must lie in [1, 2048]")


def _default_bins(cp, j: int) -> Tuple[int, int]:
    """(lo, bins) of discrete site j where the program states its support with constant parameters, else (0, 64)."""
    prog = cp.program
    if prog is not None:
        for st in prog.stmts:
            if st.kind != M.SAMPLE or st.addr != cp.site_names[j]:
                continue
            name, par = st.dist.name, [M._cval(p) for p in st.dist.params]
            if name == "Bernoulli":
                return 0, 2
            if name == "Categorical":
                return 0, len(par)
            if name == "DiscreteUniform":
                b = st.dist.i64_bounds or (tuple(int(v) for v in par) if all(v is not None and float(v).is_integer() for v in par) else None)
                if b is not None:
                    return int(b[0]), int(min(b[1] - b[0] + 1, 4096))
            if name == "Binomial" and par[0] is not None:
                return 0, int(min(int(par[0]) + 1, 4096))
    return 0, 64


def _stream_summary(eng, step, sites, d: int, n_samples: int, chunk: int, max_lag: int, quantiles: bool = False, quantile_capacity: int = 65536,
                    after_first_pass=None, result_rows=False, discrete_bins=False, predict=None, pointwise=None, checks=None):
    """step(n, buf) records n draws into buf; one chunk buffer is alive at a time.  A chunk is seen through FEEDS: a view of it as
    doubles [n][rows][C] and the diagnostics stream (with quantiles: and the quantile stream) that take the view.
      - discrete_bins False: buf is [n][d][C] doubles (the f64 sites `sites`) and is its own view.
      - discrete_bins a dict (discrete=True): buf holds EVERY site as cells [n][S][C].  `Engine.cells_f64` gathers the f64 rows into one
        view and the u64 rows (`x as f64`) into a second, each with streams of its own -- the f64 streams are handed exactly the rows
        and values of the other mode, so their figures are those bit for bit -- and a count stream watches every non-f64 row.
      - result_rows (None: the HMC draw layout, or the sorted sites of buf's rows) adds the model's return value: every chunk is turned
        into one reused [chunk][R][C] buffer (`Engine.result_eval`), a third view.
      - predict (dict(sel=observe indices, rows=as result_rows)) adds the replicated data of the selected f64 observe sites: every
        chunk is turned into one reused [chunk][n_sel][C] buffer (`Engine.predict_eval` with iter0 = the chunk's first draw: the stream
        is keyed by the absolute draw index, so a replayed chunk holds the same bits), a further view.
      - pointwise (dict(sel=observe indices, rows=as result_rows)) adds WAIC / IS-LOO of the selected observe statements: every chunk's
        log-likelihood goes into one reused [chunk][n_sel][C] buffer (`Engine.predict_eval`, loglik only) that the log-likelihood stream
        takes (`Engine.loglik_stream`).  First pass only: a replay pass for quantiles does not feed it.
      - checks (dict(sel=observe indices, rows=as result_rows, specs, tuples: `fugue_amd.checks.resolve_checks` over the addresses of sel))
        adds posterior predictive checks: every chunk's replicates of the member statements go into one reused [chunk][n_sel][C] cell
        buffer (`Engine.predict_eval`, cells only, discrete observe sites included) that the check stream takes (`Engine.ppc_stream`).
        First pass only.
    A view is called with (chunk buffer, draws in it, index of its first draw in the sampling phase).
    quantiles: the state after warmup is exported, the first sampling pass feeds every stream, `after_first_pass()` reads the
    sampler's statistics, and while a quantile stream wants another pass the blob is imported into the same engine and the same
    chunks are stepped again for the quantile streams that are still open; the count stream is complete after the first pass."""
    chunk = min(chunk, n_samples)
    cp, C_, R = eng.cp, eng.C, eng.cp.R
    discrete = discrete_bins is not False
    feeds, streams, buffers, cs = [], [], [], None

    def alloc(words):
        buffers.append(eng.device_alloc(words * 8))
        return buffers[-1]

    def feed(names, rows, view):
        f = dict(names=list(names), view=view, stream=eng.diag_stream(n_samples, rows, max_lag), qs=None)
        streams.append(f["stream"])
        if quantiles:
            f["qs"] = eng.diag_qstream(n_samples, rows, QUANTILE_PROBS, capacity=quantile_capacity)
            streams.append(f["qs"])
        feeds.append(f)
        return f

    def figures(f, names=()):
        if f is None:                                      # discrete=True on a model without such sites
            return ChainSummary(list(names), np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0), n_samples, int(C_),
                                quantiles=np.zeros((0, len(QUANTILE_PROBS))) if quantiles else None)
        r = f["stream"].rhat_ess()
        return ChainSummary(f["names"], r["mean"], r["std"], r["r_hat"], r["ess"], n_samples, int(r["chains"]))

    try:
        main, numeric, w_rows, bins = None, None, [], []
        if not discrete:
            main, chunk_rows = feed(sites, d, lambda buf, n, t0: buf), d
        else:
            chunk_rows = S = cp.S

            def gathered(rows):
                vts, dbuf = [cp.site_vtypes[j] for j in rows], alloc(chunk * len(rows) * C_)
                return feed([cp.site_names[j] for j in rows], len(rows), lambda buf, n, t0: eng.cells_f64(buf, n, S, rows, vts, out=dbuf))

            u_rows = [j for j in range(S) if cp.site_vtypes[j] == M.U64]
            w_rows = [j for j in range(S) if cp.site_vtypes[j] != M.F64]
            main = gathered(list(cp.f64_sites)) if cp.f64_sites else None
            numeric = gathered(u_rows) if u_rows else None
            bins = [tuple(int(v) for v in (discrete_bins.get(cp.site_names[j]) or _default_bins(cp, j))) for j in w_rows]
            if w_rows:
                cs = eng.diag_cstream(n_samples, S, w_rows, [cp.site_vtypes[j] for j in w_rows], [b[0] for b in bins], [b[1] for b in bins])
                streams.append(cs)
        res = None
        if result_rows is not False:
            rbuf = alloc(chunk * R * C_)
            res = feed(cp.result_names, R, lambda buf, n, t0: eng.result_eval(buf, n, rows=result_rows, out=rbuf))
        prd = None
        if predict is not None:
            psel, prows = list(predict["sel"]), predict["rows"]
            pbuf = alloc(chunk * len(psel) * C_)
            prd = feed([cp.observe_names[k] for k in psel], len(psel),
                       lambda buf, n, t0: eng.predict_eval(buf, n, rows=prows, iter0=t0, sel=psel, out=pbuf, loglik=False)[0])
        lls = None
        if pointwise is not None:
            lsel, lrows = list(pointwise["sel"]), pointwise["rows"]
            lbuf = alloc(chunk * len(lsel) * C_)
            lls = eng.loglik_stream(n_samples, len(lsel))
            streams.append(lls)
        pcs = None
        if checks is not None:
            csel, crows = list(checks["sel"]), checks["rows"]
            cbuf = alloc(chunk * len(csel) * C_)
            pcs = eng.ppc_stream(n_samples, [cp.observe_vtypes[k] for k in csel], checks["tuples"])
            streams.append(pcs)
        blob = eng.state_export() if quantiles else None
        buf = alloc(chunk * chunk_rows * C_)

        def one_pass(live, counters=(), first=False):
            done = 0
            while done < n_samples:
                n = min(chunk, n_samples - done)
                step(n, buf)
                for f in feeds:
                    mine = [c for c in (f["stream"], f["qs"]) if any(c is x for x in live)]
                    if mine:
                        view = f["view"](buf, n, done)
                        for c in mine:
                            c.update(view, n)
                for c in counters:
                    c.update(buf, n)
                if first and lls is not None:
                    eng.predict_eval(buf, n, rows=lrows, iter0=done, sel=lsel, out=False, loglik=lbuf)
                    lls.update(lbuf, n)
                if first and pcs is not None:
                    eng.predict_eval(buf, n, rows=crows, iter0=done, sel=csel, out=cbuf, loglik=False)
                    pcs.update(cbuf, n)
                done += n

        one_pass([c for f in feeds for c in (f["stream"], f["qs"]) if c is not None], [cs] if cs is not None else [], first=True)
        out = figures(main, sites)
        if res is not None:
            out.results = figures(res)
        if prd is not None:
            out.predictive = figures(prd)
        if lls is not None:
            from .comparison import PointwiseComparison
            out.comparison = PointwiseComparison.from_result([cp.observe_names[k] for k in lsel], n_samples * int(C_), lls.result())
        if pcs is not None:
            from .checks import PredictiveCheck
            out.checks = PredictiveCheck.from_stream(checks["specs"], pcs, n_samples * int(C_), int(C_))
        if discrete:
            tab = cs.result() if cs is not None else dict(counts=[], below=np.zeros(0, dtype=np.uint64), above=np.zeros(0, dtype=np.uint64), min=[], max=[])
            out.discrete = DiscreteSummary([cp.site_names[j] for j in w_rows], [cp.site_vtypes[j] for j in w_rows], [b[0] for b in bins], tab["counts"],
                                           tab["below"], tab["above"], tab["min"], tab["max"], n_samples, int(C_), figures(numeric) if numeric else None)
        if after_first_pass:
            after_first_pass(out)
        if quantiles:
            live = [f["qs"] for f in feeds if not f["qs"].end_pass()]
            while live:                                    # each selector runs until its own quantiles are decided
                eng.state_import(blob)
                one_pass(live)
                live = [q for q in live if not q.end_pass()]
            for f, target in ((main, out), (numeric, out.discrete.numeric if discrete else None), (res, out.results), (prd, out.predictive)):
                if f is not None:
                    target.quantiles, target.passes = f["qs"].result()[0], f["qs"].passes
    finally:
        eng.synchronize()
        for b in buffers:
            eng.device_free(b)
        for st in streams:
            st.close()
    return out


def _want_results(cp, results: bool, recorded=None, who: str = ""):
    if not results:
        return
    if cp.R == 0:
        raise ValueError(f"{who}: results=True, but the model returns nothing the device can evaluate (CompiledProgram.result_skipped)")
    if recorded is not None:
        missing = [cp.site_names[j] for j in cp.result_sites if j not in recorded]
        if missing:
            raise ValueError(f"{who}: results=True needs every site a result reads among the recorded f64 sites; {missing} are not "
                             "(a streamed MH run records its f64 sites only)")


def _summary_pointwise(cp, pointwise, who: str):
    """The selection of `pointwise=False | True | [addresses]`: any observe statement (the log-likelihood is f64 whatever the site's type)."""
    if pointwise is False or pointwise is None:
        return None
    return _predictive_sel(cp, pointwise, True, who)


def _summary_checks(cp, checks, who: str):
    """`checks=False | True | [CheckSpec]` of a summary driver: None, or what `_stream_summary` takes -- the union of the member
    statements in program order (`sel`, the rows of the cell buffer), and the checks over the addresses of those rows.  Any observe
    statement may be a member, discrete ones included; the observed values are the ones the model states."""
    if checks is False or checks is None:
        return None
    from .checks import resolve_checks
    if cp.O == 0:
        raise ValueError(f"{who}: checks asked for, but the model has no observe statement")
    specs, tuples = resolve_checks(checks, cp.observe_names, cp.observe_values, None, who)
    sel = sorted({k for rows, _, _ in tuples for k in rows})
    return dict(sel=sel, specs=specs, tuples=[([sel.index(k) for k in rows], stats, obs) for rows, stats, obs in tuples])


def _summary_predictive(cp, predictive, who: str):
    """The selection of a summary driver: f64 observe sites only (a discrete one would need the count stream)."""
    sel = _predictive_sel(cp, predictive, False, who)
    if sel is not None:
        bad = [cp.observe_names[k] for k in sel if cp.observe_vtypes[k] != M.F64]
        if bad:
            raise ValueError(f"{who}: predictive selects the discrete observe site(s) {bad}; the summaries take f64 observe sites only "
                             "(name the f64 ones, or store the draws with the chain driver)")
    return sel


def hmc_chain_summary(seed: int, model_fn, n_samples: int, n_warmup: int, config: Optional[HMCConfig] = None, n_chains: int = 1,
                      chunk: int = 64, max_lag: int = 64, device: int = 0, quantiles: bool = False, quantile_capacity: int = 65536,
                      results: bool = False, predictive=False, pointwise=False, checks=False) -> ChainSummary:
    """`hmc_chain` for runs longer than memory: the same transitions (`fg_hmc_step` is incremental), `chunk` at a time into one
    draw buffer that a diagnostics stream consumes, and the summary of every f64 site instead of the draws.  `max_lag` bounds how
    far Geyer's sequence may run (an ESS that needs more raises EngineError FG_E_LIMIT).  `quantiles=True` adds the five quantiles
    of summarize_f64_parameter by exact radix select (`Engine.diag_qstream`): the draws are not kept, so every pass beyond the
    first REPEATS THE SAMPLING PHASE from the state exported after warmup -- about three passes for a long run at the default
    `quantile_capacity` (keys collected per quantile once that few candidates are left; device memory 8 x 5 x n_sites x capacity
    bytes), `ChainSummary.passes` reports the count.  Every other figure is the one `quantiles=False` gives.  `results=True` adds
    `ChainSummary.results`: the same figures of the model's return value (the `A` of hmc.rs:566-583), evaluated on the device chunk
    by chunk; the site figures are the ones `results=False` gives.  `predictive=True | [addresses]` adds `ChainSummary.predictive`:
    the same figures of the replicated data of the selected f64 observe sites, sampled on the device chunk by chunk (a replay pass
    samples a chunk again to the same bits); a selected discrete observe site raises ValueError.  `pointwise=True | [addresses]` adds
    `ChainSummary.comparison`, a `PointwiseComparison`: WAIC and importance-sampling LOO per (selected) observe statement, discrete ones
    included, from the log-likelihood of every chunk (`Engine.loglik_stream`; the table is never held; device memory 80 bytes per
    statement and chain, so a model with very many observe statements names the ones to compare).  `checks=True | [CheckSpec]` adds
    `ChainSummary.checks`, a `PredictiveCheck` (fugue_amd.checks): the replicates of every chunk of the first pass are reduced to the
    test statistics of the checks on the device and compared with the observed data (`Engine.ppc_stream`; True is one check "all" over
    every observe statement with all five statistics; discrete observe sites are fine; device memory 48 bytes per statistic, check and
    chain).  Nothing else changes."""
    _summary_args(n_samples, chunk, max_lag)
    cp = _compile(model_fn)
    if cp.d == 0:
        raise ValueError("hmc_chain_summary: the model has no f64 site to summarise")
    _want_results(cp, results, who="hmc_chain_summary")
    psel = _summary_predictive(cp, predictive, "hmc_chain_summary")
    lsel = _summary_pointwise(cp, pointwise, "hmc_chain_summary")
    csel = _summary_checks(cp, checks, "hmc_chain_summary")
    cfg = config or HMCConfig()
    eng = E.Engine(cp, n_chains, seed=seed, device=device)
    try:
        eng.hmc_init(cfg.raw(), n_warmup)
        eng.hmc_step(n_warmup)
        def stats(out):
            st = eng.hmc_stats()
            out.accept_rate, out.mean_step_size, out.n_divergent = st.accept_rate, st.mean_step_size, int(st.n_divergent)

        out = _stream_summary(eng, eng.hmc_step, [cp.site_names[j] for j in cp.f64_sites], cp.d, n_samples, chunk, max_lag, quantiles, quantile_capacity, stats,
                              result_rows=None if results else False, predict=None if psel is None else dict(sel=psel, rows=None),
                              pointwise=None if lsel is None else dict(sel=lsel, rows=None), checks=None if csel is None else dict(csel, rows=None))
    finally:
        eng.close()
    return out


def adaptive_mcmc_chain_summary(seed: int, model_fn, n_samples: int, n_warmup: int, n_chains: int = 1,
                                overrides: Sequence[Tuple[str, SiteProposal]] = (), chunk: int = 64, max_lag: int = 64,
                                device: int = 0, quantiles: bool = False, quantile_capacity: int = 65536, results: bool = False,
                                discrete: bool = False, discrete_bins: Optional[Dict[str, Tuple[int, int]]] = None, predictive=False,
                                pointwise=False, checks=False) -> ChainSummary:
    """`adaptive_mcmc_chain_with_overrides` for runs longer than memory: the same steps (`fg_mh_step` is incremental), recording
    only the f64 sites, `chunk` at a time into one draw buffer that a diagnostics stream consumes.  `quantiles=True` adds the five
    quantiles as `hmc_chain_summary` does: every pass beyond the first REPEATS THE SAMPLING PHASE from the state exported after
    warmup (`ChainSummary.passes`).  `results=True` adds `ChainSummary.results` as `hmc_chain_summary` does; every site a result reads
    must be an f64 site (the recorded ones: a discrete site moves under MH and is not in the chunk).

    `discrete=True` records every site and adds `ChainSummary.discrete`, a `DiscreteSummary`: exact frequency tables of every
    discrete site (`Engine.diag_cstream`), and for the u64 sites the figures of Diagnostics<u64> (`DiscreteSummary.numeric`).  The
    bins of a site are `discrete_bins[address] = (lo, bins)`, else its support where the program states it with constant
    parameters (Bernoulli (0, 2), Categorical (0, K), DiscreteUniform (lo, hi - lo + 1), Binomial (0, n + 1), at most 4096 bins),
    else (0, 64); draws outside are counted in `below` / `above`.  A result may then read any site, a model needs no f64 site, and
    the f64 figures are those `discrete=False` gives.

    `predictive=True | [addresses]` adds `ChainSummary.predictive` as `hmc_chain_summary` does.  The parameters of an observe statement
    must come from recorded sites: a model with a discrete site needs `discrete=True` (which records every site).

    `pointwise=True | [addresses]` adds `ChainSummary.comparison` as `hmc_chain_summary` does, under the same condition on recorded sites.
    `checks=True | [CheckSpec]` adds `ChainSummary.checks` as `hmc_chain_summary` does, under the same condition; discrete OBSERVE sites
    need nothing."""
    _summary_args(n_samples, chunk, max_lag)
    cp = _compile(model_fn)
    who = "adaptive_mcmc_chain_summary"
    psel = _summary_predictive(cp, predictive, who)
    lsel = _summary_pointwise(cp, pointwise, who)
    csel = _summary_checks(cp, checks, who)
    if csel is not None and psel is None and lsel is None and not discrete and cp.d != cp.S:
        raise ValueError(f"{who}: checks on a model with discrete sites needs discrete=True (a streamed MH run records its f64 sites only, and the discrete ones move)")
    if (psel is not None or lsel is not None) and not discrete and cp.d != cp.S:
        raise ValueError(f"{who}: predictive / pointwise on a model with discrete sites needs discrete=True (a streamed MH run records its f64 sites only, "
                         "and the discrete ones move)")
    if discrete_bins is not None and not discrete:
        raise ValueError(f"{who}: discrete_bins is given, but discrete=True is not")
    if discrete:
        if cp.S == 0:
            raise ValueError(f"{who}: the model has no site to summarise")
        for a, b in (discrete_bins or {}).items():
            if a not in cp.site_names or cp.site_vtypes[cp.site_names.index(a)] == M.F64:
                raise ValueError(f"{who}: discrete_bins names {a!r}, which is no discrete site")
            if len(b) != 2 or not 1 <= int(b[1]) <= 4096:
                raise ValueError(f"{who}: discrete_bins[{a!r}] must be (lo, bins) with bins in [1, 4096]")
        rec = list(range(cp.S))
    else:
        rec = list(cp.f64_sites)
        if not rec:
            raise ValueError(f"{who}: the model has no f64 site to summarise")
    _want_results(cp, results, None if discrete else rec, who)
    ov = _override_rows(cp, overrides)
    eng = E.Engine(cp, n_chains, seed=seed, device=device)
    try:
        eng.mh_init(n_warmup, ov)
        eng.mh_step(n_warmup)
        def stats(out):
            out.accept_rate = eng.mh_stats().accept_rate

        out = _stream_summary(eng, lambda n, buf: eng.mh_step(n, rec, buf), [cp.site_names[j] for j in cp.f64_sites], cp.d, n_samples, chunk, max_lag,
                              quantiles, quantile_capacity, stats, result_rows=rec if results else False,
                              discrete_bins=dict(discrete_bins or {}) if discrete else False, predict=None if psel is None else dict(sel=psel, rows=rec),
                              pointwise=None if lsel is None else dict(sel=lsel, rows=rec), checks=None if csel is None else dict(csel, rows=rec))
    finally:
        eng.close()
    return out


def adaptive_smc(seed: int, num_particles: int, model_fn, config: Optional[SMCConfig] = None, device: int = 0, predictive=False,
                 pointwise: bool = False) -> SMCResult:
    """`predictive=` / `pointwise=`: one replicate of the (selected) observe sites per final particle, `SMCResult.predictive`
    [n_sel][N] (stream (seed, particle, 0, 9)), and the particles' pointwise log-likelihood."""
    cp = _compile(model_fn)
    cfg = config or SMCConfig()
    sel = _predictive_sel(cp, predictive, pointwise, "adaptive_smc")
    want_y = sel is not None and predictive is not False and predictive is not None
    if num_particles == 0:                                         # smc.rs:462-467
        pred = {} if sel is None else _predictive_fields(cp, sel, np.zeros((len(sel), 0), dtype=np.int64) if want_y else None, np.zeros((len(sel), 0)) if pointwise else None)
        return SMCResult(list(cp.site_names), list(cp.site_vtypes), np.zeros((cp.S, 0), dtype=np.int64), np.zeros(0), np.zeros(0), 0.0,   # empty population: log_evidence 0.0
                         result_names=list(cp.result_names), results=np.zeros((cp.R, 0)) if cp.R > 0 else None, observe_values=_observe_values(cp), **pred)
    eng = E.Engine(cp, num_particles, seed=seed, device=device)
    r = eng.smc_run(cfg.resampling_method, cfg.ess_threshold, cfg.rejuvenation_steps)
    out = SMCResult(list(cp.site_names), list(cp.site_vtypes), r["values"], r["weights"], r["log_w"], r["log_evidence"], r["betas"],
                    list(cp.result_names), eng.result_values() if cp.R > 0 else None, observe_values=_observe_values(cp))
    if sel is not None:
        y, ll = _predict(eng, sel, want_y, pointwise, None, 1)
        for k, v in _predictive_fields(cp, sel, None if y is None else y[0], None if ll is None else ll[0]).items():
            setattr(out, k, v)
    eng.close()
    return out


@dataclass
class WeightedTables:
    """Exact weighted frequency tables of the discrete sites of a population (`Engine.wpop(...).counts`): units[k][j] are the units
    (rint(w 2^52) each) of the particles whose site k equals lo[k] + j; `below` / `above` the units outside the bins; min / max over
    the particles of non-zero units (None without one)."""
    names: List[str]
    vtypes: List[int]
    lo: List[int]
    bins: List[int]
    units: List[np.ndarray]
    below: np.ndarray
    above: np.ndarray
    min: List[Optional[int]]
    max: List[Optional[int]]
    T: int

    def probs(self) -> List[np.ndarray]:
        return [u.astype(np.float64) / float(self.T) if self.T else np.full(u.shape, np.nan) for u in self.units]


@dataclass
class PopulationSummary:
    """`adaptive_smc_summary`: the final population of `adaptive_smc` summarised where it lies.  One row per name: the f64 sites,
    then (results=True) the model's return values, then (predictive=) the replicates of the selected f64 observe sites.  `quantiles`
    [rows][len(probs)] are inverse weighted CDFs on the units of the weights -- exact, and NOT summarize_f64_parameter's
    sorted[round((len - 1) p)]; mean / std / mcse use the weights as doubles (mcse = sqrt(sum w^2 (x - mean)^2) / sum w)."""
    names: List[str]
    n_particles: int
    probs: np.ndarray
    mean: np.ndarray
    std: np.ndarray
    mcse: np.ndarray
    quantiles: np.ndarray
    n_used: np.ndarray                 # particles behind the moments of a row: a good weight above zero and a finite value
    log_evidence: float
    betas: np.ndarray
    ess: float                         # effective_sample_size of the final weights (smc.rs:230-233)
    T: int                             # the units of the population (2^52 up to rounding)
    n_zero: int                        # particles whose weight rounds to zero units: no part in quantiles and tables
    sites: List[str] = field(default_factory=list)
    result_names: List[str] = field(default_factory=list)
    predictive_names: List[str] = field(default_factory=list)
    tables: Optional[WeightedTables] = None
    passes: Optional[np.ndarray] = None   # [rows][len(probs)]: the passes over its row each quantile took
    comparison: Optional["WeightedComparison"] = None          # pointwise=: weighted WAIC / IS-LOO per selected observe statement (fugue_amd.comparison)
    checks: Optional["WeightedPredictiveCheck"] = None         # checks=: weighted predictive checks of one replicate per particle (fugue_amd.checks)

    def row(self, name: str) -> int:
        if name not in self.names:
            raise M.FugueError(f"address not found: {name}", M.ErrorCode.TraceAddressNotFound)
        return self.names.index(name)


def _empty_population_summary(names, probs, sites, result_names, predictive_names) -> PopulationSummary:
    z = np.zeros(len(names))
    return PopulationSummary(list(names), 0, probs, z + np.nan, z + np.nan, z + np.nan, np.full((len(names), probs.size), np.nan), np.zeros(len(names), dtype=np.int64),
                             0.0, np.zeros(0), 0.0, 0, 0, list(sites), list(result_names), list(predictive_names))


def population_summary(eng, log_evidence: float = 0.0, betas=None, probs=(0.025, 0.25, 0.5, 0.75, 0.975), results: bool = False, predictive=False,
                       discrete: bool = False, digit_bits: int = 12, capacity: int = 65536, seed_iter: int = 0, pointwise=False, checks=False,
                       stage_words: int = 1 << 24) -> PopulationSummary:
    """The summary of the particle population an engine holds (after `smc_run(download=False)` or the standalone SMC calls), on the
    device: nothing of size N comes to the host, and neither the engine's values nor its weights change.  See `adaptive_smc_summary`.
    `stage_words`: the cells of the reused buffer `pointwise=` / `checks=` draw into, so statements are taken `stage_words // N` at a
    time, at least one (the default is the moments' staging budget; the figures do not depend on it, the number of `fg_predict_eval`
    calls does)."""
    cp, N = eng.cp, eng.C
    who = "adaptive_smc_summary"
    pr = np.ascontiguousarray(probs, dtype=np.float64).reshape(-1)
    _want_results(cp, results, who=who)
    psel = _summary_predictive(cp, predictive, who)
    lsel = _summary_pointwise(cp, pointwise, who)
    csel = _summary_checks(cp, checks, who)
    sites = [cp.site_names[j] for j in cp.f64_sites]
    rnames = list(cp.result_names) if results else []
    pnames = [cp.observe_names[k] for k in psel] if psel is not None else []
    names = sites + rnames + pnames
    disc = [j for j in range(cp.S) if cp.site_vtypes[j] != M.F64] if discrete else []
    if not names and not disc and lsel is None and csel is None:
        raise ValueError(f"{who}: nothing to summarise: the model has no f64 site, and neither results, predictive nor discrete adds a row")
    values = E.lib().fg_engine_values_device(eng.h)
    wp, buffers = None, []
    try:
        wp = eng.wpop()
        u = wp.units()
        if u["n_bad"] > 0:
            raise ValueError(f"{who}: {u['n_bad']} of {N} weights are NaN, negative, infinite or above 1: the population is not normalised")
        out = PopulationSummary(names, N, pr, np.zeros(0), np.zeros(0), np.zeros(0), np.zeros((0, pr.size)), np.zeros(0, dtype=np.int64), float(log_evidence),
                                np.zeros(0) if betas is None else np.asarray(betas, dtype=np.float64), eng.smc_ess(), u["T"], u["n_zero"], sites, rnames, pnames)
        if names:
            D = len(names)
            x = eng.device_alloc(D * N * 8)
            buffers.append(x)
            if sites:
                eng.cells_f64(values, 1, cp.S, cp.f64_sites, [M.F64] * len(sites), out=x)
            if rnames:
                eng.result_eval(None, 1, out=x + len(sites) * N * 8)
            if pnames:
                eng.predict_eval(None, 1, iter0=seed_iter, sel=psel, out=x + (len(sites) + len(rnames)) * N * 8, loglik=False)
            m = wp.moments(x, D)
            out.mean, out.std, out.mcse, out.n_used = m["mean"], m["std"], m["mcse"], m["n_used"]
            out.quantiles, out.passes = wp.quantiles(x, D, pr, digit_bits, capacity)
        if disc:
            cells = eng.cells_f64(values, 1, cp.S, disc, [M.F64] * len(disc))      # the F64 tag copies a cell's bits: a gather of the rows
            buffers.append(cells)
            vt = [cp.site_vtypes[j] for j in disc]
            lb = [_default_bins(cp, j) for j in disc]
            t = wp.counts(cells, vt, [a for a, _ in lb], [b for _, b in lb])
            out.tables = WeightedTables([cp.site_names[j] for j in disc], vt, [a for a, _ in lb], [b for _, b in lb], t["units"], t["below"], t["above"], t["min"], t["max"], t["T"])
        if lsel is not None:                             # statements in slices of at most stage_words / N into one reused buffer
            from .comparison import WeightedComparison
            per = max(1, min(len(lsel), int(stage_words) // N))
            buf = eng.device_alloc(per * N * 8)
            buffers.append(buf)
            parts = []
            for a in range(0, len(lsel), per):
                eng.predict_eval(None, 1, iter0=seed_iter, sel=lsel[a:a + per], out=False, loglik=buf)
                parts.append(wp.loglik(buf, len(lsel[a:a + per])))
            out.comparison = WeightedComparison.from_parts([cp.observe_names[k] for k in lsel], N, parts)
        if csel is not None:                             # checks in groups whose member statements fit the same budget
            from .checks import WeightedPredictiveCheck, check_groups
            groups = check_groups(csel["tuples"], N, int(stage_words))
            buf = eng.device_alloc(max(len(g[1]) for g in groups) * N * 8)
            buffers.append(buf)
            parts = []
            for q0, rows, tuples in groups:
                gsel = [csel["sel"][k] for k in rows]
                eng.predict_eval(None, 1, iter0=seed_iter, sel=gsel, out=buf, loglik=False)
                parts.append((q0, wp.checks(buf, [cp.observe_vtypes[k] for k in gsel], tuples)))
            out.checks = WeightedPredictiveCheck.from_parts(csel["specs"], parts, N, u["T"])
        return out
    finally:
        if wp is not None:
            wp.close()
        for b in buffers:
            eng.device_free(b)


def adaptive_smc_summary(seed: int, num_particles: int, model_fn, config: Optional[SMCConfig] = None, device: int = 0,
                         probs=(0.025, 0.25, 0.5, 0.75, 0.975), results: bool = False, predictive=False, discrete: bool = False, pointwise=False,
                         checks=False) -> PopulationSummary:
    """`adaptive_smc` without the download: the same run (`smc_run(download=False)` leaves particles and weights in HBM), then the
    weighted summary of the final population on the device (`Engine.wpop`): per f64 site the weighted mean, std, Monte Carlo error
    and exact weighted quantiles at `probs`; `results=True` adds the rows of the model's return value at the final particles,
    `predictive=True | [addresses]` one replicate of the selected f64 observe sites per particle (stream (seed, particle, 0, 9), as
    `adaptive_smc` draws them), `discrete=True` the exact weighted frequency tables of the discrete sites (`PopulationSummary.tables`,
    bins as `adaptive_mcmc_chain_summary` chooses them).  `pointwise=True | [addresses]` adds `PopulationSummary.comparison`, weighted
    WAIC / IS-LOO per selected observe statement, and `checks=True | [CheckSpec]` adds `PopulationSummary.checks`, weighted predictive
    checks of one replicate per particle (discrete observe sites included): log-likelihood and replicates are the bits
    `adaptive_smc(predictive=True, pointwise=True)` stores, drawn slice by slice into one reused device buffer and reduced where they
    lie (`WeightedPopulation.loglik` / `.checks`).  A population whose weights are not all in [0, 1] raises ValueError.
    `num_particles == 0` returns an empty summary with log_evidence 0.0 (smc.rs:462-467)."""
    cp = _compile(model_fn)
    cfg = config or SMCConfig()
    if num_particles == 0:
        _want_results(cp, results, who="adaptive_smc_summary")
        psel = _summary_predictive(cp, predictive, "adaptive_smc_summary")
        _summary_pointwise(cp, pointwise, "adaptive_smc_summary")
        _summary_checks(cp, checks, "adaptive_smc_summary")
        sites = [cp.site_names[j] for j in cp.f64_sites]
        rnames = list(cp.result_names) if results else []
        pnames = [cp.observe_names[k] for k in psel] if psel is not None else []
        return _empty_population_summary(sites + rnames + pnames, np.ascontiguousarray(probs, dtype=np.float64).reshape(-1), sites, rnames, pnames)
    eng = E.Engine(cp, num_particles, seed=seed, device=device)
    try:
        r = eng.smc_run(cfg.resampling_method, cfg.ess_threshold, cfg.rejuvenation_steps, download=False)
        return population_summary(eng, r["log_evidence"], r["betas"], probs, results, predictive, discrete, pointwise=pointwise, checks=checks)
    finally:
        eng.close()


@dataclass
class PriorPredictive:
    """`prior_predictive`: n_chains runs of PriorHandler (interpreters.rs:88-104) and, for each, one replicate of the observe sites
    drawn at those values -- a simulator's output."""
    sites: List[str]
    vtypes: List[int]
    cells: np.ndarray                 # [n_sites][n_chains]: the prior draws
    predictive_names: List[str]
    predictive_vtypes: List[int]
    predictive: np.ndarray            # [n_sel][n_chains] int64 cells
    log_likelihood: Optional[np.ndarray] = None   # pointwise=True: [n_sel][n_chains]
    observe_values: Dict[str, Optional[float]] = field(default_factory=dict)   # as ChainBatch.observe_values

    def get_f64(self, address: str) -> np.ndarray:
        return np.ascontiguousarray(self.cells[self.sites.index(address)]).view(np.float64)

    def get_predictive(self, address: str) -> np.ndarray:
        if address not in self.predictive_names:
            raise M.FugueError(f"address not found: {address}", M.ErrorCode.TraceAddressNotFound)
        k = self.predictive_names.index(address)
        col = np.ascontiguousarray(self.predictive[k])
        return col.view(np.float64) if self.predictive_vtypes[k] == 0 else col


def prior_predictive(seed: int, model_fn, n_chains: int, iteration: int = 0, predictive=True, pointwise: bool = False, device: int = 0) -> PriorPredictive:
    """The prior predictive: `prior_init(iteration)` draws every site from its prior, then the observe sites are drawn at those values
    from the stream (seed, chain, iteration, 9)."""
    cp = _compile(model_fn)
    sel = _predictive_sel(cp, True if predictive is False or predictive is None else predictive, pointwise, "prior_predictive")
    eng = E.Engine(cp, n_chains, seed=seed, device=device)
    try:
        eng.prior_init(iteration)
        y, ll = _predict(eng, sel, True, pointwise, None, 1, iter0=iteration)
        f = _predictive_fields(cp, sel, y[0], None if ll is None else ll[0])
        return PriorPredictive(list(cp.site_names), list(cp.site_vtypes), eng.get_values(), f["predictive_names"], f["predictive_vtypes"], f["predictive"], f["log_likelihood"],
                               _observe_values(cp))
    finally:
        eng.close()
