"""Mean-field variational inference under the reference's names (src/inference/vi.rs:104-923), over many samples:

    guide = MeanFieldGuide(); guide.add_latent(addr("mu"), Support.Real, 0.0)
    result = optimize_meanfield_vi_with_config(seed, model_fn, guide, VIConfig(n_samples_per_iter=65536))
    result.guide.params[addr("mu")]            # VariationalParam.Normal(mu=0.96, log_sigma=ln sqrt(0.2))

One Monte Carlo sample is one GPU lane: `n_samples_per_iter` / `num_samples` is the engine's chain count, and every ELBO
estimate of an optimizer iteration (the monitor and the +eps / -eps pair of each guide coordinate) runs in one launch of
k_vi_elbo (fugue_amd/csrc/fg_vi.hip).  The reference threads `&mut R`; the engine's RNG is counter-based, so a `seed`
replaces it.  Host code here is bookkeeping of the guide (a dict of a few parameters); every draw and density of the ELBO
is computed on the device."""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import engine as E
from . import model as M

LOG_SCALE_MIN, LOG_SCALE_MAX, MU_ABS_MAX = -20.0, 20.0, 1.0e6      # vi.rs:104-109
_VTYPE_NAMES = {1: "bool", 2: "u64", 3: "usize", 4: "i64"}


class Support:                        # vi.rs:118-126
    Real, Positive, Unit = "Real", "Positive", "Unit"


class ParamCoord:                     # vi.rs:166-172
    Location, Scale = 0, 1


class GuideError(M.FugueError):       # GuideError::UnsupportedDiscreteLatent, vi.rs:135-144
    def __init__(self, addr: str, value_type: str):
        super().__init__(f"mean-field VI does not support the discrete latent at {addr} (type {value_type}): only continuous latents "
                         "(Normal/LogNormal/Beta factors) can be approximated", M.ErrorCode.TypeMismatch)
        self.addr, self.value_type = addr, value_type


def init_log_sigma(value: float) -> float:        # vi.rs:412-415
    scale = abs(value) if math.isfinite(value) else 1.0
    return math.log(max(0.1 * scale, 0.1))


def _exp(x: float) -> float:
    try:
        return math.exp(x)
    except OverflowError:
        return math.inf


@dataclass
class VariationalParam:
    """One factor of the guide (vi.rs:210-232): `family` 0 Normal {mu, log_sigma}, 1 LogNormal {mu, log_sigma},
    2 Beta {log_alpha, log_beta}; `a` is the location coordinate, `b` the scale coordinate (ParamCoord)."""
    family: int
    a: float
    b: float

    NORMAL, LOGNORMAL, BETA = 0, 1, 2

    @staticmethod
    def Normal(mu: float, log_sigma: float) -> "VariationalParam": return VariationalParam(0, float(mu), float(log_sigma))
    @staticmethod
    def LogNormal(mu: float, log_sigma: float) -> "VariationalParam": return VariationalParam(1, float(mu), float(log_sigma))
    @staticmethod
    def Beta(log_alpha: float, log_beta: float) -> "VariationalParam": return VariationalParam(2, float(log_alpha), float(log_beta))

    # the reference's field names
    @property
    def mu(self): return self.a
    @property
    def log_sigma(self): return self.b
    @property
    def log_alpha(self): return self.a
    @property
    def log_beta(self): return self.b

    @staticmethod
    def for_support(support: str, init_value: float) -> "VariationalParam":       # vi.rs:245-279
        v = float(init_value)
        if support == Support.Real:
            return VariationalParam.Normal(v, init_log_sigma(v))
        if support == Support.Positive:
            safe = v if (math.isfinite(v) and v > 0.0) else 1.0
            return VariationalParam.LogNormal(math.log(safe), math.log(0.5))
        if support == Support.Unit:
            m = min(max(v, 1e-3), 1.0 - 1e-3) if math.isfinite(v) else 0.5
            return VariationalParam.Beta(math.log(2.0 * m), math.log(2.0 * (1.0 - m)))
        raise ValueError(f"unknown support {support!r}")

    def _valid(self) -> bool:
        if self.family == 2:
            al, be = _exp(self.a), _exp(self.b)
            return math.isfinite(al) and math.isfinite(be) and al > 0.0 and be > 0.0
        s = _exp(self.b)
        return math.isfinite(self.a) and math.isfinite(s) and s > 0.0

    def sample(self, seed: int) -> float:
        """One draw of this factor (vi.rs:294-323; NaN when the parameters are invalid).  A host-side convenience for
        inspecting a fitted factor: the ELBO's draws are the device's (fg_vi.hip), from its own counter-based streams."""
        if not self._valid():
            return math.nan
        rng = np.random.default_rng(seed)
        if self.family == 0:
            return float(rng.normal(self.a, _exp(self.b)))
        if self.family == 1:
            return float(rng.lognormal(self.a, _exp(self.b)))
        return float(rng.beta(_exp(self.a), _exp(self.b)))

    def log_prob(self, x: float) -> float:                                        # vi.rs:378-397 (the densities of distribution.rs)
        x = float(x)
        if not self._valid() or not math.isfinite(x):
            return -math.inf
        ln2pi = 1.8378770664093456
        if self.family == 0:
            s = _exp(self.b)
            z = (x - self.a) / s
            return -0.5 * z * z - math.log(s) - 0.5 * ln2pi
        if self.family == 1:
            if x <= 0.0:
                return -math.inf
            s, lx = _exp(self.b), math.log(x)
            z = (lx - self.a) / s
            return -0.5 * z * z - lx - math.log(s) - 0.5 * ln2pi
        al, be = _exp(self.a), _exp(self.b)
        if not 0.0 <= x <= 1.0:
            return -math.inf
        lb = math.lgamma(al) + math.lgamma(be) - math.lgamma(al + be)
        if x == 0.0:
            return -math.inf if al > 1.0 else (math.inf if al < 1.0 else -lb)
        if x == 1.0:
            return -math.inf if be > 1.0 else (math.inf if be < 1.0 else -lb)
        return (al - 1.0) * math.log(x) + (be - 1.0) * math.log(1.0 - x) - lb

    def shifted(self, coord: int, delta: float) -> "VariationalParam":            # vi.rs:418-454
        return VariationalParam(self.family, self.a + delta, self.b) if coord == ParamCoord.Location else VariationalParam(self.family, self.a, self.b + delta)

    def apply_update(self, coord: int, delta: float) -> None:                     # vi.rs:457-483
        if coord == ParamCoord.Location:
            lo, hi = (LOG_SCALE_MIN, LOG_SCALE_MAX) if self.family == 2 else (-MU_ABS_MAX, MU_ABS_MAX)
            self.a = min(max(self.a + delta, lo), hi)
        else:
            self.b = min(max(self.b + delta, LOG_SCALE_MIN), LOG_SCALE_MAX)


@dataclass
class MeanFieldGuide:                 # vi.rs:519-631
    params: Dict[str, VariationalParam] = field(default_factory=dict)

    def add_latent(self, address: str, support: str, init_value: float) -> None:
        self.params[address] = VariationalParam.for_support(support, init_value)

    @staticmethod
    def from_trace(sites: Sequence[str], vtypes: Sequence[int], cells) -> "MeanFieldGuide":
        """A real-line Normal factor for every f64 latent of one trace (vi.rs:577-600): `sites` / `vtypes` as a ChainBatch
        or CompiledProgram names them, `cells` the trace's int64 cells [n_sites].  A discrete latent raises GuideError."""
        cells = np.ascontiguousarray(cells, dtype=np.int64).reshape(-1)
        g = MeanFieldGuide()
        for j, (a, vt) in enumerate(zip(sites, vtypes)):
            if vt != 0:
                raise GuideError(a, _VTYPE_NAMES.get(int(vt), "discrete"))
            v = float(cells[j:j + 1].view(np.float64)[0])
            g.params[a] = VariationalParam.Normal(v, init_log_sigma(v))
        return g

    def sorted_addresses(self) -> List[str]:
        return sorted(self.params, key=lambda s: s.encode("utf-8"))               # Address order (address.rs:150-157)

    def copy(self) -> "MeanFieldGuide":
        return MeanFieldGuide({a: VariationalParam(p.family, p.a, p.b) for a, p in self.params.items()})

    def factor_row(self, cp: E.CompiledProgram):
        """The guide as the C ABI takes it: (family, sorted site index or -1, a, b) per factor in address order."""
        idx = {a: j for j, a in enumerate(cp.site_names)}
        return [(self.params[a].family, idx.get(a, -1), self.params[a].a, self.params[a].b) for a in self.sorted_addresses()]


@dataclass
class VIConfig:                       # vi.rs:729-759, same defaults
    n_iterations: int = 1000
    n_samples_per_iter: int = 16
    base_learning_rate: float = 0.1
    fd_eps: float = 0.01
    convergence_tol: float = 1e-4
    convergence_window: int = 20
    step_decay_exponent: float = 0.6

    def raw(self) -> E.fg_vi_config:
        return E.fg_vi_config(int(self.n_iterations), int(self.convergence_window), float(self.base_learning_rate), float(self.fd_eps),
                              float(self.convergence_tol), float(self.step_decay_exponent))


@dataclass
class VIResult:                       # vi.rs:763-772
    guide: MeanFieldGuide
    elbo_history: np.ndarray
    converged: bool
    iterations: int


def _compile(model_fn) -> E.CompiledProgram:
    return model_fn if isinstance(model_fn, E.CompiledProgram) else E.compile_model(model_fn)


def _call(fn, *args):
    try:
        return fn(*args)
    except E.EngineError as ex:
        if ex.code > 0:               # a reference ErrorCode (TraceAddressNotFound, InvalidParameters ...)
            raise M.FugueError(E.last_error(), ex.code) from None
        raise


def elbo_with_guide(seed: int, model_fn, guide: MeanFieldGuide, num_samples: int, device: int = 0) -> float:      # vi.rs:639-669
    cp = _compile(model_fn)
    eng = E.Engine(cp, num_samples, seed=seed, device=device)
    try:
        return float(_call(eng.vi_elbo_batch, [guide.factor_row(cp)], [0])[0])
    finally:
        eng.close()


def elbo_gradient_fd(seed: int, model_fn, guide: MeanFieldGuide, address: str, coord: int, eps: float, num_samples: int,
                     device: int = 0) -> float:                                                                       # vi.rs:687-725
    if address not in guide.params:
        return 0.0
    cp = _compile(model_fn)
    rows = []
    for delta in (eps, -eps):
        g = guide.copy()
        g.params[address] = guide.params[address].shifted(coord, delta)
        rows.append(g.factor_row(cp))
    eng = E.Engine(cp, num_samples, seed=seed, device=device)
    try:
        e = _call(eng.vi_elbo_batch, rows, [0, 0])            # one stream id: common random numbers
        return float((e[0] - e[1]) / (2.0 * eps))
    finally:
        eng.close()


def optimize_meanfield_vi_with_config(seed: int, model_fn, initial_guide: MeanFieldGuide, config: Optional[VIConfig] = None,
                                      device: int = 0) -> VIResult:                                                   # vi.rs:784-864
    cp = _compile(model_fn)
    cfg = config or VIConfig()
    addrs = initial_guide.sorted_addresses()
    eng = E.Engine(cp, cfg.n_samples_per_iter, seed=seed, device=device)
    try:
        out, hist, converged, iterations = _call(eng.vi_optimize, initial_guide.factor_row(cp), cfg.raw())
    finally:
        eng.close()
    guide = MeanFieldGuide({a: VariationalParam(f, x, y) for a, (f, _, x, y) in zip(addrs, out)})
    return VIResult(guide, hist, converged, iterations)


def optimize_meanfield_vi(seed: int, model_fn, initial_guide: MeanFieldGuide, n_iterations: int, n_samples_per_iter: int,
                          learning_rate: float, device: int = 0) -> MeanFieldGuide:                                  # vi.rs:874-889
    cfg = VIConfig(n_iterations=n_iterations, n_samples_per_iter=n_samples_per_iter, base_learning_rate=learning_rate)
    return optimize_meanfield_vi_with_config(seed, model_fn, initial_guide, cfg, device).guide


def estimate_elbo(seed: int, model_fn, num_samples: int, device: int = 0) -> float:                                  # vi.rs:905-923
    cp = _compile(model_fn)
    eng = E.Engine(cp, num_samples, seed=seed, device=device)
    try:
        return _call(eng.vi_estimate_elbo, 0)
    finally:
        eng.close()
