"""Log-joint surfaces on the device: `log_joint_grid` (crates/fugue-wasm/src/grid.rs) and what people do with its result.

    axis = np.linspace(-2.0, 2.0, 21)
    out = log_joint_grid(source, "a", "b", axis, axis, seed=1)             # the reference's call: flat, row-major out[j * n_a + i]

    s = log_joint_surface(model, "a", axis, "b", axis, seed=1)             # the same surface with its summary
    s.log_norm, s.peak, s.log_marginal_a, s.mean(), s.log_evidence(0.2 * 0.2)

    eng.hmc_run(...)                                                       # the bases: the current state of every chain
    s = log_joint_surface(None, "a", axis, "b", axis, engine=eng, n_bases=eng.C, keep=False)
    s.log_mixture                                                          # Rao-Blackwell estimate of the marginal posterior of (a, b)

Every cell is the total log weight of a base trace with the two sites pinned, scored by the run `Engine.log_joint` does (bit for
bit); a base is an engine chain and is read only.  One wave scores 64 consecutive cells of one base (fugue_amd/csrc/fg_grid.hip,
DESIGN.md 3.20); the normaliser, the marginals, the mode and the non-finite counts of every base and the mixture over the bases are
reduced on the device in orders that depend on the grid's shape alone.  The base of `log_joint_grid` is chain 0 of
`Engine(cp, 1, seed).prior_init()`: the reference's law, not its StdRng draw."""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import numpy as np

from . import engine as E
from . import model as M


def _site_error(site_a, site_b) -> str:
    return f"sites `{site_a}`/`{site_b}` must be f64 sample sites of the model"       # grid.rs:43-45


def _compile(model, data=None) -> E.CompiledProgram:
    if isinstance(model, E.CompiledProgram):
        return model
    if isinstance(model, str):
        return E.CompiledProgram.from_dsl(model, data)
    return E.compile_model(model)


def _site_index(cp: E.CompiledProgram, site) -> int:
    """the sorted site index of an address (or of an index), -1 unless it is an f64 sample site"""
    if isinstance(site, (int, np.integer)) and not isinstance(site, bool):
        j = int(site)
    else:
        name = str(site)
        j = cp.site_names.index(name) if name in cp.site_names else -1
    return j if 0 <= j < cp.S and cp.site_vtypes[j] == M.F64 else -1


def _sites(cp, site_a, site_b):
    ja = _site_index(cp, site_a)
    jb = None if site_b is None else _site_index(cp, site_b)
    if ja < 0 or (jb is not None and jb < 0):
        raise ValueError(_site_error(site_a, site_a if site_b is None else site_b))
    return ja, jb


def _axis(v, name) -> np.ndarray:
    a = np.ascontiguousarray(v, dtype=np.float64)
    if a.ndim != 1:
        raise ValueError(f"{name} must be one-dimensional")
    return a


class LogJointGrid(E._Stream):
    """`fg_grid` (fg_grid.hip): the surfaces of a bank of bases over the axes of one or two f64 sites.  `eval` scores engine chains
    [chain0, chain0 + n_bases) and reduces them; the read-outs cover every base that has arrived, in arrival order.  Close it before
    its engine."""

    _free = "fg_grid_free"

    def __init__(self, engine: "E.Engine", site_a, a_values, site_b=None, b_values=None, base_chunk: int = 0):
        self._integers(base_chunk=base_chunk)
        cp = engine.cp
        ja, jb = _sites(cp, site_a, site_b)
        self.a_values = _axis(a_values, "a_values")
        self.b_values = None if jb is None else _axis(b_values, "b_values")
        self.engine, self.site_a, self.site_b = engine, ja, jb
        self.n_a, self.n_b = self.a_values.size, 1 if jb is None else self.b_values.size
        self.h = None
        out = C.c_void_p()
        E._check(E.lib().fg_grid_new(engine.h, ja, -1 if jb is None else jb, E._dp(self.a_values), self.n_a,
                                     None if jb is None else E._dp(self.b_values), self.n_b, int(base_chunk), C.byref(out)))
        self.h = out.value

    @property
    def count(self) -> int:
        return int(E.lib().fg_grid_count(self._handle()))

    def eval(self, chain0: int = 0, n_bases: int = 1, keep: bool = True, want_acc: bool = False, d_out: Optional[int] = None, d_acc: Optional[int] = None):
        """Scores and reduces bases [chain0, chain0 + n_bases).  keep: the surfaces come back as [n_bases][n_b][n_a] (through a device
        table of that size); want_acc: (surfaces, acc [3][n_bases][n_b][n_a]).  d_out / d_acc: device tables of the caller's own, in
        which case nothing is downloaded and None is returned."""
        self._integers(chain0=chain0, n_bases=n_bases)
        eng, shape = self.engine, (int(n_bases), self.n_b, self.n_a)
        own = d_out is None and d_acc is None
        cells = max(1, int(np.prod(shape))) if n_bases > 0 else 1
        mine = []
        try:
            if own and keep:
                d_out = eng.device_alloc(cells * 8); mine.append(d_out)
            if own and want_acc:
                d_acc = eng.device_alloc(3 * cells * 8); mine.append(d_acc)
            E._check(E.lib().fg_grid_eval(self._handle(), int(chain0), int(n_bases), d_out, d_acc))
            if not own:
                return None
            lj = eng.download(d_out, shape) if keep else None
            return (lj, eng.download(d_acc, (3,) + shape)) if want_acc else lj
        finally:
            for p in mine:
                eng.device_free(p)

    def summary(self) -> dict:
        """log_norm [n], max [n], argmax [n] (flat index, -1 when no cell exceeds -inf), counts [n][3] = NaN, -inf, +inf cells"""
        n = self.count
        log_norm, mx = np.empty(n), np.empty(n)
        arg, cnt = np.empty(n, dtype=np.int64), np.empty((n, 3), dtype=np.int64)
        i64p = C.POINTER(C.c_int64)
        E._check(E.lib().fg_grid_summary(self._handle(), E._dp(log_norm), E._dp(mx), arg.ctypes.data_as(i64p), cnt.ctypes.data_as(i64p)))
        return dict(log_norm=log_norm, max=mx, argmax=arg, counts=cnt)

    def marginals(self):
        """(log_marginal_a [n][n_a], log_marginal_b [n][n_b])"""
        n = self.count
        la, lb = np.empty((n, self.n_a)), np.empty((n, self.n_b))
        E._check(E.lib().fg_grid_marginals(self._handle(), E._dp(la), E._dp(lb)))
        return la, lb

    def mixture(self):
        """(log_mix [n_b][n_a] = ln(mix / n_mixed), n_mixed, n_skipped)"""
        lm = np.empty((self.n_b, self.n_a))
        nm, ns = C.c_int64(), C.c_int64()
        E._check(E.lib().fg_grid_mixture(self._handle(), E._dp(lm), C.byref(nm), C.byref(ns)))
        return lm, int(nm.value), int(ns.value)


def log_joint_grid(model, site_a, site_b, a_values, b_values, seed, data=None, device: int = 0) -> np.ndarray:
    """grid.rs:22-69 under the reference's name, argument order and result: the flat row-major surface out[j * n_a + i] of
    (a_values[i], b_values[j]), every other latent site held at one seeded prior draw.  `model` is DSL source (with `data`), a model
    function, a `Program` or a `CompiledProgram`."""
    cp = _compile(model, data)
    _sites(cp, site_a, site_b)                               # ValueError before any engine exists
    eng = E.Engine(cp, 1, int(seed), device=device)
    try:
        eng.prior_init()
        g = eng.grid(site_a, a_values, site_b, b_values)
        try:
            return g.eval(0, 1).reshape(-1)
        finally:
            g.close()
    finally:
        eng.close()


class GridSurface(NamedTuple):
    """The surfaces of n bases over a_values x b_values (b_values None: one axis) with their per-base summaries; base 0's are what
    `peak`, `mean`, `std` and `log_evidence` speak of unless a base is named."""
    a_values: np.ndarray
    b_values: Optional[np.ndarray]
    log_joint: Optional[np.ndarray]          # [n][n_b][n_a], or None (keep=False)
    log_norm: np.ndarray                     # [n]
    max: np.ndarray                          # [n]
    argmax: np.ndarray                       # [n] flat index, -1: no cell above -inf
    counts: np.ndarray                       # [n][3]: NaN, -inf, +inf cells
    log_marginal_a: np.ndarray               # [n][n_a]
    log_marginal_b: np.ndarray               # [n][n_b]
    log_mixture: np.ndarray                  # [n_b][n_a]
    n_mixed: int
    n_skipped: int

    @property
    def peak(self):
        """the axis values at base 0's argmax: (a, b), or (a,) on one axis; None when no cell exceeds -inf"""
        return self.peak_of(0)

    def peak_of(self, base: int):
        k = int(self.argmax[base])
        if k < 0:
            return None
        n_a = self.a_values.size
        a = float(self.a_values[k % n_a])
        return (a,) if self.b_values is None else (a, float(self.b_values[k // n_a]))

    def log_evidence(self, cell_volume: float, base: int = 0) -> float:
        """log_norm + ln volume: the quadrature of the evidence on an evenly spaced grid"""
        return float(self.log_norm[base]) + math.log(cell_volume)

    def _moments(self, base):
        out = []
        for axis, lm in ((self.a_values, self.log_marginal_a), (self.b_values, self.log_marginal_b)):
            if axis is None:
                continue
            w = np.exp(lm[base] - self.log_norm[base])
            m = float(np.sum(w * axis) / np.sum(w))
            v = float(np.sum(w * (axis - m) ** 2) / np.sum(w))
            out.append((m, math.sqrt(max(v, 0.0))))
        return out

    def mean(self, base: int = 0):
        """per axis, from the marginals on the host"""
        return tuple(m for m, _ in self._moments(base))

    def std(self, base: int = 0):
        return tuple(s for _, s in self._moments(base))


def log_joint_surface(model, site_a, a_values, site_b=None, b_values=None, *, seed: int = 0, n_bases: int = 1, engine=None, chain0: int = 0,
                      keep: bool = True, data=None, device: int = 0) -> GridSurface:
    """The surfaces of `n_bases` bases with everything reduced on the device.  Without `engine` the bases are the chains of
    `Engine(cp, n_bases, seed).prior_init()`; with one they are its current chains [chain0, chain0 + n_bases) -- after `hmc_run`, say
    -- and `model` is not looked at."""
    own = engine is None
    if own:
        cp = _compile(model, data)
        _sites(cp, site_a, site_b)
        engine = E.Engine(cp, int(n_bases), int(seed), device=device)
    try:
        if own:
            engine.prior_init()
        g = engine.grid(site_a, a_values, site_b, b_values)
        try:
            lj = g.eval(int(chain0), int(n_bases), keep=keep)
            s = g.summary()
            la, lb = g.marginals()
            lm, nm, ns = g.mixture()
            return GridSurface(g.a_values, g.b_values, lj, s["log_norm"], s["max"], s["argmax"], s["counts"], la, lb, lm, nm, ns)
        finally:
            g.close()
    finally:
        if own:
            engine.close()
