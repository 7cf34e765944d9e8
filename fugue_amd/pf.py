"""Bootstrap particle filters on the device: `WasmParticleFilter` (crates/fugue-wasm/src/pf.rs), the reference's sequential-in-time
inference, and a bank of them.

    pf = ParticleFilter(200, 1.6, 0.7, 0.6, 0.5, 11)
    out = pf.step(0.3)                       # StepOut: prev, propagated, weights, ess_frac, log_z_inc, resampled, parents, posterior
    pf.log_evidence(), pf.t()

    bank = ParticleFilterBank(5000, 1.0, 0.5, sig_obs=np.linspace(0.2, 2.0, 64), ess_threshold=0.5, seeds=range(64))
    run = bank.run(observations)             # PFRun: ess_frac, log_z_inc, resampled, mean, var, each [T][B]
    bank.log_evidence()                      # [B]: the likelihood surface over sig_obs

The model is the reference's random walk: x_0 ~ N(0, prior_sig), x_t = x_{t-1} + N(0, sig_step), y_t ~ N(x_t, sig_obs); systematic
resampling when ESS / n < ess_threshold.  One workgroup runs one filter with the whole population in LDS and loops over the
observations of a launch inside the kernel (fugue_amd/csrc/fg_pf.hip); a filter above the cap of one workgroup
(N_CAP, at least the reference's 5000) is refused.  Random numbers are the engine's Philox streams (seed, particle, time, 11) and
(seed, 0, time, 12), not the reference's StdRng: the law is the reference's, the draws are not."""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple

import numpy as np

from . import engine as E

RNG_PF, RNG_PF_RESAMPLE = 11, 12                         # fg_ir.h
N_MIN, N_REFERENCE_MAX = 2, 5000                         # pf.rs:82
N_CAP = (160 * 1024 - 1024) // (3 * 8) // 2 * 2          # FG_PF_N_CAP (fg_pf_plan.h)


def steps_per_launch(n: int) -> int:
    """fg_pf_plan.h: how many steps of a run one launch takes at n particles (tests/test_pf_cpu.py pins it to the header)"""
    return max(1, min(256, (1 << 17) // int(n)))


class StepOut(NamedTuple):
    """pf.rs:38-56"""
    prev: np.ndarray
    propagated: np.ndarray
    weights: np.ndarray
    ess_frac: float
    log_z_inc: float
    resampled: bool
    parents: np.ndarray
    posterior: np.ndarray


class PFRun(NamedTuple):
    """the summaries of every step of a run, each [T][B]; mean and var are those of the propagated particles under the normalised
    weights, before resampling"""
    ess_frac: np.ndarray
    log_z_inc: np.ndarray
    resampled: np.ndarray
    mean: np.ndarray
    var: np.ndarray


class BankStep(NamedTuple):
    """one recorded step of a bank: the summaries [B], StepOut's arrays [B][n]"""
    prev: np.ndarray
    propagated: np.ndarray
    weights: np.ndarray
    ess_frac: np.ndarray
    log_z_inc: np.ndarray
    resampled: np.ndarray
    parents: np.ndarray
    posterior: np.ndarray
    mean: np.ndarray
    var: np.ndarray


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


class ParticleFilterBank:
    """B independent filters of n particles.  Scalars broadcast against arrays of length B; `seeds` fixes B when it is a sequence.
    n is not clamped here (ParticleFilter clamps as the reference does): outside [2, N_CAP] the library refuses it."""

    def __init__(self, n, prior_sig, sig_step, sig_obs, ess_threshold, seeds, device: int = 0):
        cols = [np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (prior_sig, sig_step, sig_obs, ess_threshold)]
        sd = np.atleast_1d(np.asarray(seeds, dtype=np.uint64))
        B = max([c.size for c in cols] + [sd.size])
        for c in cols + [sd]:
            if c.ndim != 1 or c.size not in (1, B):
                raise ValueError("ParticleFilterBank: parameters must be scalars or arrays of one length B")
        par = (E.fg_pf_params * B)()
        for b in range(B):
            p, s, o, th = (float(c[b if c.size > 1 else 0]) for c in cols)
            par[b] = E.fg_pf_params(p, s, o, th, int(sd[b if sd.size > 1 else 0]))
        self.n, self.B = int(n), B
        self._h = None
        h = C.c_void_p()
        E._check(E.lib().fg_pf_new(int(device), self.n, B, par, C.byref(h)))
        self._h = h

    def _handle(self):
        if self._h is None:
            raise RuntimeError("the particle filter bank is closed")
        return self._h

    def close(self):
        if self._h is not None:
            E.lib().fg_pf_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_sig_obs(self, sig_obs, filter: int = -1):
        """pf.rs:101-103, for one filter or (-1) all of them"""
        E._check(E.lib().fg_pf_set_sig_obs(self._handle(), int(filter), float(sig_obs)))

    def _obs(self, observations, per_step: bool):
        o = np.ascontiguousarray(observations, dtype=np.float64)
        if per_step:                                      # a step: a scalar, or one observation per filter
            if o.ndim == 0 or o.size == 1 and self.B != 1:
                return o.reshape(1), 0
            if o.shape != (self.B,):
                raise ValueError("step: one observation, or one per filter")
            return o, 1
        if o.ndim == 1:
            return o, 0
        if o.ndim != 2 or o.shape[0] != self.B:
            raise ValueError("run: observations [T] shared by the filters, or [B][T]")
        return o, 1

    def run(self, observations) -> PFRun:
        """T steps: observations [T] shared by the filters, or [B][T] one series per filter"""
        o, per = self._obs(observations, False)
        T = o.shape[-1]
        ess, lzi, mean, var = (np.empty((T, self.B)) for _ in range(4))
        res = np.zeros((T, self.B), dtype=np.int32)
        E._check(E.lib().fg_pf_run(self._handle(), E._dp(o), T, per, E._dp(ess), E._dp(lzi), _ip(res), E._dp(mean), E._dp(var)))
        return PFRun(ess, lzi, res.astype(bool), mean, var)

    def step(self, obs, record: bool = True) -> BankStep:
        """one step (pf.rs:107-172) of every filter: obs a scalar or [B]; without `record` the five arrays are None"""
        o, per = self._obs(obs, True)
        B, n = self.B, self.n
        ess, lzi, mean, var = (np.empty(B) for _ in range(4))
        res = np.zeros(B, dtype=np.int32)
        if record:
            prev, prop, w, post = (np.empty((B, n)) for _ in range(4))
            par = np.empty((B, n), dtype=np.int64)
            rec = (E._dp(prev), E._dp(prop), E._dp(w), par.ctypes.data_as(C.POINTER(C.c_int64)), E._dp(post))
        else:
            prev = prop = w = post = par = None
            rec = (None, None, None, None, None)
        E._check(E.lib().fg_pf_step(self._handle(), E._dp(o), per, E._dp(ess), E._dp(lzi), _ip(res), E._dp(mean), E._dp(var), *rec))
        return BankStep(prev, prop, w, ess, lzi, res.astype(bool), par, post, mean, var)

    def log_evidence(self) -> np.ndarray:
        out = np.empty(self.B)
        E._check(E.lib().fg_pf_log_evidence(self._handle(), E._dp(out)))
        return out

    def positions(self) -> np.ndarray:
        out = np.empty((self.B, self.n))
        E._check(E.lib().fg_pf_positions(self._handle(), E._dp(out)))
        return out

    def t(self) -> int:
        return int(E.lib().fg_pf_t(self._handle()))


class ParticleFilter:
    """`WasmParticleFilter` under the reference's shape, with its silent clamps (pf.rs:82-94): n into [2, 5000], every sigma at least
    1e-6, the threshold into [0, 1]."""

    def __init__(self, n, prior_sig, sig_step, sig_obs, ess_threshold, seed, device: int = 0):
        n = min(max(int(n), N_MIN), N_REFERENCE_MAX)
        self._bank = ParticleFilterBank(n, max(float(prior_sig), 1e-6), max(float(sig_step), 1e-6), max(float(sig_obs), 1e-6),
                                        min(max(float(ess_threshold), 0.0), 1.0), [int(seed)], device=device)
        self.n = n

    def set_sig_obs(self, sig_obs):
        self._bank.set_sig_obs(sig_obs)

    def step(self, obs) -> StepOut:
        s = self._bank.step(float(obs))
        return StepOut(s.prev[0], s.propagated[0], s.weights[0], float(s.ess_frac[0]), float(s.log_z_inc[0]), bool(s.resampled[0]), s.parents[0],
                       s.posterior[0])

    def log_evidence(self) -> float:
        return float(self._bank.log_evidence()[0])

    def t(self) -> int:
        return self._bank.t()

    def positions(self) -> np.ndarray:
        return self._bank.positions()[0]

    def close(self):
        self._bank.close()
