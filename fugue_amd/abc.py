"""Approximate Bayesian computation over the model's own simulator: the drivers of the reference's `src/inference/abc.rs` on the device.

A simulator is one of two things the engine already computes for a batch of attempts: the selected observe statements drawn at the
attempt's values (`simulator="observe"` or a list of observe addresses), or named result expressions of the model (`simulator=` a list
of result names).  The reference's user closures have no device form and are out of scope.  The attempts run in rounds of `batch`;
the result is the one the reference's sequential loop gives and does not depend on `batch` (include/fugue_amd.h, fg_abc_*).

    abc_rejection        abc.rs:283      abc_scalar_summary   abc.rs:882
    abc_smc_weighted     abc.rs:520      abc_smc              abc.rs:696
"""
from __future__ import annotations

import ctypes as C
import warnings
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np

from . import engine as E
from . import model as M

ABC_SMC_DEFAULT_ATTEMPT_FACTOR = 100      # abc.rs:403
EUCLIDEAN, MANHATTAN, SUMMARY_STATS = 0, 1, 2
SIM_OBSERVE, SIM_RESULT = 0, 1
RNG_ABC = 10                              # fg_ir.h FG_RNG_ABC


class EuclideanDistance:                  # abc.rs:130
    kind = EUCLIDEAN
    weights: Sequence[float] = ()


class ManhattanDistance:                  # abc.rs:166
    kind = MANHATTAN
    weights: Sequence[float] = ()


class SummaryStatsDistance:               # abc.rs:183-190
    kind = SUMMARY_STATS

    def __init__(self, weights: Sequence[float]):
        self.weights = [float(w) for w in weights]


@dataclass
class ABCSMCConfig:                       # abc.rs:392-399 (no defaults, as in the reference)
    initial_tolerance: float
    tolerance_schedule: List[float]
    particles_per_round: int


class ABCError(Exception):
    """abc.rs:407-429: `kind` is "EmptyInitialPopulation" (fields tolerance, attempts) or "StageExhausted" (fields tolerance, accepted,
    requested, attempts); the message is the reference's Display text."""

    def __init__(self, kind: str, tolerance: float, attempts: int, accepted: Optional[int] = None, requested: Optional[int] = None):
        self.kind, self.tolerance, self.attempts, self.accepted, self.requested = kind, float(tolerance), int(attempts), accepted, requested
        if kind == "EmptyInitialPopulation":
            msg = f"ABC-SMC initial population is empty: no draw fell within tolerance {tolerance} in {attempts} attempts"
        else:
            msg = (f"ABC-SMC stage at tolerance {tolerance} exhausted its budget of {attempts} attempts with only "
                   f"{accepted}/{requested} particles accepted")
        super().__init__(msg)


@dataclass
class ABCSMCResult:
    """abc.rs:466-472, the particles as columns: `cells` [n_sites][n] 8-byte cells in site order, `weights` [n] (sum 1)."""
    sites: List[str]
    vtypes: List[int]
    cells: np.ndarray
    weights: np.ndarray
    final_tolerance: float
    distances: Optional[np.ndarray] = None
    attempt_index: Optional[np.ndarray] = None

    def __len__(self):
        return int(self.cells.shape[1])

    def get_f64(self, address: str) -> np.ndarray:
        if address not in self.sites or self.vtypes[self.sites.index(address)] != M.F64:
            raise M.FugueError(f"address not found: {address}", M.ErrorCode.TraceAddressNotFound)
        return np.ascontiguousarray(self.cells[self.sites.index(address)]).view(np.float64)

    def weighted_mean(self, address: str) -> Optional[float]:
        """abc.rs:476-489, summed in order"""
        if address not in self.sites or self.vtypes[self.sites.index(address)] != M.F64:
            return None
        num = den = 0.0
        for v, w in zip(self.get_f64(address).tolist(), self.weights.tolist()):
            num += w * v
            den += w
        return num / den if den > 0.0 else None


def _simulator(cp: E.CompiledProgram, simulator):
    """-> (sim_kind, indices): "observe" / a list of observe addresses (program order), or a list of result names"""
    two_forms = ('simulator= is "observe" or a list of observe addresses (the selected observe statements, drawn at the attempt\'s values), '
                 "or a list of result names (result expressions of the model)")
    if isinstance(simulator, str) and simulator == "observe":
        if cp.O == 0:
            raise ValueError("simulator='observe': the model has no observe statement; " + two_forms)
        return SIM_OBSERVE, list(range(cp.O))
    if isinstance(simulator, (list, tuple)) and len(simulator) and all(isinstance(s, str) for s in simulator):
        if all(s in cp.observe_names for s in simulator):
            idx = sorted(cp.observe_names.index(s) for s in simulator)
            if len(set(idx)) != len(idx):
                raise ValueError("simulator=: an observe address is given twice; " + two_forms)
            return SIM_OBSERVE, idx
        if all(s in cp.result_names for s in simulator):
            return SIM_RESULT, [cp.result_names.index(s) for s in simulator]
    raise ValueError(f"simulator={simulator!r} is not understood: " + two_forms)


def _observed(cp: E.CompiledProgram, sim_kind: int, idx, observed_data) -> np.ndarray:
    if observed_data is not None:
        return np.ascontiguousarray(np.atleast_1d(np.asarray(observed_data, dtype=np.float64)).ravel())
    if sim_kind != SIM_OBSERVE or cp.program is None:
        raise ValueError("observed_data is required unless the simulator is the model's own observe statements")
    own = [st for st in cp.program.stmts if st.kind == M.OBSERVE]
    vals = [M._cval(own[k].value) for k in idx]
    if any(v is None for v in vals):
        raise ValueError("observed_data is required: an observed value of the model is not a constant")
    return np.asarray(vals, dtype=np.float64)


class ABCHandle:
    """`fg_abc`: the step calls (include/fugue_amd.h) on one engine whose n_chains is the batch."""

    def __init__(self, engine: E.Engine, sim_kind: int, sel: Sequence[int], observed, distance_fn, capacity: int):
        self.engine, self.n = engine, int(capacity)
        obs = np.ascontiguousarray(observed, dtype=np.float64)
        w = np.ascontiguousarray(list(getattr(distance_fn, "weights", ())), dtype=np.float64)
        sp = (C.c_int32 * max(1, len(sel)))(*[int(k) for k in sel])
        out = C.c_void_p()
        E._check(E.lib().fg_abc_new(engine.h, sim_kind, sp, len(sel), E._dp(obs), obs.size, int(distance_fn.kind), E._dp(w), w.size, self.n, C.byref(out)))
        self.h = out

    def close(self):
        if getattr(self, "h", None):
            E.lib().fg_abc_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def round_prior(self, tol: float, budget: int):
        acc, att = C.c_int64(), C.c_int64()
        E._check(E.lib().fg_abc_round_prior(self.h, float(tol), int(budget), C.byref(acc), C.byref(att)))
        return acc.value, att.value

    def stage_begin(self):
        E._check(E.lib().fg_abc_stage_begin(self.h))

    def round_stage(self, stage: int, tol: float, budget: int):
        acc, att = C.c_int64(), C.c_int64()
        E._check(E.lib().fg_abc_round_stage(self.h, int(stage), float(tol), int(budget), C.byref(acc), C.byref(att)))
        return acc.value, att.value

    def stage_end(self):
        E._check(E.lib().fg_abc_stage_end(self.h))

    def last_round(self):
        B = self.engine.C
        idx, dist, lp, acc = np.zeros(B, dtype=np.int64), np.zeros(B), np.zeros(B), np.zeros(B, dtype=np.int32)
        E._check(E.lib().fg_abc_last_round(self.h, idx.ctypes.data_as(C.POINTER(C.c_int64)), E._dp(dist), E._dp(lp), acc.ctypes.data_as(C.POINTER(C.c_int32))))
        return idx, dist, lp, acc

    def get_population(self, which: int = 0) -> dict:
        n = C.c_int64()
        E._check(E.lib().fg_abc_get_population(self.h, which, C.byref(n), None, None, None, None, None, None))
        n, S = n.value, self.engine.S
        cells = np.zeros((max(1, S), max(1, n)), dtype=np.int64)
        w, dist, lp, ld, att = np.zeros(max(1, n)), np.zeros(max(1, n)), np.zeros(max(1, n)), np.zeros(max(1, n)), np.zeros(max(1, n), dtype=np.int64)
        if n:
            E._check(E.lib().fg_abc_get_population(self.h, which, None, cells.ctypes.data, E._dp(w), E._dp(dist), att.ctypes.data_as(C.POINTER(C.c_int64)), E._dp(lp), E._dp(ld)))
        return {"n": n, "cells": cells[:S, :n], "weights": w[:n], "dist": dist[:n], "attempt": att[:n], "log_prior": lp[:n], "log_denom": ld[:n]}

    def set_population(self, cells, weights, dist=None, attempt=None, log_prior=None, log_denom=None):
        cells = np.ascontiguousarray(cells, dtype=np.int64)
        n = cells.shape[1]
        f = lambda v: None if v is None else np.ascontiguousarray(v, dtype=np.float64)
        w, dist, log_prior, log_denom = f(weights), f(dist), f(log_prior), f(log_denom)
        att = None if attempt is None else np.ascontiguousarray(attempt, dtype=np.int64)
        p = lambda v: None if v is None else E._dp(v)
        E._check(E.lib().fg_abc_set_population(self.h, n, cells.ctypes.data, p(w), p(dist), None if att is None else att.ctypes.data_as(C.POINTER(C.c_int64)),
                                               p(log_prior), p(log_denom)))


def _open(seed, model_fn, simulator, observed_data, distance_fn, capacity, batch, device, chain_offset=0):
    cp = model_fn if isinstance(model_fn, E.CompiledProgram) else E.compile_model(model_fn)
    sim_kind, idx = _simulator(cp, simulator)
    obs = _observed(cp, sim_kind, idx, observed_data)
    if not hasattr(distance_fn, "kind"):
        raise ValueError("distance_fn is EuclideanDistance(), ManhattanDistance() or SummaryStatsDistance(weights)")
    eng = E.Engine(cp, int(batch), seed=seed, chain_offset=chain_offset, device=device)
    try:
        return cp, eng, ABCHandle(eng, sim_kind, idx, obs, distance_fn, capacity)
    except Exception:
        eng.close()
        raise


def _result(cp, pop, tol) -> ABCSMCResult:
    return ABCSMCResult(list(cp.site_names), list(cp.site_vtypes), pop["cells"], pop["weights"], float(tol), pop["dist"], pop["attempt"])


def _empty(cp, tol) -> ABCSMCResult:
    return ABCSMCResult(list(cp.site_names), list(cp.site_vtypes), np.zeros((cp.S, 0), dtype=np.int64), np.zeros(0), float(tol), np.zeros(0), np.zeros(0, dtype=np.int64))


def abc_rejection(seed: int, model_fn, simulator, observed_data, distance_fn, tolerance: float, max_samples: int, batch: int = 4096,
                  device: int = 0) -> ABCSMCResult:
    """abc.rs:283-325: prior draws until `max_samples` fall within `tolerance` or `max_samples * 100` attempts are made.  The accepted
    traces are the result's columns (weights 1 / accepted); an empty result comes with the reference's warning."""
    cp, eng, h = _open(seed, model_fn, simulator, observed_data, distance_fn, max(1, int(max_samples)), batch, device)
    try:
        acc, _ = h.round_prior(tolerance, int(max_samples) * 100) if max_samples > 0 else (0, 0)
        if acc == 0:
            warnings.warn("No samples accepted in ABC. Consider increasing tolerance or max_samples.")
            return _empty(cp, tolerance)
        return _result(cp, h.get_population(0), tolerance)
    finally:
        h.close()
        eng.close()


def abc_scalar_summary(seed: int, model_fn, simulator, observed_summary: float, tolerance: float, max_samples: int, batch: int = 4096,
                       device: int = 0) -> ABCSMCResult:
    """abc.rs:882-899: abc_rejection on one scalar summary, `simulator` = one result name, Euclidean distance."""
    if not isinstance(simulator, str):
        raise ValueError("abc_scalar_summary: simulator= is one result name; simulator= of the other drivers is \"observe\" or a list of observe "
                         "addresses, or a list of result names")
    return abc_rejection(seed, model_fn, [simulator], [float(observed_summary)], EuclideanDistance(), tolerance, max_samples, batch, device)


def abc_smc_weighted(seed: int, model_fn, simulator, observed_data, distance_fn, config: ABCSMCConfig, max_attempts_per_stage: int,
                     batch: int = 4096, device: int = 0) -> ABCSMCResult:
    """abc.rs:520-650.  Raises ABCError (EmptyInitialPopulation / StageExhausted with the reference's fields)."""
    n = int(config.particles_per_round)
    cp, eng, h = _open(seed, model_fn, simulator, observed_data, distance_fn, max(1, n), batch, device)
    try:
        return _smc_weighted(cp, h, config, int(max_attempts_per_stage))[0]
    finally:
        h.close()
        eng.close()


def _smc_weighted(cp, h: ABCHandle, config: ABCSMCConfig, budget: int):
    """-> (result, number of stages run, the prior stage included)"""
    n = int(config.particles_per_round)
    acc, att = h.round_prior(config.initial_tolerance, budget) if n > 0 else (0, 0)
    if acc == 0:
        raise ABCError("EmptyInitialPopulation", config.initial_tolerance, att)
    tol, t = float(config.initial_tolerance), 0
    for new_tol in config.tolerance_schedule:
        if new_tol >= tol:                                # abc.rs:566
            continue
        t += 1
        h.stage_begin()
        acc, _ = h.round_stage(t, new_tol, budget)
        if acc < n:
            raise ABCError("StageExhausted", new_tol, budget, accepted=acc, requested=n)
        h.stage_end()
        tol = float(new_tol)
    return _result(cp, h.get_population(0), tol), t + 1


def sample_index(u: float, weights) -> int:
    """abc.rs:816-830 with the uniform handed in, summed in order"""
    total = 0.0
    for w in weights:
        total += w
    ut, cum = u * total, 0.0
    for i, w in enumerate(weights):
        cum += w
        if ut <= cum:
            return i
    return len(weights) - 1


def abc_smc(seed: int, model_fn, simulator, observed_data, distance_fn, config: ABCSMCConfig, batch: int = 4096, device: int = 0) -> ABCSMCResult:
    """abc.rs:696-728: abc_smc_weighted with the default attempt budget, then resampled to an equally-weighted population: output i is
    particle sample_index(u_i) with u_i the first uniform of the stream (seed, i, n_stages + 1, 10).  On an ABCError: a warning and an
    empty result."""
    n = int(config.particles_per_round)
    budget = ABC_SMC_DEFAULT_ATTEMPT_FACTOR * max(n, 1)
    cp, eng, h = _open(seed, model_fn, simulator, observed_data, distance_fn, max(1, n), batch, device)
    try:
        try:
            res, n_stages = _smc_weighted(cp, h, config, budget)
        except ABCError as err:
            warnings.warn(f"ABC-SMC did not complete: {err}. Returning empty population.")
            return _empty(cp, config.initial_tolerance)
    finally:
        h.close()
        eng.close()
    w = res.weights.tolist()
    u = _uniforms(seed, len(res), n_stages + 1)
    idx = np.asarray([sample_index(float(ui), w) for ui in u], dtype=np.int64)
    m = len(res)
    return ABCSMCResult(res.sites, res.vtypes, np.ascontiguousarray(res.cells[:, idx]), np.full(m, 1.0 / m), res.final_tolerance,
                        res.distances[idx], res.attempt_index[idx])


def _uniforms(seed: int, n: int, it: int) -> np.ndarray:
    """first Uniform(0,1) of the streams (seed, i, it, 10), i < n: the engine's counter-based generator (Philox4x32-10, fg_math.h),
    restated on the host -- n draws once per run"""
    M32 = 0xFFFFFFFF
    out = np.empty(n)
    k0, k1 = seed & M32, (seed >> 32) & M32
    for i in range(n):
        c = [i & M32, 0, it & M32, RNG_ABC]
        a, b = k0, k1
        for _ in range(10):
            p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
            c = [((p1 >> 32) ^ c[1] ^ a) & M32, p1 & M32, ((p0 >> 32) ^ c[3] ^ b) & M32, p0 & M32]
            a, b = (a + 0x9E3779B9) & M32, (b + 0xBB67AE85) & M32
        out[i] = ((((c[1] << 32) | c[0]) >> 11) + 0.0) * (1.0 / 9007199254740992.0)
    return out
