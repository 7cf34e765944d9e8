"""Exact Gibbs moves of the discrete sites on the device, and HMC within Gibbs.

    g = eng.gibbs()                          # every discrete site whose support constants state (Bernoulli, Categorical, ...)
    g.sweep(3)                               # three sweeps of every chain; the engine's values move
    g.probs()                                # {address: [K]}: the Rao-Blackwell estimate of P(site = lo + k | data)

    b = hmc_gibbs_chain(seed, model, n_samples, n_warmup, n_chains=4096)     # hmc_step(1), then one sweep, every iteration
    b.get_f64("mu"), b.get_int("z#0"), b.gibbs_probs["z#0"]

`hmc_chain` holds every discrete site at its prior draw (hmc.rs:68-71: "compose with `mh` to also move discrete sites").  A sweep is
that composition with the exact conditional in place of a blind proposal: per chain and listed site the trace is scored at every
value of the support by the run `Engine.log_joint` does (bit for bit), the scores are normalised and the new value is drawn with the
stream (seed, chain, sweep index, 13) -- fugue_amd/csrc/fg_gibbs.hip, fg_gibbs_plan.h, DESIGN.md 3.25.  Chain c's sweep t gives the
same bits alone or among any number of chains, in one call of several sweeps or in several calls."""
from __future__ import annotations

import ctypes as C
from typing import Dict, NamedTuple, Optional

import numpy as np

from . import engine as E

K_CAP = 4096                                             # FG_GIBBS_K_CAP
COUNT_NAMES = ("moved", "stuck", "nan_cells", "neg_inf_cells")      # FG_GIBBS_COUNTS


def site_support(cp: "E.CompiledProgram", site: int):
    """`fg_program_site_support`: (lo, hi) of sorted site `site` where constants alone state its support, else None"""
    lo, hi = C.c_int64(), C.c_int64()
    rc = E.lib().fg_program_site_support(cp.h, int(site), C.byref(lo), C.byref(hi))
    if rc < 0:
        E._check(rc)
    return (int(lo.value), int(hi.value)) if rc == 1 else None


def _site_list(cp, sites) -> Optional[list]:
    """sorted site indices of addresses or indices; None stays None (the handle picks); an unknown address is a ValueError"""
    if sites is None:
        return None
    out = []
    for s in sites:
        if isinstance(s, (int, np.integer)) and not isinstance(s, bool):
            out.append(int(s))
        elif str(s) in cp.site_names:
            out.append(cp.site_names.index(str(s)))
        else:
            raise ValueError(f"site `{s}` is no sample site of the model")
    if not out:
        raise ValueError("sites is an empty list (None selects every discrete site with a finite constant support)")
    return out


def _i32(v):
    return (C.c_int32 * max(1, len(v)))(*v)


class SweepOutput(NamedTuple):
    rec: Optional[np.ndarray]                # [n][n_rec][C] int64 cells after each sweep, or None (no rec_sites, or the caller's d_rec)
    scores: Optional[np.ndarray]             # [cells][C]: the scores of the call's last sweep
    cond: Optional[np.ndarray]               # [cells][C]: its conditional probabilities (NaN at a stuck site)


class GibbsSweep(E._Stream):
    """`fg_gibbs` (fg_gibbs.hip): the exact Gibbs transition over an ordered list of discrete sites of an engine.  Close it before its
    engine."""

    _free = "fg_gibbs_free"

    def __init__(self, engine: "E.Engine", sites=None):
        cp = engine.cp
        lst = _site_list(cp, sites)
        self.engine, self.h = engine, None
        out = C.c_void_p()
        E._check(E.lib().fg_gibbs_new(engine.h, None if lst is None else _i32(lst), 0 if lst is None else len(lst), C.byref(out)))
        self.h = out.value
        L = E.lib()
        G = L.fg_gibbs_n_sites(self.h)
        site, K = np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int32)
        lo, cell0 = np.zeros(G, dtype=np.int64), np.zeros(G, dtype=np.int64)
        i32p, i64p = C.POINTER(C.c_int32), C.POINTER(C.c_int64)
        E._check(L.fg_gibbs_layout(self.h, site.ctypes.data_as(i32p), lo.ctypes.data_as(i64p), K.ctypes.data_as(i32p), cell0.ctypes.data_as(i64p)))
        self.layout = dict(sites=site.tolist(), names=[cp.site_names[j] for j in site], lo=lo.tolist(), K=K.tolist(), cell0=cell0.tolist())
        self.n_sites, self.n_cells = int(G), int(L.fg_gibbs_n_cells(self.h))

    @property
    def count(self) -> int:
        """the sweep index of the next sweep"""
        return int(E.lib().fg_gibbs_count(self._handle()))

    def seek(self, t: int):
        self._integers(t=t)
        E._check(E.lib().fg_gibbs_seek(self._handle(), int(t)))

    def sweep(self, n: int = 1, rec_sites=(), d_rec: Optional[int] = None, scores: bool = False, cond: bool = False) -> SweepOutput:
        """n sweeps.  rec_sites (addresses or sorted indices, any sites): their cells after each sweep come back as `rec` [n][n_rec][C],
        or go to the device buffer d_rec of that shape when one is given (then nothing is downloaded for them).  scores / cond: the
        tables [cells][C] of the call's last sweep."""
        self._integers(n=n)
        eng = self.engine
        rec = _site_list(eng.cp, list(rec_sites)) if len(rec_sites) else []
        own_rec = bool(rec) and d_rec is None and n > 0
        mine = []
        try:
            if own_rec:
                d_rec = eng.device_alloc(max(1, n * len(rec) * eng.C) * 8); mine.append(d_rec)
            d_s = d_c = None
            if scores and n > 0:
                d_s = eng.device_alloc(self.n_cells * eng.C * 8); mine.append(d_s)
            if cond and n > 0:
                d_c = eng.device_alloc(self.n_cells * eng.C * 8); mine.append(d_c)
            E._check(E.lib().fg_gibbs_sweep(self._handle(), int(n), _i32(rec) if rec else None, len(rec), d_rec, d_s, d_c))
            return SweepOutput(eng.download(d_rec, (n, len(rec), eng.C), dtype=np.int64) if own_rec else None,
                               eng.download(d_s, (self.n_cells, eng.C)) if d_s else None, eng.download(d_c, (self.n_cells, eng.C)) if d_c else None)
        finally:
            for p in mine:
                eng.device_free(p)

    def stats(self) -> Dict[str, np.ndarray]:
        """moved, stuck, nan_cells, neg_inf_cells: [n_sites] each, summed over the chains and the sweeps run"""
        cnt = np.zeros((self.n_sites, len(COUNT_NAMES)), dtype=np.int64)
        E._check(E.lib().fg_gibbs_stats(self._handle(), cnt.ctypes.data_as(C.POINTER(C.c_int64))))
        return {name: cnt[:, q].copy() for q, name in enumerate(COUNT_NAMES)}

    def probs(self):
        """(mean, n): mean[i] [K_i] = the tree-pooled conditional probabilities of listed site i divided by n[i], the (sweep, chain)
        pairs that contributed (NaN when none did)"""
        mean, n = np.zeros(self.n_cells), np.zeros(self.n_sites, dtype=np.int64)
        E._check(E.lib().fg_gibbs_probs(self._handle(), E._dp(mean), n.ctypes.data_as(C.POINTER(C.c_int64))))
        return [mean[c0:c0 + K].copy() for c0, K in zip(self.layout["cell0"], self.layout["K"])], n


def _compile(model_fn) -> "E.CompiledProgram":
    return model_fn if isinstance(model_fn, E.CompiledProgram) else E.compile_model(model_fn)


def _batch(cp, g, ran: bool, cells, results, accept_rate=0.0, mean_step_size=float("nan"), n_divergent=0):
    from .inference import ChainBatch
    mean, n = g.probs() if ran else ([np.full(K, np.nan) for K in g.layout["K"]], np.zeros(g.n_sites, dtype=np.int64))
    stats = dict(sites=list(g.layout["names"]), lo=np.array(g.layout["lo"]), K=np.array(g.layout["K"]), n=n, **g.stats())
    return ChainBatch(list(cp.site_names), list(cp.site_vtypes), cells, accept_rate, mean_step_size, int(n_divergent), list(cp.result_names), results,
                      observe_values=dict(zip(cp.observe_names, cp.observe_values)), gibbs_probs=dict(zip(g.layout["names"], mean)), gibbs_stats=stats)


def _run(seed, model_fn, n_samples, n_warmup, config, n_chains, device, sites, with_hmc: bool, who: str):
    from .inference import HMCConfig
    if n_samples < 0 or n_warmup < 0:
        raise ValueError(f"{who}: n_samples and n_warmup must not be negative")
    cp = _compile(model_fn)
    hmc = with_hmc and cp.d > 0
    eng = E.Engine(cp, n_chains, seed=seed, device=device)
    g = None
    try:
        if hmc:
            eng.hmc_init((config or HMCConfig()).raw(), n_warmup)          # the prior draw of every site, the step-size search
        else:
            eng.prior_init()
        g = eng.gibbs(sites)
        for _ in range(n_warmup):
            if hmc:
                eng.hmc_step(1)
            g.sweep(1)
        # the probability sums cover the sampling sweeps only: a fresh handle, at the sweep index the warmup reached
        t = g.count
        g.close()
        g = eng.gibbs(sites)
        g.seek(t)
        S, Cn, d = cp.S, eng.C, cp.d
        other = [j for j in range(S) if j not in cp.f64_sites]
        rows = list(cp.f64_sites) + other                   # the row map of the buffer [n][S][C]: the f64 rows as fg_hmc_step records them, then the rest
        buf = eng.device_alloc(max(1, n_samples * S * Cn) * 8)
        try:
            for k in range(n_samples):
                at = buf + k * S * Cn * 8
                if hmc:
                    eng.hmc_step(1, at)
                    if other:
                        g.sweep(1, rec_sites=other, d_rec=at + d * Cn * 8)
                    else:
                        g.sweep(1)
                else:
                    g.sweep(1, rec_sites=rows, d_rec=at)
            raw = eng.download(buf, (n_samples, S, Cn), dtype=np.int64)
            results = None
            if cp.R > 0:
                results = np.zeros((n_samples, cp.R, Cn))
                if n_samples > 0:
                    rbuf = eng.result_eval(buf, n_samples, rows=rows)
                    results = eng.download(rbuf, (n_samples, cp.R, Cn))
                    eng.device_free(rbuf)
        finally:
            eng.device_free(buf)
        cells = np.empty_like(raw)
        cells[:, rows, :] = raw
        if hmc:
            st = eng.hmc_stats()
            return _batch(cp, g, n_samples > 0, cells, results, st.accept_rate, st.mean_step_size, st.n_divergent)
        return _batch(cp, g, n_samples > 0, cells, results)
    finally:
        if g is not None:
            g.close()
        eng.close()


def hmc_gibbs_chain(seed: int, model_fn, n_samples: int, n_warmup: int, config=None, n_chains: int = 1, device: int = 0, sites=None):
    """HMC within Gibbs: every iteration, warmup included, is `hmc_step(1)` (the f64 sites move, hmc.rs:566-583) followed by one sweep of
    the discrete sites `sites` (None: every one whose support constants state).  During sampling the f64 rows are recorded by the HMC
    step and every other site's row by the sweep, into one device buffer [n][S][C] that is downloaded once; the model's return value is
    evaluated on it, so a result may read a discrete site.  The batch carries `gibbs_probs` (address -> [K], over the sampling sweeps)
    and `gibbs_stats`.  A model without an f64 site runs sweeps only.  `predictive=` / `pointwise=` are not offered by this driver:
    run `Engine.predict_eval` on the draws."""
    return _run(seed, model_fn, n_samples, n_warmup, config, n_chains, device, sites, True, "hmc_gibbs_chain")


def gibbs_chain(seed: int, model_fn, n_samples: int, n_warmup: int, n_chains: int = 1, device: int = 0, sites=None):
    """Sweeps only: the discrete sites move, every f64 site stays at its prior draw.  The purely discrete case of `hmc_gibbs_chain`."""
    return _run(seed, model_fn, n_samples, n_warmup, None, n_chains, device, sites, False, "gibbs_chain")
