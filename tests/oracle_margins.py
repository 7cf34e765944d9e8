"""How far every accept decision of an ORACLE run lies from its boundary.  A parity test may leave a chain out of its comparison only where the
oracle's own run of that chain has a decision within rounding of its boundary (tests/knife.excused); these functions measure that distance for
the runs tests/parity_cases.py lists.  CPU only: the oracle and numpy, nothing of the engine.

  mh_margins   |ln u - log_alpha| of every step of adaptive_mcmc_chain (orc_mh_run_from's trace; tests/test_knife_margins_cpu.py asserts that
               its draws are orc_mh_run's, bit for bit)
  hmc_replay   hmc_one_chain (oracle/orc_inference.c:184-285, without mass adaptation) again from the oracle's primitives, so that every
               transition's u and alpha are in hand: the draws (bit for bit those of orc_hmc_run), |u - alpha| per transition and the distance
               of the step-size search
  eps_search   Hoffman-Gelman Alg. 4 (orc_find_reasonable_epsilon, orc_inference.c:107-132) restated from leapfrog and log_joint_at, with the
               smallest distance of an evaluated log-ratio to the threshold it was compared with"""
import math

import numpy as np

from oracle import oracle as orc

RNG_PRIOR, RNG_HMC, RNG_EPS = 1, 2, 3                  # stream purposes (oracle/fugue_oracle.h)
INF = math.inf


def mh_margins(om, seed, C, nw, ns, overrides=None, chain0=0, n_threads=8):
    """(dist [nw + ns][C], trace): dist = |ln u - log_alpha| of every step; +inf where the step was decided without a uniform (u is NaN:
    log_alpha >= 0 accepts, mh.rs:733) or where log_alpha is not finite (NaN rejects, -inf rejects whatever u is).  trace: mh_run_from's dict."""
    o = om.mh_run_from(seed, C, nw, ns, start=None, overrides=overrides, chain0=chain0, n_threads=n_threads)
    la, u = o["log_alpha"], o["u"]
    with np.errstate(divide="ignore", invalid="ignore"):
        dist = np.abs(np.log(u) - la)
    dist[np.isnan(u) | ~np.isfinite(la)] = INF
    return dist, o


def _kinetic(p):
    s = 0.0
    for x in p: s += x * x * 1.0                         # kinetic(), orc_inference.c:80-84, unit mass
    return 0.5 * s


def eps_search(om, cells, q, lj, p0, h=1e-5):
    """(eps, dist) of find_reasonable_epsilon from (cells, q) with log-joint lj and momentum p0.  dist: the smallest |log-ratio - threshold| over
    the comparisons made -- the log-ratio with ln 0.5 for the direction a, then a * log-ratio with -a ln 2 (-ln 2 while doubling, +ln 2 while
    halving) at every test of the loop; a log-ratio of -inf (a divergent or non-finite trial) is infinitely far from any of them."""
    q, p0 = np.asarray(q, dtype=np.float64), np.asarray(p0, dtype=np.float64)
    h0 = -lj + _kinetic(p0)

    def log_ratio(eps):
        q1, p1, div = om.leapfrog(cells, q, p0, eps, 1, h)
        if div: return -INF
        lj1 = om.log_joint_at(cells, q1)
        if not math.isfinite(lj1): return -INF
        return h0 - (-lj1 + _kinetic(p1))

    eps = 1.0
    lr = log_ratio(eps)
    ln_half, ln2 = math.log(0.5), math.log(2.0)
    dist = abs(lr - ln_half)
    a = 1.0 if lr > ln_half else -1.0
    iters = 0
    while True:
        dist = min(dist, abs(a * lr - (-a * ln2)))      # a lr against -a ln 2: lr > -ln 2 goes on doubling (a = 1), lr < -ln 2 goes on halving (a = -1)
        if not a * lr > -a * ln2: break
        eps *= 2.0 if a > 0.0 else 0.5
        lr = log_ratio(eps)
        iters += 1
        if iters > 100 or not (1e-12 <= eps <= 1e12): break
        if a > 0.0 and lr == -INF:
            eps /= 2.0
            break
    return min(max(eps, 1e-6), 1e3), dist


def hmc_replay(om, seed, C, nw, ns, cfg, chain0=0):
    """hmc_chain of chains chain0 .. chain0 + C - 1, one transition at a time.  cfg: oracle.HmcConfig (adapt_mass off).  Returns
    (draws [ns][d][C], dist [nw + ns][C], search [C]): dist = |u - alpha| of every transition, +inf where alpha == 1 (every u accepts) or the
    transition diverged (u is not consulted); search = eps_search's distance, +inf where the step size was given."""
    assert not cfg.adapt_mass and om.d > 0
    d, T = om.d, nw + ns
    l, h, target = max(int(cfg.n_leapfrog), 1), cfg.finite_diff_eps, cfg.target_accept
    draws = np.zeros((ns, d, C))
    dist = np.full((T, C), INF)
    search = np.full(C, INF)
    for c in range(C):
        chain = chain0 + c
        cells, acc, _ = om.run_prior(seed, chain, 0, RNG_PRIOR)
        cells = cells.copy()
        q = np.ascontiguousarray(cells[om.f64_sites]).view(np.float64).copy()
        lj = acc[0] + acc[1] + acc[2]
        if not math.isnan(cfg.init_step_size): eps0 = cfg.init_step_size
        else:
            p0, _ = orc.hmc_momentum(seed, chain, 0, d, purpose=RNG_EPS)
            eps0 = om.find_reasonable_epsilon(cells, q, lj, p0, h)
            e2, search[c] = eps_search(om, cells, q, lj, p0, h)
            assert e2 == eps0, (chain, e2, eps0)
        eps, frozen, alphas = eps0, None, []
        for it in range(T):
            if it < nw: e = eps
            else:
                if frozen is None: frozen = orc.dual_averaging(eps0, target, alphas)[2] if nw > 0 else eps
                e = frozen
            p0, u = orc.hmc_momentum(seed, chain, it, d, purpose=RNG_HMC)
            qo, ljo, accepted, alpha, div = om.hmc_transition(cells, q, lj, e, l, p0, u, h)
            if not div and alpha != 1.0: dist[it, c] = abs(u - alpha)
            if accepted:
                q, lj = qo.copy(), ljo
                cells[om.f64_sites] = q.view(np.int64)
            if it < nw:
                alphas.append(alpha)
                eps = orc.dual_averaging(eps0, target, alphas)[0]
            else:
                draws[it - nw, :, c] = q
    return draws, dist, search
