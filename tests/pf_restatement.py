"""A plain restatement of one step of the bootstrap particle filter (crates/fugue-wasm/src/pf.rs:107-172 on the engine's Philox streams),
built from what oracle/oracle.py exports: `sample_dist_many` for the Normal draws of the streams (seed, i, t, 11), `sample_dist` on
`stream(seed, 0, t, 12)` for the resampling uniform (the way fugue_amd/abc.py::_uniforms takes its uniforms), `logpdf`, `log_sum_exp`,
`systematic_indices`, `ess_particles`.

Two summation modes:
  "seq"   the reference's order: every sum runs over the particles in index order, the cumulative weights are the running sum of
          `systematic_indices` (oracle.log_sum_exp, oracle.ess_particles, oracle.systematic_indices themselves);
  "plan"  the order fugue_amd/csrc/fg_pf_plan.h states for the kernel: `plan_sum` and `plan_cumsum` below.

The Normal log-density of a whole population is `normal_logpdf`, the operations of oracle.logpdf("Normal", ...) in numpy (IEEE: the
same bits; tests/test_pf_cpu.py pins it to oracle.logpdf).  Used by tests/test_pf_cpu.py, tests/test_gpu_pf.py and tools/bench_pf.py."""
from __future__ import annotations

import math

import numpy as np

from oracle import oracle as orc

RNG_PF, RNG_PF_RESAMPLE = 11, 12
LN_2PI = 1.8378770664093456                              # distribution.rs:206
EPS = 2.0 ** -52                                         # one ulp, relative, at most (tests/smc_judge.py's EPS); one rounding is EPS / 2
ULP_EXP, ULP_LOG = 1.0, 1.0                               # ocml's stated bounds for the f64 exp and log (and glibc's), in ulp
WAVE, MAX_THREADS, TARGET_PER_THREAD = 64, 1024, 4       # fg_pf_plan.h
N_CAP = (160 * 1024 - 1024) // (3 * 8) // 2 * 2


# ---- the plan (fg_pf_plan.h) -------------------------------------------------------------------------------------------------------
def plan(n: int):
    """-> (threads, per_thread, steps_per_launch)"""
    threads = WAVE
    while threads < MAX_THREADS and threads * TARGET_PER_THREAD < n:
        threads *= 2
    return threads, -(-n // threads), max(1, min(256, (1 << 17) // n))


def plan_depth(n: int) -> int:
    """additions on the longest path of `plan_sum`: a thread's slots, the six halvings of a wave, the waves in sequence"""
    threads, per, _ = plan(n)
    return per + 6 + threads // WAVE


def plan_sum(v) -> float:
    """the kernel's sum of one term per particle"""
    v = np.asarray(v, dtype=np.float64)
    threads, per, _ = plan(v.size)
    pad = np.zeros(threads * per)
    pad[:v.size] = v
    acc = np.zeros(threads)
    for row in pad.reshape(per, threads):                # thread t: particles t, t + threads, ... in sequence, from +0.0
        acc = acc + row
    a = acc.reshape(threads // WAVE, WAVE)
    for s in (32, 16, 8, 4, 2, 1):                       # lane l: v[l] + v[l ^ s]
        a = a[:, :s] + a[:, s:2 * s]
    tot = 0.0
    for w in a[:, 0]:                                    # wave totals in wave order, from +0.0
        tot = tot + float(w)
    return tot


def plan_cumsum(w) -> np.ndarray:
    """the kernel's inclusive scan of the weights"""
    w = np.asarray(w, dtype=np.float64)
    n = w.size
    threads, per, _ = plan(n)
    pad = np.zeros(threads * per)
    pad[:n] = w
    local = np.cumsum(pad.reshape(threads, per), axis=1)     # thread t: its run in index order (np.cumsum is sequential)
    tot = local[:, -1].reshape(threads // WAVE, WAVE)
    incl = tot.copy()
    for o in (1, 2, 4, 8, 16, 32):                           # lane l adds lane l - o
        nxt = incl.copy()
        nxt[:, o:] = incl[:, o:] + incl[:, :-o]
        incl = nxt
    excl = np.concatenate([np.zeros((incl.shape[0], 1)), incl[:, :-1]], axis=1)
    woff = np.zeros(incl.shape[0])
    run = 0.0
    for k in range(incl.shape[0]):                           # a wave's offset: the totals of the waves before it, in order, from +0.0
        woff[k] = run
        run = run + float(incl[k, -1])
    off = (woff[:, None] + excl).reshape(threads)
    return (off[:, None] + local).reshape(-1)[:n]


def seq_sum(v) -> float:
    v = np.asarray(v, dtype=np.float64)
    return float(np.cumsum(v)[-1]) if v.size else 0.0        # np.cumsum adds in index order (np.sum does not)


# ---- the pieces of a step ----------------------------------------------------------------------------------------------------------
def clamp_params(n, prior_sig, sig_step, sig_obs, ess_threshold):
    """pf.rs:82-94"""
    return (min(max(int(n), 2), 5000), max(float(prior_sig), 1e-6), max(float(sig_step), 1e-6), max(float(sig_obs), 1e-6),
            min(max(float(ess_threshold), 0.0), 1.0))


def normal_draws(seed: int, n: int, t: int, sigma: float) -> np.ndarray:
    """draw i: one Normal(0, sigma) from the fresh stream (seed, i, t, 11); t = 0 the initial population"""
    return orc.sample_dist_many("Normal", [0.0, sigma], seed, n, 0, t, RNG_PF)[0].copy()


def resample_uniform(seed: int, t: int) -> float:
    return orc.sample_dist("Uniform", [0.0, 1.0], orc.stream(seed, 0, t, RNG_PF_RESAMPLE))


def normal_logpdf(x, mu: float, sigma: float) -> np.ndarray:
    """oracle.logpdf("Normal", x_i, [mu, sigma]) for every i: distribution.rs:189-208"""
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        z = (x - mu) / sigma
        lp = -0.5 * z * z - math.log(sigma) - 0.5 * LN_2PI
    return np.where(np.isfinite(x), lp, -np.inf)


def log_sum_exp(lw, mode: str) -> float:
    if mode == "seq":
        return orc.log_sum_exp(lw)
    m = float(np.max(lw))
    if m == -np.inf:
        return -np.inf
    se = plan_sum(np.exp(lw - m))
    return -np.inf if se == 0.0 else m + math.log(se)


def normalize(lw, lse: float, mode: str) -> np.ndarray:
    """normalize_particles (smc.rs:719-753)"""
    n = lw.size
    if lse == -np.inf:
        return np.full(n, 1.0 / n)
    w = np.exp(lw - lse)
    s = seq_sum(w) if mode == "seq" else plan_sum(w)
    return w / s if s > 0.0 else w


def systematic(w, U: float, mode: str):
    """-> (parents, the cumulative weights the mode walks)"""
    n = w.size
    if mode == "seq":
        return orc.systematic_indices(w, U), np.cumsum(w)
    cum = plan_cumsum(w)
    thr = U / n + np.arange(n, dtype=np.float64) / n
    return np.minimum(np.searchsorted(cum, thr, side="left"), n - 1).astype(np.int64), cum


def thresholds(n: int, U: float) -> np.ndarray:
    return U / n + np.arange(n, dtype=np.float64) / n        # smc.rs:258,264


def carried(w, resampled: bool) -> np.ndarray:
    """the log-weights a step leaves: pf.rs:145 / :155"""
    if resampled:
        return np.zeros(w.size)
    with np.errstate(all="ignore"):
        return np.log(np.maximum(w * float(w.size), 1e-300))


def step_from(prev, lw_prev, sig_step, sig_obs, threshold, seed, t, obs, mode="seq", propagated=None):
    """One step (pf.rs:107-172) into time t from positions `prev` and carried log-weights `lw_prev` -> dict of every intermediate.
    propagated: take these positions after the transition instead of prev + draw (judging a device step from the device's own arrays)."""
    prev = np.asarray(prev, dtype=np.float64)
    n = prev.size
    s = (lambda v: seq_sum(v)) if mode == "seq" else plan_sum
    draw = normal_draws(seed, n, t, sig_step)
    prop = prev + draw if propagated is None else np.asarray(propagated, dtype=np.float64)
    score = normal_logpdf(prop, obs, sig_obs)
    with np.errstate(all="ignore"):
        lw = np.asarray(lw_prev, dtype=np.float64) + score
    lse = log_sum_exp(lw, mode)
    log_z_inc = lse - math.log(n)
    w = normalize(lw, lse, mode)
    ess = orc.ess_particles(w) if mode == "seq" else 1.0 / plan_sum(w * w)       # smc.rs:230-233
    ess_frac = ess / n
    mean = s(w * prop)
    d = prop - mean
    var = s(w * (d * d))
    resampled = bool(ess_frac < threshold)
    U = resample_uniform(seed, t)
    if resampled:
        parents, cum = systematic(w, U, mode)
        post = prop[parents]
    else:
        parents, cum, post = np.arange(n, dtype=np.int64), None, prop.copy()
    return dict(prev=prev, draw=draw, propagated=prop, score=score, lw=lw, lse=lse, log_z_inc=log_z_inc, weights=w, ess_frac=ess_frac, mean=mean,
                var=var, resampled=resampled, U=U, parents=parents, cum=cum, posterior=post, lw_next=carried(w, resampled))


class Filter:
    """The filter as a host object: ParticleFilter's interface, the restatement's arithmetic."""

    def __init__(self, n, prior_sig, sig_step, sig_obs, ess_threshold, seed, mode="seq", clamp=True):
        if clamp:
            n, prior_sig, sig_step, sig_obs, ess_threshold = clamp_params(n, prior_sig, sig_step, sig_obs, ess_threshold)
        self.n, self.sig_step, self.sig_obs, self.threshold, self.seed, self.mode = n, sig_step, sig_obs, ess_threshold, int(seed), mode
        self.x = normal_draws(self.seed, n, 0, prior_sig)        # pf.rs:86-88
        self.lw = np.zeros(n)
        self.log_z, self.steps = 0.0, 0

    def set_sig_obs(self, sig_obs):
        self.sig_obs = max(float(sig_obs), 1e-6)

    def step(self, obs):
        if not math.isfinite(obs):
            raise ValueError("a non-finite observation (Normal::new(obs, .).unwrap() panics: pf.rs:121)")
        r = step_from(self.x, self.lw, self.sig_step, self.sig_obs, self.threshold, self.seed, self.steps + 1, float(obs), self.mode)
        self.x, self.lw = r["posterior"], r["lw_next"]
        self.log_z += r["log_z_inc"]
        self.steps += 1
        return r

    def log_evidence(self):
        return self.log_z

    def t(self):
        return self.steps


# ---- the inputs of the step-parity tests (tests/test_pf_cpu.py checks them here, tests/test_gpu_pf.py runs them on the device) ----------
PARITY_SIZES = (2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4999, 5000)   # a wave, every workgroup size of the plan and their neighbours, the reference's cap
PARITY_STEPS = 8


def parity_case(n: int, b: int = 0):
    """filter b of the case -> (prior_sig, sig_step, sig_obs, ess_threshold, seed, observations): the reference's test scenario (wasm.rs:69-86) at n particles.
    Two and three particles cannot reach an ESS fraction below 1 / n: their threshold sits between 1 / n and 1, off the lattice of
    values a population of equal or single survivors takes."""
    return 1.6, 0.7, 0.6, (0.5 if n > 3 else 0.8), 100 + n + 1000 * b, [0.3 * t for t in range(PARITY_STEPS)]


PARITY_FILTERS = 2


# ---- the 1e-300 floor of the carried log-weights (pf.rs:155) ---------------------------------------------------------------------------
# Step 1 (threshold 0: never resampled) sees an observation 60 prior sigmas away: most particles get w_i n < 1e-300 and carry ln(1e-300).
# Step 2's observation lies on the OTHER side of the population, so the floored particles (x < 0.2) are the likely ones and the one
# survivor of step 1 (x near 3) is not: the floored particles regain representable weights -- they hold the whole mass -- and
# log_z_inc = ln(1e-300) + ... reads the floor's constant directly.  A second observation near the first would leave every floored
# particle at weight exactly 0 (exp underflows) and the floor unseen.
FLOOR_CASE = dict(n=256, prior_sig=1.0, sig_step=0.5, sig_obs=0.5, threshold=0.0, seed=8, obs=(60.0, -30.0))


def floor_step_two(w1, x1, propagated=None):
    """Step 2 of FLOOR_CASE from step 1's weights and positions (the restatement's or the device's), restated twice: with the floored
    carry of pf.rs:155 and with ln(w n) unfloored (-inf for w = 0) -> (floored mask, step with the floor, step without, the carried
    log-weights with the floor)."""
    c = FLOOR_CASE
    w1 = np.asarray(w1, dtype=np.float64)
    floored = w1 * c["n"] < 1e-300
    lw_floor = carried(w1, False)
    with np.errstate(all="ignore"):
        lw_none = np.log(w1 * float(c["n"]))
    args = (c["sig_step"], c["sig_obs"], c["threshold"], c["seed"], 2, c["obs"][1])
    return (floored, step_from(x1, lw_floor, *args, mode="seq", propagated=propagated), step_from(x1, lw_none, *args, mode="seq", propagated=propagated), lw_floor)


def assert_floor_is_seen(floored, with_floor, without, lw_floor):
    """the inputs make step 2 depend on the floor: floored particles exist, every one has a weight above zero in step 2, and log_z_inc and
    the weights with the floor differ from those without by far more than the bounds of `tolerances`"""
    tol = tolerances(with_floor, lw_floor, same_math=False)
    n = floored.size
    assert 0 < floored.sum() < n
    assert np.all(with_floor["weights"][floored] > 0.0) and with_floor["weights"][floored].sum() > 0.5
    assert abs(with_floor["log_z_inc"] - without["log_z_inc"]) > 1.0 > 1e6 * tol["log_z_inc"]
    rel = np.abs(with_floor["weights"] - without["weights"])[floored] / with_floor["weights"][floored]
    assert np.all(rel > 1e6 * tol["weights_rel"])
    return tol


# ---- error bounds (derived, not fitted) ------------------------------------------------------------------------------------------
def order_eps(n: int) -> float:
    """Two sums of the same n non-negative terms, one in index order and one in the plan's order, differ by at most this, relative to
    the sum: a sequential sum is within (n - 1) roundings of the exact one (Higham, Accuracy and Stability, 4.2), a tree of depth d
    within d roundings; a rounding is EPS / 2, and the first-order bound is inflated by 1 / (1 - n EPS)."""
    return 0.5 * EPS * ((n - 1) + plan_depth(n)) / (1.0 - n * EPS)


def tolerances(r, lw_prev, same_math: bool):
    """Bounds on |device - restatement| for the step `r` = step_from(...) taken from the device's own positions and the carried
    log-weights `lw_prev` the host recomputed from the device's previous weights.  same_math: both sides run the SAME exp / log (the two
    modes of this file against each other) -- the ulp terms of the transcendentals and of the carried log-weights drop out.
      carried log-weights: ln(max(w n, 1e-300)) by two logs of <= ULP_LOG ulp each: dc_i = 2 ULP_LOG EPS |lw_prev_i| (0 after a
        resampling step: the value is exactly 0);
      lw_i = lw_prev_i + score_i (the score is the same IEEE operations on the same bits on both sides: 0): dl_i = dc_i + EPS |lw_i|;
      log-sum-exp is 1-Lipschitz in the maximum norm: Dl = max_i dl_i moves it by at most Dl; its terms exp(lw_i - max) carry
        2 ULP_EXP EPS (two implementations), their sum order_eps(n), the log of the sum turns relative into absolute error and adds
        2 ULP_LOG EPS ln n (the sum lies in [1, n]), the additions max + . and . - ln n a rounding each per side;
      weights: w_i = exp(lw_i - lse) / sum: the argument moves by dl_i + (bound of lse) + EPS |lw_i - lse| (relative error of w_i), the
        exp adds 2 ULP_EXP EPS, the sum inherits the largest relative error of its terms plus order_eps(n), the division a rounding per side;
      sum w^2: twice the relative error of w, a rounding per square and side, order_eps(n); 1 / . and / n two roundings per side;
      mean = sum w x (x the same bits on both sides): relative to sum |w x|: the error of w, the products, order_eps(n);
      var = sum w (x - mean)^2: each d_i moves by the bound of the mean plus a rounding, t_i = w_i d_i^2."""
    n = r["weights"].size
    lw, w, x = r["lw"], r["weights"], r["propagated"]
    fin = np.isfinite(lw)
    k_t = 0.0 if same_math else 1.0
    lwp = np.asarray(lw_prev, dtype=np.float64)
    dc = k_t * 2.0 * ULP_LOG * EPS * np.abs(np.where(np.isfinite(lwp), lwp, 0.0))
    dl = np.where(fin, dc + k_t * EPS * np.abs(np.where(fin, lw, 0.0)), 0.0)
    Dl = float(dl.max())
    oe = order_eps(n)
    lse = r["lse"]
    if not math.isfinite(lse):
        t_inc, Rw = 0.0, 0.0                                  # -inf on both sides, uniform weights 1 / n: the same bits
    else:
        t_lse = Dl + k_t * 2.0 * ULP_EXP * EPS + oe + 2.0 * ULP_LOG * EPS * math.log(n) + EPS * abs(lse)
        t_inc = t_lse + EPS * abs(r["log_z_inc"])
        arg = np.where(fin, dl + t_lse + EPS * np.abs(np.where(fin, lw - lse, 0.0)), 0.0)
        A = float(arg[w > 0.0].max()) if (w > 0.0).any() else 0.0
        Rw = 2.0 * (A + k_t * 2.0 * ULP_EXP * EPS) + oe + EPS
    Ress = 2.0 * Rw + EPS + oe + 2.0 * EPS
    awx = float(np.abs(w * x).sum())
    t_mean = (Rw + EPS + oe) * awx * (1.0 + 8.0 * EPS)
    d = x - r["mean"]
    t_var = (Rw + 3.0 * EPS + oe) * float((w * d * d).sum()) + 2.0 * (t_mean + EPS * float(np.abs(d).max())) * float((w * np.abs(d)).sum())
    return dict(log_z_inc=t_inc, weights_rel=Rw, ess_frac_rel=Ress, mean=t_mean, var=t_var * (1.0 + 8.0 * EPS))


def parent_band(r_cum_seq, thr, n: int):
    """slots whose threshold lies within (n - 1) EPS, relative, of a cumulative weight of the sequential order: where the plan's scan
    may put the boundary one index away"""
    k = np.minimum(np.searchsorted(r_cum_seq, thr, side="left"), n - 1)
    near = np.zeros(n, dtype=bool)
    for kk in (np.maximum(k - 1, 0), k):
        near |= np.abs(r_cum_seq[kk] - thr) <= (n - 1) * EPS * np.maximum(np.abs(thr), np.abs(r_cum_seq[kk]))
    return near


def kalman(obs, prior_sig, sig_step, sig_obs):
    """the exact filter of the model: -> (log-evidence, filtering mean and variance after the last observation)"""
    m, P, lz = 0.0, prior_sig ** 2, 0.0
    for y in obs:
        P = P + sig_step ** 2
        S = P + sig_obs ** 2
        lz += -0.5 * (math.log(2.0 * math.pi * S) + (y - m) ** 2 / S)
        K = P / S
        m, P = m + K * (y - m), (1.0 - K) * P
    return lz, m, P
