"""The exact Gibbs moves of the discrete sites (fugue_amd/csrc/fg_gibbs.hip, fg_gibbs_plan.h) restated in numpy: test infrastructure.

One sweep visits the listed sites in order; for site i it scores the trace at every value of the support through a scorer handed in
(`oracle_scorer`: oracle.run_score; on the device tests a twin engine's log_joint), folds the maximum from -inf with fmax, forms
w_k = exp(l_k - m) (+0.0 for NaN), their running sums in index order, x = u T with u the (i + 1)-th uniform of the stream
(seed, chain, t, 13), and picks the smallest k with x < s_k, else the largest k with w_k > 0.  `margin` is, per (site, chain), the
distance of x from the nearest running sum in units of (2 K + 3) 2^-52 T: the bound within which two evaluations whose exp differ by
2 ulp and whose K-term sums and one product round differently can disagree on a pick.  No bound here comes from a device's output."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from oracle import oracle as orc

EPS = 2.0 ** -52
ULP_EXP = 1.0                                            # tests/grid_restatement.py: ocml's, glibc's and numpy's stated bound for the f64 exp
RNG_GIBBS = 13                                           # FG_RNG_GIBBS (fg_ir.h)
K_CAP, COUNTS = 4096, 4                                  # FG_GIBBS_K_CAP, FG_GIBBS_COUNTS (include/fugue_amd.h)
MOVED, STUCK, NAN_CELLS, NEG_INF_CELLS = range(4)
POOL_THREADS = 256                                       # fg_chain_pool.h


def layout(sites):
    """sites: [(site, lo, K)] -> cell0 of each and the number of cells (fg_gibbs_plan)"""
    cell0, n = [], 0
    for _, _, K in sites:
        cell0.append(n)
        n += K
    return cell0, n


def oracle_uniform(seed: int):
    """u(chains, t, i): the (i + 1)-th fg_rng_u01 of the stream (seed, chain, t, 13) for every global chain id of `chains`"""
    L = orc.lib()

    def u(chains, t, i):
        out = np.empty(len(chains))
        for n, c in enumerate(chains):
            s = orc.stream(seed, int(c), int(t), RNG_GIBBS)
            for _ in range(i + 1):
                v = L.orc_stream_u01(C.byref(s))
            out[n] = v
        return out
    return u


def oracle_scorer(om):
    """score(cells [S][C]) -> (prior + likelihood) + factors of oracle.run_score per column; equal columns are scored once"""
    memo = {}

    def score(cells):
        cells = np.ascontiguousarray(cells.T)
        out = np.empty(cells.shape[0])
        for c, col in enumerate(cells):
            key = col.tobytes()
            if key not in memo:
                acc, _ = om.run_score(col)
                memo[key] = (acc[0] + acc[1]) + acc[2]
            out[c] = memo[key]
        return out
    return score


def sweep(cells, sites, score, uniform, t: int, chain0: int = 0):
    """One sweep of every column of cells [S][C] (int64; not modified).  sites: [(site, lo, K)].  Returns a dict: cells (after), scores
    and cond [n_cells][C] (cond NaN at a stuck site), picks [G][C] (-1: stuck), stuck [G][C], counts [G][4], margin [G][C] (inf: stuck)."""
    cells = np.array(cells, dtype=np.int64)
    S, Cn = cells.shape
    cell0, n_cells = layout(sites)
    chains = chain0 + np.arange(Cn)
    scores, cond = np.empty((n_cells, Cn)), np.empty((n_cells, Cn))
    picks, stuck_all = np.empty((len(sites), Cn), dtype=np.int64), np.zeros((len(sites), Cn), dtype=bool)
    counts, margin = np.zeros((len(sites), COUNTS), dtype=np.int64), np.full((len(sites), Cn), np.inf)
    for i, (site, lo, K) in enumerate(sites):
        old = cells[site].copy()
        l = np.empty((K, Cn))
        for k in range(K):
            cells[site] = lo + k
            l[k] = score(cells)
        m = np.full(Cn, -np.inf)
        for k in range(K):
            m = np.fmax(m, l[k])                             # NaN never wins
        stuck = np.isinf(m)
        with np.errstate(invalid="ignore", over="ignore"):
            w = np.where(np.isnan(l), 0.0, np.exp(l - m[None]))
        s = np.empty((K, Cn))
        s[0] = w[0]
        for k in range(1, K):
            s[k] = s[k - 1] + w[k]
        T = s[K - 1]
        u = uniform(chains, t, i)
        x = u * T
        below = x[None] < s
        first = np.where(below.any(axis=0), np.argmax(below, axis=0), -1)
        last = (K - 1) - np.argmax((w > 0.0)[::-1], axis=0)
        pick = np.where(first >= 0, first, last)
        pick = np.where(stuck, -1, pick)
        with np.errstate(invalid="ignore", divide="ignore"):
            p = w / T[None]
            mg = np.min(np.abs(x[None] - s), axis=0) / ((2 * K + 3) * EPS * T)
        cells[site] = np.where(stuck, old, lo + pick)
        scores[cell0[i]:cell0[i] + K] = l
        cond[cell0[i]:cell0[i] + K] = np.where(stuck[None], np.nan, p)
        picks[i], stuck_all[i] = pick, stuck
        margin[i] = np.where(stuck, np.inf, mg)
        counts[i] = [int(np.sum(~stuck & (cells[site] != old))), int(stuck.sum()), int(np.isnan(l).sum()), int(np.sum(l == -np.inf))]
    return dict(cells=cells, scores=scores, cond=cond, picks=picks, stuck=stuck_all, counts=counts, margin=margin)


def pool_sum(v):
    """fg_chain_pool.h's fixed tree over the last axis with merge = a + b: for stride s = 1, 2, 4, ... element i (a multiple of 2 s)
    takes in element i + s when it exists"""
    v = np.array(v, dtype=np.float64)
    n = v.shape[-1]
    s = 1
    while s < n:
        idx = np.arange(0, n - s, 2 * s)
        v[..., idx] = v[..., idx] + v[..., idx + s]
        s *= 2
    return v[..., 0]


def cond_tolerance(K: int) -> float:
    """relative, between p_k of two evaluations on the same scores: 2 ulp between two exp of at most ULP_EXP each, K - 1 additions, one division"""
    return (K + 2) * EPS


# ---- the invariance law -------------------------------------------------------------------------------------------------------------------
LAW_CHAINS, LAW_SEED = 16384, 7


def law_program_ab():
    """a ~ Bernoulli(0.3), b ~ Categorical([0.2, 0.3, 0.5]), y = 1.2 ~ Normal(a + b, 1): both sites in one likelihood term"""
    from fugue_amd import model as M
    P = M.Program()
    a = P.sample(M.addr("a"), M.Bernoulli(0.3))
    b = P.sample(M.addr("b"), M.Categorical([0.2, 0.3, 0.5]))
    P.observe(M.addr("y"), M.Normal(a + b, 1.0), 1.2)
    return P


LAW_SELECT_MEANS = [[-1.0, 0.5, 2.0], [0.0, 1.5, 3.0]]


def law_program_select():
    """i ~ Categorical([0.4, 0.6]), j ~ Categorical([0.5, 0.25, 0.25]), y = 0.8 ~ Normal(select(i, [select(j, row 0), select(j, row 1)]), 1)"""
    from fugue_amd import model as M
    P = M.Program()
    i = P.sample(M.addr("i"), M.Categorical([0.4, 0.6]))
    j = P.sample(M.addr("j"), M.Categorical([0.5, 0.25, 0.25]))
    P.observe(M.addr("y"), M.Normal(M.select(i, [M.select(j, row) for row in LAW_SELECT_MEANS]), 1.0), 0.8)
    return P


def _normal_pdf(x, mu):
    return math.exp(-0.5 * (x - mu) ** 2) / math.sqrt(2.0 * math.pi)


def law_exact(which: str) -> np.ndarray:
    """the exact joint mass [K_0][K_1] of the two sites (sorted site order: a, b / i, j)"""
    if which == "ab":
        pa, pb = [0.7, 0.3], [0.2, 0.3, 0.5]
        j = np.array([[pa[a] * pb[b] * _normal_pdf(1.2, a + b) for b in range(3)] for a in range(2)])
    else:
        pi, pj = [0.4, 0.6], [0.5, 0.25, 0.25]
        j = np.array([[pi[i] * pj[k] * _normal_pdf(0.8, LAW_SELECT_MEANS[i][k]) for k in range(3)] for i in range(2)])
    return j / j.sum()


def law_start(which: str, n: int = LAW_CHAINS, seed: int = LAW_SEED) -> np.ndarray:
    """cells [2][n] drawn from the exact joint with numpy"""
    exact = law_exact(which)
    flat = np.random.default_rng(seed).choice(exact.size, size=n, p=exact.reshape(-1))
    return np.stack([flat // exact.shape[1], flat % exact.shape[1]]).astype(np.int64)


def judge_law(which: str, cells_after):
    """every joint cell's frequency after one sweep lies within 5 binomial standard errors of the exact mass"""
    exact = law_exact(which)
    n = cells_after.shape[1]
    freq = np.zeros_like(exact)
    np.add.at(freq, (cells_after[0], cells_after[1]), 1.0)
    freq /= n
    se = np.sqrt(exact * (1.0 - exact) / n)
    z = np.abs(freq - exact) / se
    print(f"law {which}: largest deviation {z.max():.2f} standard errors over {exact.size} joint cells")
    assert np.all(z <= 5.0), (freq, exact, z)


LAW_SITES = [(0, 0, 2), (1, 0, 3)]


# ---- scores and picks on tests/models.all_dists_model: shared by the CPU test (oracle scores) and the device test -------------------------------
PICK_SEED = 11                                           # fixed by tests/test_gibbs_cpu.py's margin (a factor 1000 to spare) before a device sees it
PICK_SHAPES = (1, 5, 65, 130)
PICK_SWEEPS = 2
PICK_ADDRS = ("be", "cat", "cat#2", "bi", "du")
PICK_SUPPORT = {"be": (0, 1), "cat": (0, 1), "cat#2": (0, 2), "bi": (0, 10), "du": (-2, 5)}


def pick_sites(site_names):
    return [(site_names.index(a), PICK_SUPPORT[a][0], PICK_SUPPORT[a][1] - PICK_SUPPORT[a][0] + 1) for a in PICK_ADDRS]
