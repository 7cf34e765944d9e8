"""Predictive checks and WAIC / IS-LOO of a weighted population (fugue_amd/csrc/fg_wpop_eval_plan.h) restated in Python:
the categories and their unit sums in Python ints, the moments of the replicated statistics and every sum of doubles over the fixed tree
on the particle index (tests/wpop_restatement.py's), the statistics and the cell conversion of tests/ppc_restatement.py, math.exp /
math.log (glibc's, like the host build).  No numpy arithmetic on the path of a compared figure.  Also the exact references (mpmath), the
error bounds the tests hold the exp-based figures to, and the inputs the CPU and GPU tests share."""
import math

import numpy as np

from tests import ppc_restatement as PR
from tests import wpop_restatement as WR

INF, NAN = float("inf"), float("nan")
LT, EQ, GT, CNAN = range(4)
FIGURE_NAMES = ("lppd", "mean_ll", "p_waic", "elpd_waic", "elpd_loo", "p_loo", "is_ess", "max_weight")
WORD_NAMES = ("W", "W_fin", "W2", "mean", "ssd", "n_used", "mx", "mn", "sp", "sn", "sn2", "tmax")
COUNT_NAMES = ("n_fin", "n_neg_inf", "n_pos_inf", "n_nan")
EXP_FIGURES = ("lppd", "elpd_loo", "is_ess", "max_weight")
U = 2.0 ** -53                       # the unit roundoff
E_EXP = 2.0 ** -52                   # exp within one ulp: glibc's (below 1 ulp) and ocml's (1 ulp) both


def bits(v):
    return WR.bits(v)


def category(T, t_obs):
    if T != T or t_obs != t_obs:
        return CNAN
    return LT if T < t_obs else (EQ if T == t_obs else GT)


def p_values(u):
    """[p_ge, p_gt, p_mid] from the four unit sums: integers first, one division each"""
    den = u[LT] + u[EQ] + u[GT]
    if den == 0:
        return [NAN, NAN, NAN]
    return [float(u[GT] + u[EQ]) / float(den), float(u[GT]) / float(den), float(2 * u[GT] + u[EQ]) / float(2 * den)]


def checks(cells, vtypes, checks_, w):
    """cells uint64 [n_rows][N], checks_ [(rows, mask, observed)], w [N] -> dict(t_obs [n_slots], T [n_slots][N], units [n_slots][4],
    counts [n_slots][4], moments [n_slots][6], p [n_slots][3])"""
    q, T_units, _, _ = WR.units(w)
    q = [int(v) for v in q]
    t_obs = PR.observed_stats(checks_)
    T = PR.statistics_table(np.ascontiguousarray(cells)[None], vtypes, checks_)[0]
    units, counts, moments, p = [], [], [], []
    for k, ob in enumerate(t_obs):
        u, c = [0, 0, 0, 0], [0, 0, 0, 0]
        for t, qi in zip(T[k], q):
            g = category(t, ob)
            u[g] += qi
            c[g] += 1 if qi > 0 else 0
        assert sum(u) == T_units
        units.append(u)
        counts.append(c)
        moments.append(WR.moments(T[k], w))
        p.append(p_values(u))
    return dict(t_obs=t_obs, T=T, units=units, counts=counts, moments=moments, p=p)


def weight(w):
    return w if WR.good(w) and w > 0.0 else 0.0


def kind(x):
    return 3 if x != x else (2 if x == INF else (1 if x == -INF else 0))


def add(a, b):
    return a + b


def loglik_row(x, w, W=None):
    """one row -> (words [12], counts [4], figures [8], arg_tmax)"""
    x, w = [float(v) for v in x], [float(v) for v in w]
    if W is None:
        W = WR.tree([weight(a) for a in w], add)
    c = [0, 0, 0, 0]
    fin = []
    for a, b in zip(w, x):
        if weight(a) > 0.0:
            c[kind(b)] += 1
            if kind(b) == 0:
                fin.append(b)
    lw = [WR.leaf_weight(a, b) for a, b in zip(w, x)]
    Wf, mean, ssd, n = WR.tree([(a, b, 0.0, 1) if a > 0.0 else (0.0, 0.0, 0.0, 0) for a, b in zip(lw, x)], WR.merge)
    assert n == c[0]
    W2 = WR.tree([a * a if a > 0.0 else 0.0 for a in lw], add)
    mx, mn = (max(fin), min(fin)) if fin else (0.0, 0.0)
    if fin and mx == 0.0:                # the key order: +0.0 above -0.0
        mx = 0.0 if any(WR.bits(v) == 0 for v in fin) else -0.0
    if fin and mn == 0.0:
        mn = -0.0 if any(WR.bits(v) != 0 for v in fin if v == 0.0) else 0.0
    tp = [a * math.exp(b - mx) if a > 0.0 else 0.0 for a, b in zip(lw, x)]
    tn = [a * math.exp(mn - b) if a > 0.0 else 0.0 for a, b in zip(lw, x)]
    sp, sn, sn2 = WR.tree(tp, add), WR.tree(tn, add), WR.tree([t * t for t in tn], add)
    tmax = max(tn) if tn else 0.0
    words = [W, Wf, W2, mean if n else NAN, ssd if n else NAN, float(n), mx if n else NAN, mn if n else NAN, sp, sn, sn2, tmax]
    return words, c, finish(words, c), (tn.index(tmax) if n else None)


def finish(w, c):
    a, b = c[1], c[2]
    if c[3] > 0 or c[0] == 0:
        return [NAN] * 8
    W, Wf = w[0], w[1]
    lppd = INF if b > 0 else w[6] + math.log(w[8] / W)
    loo = -INF if a > 0 else w[7] - math.log(w[9] / W)
    mean = NAN if (a > 0 and b > 0) else (-INF if a > 0 else (INF if b > 0 else w[3]))
    den = Wf - w[2] / Wf
    p_waic = w[4] / den if (a == 0 and b == 0 and w[5] >= 2.0 and den > 0.0) else NAN
    return [lppd, mean, p_waic, lppd - p_waic, loo, lppd - loo, w[9] * w[9] / w[10] if a == 0 else NAN, w[11] / w[9] if a == 0 else NAN]


def loglik(ll, w):
    """ll [n_sel][N] -> dict(words [n_sel][12], counts [n_sel][4], figures [n_sel][8], arg_tmax [n_sel])"""
    W = WR.tree([weight(float(a)) for a in w], add)
    rows = [loglik_row(r, w, W) for r in np.asarray(ll, dtype=np.float64)]
    return dict(words=[r[0] for r in rows], counts=[r[1] for r in rows], figures=[r[2] for r in rows], arg_tmax=[r[3] for r in rows])


# ---- the exact figures and the bounds ---------------------------------------------------------------------------------------------
def exact_row(x, w):
    """lppd, elpd_loo, is_ess, max_weight of the row's finite participating cells -> dict of floats (and ln_p, ln_n, the two
    logarithms, for the bounds).  With mpmath: every operation at 50 digits.  Without it: math.fsum of the terms in doubles -- the sums
    exact, each term carrying its own three roundings, which `bounds` allows for anyway."""
    part = [(float(a), float(b)) for a, b in zip(w, x) if weight(float(a)) > 0.0]
    fin = [(a, b) for a, b in part if math.isfinite(b)]
    try:
        import mpmath
    except ImportError:
        W = math.fsum(a for a, _ in part)
        mx, mn = max(b for _, b in fin), min(b for _, b in fin)
        sp = math.fsum(a * math.exp(b - mx) for a, b in fin)
        tn = [a * math.exp(mn - b) for a, b in fin]
        sn, sn2 = math.fsum(tn), math.fsum(t * t for t in tn)
        return dict(lppd=mx + math.log(sp / W), elpd_loo=mn - math.log(sn / W), is_ess=sn * sn / sn2, max_weight=max(tn) / sn, ln_p=math.log(sp / W), ln_n=math.log(sn / W))
    mpmath.mp.dps = 50
    part = [(mpmath.mpf(a), b) for a, b in part]
    fin = [(a, mpmath.mpf(b)) for a, b in part if math.isfinite(b)]
    W = sum(a for a, _ in part)
    mx, mn = max(b for _, b in fin), min(b for _, b in fin)
    sp = sum(a * mpmath.exp(b - mx) for a, b in fin)
    tn = [a * mpmath.exp(mn - b) for a, b in fin]
    sn, sn2 = sum(tn), sum(t * t for t in tn)
    return dict(lppd=float(mx + mpmath.log(sp / W)), elpd_loo=float(mn - mpmath.log(sn / W)), is_ess=float(sn * sn / sn2), max_weight=float(max(tn) / sn),
                ln_p=float(mpmath.log(sp / W)), ln_n=float(mpmath.log(sn / W)))


def ceiling(N, exact):
    """(N + 8) 2^-52, what tests/test_gpu_loglik_stream.py holds the chain figures to: relative to max(1, |figure|) for lppd and elpd_loo
    (a figure near -1e4 cannot be held to an absolute 2^-49), relative for is_ess and max_weight.  No bound here is looser."""
    c = (N + 8) * 2.0 ** -52
    return dict(lppd=c * max(1.0, abs(exact["lppd"])), elpd_loo=c * max(1.0, abs(exact["elpd_loo"])), is_ess=c * abs(exact["is_ess"]), max_weight=c * abs(exact["max_weight"]))


def bounds(x, w, exact, e_exp=E_EXP):
    """The error bounds of the exp-based figures of one row, from the inputs alone.  u = 2^-53, L = ceil(log2 N) the depth of the tree,
    D = the largest |x_i - reference point| over the leaves (capped at 746, past which a term is 0), E the relative error of exp.
    A term t_i = fl(w_i fl(exp(fl(x_i - ref)))): the difference is off by at most D u absolutely, which exp turns into a relative
    D u; exp adds E, the product u: (D + 1) u + E.  A tree of depth L over positive terms adds L u: sp and sn are within
    R1 = (L + 1 + D) u + E.  The squared term is within 2 ((D + 1) u + E) + u, so sn2 within R2 = (L + 3 + 2 D) u + 2 E.  W, a tree
    sum of exact leaves: L u; the quotient sp / W: + u.  So
      lppd, elpd_loo (absolute): R1 + (L + 1) u, then log's own ulp 2 u |ln v| and the last addition's u |figure|
      is_ess (relative): 2 R1 + u + R2 + u            max_weight (relative): (D + 1) u + E + R1 + u
    to first order.  Where that is looser than `ceiling` (small N: the D terms) the ceiling holds instead.  -> dict of the four bounds."""
    N = len(x)
    L = max(0, math.ceil(math.log2(N))) if N > 1 else 0
    fin = [float(b) for a, b in zip(w, x) if weight(float(a)) > 0.0 and math.isfinite(float(b))]
    D = min(746.0, max(fin) - min(fin))
    R1 = (L + 1 + D) * U + e_exp
    R2 = (L + 3 + 2 * D) * U + 2 * e_exp
    derived = dict(lppd=R1 + (L + 1) * U + 2 * U * abs(exact["ln_p"]) + U * abs(exact["lppd"]),
                   elpd_loo=R1 + (L + 1) * U + 2 * U * abs(exact["ln_n"]) + U * abs(exact["elpd_loo"]),
                   is_ess=(2 * R1 + R2 + 2 * U) * abs(exact["is_ess"]),
                   max_weight=((D + 2) * U + e_exp + R1) * abs(exact["max_weight"]))
    top = ceiling(N, exact)
    return {n: min(derived[n], top[n]) for n in derived}


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
LL_KINDS = ("normal", "far", "constant", "neg_inf", "pos_inf", "nan", "both_inf", "all_neg_inf", "dead_cells")
LL_FINITE = ("normal", "far", "constant", "dead_cells")


def ll_row(kind_, N, w, seed=0):
    """One log-likelihood row [N].  `dead_cells`: -inf and NaN cells under the zero and bad weights only (no effect)."""
    rng = np.random.default_rng([seed, LL_KINDS.index(kind_), N])
    x = rng.normal(-3.0, 1.0, N)
    live = [i for i in range(N) if weight(float(w[i])) > 0.0]
    at = live[int(rng.integers(0, len(live)))] if live else 0
    if kind_ == "far":                               # exp(x) underflows and exp(-x) overflows without the reference points
        x = -1e4 + rng.normal(0.0, 1.0, N)
    elif kind_ == "constant":
        x = np.full(N, -1.25)
    elif kind_ == "neg_inf":
        x[at] = -np.inf
    elif kind_ == "pos_inf":
        x[at] = np.inf
    elif kind_ == "nan":
        x[at] = np.nan
    elif kind_ == "both_inf":
        x[at] = np.inf
        if len(live) > 1:
            x[live[(live.index(at) + 1) % len(live)]] = -np.inf
    elif kind_ == "all_neg_inf":
        x[:] = -np.inf
    elif kind_ == "dead_cells":
        for j, i in enumerate(i for i in range(N) if weight(float(w[i])) == 0.0):
            x[i] = -np.inf if j % 2 == 0 else np.nan
    return x


def ll_table(kinds, N, w, seed=0):
    return np.ascontiguousarray(np.stack([ll_row(k, N, w, seed + 31 * j) for j, k in enumerate(kinds)]))


WEIGHT_KINDS = ("dirichlet", "uniform", "quarter_zero", "one_heavy", "below_unit", "bad")


def weights(kind_, N, seed=0):
    """-> (w [N], n_bad).  one_heavy: one weight about 1 and the rest tiny; below_unit: a weight below 2^-53 (zero units, but a leaf)."""
    if kind_ == "bad":
        return WR.bad_weights(N, seed)
    if kind_ == "one_heavy":
        w = np.full(N, 1e-12 / max(N, 1))
        w[N // 2] = 1.0 - 1e-12 if N > 1 else 1.0
        return w, 0
    if kind_ == "below_unit":
        w = WR.weights("dirichlet", N, seed).copy()
        if N > 1:
            w[N // 3] = 2.0 ** -60
            w[(N // 3 + 1) % N] = 0.0
        return w, 0
    return WR.weights(kind_, N, seed), 0


def check_table(N, seed=0):
    """Cells [6][N]: three f64 rows, a bool row, a u64 row, an i64 row; 3 + 2 checks: all f64 rows with five statistics, a marginal one,
    one sharing a row (with a K = 1 variance: a NaN slot), the integer rows, a NaN in the observed vector.  -> (cells, vtypes, checks)"""
    kinds = ["normal", "normal", "constant", "bernoulli", "u64_big", "neg_i64"]
    cells, vt = PR.table(kinds, 1, N, seed)
    cells = np.ascontiguousarray(cells[0])
    rng = np.random.default_rng([seed, N, 77])
    obs = [float(v) for v in rng.normal(0.0, 1.0, 3)]
    obs[2] = PR.CONSTANT
    if N > 4:                                        # a NaN replicate and an exact tie with the observed mean of the marginal check
        f = cells[1].view(np.float64)
        f[1] = np.nan
        f[3] = obs[1]
        f[4] = -0.0
    chk = [([0, 1, 2], PR.ALL, obs),
           ([1], 1 << PR.MEAN, [obs[1]]),
           ([2, 0], (1 << PR.MAX) | (1 << PR.MIN), [PR.CONSTANT, obs[0]]),
           ([0], (1 << PR.VAR) | (1 << PR.MEAN), [0.0]),                          # K = 1: the variance slot is all nan
           ([3, 4, 5], (1 << PR.SUM) | (1 << PR.MAX), [1.0, float(2 ** 53), -2.0]),
           ([1, 0], PR.ALL, [NAN, 0.5]),                                          # NaN T_obs: all nan, the moments stay
           ([4], 1 << PR.MEAN, [0.0])]
    return cells, vt, chk
