"""The log-likelihood stream (fugue_amd/csrc/fg_loglik_stream_plan.h) restated operation by operation in Python floats, with
math.exp / math.log (glibc's, like the host build; numpy's vectorised exp may differ in the last bit).  No numpy arithmetic on the
path of a compared figure.  Also the inputs the CPU and GPU tests share, and the two-pass textbook formulas.

A column is [mx, sp, mn, sn, sn2, pivot, s1, s2, n_fin, n_neg_inf, n_pos_inf, n_nan]; a tree element is
[mx, sp, mn, sn, sn2, n, mean, ssd, n_neg_inf, n_pos_inf, n_nan]."""
import math
import struct

import numpy as np

POOLED, FIGURES, BLOCK = 8, 8, 256
FIGURE_NAMES = ("lppd", "mean_ll", "p_waic", "elpd_waic", "elpd_loo", "p_loo", "is_ess", "max_weight")
INF, NAN = float("inf"), float("nan")


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def new_column():
    return [0.0] * 8 + [0, 0, 0, 0]


def update(s, x):
    if x != x:
        s[11] += 1
        return
    if x == INF:
        s[10] += 1
        return
    if x == -INF:
        s[9] += 1
        return
    if s[8] == 0:
        s[0] = s[2] = s[5] = x
        s[1] = s[3] = s[4] = 1.0
        s[6] = s[7] = 0.0
        s[8] = 1
        return
    mx, mn = s[0], s[2]
    if x <= mx:
        s[1] = s[1] + math.exp(x - mx)
    else:
        s[1] = s[1] * math.exp(mx - x) + 1.0
        s[0] = x
    if x >= mn:
        e = math.exp(mn - x)
        s[3] = s[3] + e
        s[4] = s[4] + e * e
    else:
        f = math.exp(x - mn)
        s[3] = s[3] * f + 1.0
        s[4] = s[4] * (f * f) + 1.0
        s[2] = x
    d = x - s[5]
    s[6] = s[6] + d
    s[7] = s[7] + d * d
    s[8] += 1


def leaf(s):
    e = [0.0] * 8 + [s[9], s[10], s[11]]
    if s[8] == 0:
        return e
    n = float(s[8])
    mu = s[6] / n
    e[0:5] = s[0:5]
    e[5], e[6], e[7] = n, s[5] + mu, s[7] - s[6] * mu
    return e


def merge(a, b):
    if a[5] == 0.0:
        r = list(b)
    elif b[5] == 0.0:
        r = list(a)
    else:
        r = list(a)
        if a[0] >= b[0]:
            r[1], r[0] = a[1] + b[1] * math.exp(b[0] - a[0]), a[0]
        else:
            r[1], r[0] = b[1] + a[1] * math.exp(a[0] - b[0]), b[0]
        if a[2] <= b[2]:
            f = math.exp(a[2] - b[2])
            r[3], r[4], r[2] = a[3] + b[3] * f, a[4] + b[4] * (f * f), a[2]
        else:
            f = math.exp(b[2] - a[2])
            r[3], r[4], r[2] = b[3] + a[3] * f, b[4] + a[4] * (f * f), b[2]
        n = a[5] + b[5]
        delta = b[6] - a[6]
        r[5] = n
        r[6] = a[6] + delta * (b[5] / n)
        r[7] = a[7] + b[7] + delta * delta * (a[5] * b[5] / n)
    r[8], r[9], r[10] = a[8] + b[8], a[9] + b[9], a[10] + b[10]
    return r


def tree(elems):
    """The fixed tree on the chain index: stride s = 1, 2, 4, ...; element i (a multiple of 2 s) takes in i + s when that exists."""
    e = [list(v) for v in elems]
    s = 1
    while s < len(e):
        for i in range(0, len(e) - s, 2 * s):
            e[i] = merge(e[i], e[i + s])
        s *= 2
    return e[0]


def finish(e, N):
    a, b, z = e[8], e[9], e[10]
    none = e[5] == 0.0
    if z > 0:
        return [NAN] * FIGURES
    N = float(N)
    ln_n = math.log(N)
    lppd = INF if b > 0 else (-INF if none else e[0] + math.log(e[1]) - ln_n)
    loo = -INF if a > 0 else (INF if none else ln_n + e[2] - math.log(e[3]))
    mean = NAN if (a > 0 and b > 0) else (-INF if a > 0 else (INF if b > 0 else e[6]))
    p_waic = e[7] / (N - 1.0) if (a == 0 and b == 0 and N > 1.0) else NAN
    ratios = a == 0 and not none
    return [lppd, mean, p_waic, lppd - p_waic, loo, lppd - loo, e[3] * e[3] / e[4] if ratios else NAN, 1.0 / e[3] if ratios else NAN]


def columns(table):
    """table [n][n_sel][C] -> the columns [n_sel][C] after every draw, in draw order."""
    n, n_sel, C = table.shape
    cols = [[new_column() for _ in range(C)] for _ in range(n_sel)]
    t = table.tolist()
    for row in t:
        for k in range(n_sel):
            ck, rk = cols[k], row[k]
            for c in range(C):
                update(ck[c], rk[c])
    return cols


def stream(table):
    """-> (pooled elements [n_sel][11], figures [n_sel][8])."""
    n, n_sel, C = table.shape
    out, figs = [], []
    for ck in columns(table):
        e = tree([leaf(s) for s in ck])
        out.append(e)
        figs.append(finish(e, n * C))
    return out, figs


# ---- the two-pass formulas on the pooled row ---------------------------------------------------------------------------------
def two_pass(x):
    """x: the pooled row (any order) -> the eight figures by scipy's logsumexp and numpy's variance, non-finite cells as IEEE has them."""
    from scipy.special import logsumexp
    x = np.asarray(x, dtype=np.float64).ravel()
    N = x.size
    with np.errstate(all="ignore"):
        lppd = float(logsumexp(x)) - math.log(N) if not np.isnan(x).any() else NAN
        loo = -(float(logsumexp(-x)) - math.log(N)) if not np.isnan(x).any() else NAN
        mean = float(np.mean(x))
        p_waic = float(np.var(x, ddof=1)) if N > 1 else NAN
        r = np.exp(-(x - np.min(x[np.isfinite(x)]))) if np.isfinite(x).any() and not np.isneginf(x).any() else np.exp(-x)
        ess = float(np.sum(r) ** 2 / np.sum(r * r))
        mw = float(np.max(r) / np.sum(r))
    return [lppd, mean, p_waic, lppd - p_waic, loo, lppd - loo, ess, mw]


# ---- inputs ------------------------------------------------------------------------------------------------------------------
ROW_KINDS = ("normal", "far", "increasing", "decreasing", "constant", "neg_inf", "pos_inf", "nan", "all_neg_inf", "both_inf")
FINITE_KINDS = ("normal", "far", "increasing", "decreasing", "constant")


def row(kind, n, C, seed=0):
    """One statement's cells [n][C] of the given kind (draw-major: the pooled order is chains inside draws)."""
    rng = np.random.default_rng([seed, ROW_KINDS.index(kind), n, C])
    N = n * C
    if kind == "normal":
        x = rng.normal(-3.0, 1.0, N)
    elif kind == "far":                              # exp(x) underflows and exp(-x) overflows without the running max and min
        x = -1e4 + 800.0 * rng.normal(0.0, 1.0, N)
    elif kind == "increasing":                       # along every chain and along the chain index: the upper side rescales on every cell
        x = -5.0 + 0.37 * np.arange(N, dtype=np.float64)
    elif kind == "decreasing":
        x = 2.0 - 0.37 * np.arange(N, dtype=np.float64)
    elif kind == "constant":
        x = np.full(N, -1.25)
    else:
        x = rng.normal(-3.0, 1.0, N)
        at = int(rng.integers(0, N))
        if kind == "neg_inf":
            x[at] = -np.inf
        elif kind == "pos_inf":
            x[at] = np.inf
        elif kind == "nan":
            x[at] = np.nan
        elif kind == "all_neg_inf":
            x[:] = -np.inf
        elif kind == "both_inf":
            x[at] = np.inf
            x[(at + 1) % N] = -np.inf
    return x.reshape(n, C)


def table(kinds, n, C, seed=0):
    """[n][len(kinds)][C]."""
    return np.ascontiguousarray(np.stack([row(k, n, C, seed) for k in kinds], axis=1))


def same_class(a, b):
    """Both NaN, or the same infinity, or both finite."""
    if a != a or b != b:
        return a != a and b != b
    if math.isinf(a) or math.isinf(b):
        return a == b
    return True
