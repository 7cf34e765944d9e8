"""A numpy restatement of Pareto-smoothed importance-sampling LOO per observe statement (Vehtari, Simpson, Gelman, Yao, Gabry; the
generalised Pareto fit of Zhang and Stephens 2009 with the weakly informative prior, as the R `loo` package's psis / gpdfit compute
it; r_eff = 1), written from the formulas of DESIGN 3.22 with every sum in the order fugue_amd/csrc/fg_psis_plan.h states (`cell_sum`,
`tail_sum`).  The reference project has none of this: this file is the yardstick of fg_psis.hip.

`psis_statement(x)` evaluates the rule in IEEE double; `psis_statement(x, ld=True)` evaluates the SAME formulas in numpy.longdouble,
step 1 (lw = x_min - x) included (the selection, which is integer work on the keys, is shared).  The device takes the rule's double
lw as data and evaluates what follows in double-double, so it sits between the two evaluations.  The second
evaluation is used only to size the tolerances: the difference of the two is the sensitivity of the rule to rounding on that input.
Used by tests/test_psis_cpu.py, tests/test_gpu_psis.py and tools/bench_psis.py."""
from __future__ import annotations

import math

import numpy as np

EPS = 2.0 ** -52                                         # one ulp, relative, at most; one rounding is EPS / 2
ULP_EXP, ULP_LOG = 1.0, 1.0                               # ocml's stated bounds for the f64 exp / log (glibc's are below 1), in ulp
ULP_LOG1P, ULP_EXPM1 = 2.0, 1.0                           # ... log1p, expm1
FACTOR = 4.0                                              # device - float64 restatement <= FACTOR x (float64 - longdouble)
THREADS, WAVE, CELLS_PER_BLOCK, MAX_BLOCKS, MIN_TAIL = 256, 64, 4096, 256, 5
FITTED, TOO_FEW, DEGENERATE, NONFINITE = range(4)
WORD_NAMES = ("elpd_loo_psis", "p_loo_psis", "khat", "sigma", "khat_threshold", "lppd", "x_min", "x_cut", "exp_cutoff", "t_star", "theta_hat",
              "body_sum", "tail_sum", "tail_num")
COUNT_NAMES = ("tail_len", "status", "n_capped", "n_fin", "n_neg_inf", "n_pos_inf", "n_nan", "n_below", "n_equal", "n_collected")
EXACT_WORDS = ("x_min", "x_cut")
FIT_WORDS = ("elpd_loo_psis", "p_loo_psis", "khat", "sigma", "theta_hat", "tail_sum", "tail_num")       # downstream of the profile


# ---- the plan (fg_psis_plan.h) -------------------------------------------------------------------------------------------------------
def isqrt_ceil(v: int) -> int:
    r = math.isqrt(v)
    return r if r * r == v else r + 1


def tail_len(S: int) -> int:
    """M = min(ceil(S / 5), b), b the smallest integer with b b >= 9 S"""
    return min((S + 4) // 5, isqrt_ceil(9 * S))


def profile_points(M: int) -> int:
    return 30 + math.isqrt(M)


def quartile_index(M: int) -> int:
    return (M + 2) // 4                                  # 1-based


def blocks(S: int) -> int:
    return max(1, min(MAX_BLOCKS, -(-S // CELLS_PER_BLOCK)))


def pow2(v: int) -> int:
    p = 1
    while p < v:
        p *= 2
    return p


def sort_len(M: int) -> int:
    return pow2(max(M, 2))


def threshold(S: int) -> float:
    with np.errstate(all="ignore"):
        return float(min(np.float64(1.0) - np.float64(1.0) / np.float64(math.log10(S)), 0.7))


def keys(x) -> np.ndarray:
    """fg_qs_key: ascending in the double's order, -0.0 below +0.0, positive-sign NaN above +inf"""
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))


def _fold(a):
    """the last axis (a power of two) by halves: v[l] + v[l + h] for h = len / 2, ..., 1"""
    h = a.shape[-1] // 2
    while h >= 1:
        a = a[..., :h] + a[..., h:2 * h]
        h //= 2
    return a[..., 0]


def cell_depth(S: int) -> int:
    nb = blocks(S)
    return -(-S // (nb * THREADS)) + 6 + THREADS // WAVE + int(math.log2(pow2(nb)))


def cell_sum(v):
    """the plan's sum of one term per pooled cell"""
    v = np.asarray(v)
    S, nb = v.size, blocks(v.size)
    stride = nb * THREADS
    per = -(-S // stride)
    pad = np.zeros(per * stride, dtype=v.dtype)
    pad[:S] = v
    acc = np.zeros(stride, dtype=v.dtype)
    for row in pad.reshape(per, stride):                 # thread t of block b: cells b T + t, + NB T, ... in sequence, from +0.0
        acc = acc + row
    waves = _fold(acc.reshape(nb, THREADS // WAVE, WAVE))
    part = np.zeros(pow2(nb), dtype=v.dtype)
    for w in range(THREADS // WAVE):                     # wave totals in wave order, from +0.0
        part[:nb] = part[:nb] + waves[:, w]
    return _fold(part)


def tail_depth(M: int) -> int:
    return -(-M // WAVE) + 6


def tail_sum(v):
    """the plan's sum of one term per tail value, by one wave"""
    v = np.asarray(v)
    per = -(-v.size // WAVE)
    pad = np.zeros(per * WAVE, dtype=v.dtype)
    pad[:v.size] = v
    acc = np.zeros(WAVE, dtype=v.dtype)
    for row in pad.reshape(per, WAVE):
        acc = acc + row
    return _fold(acc)


def pooled(table, k: int) -> np.ndarray:
    """the S = n C pooled cells of statement k of a table [n][n_sel][C], draw-major"""
    return np.ascontiguousarray(np.asarray(table, dtype=np.float64)[:, k, :]).reshape(-1)


# ---- the rule ------------------------------------------------------------------------------------------------------------------------
def psis_statement(x, ld: bool = False) -> dict:
    """One statement over its pooled cells `x` -> every word and count of fg_psis_loo's rows, the sorted raw `tail` and the
    exceedances `t`."""
    F = np.longdouble if ld else np.float64
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    S = x.size
    M = tail_len(S)
    ky = keys(x)
    order = np.argsort(ky, kind="stable")
    n_nan, n_ninf, n_pinf = int(np.isnan(x).sum()), int((x == -np.inf).sum()), int((x == np.inf).sum())
    rank = min(M + 1, S)
    kc, xc = ky[order[rank - 1]], float(x[order[rank - 1]])
    below, equal = int((ky < kc).sum()), int((ky == kc).sum())
    tail = x[order[:M]].copy()                            # ascending; ties at the boundary are one value
    xmin = float(x[order[0]])
    nn = x[~np.isnan(x)]
    xmax = float(nn[np.argmax(keys(nn))]) if nn.size else math.nan
    status = FITTED
    if n_nan or n_ninf or xc == np.inf:
        status = NONFINITE
    elif M < MIN_TAIL:
        status = TOO_FEW
    with np.errstate(all="ignore"):
        xF, mnF = x.astype(F), F(xmin)
        ecut = np.exp(mnF - F(xc))
        lw = mnF - tail[::-1].astype(F)                   # ascending ratio
        t = np.exp(lw) - ecut
        body = cell_sum(np.where(ky > kc, np.exp(mnF - xF), F(0.0)))
        ties = equal - (M - min(below, M))
        if ties > 0:
            body = body + F(ties) * ecut
        lsum = cell_sum(np.exp(xF - F(xmax)))
        tstar = t[max(quartile_index(M) - 1, 0)]
        if status == FITTED and not tstar > 0:
            status = DEGENERATE
        khat, sigma, theta = F(np.inf), F(np.nan), F(np.nan)
        dM, kmax = F(M), 0.0
        if status == FITTED:
            G = profile_points(M)
            j = np.arange(1, G + 1).astype(F)
            th = F(1.0) / t[-1] + (F(1.0) - np.sqrt(F(G) / (j - F(0.5)))) / (F(3.0) * tstar)
            l = np.zeros(G, dtype=F)
            for m in range(G):
                kj = tail_sum(np.log1p(-th[m] * t)) / dM
                l[m] = dM * (np.log(-th[m] / kj) - kj - F(1.0))
                kmax = max(kmax, abs(float(kj)))
            lmax = l[0]
            for m in range(1, G):
                lmax = l[m] if l[m] > lmax else lmax
            Z, num = F(0.0), F(0.0)
            for m in range(G):                            # index order, from +0.0
                e = np.exp(l[m] - lmax)
                Z = Z + e
                num = num + th[m] * e
            theta = num / Z
            kraw = tail_sum(np.log1p(-theta * t)) / dM
            sigma = -kraw / theta
            khat = (kraw * dM + F(5.0)) / (dM + F(10.0))
        lwt, n_capped = lw, 0
        if status == FITTED and np.isfinite(khat):
            p = (np.arange(1, M + 1).astype(F) - F(0.5)) / dM
            q = sigma * np.expm1(-khat * np.log1p(-p)) / khat
            v = np.log(q + ecut)
            n_capped = int((v > 0).sum())
            lwt = np.where(v > 0, F(0.0), v)
        sa, sb = tail_sum(np.exp(lwt - lw)), tail_sum(np.exp(lwt))
        elpd = mnF + (np.log(F(S - M) + sa) - np.log(body + sb))
        lppd = F(xmax) + np.log(lsum) - np.log(F(S))
        if n_pinf:
            lppd = F(np.inf)
        elif n_ninf == S:
            lppd = F(-np.inf)
        if n_ninf:
            elpd = F(-np.inf)
        elif n_pinf == S:
            elpd = F(np.inf)
        words = dict(elpd_loo_psis=elpd, p_loo_psis=lppd - elpd, khat=khat, sigma=sigma, khat_threshold=F(threshold(S)), lppd=lppd, x_min=F(xmin), x_cut=F(xc),
                     exp_cutoff=ecut, t_star=tstar, theta_hat=theta, body_sum=body, tail_sum=sb, tail_num=sa)
    if n_nan:
        words = {k: (v if k == "khat_threshold" else F(np.nan)) for k, v in words.items()}
    counts = dict(tail_len=M, status=status, n_capped=n_capped, n_fin=S - n_nan - n_ninf - n_pinf, n_neg_inf=n_ninf, n_pos_inf=n_pinf, n_nan=n_nan, n_below=below,
                  n_equal=equal, n_collected=below)
    out = dict(words)
    out.update(counts)
    out.update(tail=tail, t=t, lw=lw, S=S, M=M, kmax=kmax)
    return out


def psis_table(table, ld: bool = False):
    table = np.asarray(table, dtype=np.float64)
    return [psis_statement(pooled(table, k), ld) for k in range(table.shape[1])]


# ---- error bounds ----------------------------------------------------------------------------------------------------------------------
def tolerances(case: dict, case_ld: dict) -> dict:
    """Bounds on |device - float64 restatement| per word for one statement: `case` = psis_statement(x), `case_ld` = psis_statement(x, True).
      x_min, x_cut: selected cells, 0.  khat_threshold: two roundings and a log10 of either libm: 4 EPS.
      exp_cutoff = exp(x_min - x_cut), the same argument on both sides: (ULP_EXP + 1) EPS relative (ocml's bound and glibc's).
      t* = exp(lw) - exp(lw_cut): both exps as above, the subtraction a rounding per side.
      body_sum: non-negative terms, each within (ULP_EXP + 1) EPS relative; the same order on both sides, so the sums differ by the
        terms' relative error plus a rounding per level and side: cell_depth(S) EPS; the ties' product two roundings more.
      lppd = x_max + ln(sum) - ln S: the sum as above (absolute, after the log), each log (ULP_LOG + 1) EPS of its value, the two
        additions a rounding per side.
      WITHOUT A FIT (too few draws, degenerate, non-finite): tail_num = M exactly (a sum of ones); tail_sum = sum exp(lw) as the body with
        tail_depth(M); elpd = x_min + ln(S - M + tail_num) - ln(body + tail): the relative error of the denominator, the two logs, the
        additions.  These closed bounds are tight, so they are used as they stand.
      WITH A FIT: l_j multiplies the rounding of a profile mean by M ahead of a softmax and no closed bound is tight, so theta_hat, khat,
        sigma, and what is computed from them (tail_sum, tail_num, elpd_loo_psis, p_loo_psis) may differ from the float64 restatement by
        FACTOR = 4 times |float64 - longdouble| of that word on that input: the device's libm is bounded at 1-2 ulp per call where the
        host's is about 0.5-1, so the same propagation scales by at most 2, doubled for opposite signs.  The difference is taken
        between the two results AS DOUBLES (the longdouble word rounded to double): what two double evaluations of the word can show of
        each other.  Where the two round to the same double the difference is zero and says nothing -- two correctly propagated doubles
        may still sit an ulp apart -- and the first-order bound of the word applies: a profile mean k_j is a sum of same-signed log1p
        terms, each within (ULP_LOG1P + 1) EPS, so l_j = M (ln(-theta_j / k_j) - k_j - 1) moves by at most M (ULP_LOG1P + 1) EPS
        (1 + |k_j|), a softmax weight by twice the largest such move, relative, and theta_hat with it: 2 M (1 + max_j |k_j|)
        (ULP_LOG1P + 1) EPS relative, with max_j |k_j| of the case (`kmax`); k_raw, sigma, khat, the smoothed tail's sums and the elpd
        are smooth functions of theta_hat whose own roundings are a few EPS beside it, so the same relative bound is used for them."""
    S, M = case["S"], case["M"]
    e_exp, e_log = (ULP_EXP + 1.0) * EPS, (ULP_LOG + 1.0) * EPS
    f = lambda name: float(case[name])
    tol = dict(x_min=0.0, x_cut=0.0, khat_threshold=4.0 * EPS)
    fin = lambda v: v if math.isfinite(v) else 0.0
    tol["exp_cutoff"] = e_exp * fin(f("exp_cutoff"))
    q = max(quartile_index(M) - 1, 0)
    with np.errstate(all="ignore"):
        tol["t_star"] = fin(e_exp * (float(np.exp(case["lw"][q])) + f("exp_cutoff")) + EPS * abs(f("t_star")))
    r_body = e_exp + (cell_depth(S) + 2) * EPS
    tol["body_sum"] = fin(r_body * f("body_sum"))
    with np.errstate(all="ignore"):
        lsum = f("lppd") - f("x_min")                     # the order of magnitude of the two logs
    tol["lppd"] = fin(r_body + e_log * (abs(fin(f("lppd"))) + abs(fin(lsum)) + 2.0 * math.log(max(S, 2))) + 4.0 * EPS * abs(fin(f("lppd"))))
    if case["status"] != FITTED:
        r_tail = e_exp + tail_depth(M) * EPS
        tol["tail_num"] = 0.0
        tol["tail_sum"] = fin(r_tail * f("tail_sum"))
        den = f("body_sum") + f("tail_sum")
        r_den = (tol["body_sum"] + tol["tail_sum"]) / den + EPS if den > 0 and math.isfinite(den) else 0.0
        ln_num, ln_den = math.log(S), (math.log(den) if den > 0 and math.isfinite(den) else 0.0)
        tol["elpd_loo_psis"] = fin(r_den + e_log * (abs(ln_num) + abs(ln_den)) + 4.0 * EPS * (abs(fin(f("x_min"))) + abs(ln_num) + abs(ln_den)))
        tol["p_loo_psis"] = tol["lppd"] + tol["elpd_loo_psis"] + EPS * abs(fin(f("p_loo_psis")))
        for name in ("khat", "sigma", "theta_hat"):
            tol[name] = 0.0                               # +inf / NaN on both sides: compared by class
        return tol
    first_order = 2.0 * M * (1.0 + case["kmax"]) * (ULP_LOG1P + 1.0) * EPS
    for name in FIT_WORDS:
        d = abs(f(name) - float(case_ld[name])) if math.isfinite(f(name)) and math.isfinite(float(case_ld[name])) else 0.0
        tol[name] = FACTOR * d if d > 0.0 else first_order * abs(fin(f(name)))
    return tol


# |float64 - longdouble| of the words downstream of the profile, relative to the word, in units of 2^-52: the largest over the three
# statements of table(n, C, 3, seed=100 n + C), the tables of tests/test_gpu_psis.py (an x86-64 host, 80-bit longdouble).  One
# statement's value is one draw of the rule's rounding sensitivity: within a table it ranges from below one unit to the figure here.
#   (n, C)       elpd_loo_psis  p_loo_psis   khat   sigma  theta_hat  tail_sum  tail_num
#   (1, 20)           0.0           2.3        -       -       -         0.0      0.0      (no fit: the closed bounds apply)
#   (1, 21)           0.8          12.3       1.1     2.1     8.0        0.8      0.7
#   (5, 5)            0.8           5.3       2.2     7.8     9.8        2.0      5.5
#   (3, 75)           2.4           3.0       8.3    29.8    38.8       52.4     11.9
#   (7, 193)          2.6          23.0      15.2    36.5    50.9       23.0      3.2
#   (2, 4097)        38.6          49.9      44.9    88.5   133.3      363.9      0.9
#   (16, 1024)       36.8          43.0      33.0   124.2   157.2     1137.1      0.0
#   (1, 65536)       43.9         107.2      68.0   212.5   280.3     1234.5     15.2
def sensitivity(case: dict, case_ld: dict) -> dict:
    """|float64 - longdouble| of the words the profile feeds, for the record"""
    with np.errstate(all="ignore"):
        return {name: abs(float(case[name]) - float(case_ld[name])) for name in FIT_WORDS}


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
GPU_SHAPES = ((1, 20), (1, 21), (5, 5), (3, 75), (7, 193), (2, 4097), (16, 1024), (1, 65536))


def table(n: int, C: int, n_sel: int, seed: int) -> np.ndarray:
    """pointwise log-likelihoods of a Normal observation under draws of its mean and scale: continuous, ties have probability zero"""
    rng = np.random.default_rng(seed)
    mu, sig = rng.normal(0.0, 0.6, size=(n, 1, C)), np.exp(rng.normal(0.0, 0.25, size=(n, 1, C)))
    y = rng.normal(0.0, 1.5, size=(1, n_sel, 1))
    z = (y - mu) / sig
    return np.ascontiguousarray(-0.5 * z * z - np.log(sig) - 0.5 * math.log(2.0 * math.pi))


def pareto_ratios(k: float, S: int, seed: int) -> np.ndarray:
    """log-likelihood cells whose importance ratios exp(-x) are r = U^(-k): an exact Pareto tail of shape k"""
    u = np.random.default_rng(seed).uniform(size=S)
    return k * np.log(u)                                  # x = -ln r


def gpd_ratios(k: float, S: int, seed: int) -> np.ndarray:
    """cells whose ratios are r = 1 + (U^(-k) - 1) / k: a generalised Pareto law of shape k at every threshold, for k < 0 as well
    (U^(-k) with k < 0 is bounded by 1 with a density that stays positive there: its tail has shape -1, not k)"""
    u = np.random.default_rng(seed).uniform(size=S)
    return -np.log1p(np.expm1(-k * np.log(u)) / k)


def normal_loo_exact(y: np.ndarray, sigma: float, tau: float):
    """The conjugate Normal model y_i ~ N(mu, sigma), mu ~ N(0, tau): posterior of mu and the exact leave-one-out predictive
    log-density of every y_i -> (posterior mean, posterior sd, elpd_loo_i exact)"""
    y = np.asarray(y, dtype=np.float64)
    n = y.size
    prec = 1.0 / tau ** 2 + n / sigma ** 2
    mean, sd = (y.sum() / sigma ** 2) / prec, math.sqrt(1.0 / prec)
    out = np.zeros(n)
    for i in range(n):
        p_i = 1.0 / tau ** 2 + (n - 1) / sigma ** 2
        m_i, v_i = ((y.sum() - y[i]) / sigma ** 2) / p_i, 1.0 / p_i
        s2 = v_i + sigma ** 2
        out[i] = -0.5 * math.log(2.0 * math.pi * s2) - 0.5 * (y[i] - m_i) ** 2 / s2
    return mean, sd, out
