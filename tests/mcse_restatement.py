"""A numpy restatement of the rule of the Monte Carlo standard errors and effective sample sizes of a mean, a standard deviation and
quantiles (fugue_amd/csrc/fg_diag_mcse_plan.h; the figures of the R `posterior` package's summarise_draws), written from
the rule: np.sort on the value keys of tests/rank_restatement.py, the centred rows, the indicators by integer comparison of keys, the
type-7 quantile, the Beta rule through this file's own regularised incomplete beta function and its inverse, the median and the mad.
The effective sample sizes, the pooled mean and the pooled standard deviation come from the oracle's combination on the rows in their
[n][C] layout.  No device and no library of the product enters."""
import math

import numpy as np

from tests import rank_restatement as R

WORD_NAMES = ("mean", "sd", "rhat", "ess_mean", "mcse_mean", "ess_sd", "ess_sq", "mcse_sd", "median", "mad")
PROB_WORD_NAMES = ("q", "q7", "ess_quantile", "mcse_quantile", "th_lo", "th_hi")
COUNT_NAMES = ("n_cells", "n_nan", "n_neg_inf", "n_pos_inf", "n_nan_folded", "n_passes")
PROB_COUNT_NAMES = ("k_p", "i_lo", "i_hi")
Y_LO, Y_HI = 0.15865525393145707, 0.8413447460685429
MAD_CONSTANT = 1.4826

# fg_mcse_betaincinv against mpmath at 50 digits (tests/test_diag_mcse_cpu.py measures it again): the largest relative deviation over
# ess in {0.7, 9.3, 211.7, 3 100.2, 80 000.5, 2.1e9} x p in {0, 0.05, 0.5, 0.95, 1} x both levels, and four times that as the tolerance.
BETA_MEASURED_DEV = 2.3e-15
BETA_TOL = 4.0 * BETA_MEASURED_DEV
BETA_ESS = (0.7, 9.3, 211.7, 3100.2, 80000.5, 2.1e9)
BETA_P = (0.0, 0.05, 0.5, 0.95, 1.0)
RANK_S = (1, 21, 600, 12707, 309300, 2 ** 31 - 1)


# ---- the regularised incomplete beta function and its inverse (a, b >= 1) ---------------------------------------------------------------
def _stirling_corr(x):
    """lgamma(x) - ((x - 1/2) log x - x + log(2 pi) / 2)"""
    if x < 10.0:
        return math.lgamma(x) - ((x - 0.5) * math.log(x) - x + 0.91893853320467274178)
    r = 1.0 / x
    r2 = r * r
    return r * (1.0 / 12.0 + r2 * (-1.0 / 360.0 + r2 * (1.0 / 1260.0 + r2 * (-1.0 / 1680.0 + r2 * (1.0 / 1188.0 + r2 * (-691.0 / 360360.0 + r2 * (1.0 / 156.0)))))))


def _log1pmx(u):
    if abs(u) >= 0.1:
        return math.log1p(u) - u
    term, total = -u, 0.0
    for k in range(2, 64):
        term *= -u
        add = -term / k
        total += add
        if abs(add) <= 1e-18 * abs(total):
            break
    return total


def _front(a, b, x):
    """x^a (1 - x)^b / B(a, b)"""
    s = a + b
    u1, u2 = (x * s - a) / a, ((1.0 - x) * s - b) / b
    e = a * _log1pmx(u1) + b * _log1pmx(u2) - (_stirling_corr(a) + _stirling_corr(b) - _stirling_corr(s))
    return math.sqrt(a * b / (s * 6.283185307179586476925)) * math.exp(e)


def _cf(a, b, x):
    tiny, eps = 1e-300, 2.3e-16
    qab, qap, qam = a + b, a + 1.0, a - 1.0
    c, d = 1.0, 1.0 - qab * x / qap
    d = 1.0 / (tiny if abs(d) < tiny else d)
    h = d
    for m in range(1, 4000001):
        m2 = 2.0 * m
        for aa in (m * (b - m) * x / ((qam + m2) * (a + m2)), -(a + m) * (qab + m) * x / ((a + m2) * (qap + m2))):
            d = 1.0 + aa * d
            d = 1.0 / (tiny if abs(d) < tiny else d)
            c = 1.0 + aa / c
            c = tiny if abs(c) < tiny else c
            h *= d * c
        if abs(d * c - 1.0) <= eps:
            break
    return h


def betainc(a, b, x):
    """-> (I_x(a, b), 1 - I_x(a, b)), each computed directly on its side of the symmetry switch"""
    if not x > 0.0:
        return 0.0, 1.0
    if not x < 1.0:
        return 1.0, 0.0
    if x < (a + 1.0) / (a + b + 2.0):
        lo = _front(a, b, x) * _cf(a, b, x) / a
        return lo, 1.0 - lo
    hi = _front(a, b, x) * _cf(b, a, 1.0 - x) / b
    return 1.0 - hi, hi


def betaincinv(a, b, y):
    """x in [0, 1] with I_x(a, b) = y: Newton steps inside a bracket that only shrinks, bisection where a step would leave it"""
    if not y > 0.0:
        return 0.0
    if not y < 1.0:
        return 1.0
    lo, hi = 0.0, 1.0
    s = a + b
    x = a / s + (-1.0 if y < 0.5 else 1.0) * math.sqrt(a * b / (s * s * (s + 1.0)))
    if not 0.0 < x < 1.0:
        x = 0.5
    for _ in range(400):
        low, up = betainc(a, b, x)
        f = low - y if low <= 0.5 else (1.0 - y) - up
        if f == 0.0:
            return x
        if f < 0.0:
            lo = x
        else:
            hi = x
        pdf = _front(a, b, x) / (x * (1.0 - x))
        nx = x - f / pdf if pdf > 0.0 else math.nan          # a density that underflowed: the step is a bisection
        if not lo < nx < hi:
            nx = 0.5 * lo + 0.5 * hi
        if not lo < nx < hi:
            return x
        step, x = abs(nx - x), nx
        if step <= 4.5e-16 * x:
            break
    return x


def quantile_ranks(S, p, ess):
    """-> (i_lo, i_hi), or (-1, -1) where ess is not finite or not positive"""
    if not (math.isfinite(ess) and ess > 0.0):
        return -1, -1
    alpha, beta = ess * p + 1.0, ess * (1.0 - p) + 1.0
    a1, a2 = betaincinv(alpha, beta, Y_LO), betaincinv(alpha, beta, Y_HI)
    return max(int(math.floor(a1 * float(S))), 1) - 1, min(int(math.ceil(a2 * float(S))), S) - 1


# ---- mpmath's side: the inverse at 50 digits -------------------------------------------------------------------------------------------
def mp_betainc(A, B, z):
    """I_z(A, B) in mpmath's working precision: mpmath's own betainc, and where its hypergeometric series cancels (both parameters
    large) the integral of the density over the 80 standard deviations next to z (what lies beyond is below exp(-3000))"""
    import mpmath as mp
    if min(A, B) <= 50:
        return mp.betainc(A, B, 0, z, regularized=True)
    s = A + B
    x0, sd = A / s, mp.sqrt(A * B / (s * s * (s + 1)))
    lb = mp.loggamma(A) + mp.loggamma(B) - mp.loggamma(s)
    dens = lambda t: mp.exp((A - 1) * mp.log(t) + (B - 1) * mp.log1p(-t) - lb)
    if z <= x0:
        pts = sorted(set(p for p in [max(mp.mpf(0), x0 - k * sd) for k in (80, 40, 20, 10, 5)] + [z] if p <= z))
        return mp.quad(dens, pts if len(pts) > 1 else [mp.mpf(0), z])
    pts = sorted(set(p for p in [min(mp.mpf(1), x0 + k * sd) for k in (80, 40, 20, 10, 5)] + [z] if p >= z))
    return 1 - mp.quad(dens, pts if len(pts) > 1 else [z, mp.mpf(1)])


def mp_betaincinv(a, b, y, start):
    """the root of I_z(a, b) = y at 50 digits by Newton steps in mpmath from the double `start`; a, b, y are taken as the doubles they are"""
    import mpmath as mp
    A, B, Y = mp.mpf(a), mp.mpf(b), mp.mpf(y)
    lb = mp.loggamma(A) + mp.loggamma(B) - mp.loggamma(A + B)
    z = mp.mpf(start)
    for _ in range(12):
        dz = (mp_betainc(A, B, z) - Y) / mp.exp((A - 1) * mp.log(z) + (B - 1) * mp.log1p(-z) - lb)
        z -= dz
        if abs(dz) < mp.mpf(10) ** -40 * z:
            return z
    raise AssertionError(f"mpmath's Newton iteration did not settle for a = {a}, b = {b}, y = {y}")


# ---- one coordinate ----------------------------------------------------------------------------------------------------------------------
def q7_of(S, p, k_p, a, b):
    h = float(S - 1) * p
    g = h - float(k_p)
    if a == b or g == 0.0:
        return a
    return (1.0 - g) * a + g * b


def order_stats(x, probs):
    """one coordinate's pooled cells -> sorted keys, the median, the folded cells, the mad, per probability k_p, q and q7, the counts"""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    S = x.size
    k = R.keys(x)
    s = np.sort(k)
    med = R.median_of(s)
    with np.errstate(invalid="ignore"):
        folded = np.abs(x - med)
    fs = np.sort(R.keys(folded))
    n_nan_folded = int(np.isnan(folded).sum())
    mad = float("nan") if n_nan_folded else MAD_CONSTANT * R.median_of(fs)
    k_p = [R.kp(S, p) for p in probs]
    q = [R.unkey(s[kk]) for kk in k_p]
    q7 = [q7_of(S, p, kk, R.unkey(s[kk]), R.unkey(s[min(kk + 1, S - 1)])) for p, kk in zip(probs, k_p)]
    counts = dict(n_cells=S, n_nan=int(np.isnan(x).sum()), n_neg_inf=int((x == -np.inf).sum()), n_pos_inf=int((x == np.inf).sum()), n_nan_folded=n_nan_folded,
                  n_passes=R.passes_run(k) + R.passes_run(R.keys(folded)))
    return dict(keys=k, sorted_keys=s, median=med, mad=mad, k_p=k_p, q=q, q7=q7, counts=counts)


def rows_of(x, mean, probs, st=None):
    """-> the rows [2 + len(probs)][S]: |c|, c c, I_p ... with c = x - mean"""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    st = order_stats(x, probs) if st is None else st
    with np.errstate(invalid="ignore", over="ignore"):
        c = x - np.float64(mean)
        rows = [np.abs(c), c * c]
    rows += [(st["keys"] <= st["sorted_keys"][kk]).astype(np.float64) for kk in st["k_p"]]
    return np.stack(rows, axis=0)


def sorted_values(st):
    """the sorted cells as doubles (-0.0 as +0.0, every NaN the one NaN at the top)"""
    s = st["sorted_keys"]
    u = np.where((s >> np.uint64(63)) != 0, s & ~R.TOP, ~s)
    return np.where(s == R.NAN_KEY, np.float64("nan"), u.view(np.float64))


def at_position(st, i):
    return R.unkey(st["sorted_keys"][i])


def combination(row_nc):
    """the oracle's figures of one row [n][C]: ess, pooled mean, pooled std (n - 1)"""
    from oracle import oracle as orc
    chains = np.ascontiguousarray(np.asarray(row_nc, dtype=np.float64).T)
    sm = orc.summarize(chains)
    return dict(ess=orc.ess_multichain(chains), mean=sm["mean"], std=sm["std"], rhat=orc.split_rhat(chains))


def mcse_sd_of(std_b, evar, ess_sq, S):
    with np.errstate(all="ignore"):
        V = np.float64(std_b) * np.float64(std_b) * np.float64(S - 1) / np.float64(S)
        return float(np.sqrt(V / np.float64(ess_sq) / np.float64(evar) / np.float64(4.0)))


def mcse_mean_of(sd, ess_mean):
    with np.errstate(all="ignore"):
        return float(np.float64(sd) / np.sqrt(np.float64(ess_mean)))


def coordinate(draws, j, probs=(0.05, 0.5, 0.95)):
    """draws [n][d][C], coordinate j -> the rows [n][R][C], the words, the per-probability words and the counts of the whole rule"""
    draws = np.ascontiguousarray(draws, dtype=np.float64)
    n, _, C = draws.shape
    x = draws[:, j, :].reshape(-1)
    S = x.size
    st = order_stats(x, probs)
    raw = combination(draws[:, j, :])
    rows = rows_of(x, raw["mean"], probs, st).reshape(-1, n, C).transpose(1, 0, 2)
    comb = [combination(rows[:, i, :]) for i in range(rows.shape[1])]
    w = dict(mean=raw["mean"], sd=raw["std"], rhat=raw["rhat"], ess_mean=raw["ess"], mcse_mean=mcse_mean_of(raw["std"], raw["ess"]), ess_sd=comb[0]["ess"], ess_sq=comb[1]["ess"],
             mcse_sd=mcse_sd_of(comb[1]["std"], comb[1]["mean"], comb[1]["ess"], S), median=st["median"], mad=st["mad"])
    pw = {k: [] for k in PROB_WORD_NAMES}
    pc = {k: [] for k in PROB_COUNT_NAMES}
    for i, p in enumerate(probs):
        ess = comb[2 + i]["ess"]
        lo, hi = quantile_ranks(S, p, ess)
        th_lo, th_hi = (at_position(st, lo), at_position(st, hi)) if lo >= 0 else (float("nan"), float("nan"))
        with np.errstate(invalid="ignore"):
            mq = float(np.float64(0.5) * (np.float64(th_hi) - np.float64(th_lo)))
        for k, v in zip(PROB_WORD_NAMES, (st["q"][i], st["q7"][i], ess, mq, th_lo, th_hi)):
            pw[k].append(v)
        for k, v in zip(PROB_COUNT_NAMES, (st["k_p"][i], lo, hi)):
            pc[k].append(v)
    if st["counts"]["n_nan"] > 0:
        w = {k: float("nan") for k in w}
        pw = {k: [float("nan")] * len(probs) for k in pw}
    return dict(rows=rows, words=w, prob_words=pw, counts=st["counts"], prob_counts=pc, stats=st, Evar=comb[1]["mean"], std_B=comb[1]["std"])


# ---- the law: what the figures claim against what seeds show -------------------------------------------------------------------------------
def law_figures(x_nc, p=0.5):
    """draws [n][C] -> mcse_mean, mcse_sd, mcse_quantile(p) of the restatement, and the mean, sd (n - 1) and type-7 quantile themselves"""
    x_nc = np.ascontiguousarray(x_nc, dtype=np.float64)
    t = coordinate(x_nc[:, None, :], 0, probs=(p,))
    return dict(mcse_mean=t["words"]["mcse_mean"], mcse_sd=t["words"]["mcse_sd"], mcse_quantile=t["prob_words"]["mcse_quantile"][0], mean=t["words"]["mean"], sd=t["words"]["sd"],
                quantile=t["prob_words"]["q7"][0])
