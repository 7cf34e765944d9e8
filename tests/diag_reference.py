"""A plain restatement of the documented diagnostics (fugue_amd/csrc/fg_diag.hip, fg_diag_host.cpp), for the tests of the
diagnostics kernels.  Not a GPU test, and nothing here calls the engine.

Two families:

* in-order float64 forms -- the operation order the kernel header documents, one IEEE operation at a time (numpy's
  elementwise add / multiply / divide round once each, and the loops below run over the draw index, so every chain sees
  exactly the sequence of operations a kernel thread performs).  They pin per-chain results to the bit.
* high-precision forms (`numpy.longdouble` about a pivot, `math.fsum`) of the same quantities and of the combined statistics:
  split R-hat, multi-chain ESS (Geyer pairs, monotone correction, cap 2 048), pooled mean / std, Geweke z (cap 1 024).  The
  ESS form also returns `max_t` and the number of monotone corrections; the Geweke form the number of lags each segment summed.

The seeded inputs of tests/test_gpu_diag_edges.py live here as well, so that tests/test_diag_reference_cpu.py can prove on
the CPU, from the reference alone, that each input reaches the path it is named for.
"""
import math

import numpy as np

LD = np.longdouble
ESS_LAG_CAP = 2048          # mcmc_utils.rs:266
GEWEKE_LAG_CAP = 1024       # mcmc_utils.rs:406


# ---- in-order float64 forms ------------------------------------------------------------------------------------------
def chain_moments_inorder(x: np.ndarray) -> np.ndarray:
    """[n][d][C] -> [d][6][C]: mean and sum of squared deviations of the full chain, the first half [0, n/2) and the second
    half [n/2, 2 (n/2)), in k_diag_moments' order: three running sums in one sweep (the first half's sum IS the running sum
    at t = n/2 - 1), a division each, then three running sums of squared deviations.  n = 1: the half means are NaN."""
    x = np.asarray(x, dtype=np.float64)
    n, d, C = x.shape
    half = n // 2
    s_full, s_h1, s_h2 = np.zeros((d, C)), np.zeros((d, C)), np.zeros((d, C))
    for t in range(n):
        s_full = s_full + x[t]
        if t == half - 1:
            s_h1 = s_full.copy()
        if half <= t < 2 * half:
            s_h2 = s_h2 + x[t]
    m_full = s_full / float(n)
    m_h1 = s_h1 / float(half) if half > 0 else np.full((d, C), np.nan)
    m_h2 = s_h2 / float(half) if half > 0 else np.full((d, C), np.nan)
    q_full, q_h1, q_h2 = np.zeros((d, C)), np.zeros((d, C)), np.zeros((d, C))
    for t in range(n):
        a = x[t] - m_full
        q_full = q_full + a * a
        if t < half:
            b = x[t] - m_h1
            q_h1 = q_h1 + b * b
        elif t < 2 * half:
            b = x[t] - m_h2
            q_h2 = q_h2 + b * b
    return np.stack([m_full, q_full, m_h1, q_h1, m_h2, q_h2], axis=1)


def chain_autocov_inorder(x: np.ndarray, lag: int) -> np.ndarray:
    """[n][d][C] -> [d][C]: the biased lag autocovariance (1/n) sum_i c_i c_{i + lag} of every chain, c = x - mean with the
    in-order mean of chain_moments_inorder, the products added in ascending i (k_diag_autocov; mcmc_utils.rs:231-244)."""
    x = np.asarray(x, dtype=np.float64)
    n, d, C = x.shape
    s = np.zeros((d, C))
    for t in range(n):
        s = s + x[t]
    c = x - (s / float(n))
    acc = np.zeros((d, C))
    for i in range(n - lag):
        acc = acc + c[i] * c[i + lag]
    return acc / float(n)


def pooled_autocov_fsum(x: np.ndarray, lag: int):
    """([d] fsum over chains of the in-order per-chain autocovariances, [d] sum over chains of their magnitudes): the
    centre and the scale of the bound on fg_diag_autocov_sums' fixed summation tree."""
    a = chain_autocov_inorder(x, lag)
    return (np.array([math.fsum(row) for row in a]), np.array([math.fsum(np.abs(row)) for row in a]))


def pooled_autocov_bound(C: int, scale: np.ndarray) -> np.ndarray:
    """The tree of k_diag_autocov + k_diag_acov_finish puts at most 6 shuffle adds, 3 wave adds and nblk block adds on any
    path from a chain's value to the result; each add loses at most half an ulp of a partial sum that never exceeds
    sum_c |acov_c| (1 + small), so (9 + nblk) 2^-52 sum_c |acov_c| bounds the difference from the exact sum with a factor
    of two to spare."""
    nblk = (C + 255) // 256
    return (9 + nblk) * 2.0 ** -52 * scale


# ---- high-precision forms ----------------------------------------------------------------------------------------------
def _pivoted(col: np.ndarray):
    """[n][C] float64 -> (longdouble values about a pivot, the pivot).  Subtracting one of the column's own values in
    extended precision is exact for every input used here (equal or neighbouring exponents), and keeps what follows at the
    scale of the deviations: this is what makes the forms below insensitive to an offset of 1e8."""
    col = np.asarray(col, dtype=np.float64)
    pivot = LD(col.flat[0]) if col.size else LD(0)
    return col.astype(LD) - pivot, pivot


def _lsum(a) -> LD:
    return np.sum(np.asarray(a, dtype=LD), dtype=LD)


def _rhat_ld(means, ssds, m, n):                     # diagnostics.rs:262-304
    if m < 2:
        return 1.0
    if n == 0:
        return float("nan")
    mf, nf = LD(m), LD(n)
    overall = _lsum(means) / mf
    with np.errstate(all="ignore"):
        b = nf / (mf - 1) * _lsum((means - overall) ** 2)
        w = _lsum(ssds / (nf - 1)) / mf
        var_plus = ((nf - 1) / nf) * w + (1 / nf) * b
        return float(np.sqrt(var_plus / w))


def split_rhat_hp(col: np.ndarray) -> float:
    """Split R-hat of one coordinate, [n][C] (r_hat_f64: diagnostics.rs:218-224, 240-304)."""
    y, _ = _pivoted(col)
    n, m = y.shape
    half = n // 2
    if half == 0:
        mean = y.sum(axis=0, dtype=LD) / LD(max(n, 1))
        return _rhat_ld(mean, ((y - mean) ** 2).sum(axis=0, dtype=LD), m, n)
    parts = [y[:half], y[half:2 * half]]
    means = np.stack([p.sum(axis=0, dtype=LD) / LD(half) for p in parts], axis=1).ravel()          # c0h0, c0h1, c1h0, ...
    ssds = np.stack([((p - p.sum(axis=0, dtype=LD) / LD(half)) ** 2).sum(axis=0, dtype=LD) for p in parts], axis=1).ravel()
    return _rhat_ld(means, ssds, 2 * m, half)


def pooled_mean_std_hp(col: np.ndarray):
    """Mean and sample standard deviation of all m n values (summarize_f64_parameter: diagnostics.rs:331-352)."""
    y, pivot = _pivoted(col)
    N = y.size
    mean = _lsum(y) / LD(N)
    with np.errstate(all="ignore"):
        std = np.sqrt(_lsum((y - mean) ** 2) / LD(N - 1)) if N > 1 else LD("nan")
    return float(mean + pivot), float(std)


def ess_hp(col: np.ndarray, lag_cap: int = ESS_LAG_CAP) -> dict:
    """effective_sample_size_multichain of one coordinate, [n][C] (ess_from_chains: mcmc_utils.rs:253-339).  Returns ess,
    tau before the clamp at 1, max_t (the last lag of the initial positive sequence) and `corrected`, the number of pairs the
    monotone correction replaced (cur > prev)."""
    with np.errstate(invalid="ignore"):                      # non-finite draws are an input here, not an accident
        return _ess_hp(col, lag_cap)


def _ess_hp(col, lag_cap):
    y, _ = _pivoted(col)
    n, m = y.shape
    out = dict(ess=0.0, tau=float("nan"), max_t=0, corrected=0, rho=[])
    if m == 0:
        return out
    if n < 4:
        out["ess"] = float(max(m * n, 1))
        return out
    max_lag = min(n - 1, lag_cap)
    nf, mf = LD(n), LD(m)
    means = y.sum(axis=0, dtype=LD) / nf
    c = y - means

    def acov_mean(t):
        return _lsum((c[:n - t] * c[t:]).sum(axis=0, dtype=LD) / nf) / mf

    mean_var = acov_mean(0) * nf / (nf - 1)
    if not mean_var > 0 and not np.isnan(mean_var):          # `mean_var <= 0.0`: false for NaN, like the reference
        out["ess"] = float(m * n)
        return out
    var_plus = mean_var * (nf - 1) / nf
    if m > 1:
        var_plus = var_plus + _lsum((means - _lsum(means) / mf) ** 2) / (mf - 1)

    def rho(t):
        return 1 - (mean_var - acov_mean(t)) / var_plus

    rho_hat = [LD(0)] * (max_lag + 1)
    rho_hat[0] = LD(1)
    if max_lag >= 1:
        rho_hat[1] = rho(1)
    t, max_t = 1, min(1, max_lag)
    while t + 2 <= max_lag:
        re, ro = rho(t + 1), rho(t + 2)
        if re + ro < 0:
            break
        rho_hat[t + 1], rho_hat[t + 2] = re, ro
        max_t = t + 2
        t += 2
    out["rho"] = [float(r) for r in rho_hat[:max_t + 1]]
    k = 1
    while k + 2 <= max_t:
        prev, cur = rho_hat[k - 1] + rho_hat[k], rho_hat[k + 1] + rho_hat[k + 2]
        if cur > prev:
            rho_hat[k + 1] = rho_hat[k + 2] = prev / 2
            out["corrected"] += 1
        k += 2
    tau = -1 + 2 * _lsum(rho_hat[:max_t + 1])
    out["tau"], out["max_t"] = float(tau), max_t
    out["ess"] = float(LD(m * n) / (tau if tau > 1 else LD(1)))          # f64::max(tau, 1.0): a NaN tau gives 1.0
    return out


def stats_hp(col: np.ndarray) -> dict:
    """The four figures fg_diag_rhat_ess reports for one coordinate [n][C], in high precision."""
    mean, std = pooled_mean_std_hp(col)
    return dict(r_hat=split_rhat_hp(col), ess=ess_hp(col)["ess"], mean=mean, std=std)


def _spectral_var_of_mean_hp(seg: np.ndarray, lag_cap):
    """spectral_variance_of_mean (mcmc_utils.rs:392-421) -> (value, number of lags added to tau)."""
    k = len(seg)
    if k < 2:
        return LD(0), 0
    y, _ = _pivoted(seg)
    c = y - _lsum(y) / LD(k)
    q = _lsum(c * c)
    s2 = q / (LD(k) - 1)
    if s2 == 0:
        return LD(0), 0
    max_lag = k - 1 if lag_cap is None else min(k - 1, lag_cap)
    var0 = q / LD(k)
    tau, lags = LD(1), 0
    for lag in range(1, max_lag + 1):
        r = _lsum(c[:k - lag] * c[lag:]) / LD(k) / var0
        if r <= 0:
            break
        tau = tau + 2 * r
        lags += 1
    return s2 * tau / LD(k), lags


def geweke_hp(chain: np.ndarray, lag_cap=GEWEKE_LAG_CAP):
    """geweke_diagnostic (mcmc_utils.rs:354-384) of one chain -> (z, (lags summed by the first-10 % segment, by the
    last-50 % segment)).  `lag_cap=None` lifts the cap of 1 024 lags."""
    x = np.asarray(chain, dtype=np.float64)
    n = len(x)
    if n < 20:
        return float("nan"), (0, 0)
    a, b = x[:n // 10], x[n // 2:]
    if len(a) < 2 or len(b) < 2:
        return float("nan"), (0, 0)
    va, la = _spectral_var_of_mean_hp(a, lag_cap)
    vb, lb = _spectral_var_of_mean_hp(b, lag_cap)
    se = np.sqrt(va + vb)
    if se == 0:
        return 0.0, (la, lb)
    pa, pivot = _pivoted(a)
    mean_a = _lsum(pa) / LD(len(a))
    mean_b = _lsum(b.astype(LD) - pivot) / LD(len(b))
    return float((mean_a - mean_b) / se), (la, lb)


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------
def ar1(rng, n, m, phi):
    x = np.zeros((n, m))
    x[0] = rng.standard_normal(m) / np.sqrt(1 - phi ** 2)
    for t in range(1, n):
        x[t] = phi * x[t - 1] + rng.standard_normal(m)
    return x


# three visibly different columns: (offset, scale) of column j; the autocorrelation differs per case below
COLUMNS = ((0.0, 1.0), (3.0, 0.125), (-50.0, 20.0))


def _columns(cols):
    return np.ascontiguousarray(np.stack([off + sc * c for (off, sc), c in zip(COLUMNS, cols)], axis=1))


def three_columns(seed: int, n: int, C: int, phis=(0.9, 0.5, -0.3)) -> np.ndarray:
    """[n][3][C]: AR(1) columns of different offset, scale and autocorrelation."""
    rng = np.random.default_rng(seed)
    return _columns([ar1(rng, n, C, p) for p in phis])


def rhat_ess_case(name: str) -> np.ndarray:
    """The [n][3][C] input of the fg_diag_rhat_ess case `name` (cases a-h; e and f carry their n and C in the name)."""
    seed = sum(ord(ch) * (k + 1) for k, ch in enumerate(name))
    rng = np.random.default_rng(seed)
    if name == "a_multiblock":                       # AR(1) phi = 0.9 at C = 600, n = 100: sums over three blocks
        return _columns([ar1(rng, 100, 600, p) for p in (0.9, 0.7, 0.5)])
    if name == "b_deep_window":                      # AR(1) phi = 0.99, C = 6, n = 3 000: the window runs many chunks deep
        return _columns([ar1(rng, 3000, 6, p) for p in (0.99, 0.98, 0.97)])
    if name == "c_cap_2048":                         # iid N(mu_j, 1), mu_j spread over +-10: rho stays positive to the cap
        return _columns([np.linspace(-s, s, 5)[None, :] + rng.standard_normal((2100, 5)) for s in (10.0, 8.0, 6.0)])
    if name == "d_monotone":                         # chain offsets + a period-12 wave: pair sums rise again while positive
        t = np.arange(240)[:, None]
        return _columns([np.linspace(-1.5, 1.5, 8)[None, :] + a * np.sin(2 * np.pi * (t / p + rng.random(8)[None, :])) + 0.3 * rng.standard_normal((240, 8))
                         for a, p in ((1.0, 12.0), (0.8, 10.0), (1.2, 16.0))])
    if name.startswith("e_n"):                       # n - 1 = 31 / 32 / 33 with positive rho throughout
        n = int(name[3:])
        return _columns([np.linspace(-s, s, 5)[None, :] + rng.standard_normal((n, 5)) for s in (10.0, 8.0, 6.0)])
    if name.startswith("f_n"):                       # f_n{3,4,5}_c{1,2}: the n < 4 rule; one chain still splits in two
        n, C = int(name[3]), int(name[6])
        return _columns([ar1(rng, n, C, p) for p in (0.5, 0.2, -0.2)])
    if name == "g_antithetic":                       # phi = -0.9: tau clamps at 1, ESS = m n
        return _columns([ar1(rng, 200, 8, p) for p in (-0.9, -0.8, -0.7)])
    if name == "h_constant":                         # exactly summable constants: every sum of them is exact
        return np.ascontiguousarray(np.broadcast_to(np.array([2.5, -4.0, 1024.5])[None, :, None], (50, 3, 70)))
    raise KeyError(name)


RHAT_ESS_CASES = ("a_multiblock", "b_deep_window", "c_cap_2048", "d_monotone", "e_n32", "e_n33", "e_n34",
                  "f_n3_c1", "f_n3_c2", "f_n4_c1", "f_n4_c2", "f_n5_c1", "f_n5_c2", "g_antithetic", "h_constant")


def conditioning_input() -> np.ndarray:
    """[200][3][300]: 1e8 + 1e-3 N(0, 1) -- twelve of a double's sixteen digits go to the offset.  The three columns differ in
    offset (1e8, 1e8 + 3, 1e8 - 50), scale (1e-3, 2e-3, 3e-3) and autocorrelation (0, 0.3, 0.6) like every other input."""
    rng = np.random.default_rng(1008)
    cols = [ar1(rng, 200, 300, p) * np.sqrt(1 - p * p) for p in (0.0, 0.3, 0.6)]
    return np.ascontiguousarray(np.stack([1e8 + off + 1e-3 * (1 + j) * c for j, ((off, _), c) in enumerate(zip(COLUMNS, cols))], axis=1))


FIGURE_TOL = dict(r_hat=1e-10, ess=1e-8, mean=1e-11, std=1e-10)          # test_native_rhat_ess_entry_point_and_geweke's


def oracle_deviation(oracle, x: np.ndarray) -> list:
    """Per column of x [n][d][C]: the relative deviation of the oracle's float64 R-hat / ESS / mean / std from the
    high-precision forms -- how far a faithful float64 restatement of the reference lands on this input.  Measured on the
    CPU, from the oracle alone; a GPU test scales its tolerance by it and never by what the engine returns."""
    out = []
    for i in range(x.shape[1]):
        col = x[:, i, :]
        ch = np.ascontiguousarray(col.T)
        hp, s = stats_hp(col), oracle.summarize(ch)
        got = dict(r_hat=oracle.split_rhat(ch), ess=oracle.ess_multichain(ch), mean=s["mean"], std=s["std"])
        out.append({k: abs(got[k] - hp[k]) / abs(hp[k]) for k in hp})
    return out


def conditioning_tolerance(oracle, x: np.ndarray) -> list:
    """Per column: {figure: (relative tolerance, the oracle's own deviation)}; tolerance = max(the usual one, 4 x deviation)."""
    return [{k: (max(FIGURE_TOL[k], 4.0 * dev[k]), dev[k]) for k in dev} for dev in oracle_deviation(oracle, x)]


def nonfinite_input():
    """([96][3][70] clean draws, the same with one NaN in one chain of column 0 and one +inf in one chain of column 1)."""
    clean = three_columns(77, 96, 70)
    bad = clean.copy()
    bad[41, 0, 13] = np.nan
    bad[17, 1, 64] = np.inf
    return clean, bad


def geweke_input(n: int, C: int) -> np.ndarray:
    """[n][3][C]: column 0 AR(1); column 1 constant on its first 10 % only; column 2 fully constant (z = 0)."""
    rng = np.random.default_rng(1000 * n + C)
    x = _columns([ar1(rng, n, C, 0.6), ar1(rng, n, C, 0.3), np.zeros((n, C))])
    x[:n // 10, 1, :] = 2.75
    x[:, 2, :] = -50.0
    return x


def geweke_cap_input(n: int = 7200, C: int = 3) -> np.ndarray:
    """[n][3][C]: a ramp plus small noise.  The lag autocorrelation of a ramp of k draws stays positive up to about 0.29 k, so
    the last 50 % (3 600 draws) is still positive at lag 1 024 and the cap ends the sum."""
    rng = np.random.default_rng(7200)
    t = np.arange(n)[:, None] / float(n)
    return _columns([s * t + 0.01 * rng.standard_normal((n, C)) for s in (1.0, -2.0, 0.5)])
