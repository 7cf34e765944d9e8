"""A numpy restatement of the rank-normalised diagnostics' rule (fugue_amd/csrc/fg_diag_rank_plan.h; Vehtari, Gelman,
Simpson, Carpenter, Buerkner 2021): the value key, the doubled average ranks from np.sort + searchsorted on the keys, the normal
score through integer numerators and Wichura's AS241 PPND16 operation by operation, the median, the folded pass, the tail indicators
and the counts.  The figures come from the oracle's split R-hat and multi-chain ESS on the transformed rows in their [n][C] layout.
No device and no library of the product enters."""
import math

import numpy as np

WORD_NAMES = ("rhat_rank", "rhat_bulk", "rhat_folded", "ess_bulk", "ess_tail", "ess_lower", "ess_upper", "median", "x_lo", "x_hi")
COUNT_NAMES = ("n_cells", "n_runs", "longest_run", "n_nan", "n_neg_inf", "n_pos_inf", "n_nan_folded", "n_passes")
NAN_KEY = np.uint64(0xFFF8000000000000)
TOP = np.uint64(0x8000000000000000)
TILE, RUN_TILE = 4096, 1024                      # positions of a block of a radix pass / of the run pass (the tests aim at their edges)

# AS241 PPND16, highest power first
A = (2.5090809287301226727e+3, 3.3430575583588128105e+4, 6.7265770927008700853e+4, 4.5921953931549871457e+4,
     1.3731693765509461125e+4, 1.9715909503065514427e+3, 1.3314166789178437745e+2, 3.3871328727963666080e+0)
B = (5.2264952788528545610e+3, 2.8729085735721942674e+4, 3.9307895800092710610e+4, 2.1213794301586595867e+4,
     5.3941960214247511077e+3, 6.8718700749205790830e+2, 4.2313330701600911252e+1, 1.0)
CC = (7.74545014278341407640e-4, 2.27238449892691845833e-2, 2.41780725177450611770e-1, 1.27045825245236838258e+0,
      3.64784832476320460504e+0, 5.76949722146069140550e+0, 4.63033784615654529590e+0, 1.42343711074968357734e+0)
D = (1.05075007164441684324e-9, 5.47593808499534494600e-4, 1.51986665636164571966e-2, 1.48103976427480074590e-1,
     6.89767334985100004550e-1, 1.67638483018380384940e+0, 2.05319162663775882187e+0, 1.0)
EE = (2.01033439929228813265e-7, 2.71155556874348757815e-5, 1.24266094738807843860e-3, 2.65321895265761230930e-2,
      2.96560571828504891230e-1, 1.78482653991729133580e+0, 5.46378491116411436990e+0, 6.65790464350110377720e+0)
F = (2.04426310338993978564e-15, 1.42151175831644588870e-7, 1.84631831751005468180e-5, 7.86869131145613259100e-4,
     1.48753612908506148525e-2, 1.36929880922735805310e-1, 5.99832206555887937690e-1, 1.0)


# The restatement's z against mpmath's inverse normal CDF at 50 digits (tests/test_diag_rank_cpu.py measures it again): the largest
# relative deviation over every doubled rank of S = 1, 2, 21, 4 096 and 2 000 ranks spread over S = 2^31 - 1, and four times that --
# so that a last-place difference of log between two machines cannot trip a comparison -- as the tolerance of the tails.
Z_MEASURED_DEV = 5.9e-16
Z_TOL = 4.0 * Z_MEASURED_DEV


def big_ranks(S=2 ** 31 - 1):
    """2 000 doubled ranks spread over S = 2^31 - 1: both ends one by one, the lower half geometrically, the upper half evenly"""
    r = np.r_[np.arange(2, 502), 2 * S + 2 - np.arange(2, 502), np.geomspace(502, S, 500).astype(np.int64), np.linspace(S + 1, 2 * S - 501, 500).astype(np.int64)]
    r = np.unique(r)
    assert r.size == 2000
    return r


def inputs(S, seed):
    """the named pooled inputs of the tests, S cells each (S >= 1); `tie_runs` aims at the sort's tile and the run pass's tile"""
    rng = np.random.default_rng(seed)
    one = np.array([1.5]).view(np.uint64)[0]
    out = {
        "normal": rng.normal(size=S),
        "cauchy": rng.standard_cauchy(size=S),
        "thirds": np.round(rng.normal(size=S) * 3.0) / 3.0,
        "constant": np.full(S, -2.75),
        "low_byte": ((one & ~np.uint64(255)) | rng.integers(0, 256, size=S).astype(np.uint64)).view(np.float64),
        "top_byte": ((rng.integers(0x30, 0x50, size=S).astype(np.uint64) << np.uint64(56)) | np.uint64(0x0008765432100000)).view(np.float64),
    }
    t = rng.normal(size=S)
    if S > 8:
        srt = np.sort(t)
        a, b = S // 3, min(S - 1, S // 3 + TILE + 37)              # one run longer than a radix tile (where S allows) ...
        srt[a:b] = srt[a]
        c = (b // TILE + 1) * TILE
        if c + 5 < S:
            srt[c - 5:c + 5] = srt[c - 5]                            # ... and a short one that straddles a block boundary of both passes
        t = rng.permutation(srt)
    out["tie_runs"] = t
    z = rng.normal(size=S)
    z[rng.integers(0, S, size=max(1, S // 7))] = 0.0
    z[rng.integers(0, S, size=max(1, S // 7))] = -0.0
    z[rng.integers(0, S, size=max(1, S // 9))] = 5e-324
    z[rng.integers(0, S, size=max(1, S // 9))] = -2.5e-310
    out["zeros_denormals"] = z
    i = rng.normal(size=S)
    i[rng.integers(0, S, size=max(1, S // 11))] = np.inf
    i[rng.integers(0, S, size=max(1, S // 13))] = -np.inf
    out["infs"] = i
    m = rng.normal(size=S)
    m[rng.integers(0, S, size=max(1, S // 17))] = np.nan
    m[rng.integers(0, S, size=max(1, S // 19))] = -np.nan
    out["nans"] = m
    return out


def scipy_r2(x):
    """2 x scipy.stats.rankdata (average ranks) after -0.0 -> 0.0; NaN cells (columns without +inf) rank as the top value"""
    from scipy.stats import rankdata
    x = np.asarray(x, dtype=np.float64)
    x = np.where(x == 0.0, 0.0, x)
    if np.isnan(x).any():
        assert not (x == np.inf).any()
        x = np.where(np.isnan(x), np.inf, x)
    return np.rint(2.0 * rankdata(x, method="average")).astype(np.int64)


def keys(x):
    """ascending in the doubles' order; -0.0 keyed as +0.0; every NaN on one key above +inf"""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    x = np.where(x == 0.0, 0.0, x)
    u = x.view(np.uint64)
    k = np.where((u >> np.uint64(63)) != 0, ~u, u | TOP)
    return np.where(np.isnan(x), NAN_KEY, k).astype(np.uint64)


def unkey(k):
    k = np.uint64(k)
    if k == NAN_KEY:
        return float("nan")
    u = (k & ~TOP) if (k >> np.uint64(63)) else ~k
    return float(np.array([u], dtype=np.uint64).view(np.float64)[0])


def _horner(c, r):
    v = np.full_like(r, c[0])
    for ci in c[1:]:
        v = v * r + ci
    return v


def q_of(r2, S):
    return (2 * np.asarray(r2, dtype=np.int64) - 2 * S - 2).astype(np.float64) / np.float64(4 * S + 1)


def central(r2, S):
    return np.abs(q_of(r2, S)) <= 0.425


def z_of(r2, S):
    """fg_rank_z for an array of doubled ranks"""
    r2 = np.atleast_1d(np.asarray(r2, dtype=np.int64))
    q = q_of(r2, S)
    cen = np.abs(q) <= 0.425
    out = np.empty(r2.shape, dtype=np.float64)
    r = 0.180625 - q[cen] * q[cen]
    out[cen] = _horner(A, r) * q[cen] / _horner(B, r)
    a = 4 * r2[~cen] - 3
    pt = np.minimum(a, 8 * S + 2 - a).astype(np.float64) / np.float64(8 * S + 2)
    r = np.sqrt(-np.array([math.log(v) for v in pt], dtype=np.float64))        # the C library's log, one cell at a time
    near = r <= 5.0
    x = np.empty(r.shape, dtype=np.float64)
    x[near] = _horner(CC, r[near] - 1.6) / _horner(D, r[near] - 1.6)
    x[~near] = _horner(EE, r[~near] - 5.0) / _horner(F, r[~near] - 5.0)
    out[~cen] = np.where(q[~cen] < 0.0, -x, x)
    return out


def ranks(x):
    """-> lo, hi (int64 per cell) and the sorted keys"""
    k = keys(x)
    s = np.sort(k)
    return np.searchsorted(s, k, side="left").astype(np.int64), np.searchsorted(s, k, side="right").astype(np.int64), s


def median_of(s):
    S = s.size
    a, b = unkey(s[(S - 1) // 2]), unkey(s[S // 2])
    return a if a == b else 0.5 * a + 0.5 * b


def kp(S, p):
    return int(math.floor(float(S - 1) * p))


def passes_run(k):
    """radix passes of one sort: the 8-bit digits that are not equal in every cell"""
    return sum(1 for p in range(8) if np.unique((k >> np.uint64(8 * p)) & np.uint64(255)).size > 1)


def transform(x, probs=(0.05, 0.95)):
    """one coordinate's pooled cells x [S] (cell i = draw i // C, chain i % C) -> dict of the rows, r2, median and counts"""
    x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
    S = x.size
    lo, hi, s = ranks(x)
    r2 = lo + hi + 1
    med = median_of(s)
    with np.errstate(invalid="ignore"):
        folded = np.abs(x - med)
    flo, fhi, _ = ranks(folded)
    k_lo, k_hi = kp(S, probs[0]), kp(S, probs[1])
    starts = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])
    counts = dict(n_cells=S, n_runs=int(starts.size), longest_run=int(np.diff(np.r_[starts, S]).max()), n_nan=int(np.isnan(x).sum()), n_neg_inf=int((x == -np.inf).sum()),
                  n_pos_inf=int((x == np.inf).sum()), n_nan_folded=int(np.isnan(folded).sum()), n_passes=passes_run(keys(x)) + passes_run(keys(folded)))
    return dict(r2=r2, z=z_of(r2, S), z_folded=z_of(flo + fhi + 1, S), i_lo=(lo <= k_lo).astype(np.float64), i_hi=(lo <= k_hi).astype(np.float64), median=med,
                x_lo=unkey(s[k_lo]), x_hi=unkey(s[k_hi]), central=central(r2, S), central_folded=central(flo + fhi + 1, S), counts=counts)


def figures_from_rows(rows, counts, median, x_lo, x_hi):
    """rows [n][4][C] (z, z_folded, I_lo, I_hi) -> the ten words, through the oracle's combination"""
    from oracle import oracle as orc
    rows = np.ascontiguousarray(rows, dtype=np.float64)
    rh = [orc.split_rhat(np.ascontiguousarray(rows[:, i, :].T)) for i in range(4)]
    es = [orc.ess_multichain(np.ascontiguousarray(rows[:, i, :].T)) for i in range(4)]
    nan = float("nan")
    rb, rf = rh[0], (nan if counts["n_nan_folded"] > 0 else rh[1])
    w = dict(rhat_bulk=rb, rhat_folded=rf, rhat_rank=nan if (math.isnan(rb) or math.isnan(rf)) else max(rb, rf), ess_bulk=es[0], ess_lower=es[2], ess_upper=es[3],
             median=median, x_lo=x_lo, x_hi=x_hi)
    w["ess_tail"] = nan if (math.isnan(es[2]) or math.isnan(es[3])) else min(es[2], es[3])
    if counts["n_nan"] > 0:
        w = {k: nan for k in w}
    return w


def coordinate(draws, j, probs=(0.05, 0.95)):
    """draws [n][d][C], coordinate j -> the transform (rows reshaped to [n][C]) and the figures"""
    draws = np.ascontiguousarray(draws, dtype=np.float64)
    n, _, C = draws.shape
    t = transform(draws[:, j, :].reshape(-1), probs)
    rows = np.stack([t[k].reshape(n, C) for k in ("z", "z_folded", "i_lo", "i_hi")], axis=1)
    t["rows"] = rows
    t["figures"] = figures_from_rows(rows, t["counts"], t["median"], t["x_lo"], t["x_hi"])
    return t
