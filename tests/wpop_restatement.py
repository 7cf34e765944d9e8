"""The summary of a weighted population restated in Python (fg_wpop_plan.h): units, moments over the fixed tree on the
particle index, the radix select with its pass count, the tables -- and, independent of the selection, the brute-force definitions
the tests hold it against.  Integers are numpy uint64 or Python ints (exact), doubles are Python floats (IEEE, never fused)."""
import math
import struct
from collections import Counter

import numpy as np

SCALE = 2.0 ** 52
MOMENT_NAMES = ("W", "mean", "var", "std", "mcse", "n_used")
PROBS = (0.0, 0.025, 0.5, 0.975, 1.0)
PLANS = ((12, 65536), (3, 0), (5, 4))            # (digit_bits, capacity)
NAN = float("nan")


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def good(w):
    return 0.0 <= w <= 1.0


def units(w):
    """-> (q uint64 [N], T, n_bad, n_zero); round() of a float is half to even, as rint"""
    q = [round(v * SCALE) if good(v) else 0 for v in (float(v) for v in w)]
    n_bad = sum(1 for v in w if not good(float(v)))
    n_zero = sum(1 for v, u in zip(w, q) if good(float(v)) and u == 0)
    T = sum(q)
    assert T < 2 ** 53, "not normalised"
    return np.array(q, dtype=np.uint64), T, n_bad, n_zero


def keys(x):
    u = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | np.uint64(1 << 63))


def unkey(k):
    k = int(k)
    u = (k & (2 ** 63 - 1)) if k >> 63 else (~k & (2 ** 64 - 1))
    return struct.unpack("<d", struct.pack("<Q", u))[0]


def target(T, p):
    return min(T, max(1, math.ceil(p * float(T))))


# ---- moments ----------------------------------------------------------------------------------------------------------------
def leaf_weight(w, x):
    return w if good(w) and w > 0.0 and math.isfinite(x) else 0.0


def merge(a, b):
    if a[3] == 0:
        return b
    if b[3] == 0:
        return a
    W = a[0] + b[0]
    delta = b[1] - a[1]
    return (W, a[1] + delta * (b[0] / W), a[2] + b[2] + delta * delta * (a[0] * b[0] / W), a[3] + b[3])


def tree(elems, merge_fn):
    """stride s = 1, 2, 4, ...: element i (a multiple of 2 s) takes in i + s when that exists"""
    e = list(elems)
    s = 1
    while s < len(e):
        for i in range(0, len(e) - s, 2 * s):
            e[i] = merge_fn(e[i], e[i + s])
        s *= 2
    return e[0]


def moments(x, w):
    """one row -> [W, mean, var, std, mcse, n_used] as floats"""
    x, w = [float(v) for v in x], [float(v) for v in w]
    lw = [leaf_weight(a, b) for a, b in zip(w, x)]
    W, mean, ssd, n = tree([(a, b, 0.0, 1) if a > 0.0 else (0.0, 0.0, 0.0, 0) for a, b in zip(lw, x)], merge)
    if n == 0:
        return [0.0, NAN, NAN, NAN, NAN, 0.0]
    terms = []
    for a, b in zip(lw, x):
        u = a * (b - mean) if a > 0.0 else 0.0
        terms.append(u * u if a > 0.0 else 0.0)
    s2 = tree(terms, lambda a, b: a + b)
    var = ssd / W
    return [W, mean, var, math.sqrt(var), math.sqrt(s2) / W, float(n)]


# ---- quantiles --------------------------------------------------------------------------------------------------------------
def select(x, q, T, p, digit_bits, capacity):
    """one slot by the selection step of fg_wp_end_pass -> (value, passes over the row)"""
    if T == 0:
        return NAN, 0
    live = q > 0
    k, u = keys(x)[live], q[live]
    t, b, prefix, passes = target(T, p), 0, 0, 0
    while True:
        passes += 1
        if len(k) <= capacity:
            order = np.argsort(k, kind="stable")
            cum = 0
            for j in order:
                cum += int(u[j])
                if cum >= t:
                    return unkey(k[j]), passes
            raise AssertionError("the bucket holds fewer units than its target")
        if k.min() == k.max():
            return unkey(k.min()), passes
        w = min(digit_bits, 64 - b)
        nb = 1 << w
        digit = ((k >> np.uint64(64 - b - w)) & np.uint64(nb - 1)).astype(np.int64)
        U = np.zeros(nb, dtype=np.uint64)
        np.add.at(U, digit, u)
        cum, dg = 0, 0
        while dg < nb - 1:
            if cum + int(U[dg]) >= t:
                break
            cum += int(U[dg])
            dg += 1
        t -= cum
        prefix |= dg << (64 - b - w)
        b += w
        keep = digit == dg
        k, u = k[keep], u[keep]
        if b == 64:
            return unkey(prefix), passes


def quantiles(x, q, T, probs, digit_bits, capacity):
    """one row -> (values, passes), one entry per probability"""
    out = [select(x, q, T, p, digit_bits, capacity) for p in probs]
    return [v for v, _ in out], [n for _, n in out]


def quantile_brute(x, q, T, p):
    """the definition: a stable sort by key, the cumulative units in Python integers, the first value that reaches t"""
    if T == 0:
        return NAN
    t = target(T, p)
    ks = [int(v) for v in keys(x)]
    cum = 0
    for k, u in sorted(zip(ks, (int(v) for v in q)), key=lambda kv: kv[0]):
        cum += u
        if u and cum >= t:
            return unkey(k)
    raise AssertionError("unreachable: t <= T")


# ---- tables -----------------------------------------------------------------------------------------------------------------
def encode(values, unsigned):
    """typed integers -> the 8-byte cells of a row"""
    return np.array([int(v) & (2 ** 64 - 1) for v in values], dtype=np.uint64)


def table(values, q, T, lo, bins):
    """values: the row's integers (Python ints) -> dict(units [bins], below, above, min, max); min / max None when T == 0"""
    U, below, above = [0] * bins, 0, 0
    seen = []
    for v, u in zip(values, (int(a) for a in q)):
        if u == 0:
            continue
        seen.append(int(v))
        j = int(v) - lo
        if j < 0:
            below += u
        elif j >= bins:
            above += u
        else:
            U[j] += u
    return dict(units=U, below=below, above=above, min=min(seen) if seen else None, max=max(seen) if seen else None)


def table_counter(values, q):
    c = Counter()
    for v, u in zip(values, (int(a) for a in q)):
        if u:
            c[int(v)] += u
    return c


# ---- the rows and weights of the tests ----------------------------------------------------------------------------------------
ROW_KINDS = ("normal", "constant", "three", "zeros", "non_finite")
WEIGHT_KINDS = ("dirichlet", "uniform", "one", "quarter_zero", "tiny")


def row(kind, N, seed=0):
    rng = np.random.default_rng(1000 + seed)
    if kind == "normal":
        return rng.standard_normal(N)
    if kind == "constant":
        return np.full(N, 2.5)
    if kind == "three":                       # ties across digits
        return rng.choice(np.array([-1.5, 0.25, 3.0]), size=N)
    if kind == "zeros":                       # -0.0 below +0.0
        return rng.choice(np.array([-0.0, 0.0, -1.0, 1.0]), size=N)
    if kind == "non_finite":
        x = rng.standard_normal(N)
        for j, v in enumerate((-np.inf, np.inf, np.nan)):
            x[(3 * j + 1) % N::7] = v
        return x
    raise ValueError(kind)


def weights(kind, N, seed=0):
    rng = np.random.default_rng(2000 + seed)
    if kind == "dirichlet":
        g = rng.gamma(0.7, size=N)
        return g / g.sum()
    if kind == "uniform":
        return np.full(N, 1.0 / N)
    if kind == "one":
        w = np.zeros(N)
        w[N // 2] = 1.0
        return w
    if kind == "quarter_zero":
        g = rng.gamma(0.7, size=N)
        g[::4] = 0.0
        s = g.sum()
        return g / s if s > 0 else g
    if kind == "tiny":                        # zero units each, counted in n_zero: T == 0
        return np.full(N, 2.0 ** -54)
    raise ValueError(kind)


def bad_weights(N, seed=0):
    """Dirichlet-like with a NaN, a -1 and a 2 put in (as far as N allows) -> (w, the exact number of bad ones)"""
    w = weights("dirichlet", N, seed).copy()
    put = [np.nan, -1.0, 2.0][:N]
    for j, v in enumerate(put):
        w[(j * 5) % N if N > 10 else j] = v
    return w, len(put)


def rows(kinds, N, seed=0):
    return np.stack([row(k, N, seed + 17 * j) for j, k in enumerate(kinds)])
