"""A judge for next_beta's answer: is beta' a root of ESS(b) = target to working precision?

adaptive_smc's tempering step (smc.rs:588-622) bisects [beta, 1] 64 times on `ESS(mid) < target`, with ESS evaluated in doubles.  The
device reaches its answer another way (zoom passes, then a replay of the halvings) and evaluates ESS in another form
(sum_i E_i R_i^j instead of two log-sum-exps).  Where the evaluated ESS is monotone both give the same bits; inside the band where rounding
makes the evaluated ESS wiggle, either answer is a root to working precision.  This module says what "to working precision" means and checks
it against an ESS evaluated at 40 significant digits from the exact double inputs.

Under uniform incoming weights, ESS(b) = (sum_i t_i)^2 / sum_i t_i^2 with t_i = exp((b - beta)(ll_i - L)), L = max ll.

Criterion (`accept`).  An answer beta' is accepted against the oracle's answer if it equals it bit for bit, or if
  * beta' is found, not clamped (neither 1 nor beta + 1e-9, smc.rs:604-607 / :621), and with lo' = beta' - max(2^-64 (1 - beta), ulp(beta'))
    -- no wider than the reference's final bracket -- the exact ESS satisfies ESS(lo') >= target (1 - D) and ESS(beta') <= target (1 + D).
    So beta' is the upper end of a bracket no wider than the reference's, and the exact ESS crosses the target across it to within D;
  * or beta' is a clamp the oracle did not take, and the exact ESS puts the crossing there to within D: beta' = 1 needs
    ESS(1) >= target (1 - D) (smc.rs:604-607), beta' = beta + 1e-9 needs ESS(beta + 1e-9) <= target (1 + D) -- the crossing lies in
    [beta, beta + 1e-9], where ESS(beta) = n.  (This only arises where the exact ESS stays within D of the target over a long stretch --
    a target of n, which ESS reaches only at b = beta -- so that which side of it a double evaluation falls on is rounding; a clamp away
    from the crossing fails by the whole ESS change.)

D (`delta`) bounds the error of an ESS evaluated in doubles, relative to the exact value at the same double b, in the form of the answer
being judged -- the device's (`accept`) or the reference's (reference=True: the CPU tests of the judge itself):
  * each term t_i = exp(y_i), y_i = (b - beta)(ll_i - L), carries the rounding of its exponent -- (b - beta), ll_i - L and their product,
    about 3 eps |y_i| -- and of exp and the few multiplications of the product form E_i R_i^j (up to 8 roundings, plus j (<= 8) times the
    exponent error of R): a relative error of at most ~4 eps (1 + |y_i|) per term, and 8 eps (1 + |y_i|) for t_i^2.  ESS = s1^2 / s2 then
    carries 2 * 4 + 8 = 16 eps (1 + Y), Y = max |y_i| over the particles whose term is not negligible (t_i >= eps / n: the others add less
    than eps to the sums whatever their error);
  * summation: the sums are positive, so each has a relative error of at most eps per addition on the longest path, three times that for
    s1^2 / s2.  The device's fixed tree has k items per thread, then ~24 levels of lanes, waves, blocks and partials: 3 (k + 24) eps.
    The reference's sequential sums have n - 1 additions on the path -- and with tied values their roundings do not cancel (adding the same
    term again and again rounds the same way) -- 3 (n - 1) eps;
  * the reference's form v_i = lw0 + (b - beta) ll_i and its two log-sum-exps also round v at the scale of |lw0| + |(b - beta) L|: 4 eps
    (ln n + |(b - beta) L|) more.
Device: D = eps (16 (1 + Y) + 3 (k + 24)); reference: D = eps (16 (1 + Y) + 3 (n - 1) + 4 (ln n + |(b - beta) L|)); both capped at 1e-10.

Every acceptance that is not bit-identical is reported through knife.used with the case, both betas, ESS(beta') / target - 1 and the
side that was not bitwise."""
from __future__ import annotations

import math

import mpmath
import numpy as np

from tests import knife

EPS = 2.0 ** -52
DPS = 40
DELTA_CAP = 1e-10
ESS2_BLOCKS, ESS2_THREADS = 256, 512            # fg_smc.hip: the grid of k_smc_ess2_pass (the per-thread depth of the device's sums)


class Curve:
    """ESS(b) of one log-likelihood array under uniform incoming weights, at DPS digits.  Particles are grouped by value (ties cost one
    exp), and terms below exp(-(DPS ln 10 + ln n + 10)) of the largest (which is 1) are dropped: they cannot move a DPS-digit sum."""

    def __init__(self, ll, beta):
        self.ll = np.asarray(ll, dtype=np.float64)
        self.n = self.ll.size
        self.beta = float(beta)
        fin = self.ll[np.isfinite(self.ll)]
        self.nonfinite = bool(np.isnan(self.ll).any() or np.isposinf(self.ll).any())
        self.L = float(fin.max()) if fin.size else -math.inf
        vals, counts = np.unique(fin, return_counts=True)
        self.vals, self.counts = vals, counts
        self.cut = DPS * math.log(10.0) + math.log(max(self.n, 1)) + 10.0

    def _terms(self, b):
        """(y as doubles, mp exponents, counts) of the terms that matter at b"""
        db = float(b) - self.beta                     # only for the filter; the exact exponent is formed in mp below
        x = self.vals - self.L
        keep = db * x > -(self.cut + 1.0)
        return x[keep], self.vals[keep], self.counts[keep]

    def ess(self, b):
        """the exact ESS at the double b (the reference's rule: n where the sums are not finite numbers)"""
        if self.nonfinite or not math.isfinite(self.L):
            return mpmath.mpf(self.n)
        with mpmath.workdps(DPS):
            db = mpmath.mpf(float(b)) - mpmath.mpf(self.beta)
            L = mpmath.mpf(self.L)
            _, vals, counts = self._terms(b)
            s1 = s2 = mpmath.mpf(0)
            for v, c in zip(vals.tolist(), counts.tolist()):
                t = mpmath.exp(db * (mpmath.mpf(v) - L))
                s1 += c * t
                s2 += c * t * t
            return s1 * s1 / s2

    def root(self, target, iters=200):
        """the exact crossing ESS(b) = target in (beta, 1], by bisection at DPS digits (b as an mp number, not a double)"""
        with mpmath.workdps(DPS):
            L, tgt = mpmath.mpf(self.L), mpmath.mpf(target)
            pairs = [(mpmath.mpf(v) - L, c) for v, c in zip(self.vals.tolist(), self.counts.tolist())]

            def ess(db):
                s1 = s2 = mpmath.mpf(0)
                for x, c in pairs:
                    t = mpmath.exp(db * x)
                    s1 += c * t
                    s2 += c * t * t
                return s1 * s1 / s2
            lo, hi = mpmath.mpf(0), mpmath.mpf(1) - mpmath.mpf(self.beta)
            for _ in range(iters):
                mid = (lo + hi) / 2
                if ess(mid) < tgt:
                    hi = mid
                else:
                    lo = mid
            return mpmath.mpf(self.beta) + hi

    def delta(self, b, reference=False):
        """D at b (module docstring) for an ESS evaluated in the device's form, or in the reference's"""
        db = float(b) - self.beta
        n = max(self.n, 1)
        if not math.isfinite(self.L):
            return DELTA_CAP
        with np.errstate(invalid="ignore", over="ignore"):
            y = db * (self.vals - self.L)
        y = y[np.isfinite(y) & (y >= math.log(EPS / n))]
        Y = float(np.abs(y).max()) if y.size else 0.0
        nb = min(ESS2_BLOCKS, (n + ESS2_THREADS - 1) // ESS2_THREADS)
        k = -(-n // (nb * ESS2_THREADS))
        if reference:
            d = EPS * (16.0 * (1.0 + Y) + 3.0 * (n - 1) + 4.0 * (math.log(n) + abs(db * self.L)))
        else:
            d = EPS * (16.0 * (1.0 + Y) + 3.0 * (k + 24))
        return min(d, DELTA_CAP)


def lo_prime(beta, b):
    """the lower end of the bracket beta' closes: no wider than the reference's final bracket, at least one ulp"""
    return b - max(2.0 ** -64 * (1.0 - beta), math.ulp(b))


def clamped(beta, b):
    """beta' is one of the values next_beta decides rather than finds: 1 (smc.rs:604-607, :621) or beta + 1e-9 (:621)"""
    return b == 1.0 or b == beta + 1e-9


def is_root(curve: Curve, target, b, reference=False):
    """(ok, ESS(beta') / target - 1, ESS(lo') / target - 1, D): the bracket criterion alone, without the bitwise shortcut"""
    D = curve.delta(b, reference)
    with mpmath.workdps(DPS):
        tgt = mpmath.mpf(target)
        e_hi = curve.ess(b) / tgt - 1
        e_lo = curve.ess(lo_prime(curve.beta, b)) / tgt - 1
        ok = e_lo >= -D and e_hi <= D
    return bool(ok), float(e_hi), float(e_lo), D


def accept(curve: Curve, target, got, want, case="", report=True):
    """the criterion of the module docstring for a device answer `got` against the oracle's `want`; reports a non-bitwise acceptance"""
    if got == want:
        return True
    if clamped(curve.beta, got):
        D = curve.delta(got)
        with mpmath.workdps(DPS):
            e_hi = float(curve.ess(got) / mpmath.mpf(target) - 1)
        ok = e_hi >= -D if got == 1.0 else e_hi <= D
        e_lo = float("nan")
    else:
        ok, e_hi, e_lo, D = is_root(curve, target, got)
    if ok and report:
        knife.used("next_beta: a root to working precision, not the oracle's bits", case=case, gpu=repr(got), oracle=repr(want),
                   ess_over_target_minus_1=f"{e_hi:.3e}", ess_lo_over_target_minus_1=f"{e_lo:.3e}", delta=f"{D:.3e}",
                   not_bitwise="gpu above oracle" if got > want else "gpu below oracle")
    return ok


def exact_log_norm(ll, beta, b):
    """log_sum_exp(lw0 + (b - beta) ll) at DPS digits from the double inputs (lw0 = -ln n); -inf when every term is -inf"""
    ll = np.asarray(ll, dtype=np.float64)
    n = ll.size
    fin = ll[np.isfinite(ll)]
    if fin.size == 0:
        return -math.inf
    with mpmath.workdps(DPS):
        db = mpmath.mpf(float(b)) - mpmath.mpf(float(beta))
        vals, counts = np.unique(fin, return_counts=True)
        L = mpmath.mpf(float(vals[-1]))
        dbf = float(b) - float(beta)
        keep = dbf * (vals - vals[-1]) > -(DPS * math.log(10.0) + math.log(n) + 11.0)
        s = mpmath.mpf(0)
        for v, c in zip(vals[keep].tolist(), counts[keep].tolist()):
            s += c * mpmath.exp(db * (mpmath.mpf(v) - L))
        return float(-mpmath.log(n) + db * L + mpmath.log(s))


def log_norm_tol(ll, beta, b):
    """the reweight's log-normaliser is max + ln(sum) with the sum formed in the product form E R^j of a pass: its absolute error is at most
    ~64 eps (1 + max |(b - beta)(ll_i - L)|) over the terms that matter, plus the rounding of max v = lw0 + (b - beta) L itself, plus the
    summation terms of `Curve.delta` (the device's tree, the reference's sequential sum)"""
    ll = np.asarray(ll, dtype=np.float64)
    fin = ll[np.isfinite(ll)]
    n = max(ll.size, 1)
    if fin.size == 0:
        return 0.0
    db = float(b) - float(beta)
    L = float(fin.max())
    y = db * (fin - L)
    y = y[y >= math.log(EPS / n)]
    Y = float(np.abs(y).max()) if y.size else 0.0
    nb = min(ESS2_BLOCKS, (n + ESS2_THREADS - 1) // ESS2_THREADS)
    k = -(-n // (nb * ESS2_THREADS))
    return 64.0 * EPS * (1.0 + Y) + 4.0 * EPS * (math.log(n) + abs(db * L)) + EPS * (k + 24 + math.sqrt(n))


# ---- the case matrix of the tempering-step tests (tests/test_smc_judge_cpu.py, tests/test_gpu_smc_step.py) ---------------------------
# n: a wave (64), ESS2_THREADS (512), SCAN_CHUNK (2 048), the point where the pass grid saturates at ESS2_BLOCKS blocks (131 072), one
# ESS2_UNROLL trip over that grid (524 288), 2^20, a prime; and their neighbours
SIZES = (1, 2, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 131071, 131072, 131073, 524287, 524288, 524289, 1048576, 2097169)
FULL_SIZES = (65, 2049)              # the whole value-shape list; every other size: a smooth case and a tie case
SIGMAS = (1e-3, 1.0, 30.0, 1e4, 1e6)
BETAS = (0.0, 0.3, 1.0 - 1e-6, 1.0 - 5e-10)  # the last: beta + 1e-9 > 1
THRS = (0.01, 0.5, 0.999, 1.0)
GRID_ABOVE = 65536                    # above this many particles a smooth ll lies on a grid of ~2 000 values (the 40-digit judge stays fast)


class StepCase:
    """one tempering step: ll (built on demand), beta, target = thr n; kind: 'smooth', 'tie', 'steep' (beta + 1e-9 wins: need_sum without
    forcing it), 'nonfinite'"""

    def __init__(self, name, n, make, beta, thr, kind):
        self.name, self.n, self.make, self.beta, self.thr, self.kind = name, n, make, float(beta), float(thr), kind

    @property
    def target(self):
        return self.thr * self.n

    def ll(self):
        import zlib
        return np.ascontiguousarray(self.make(np.random.default_rng(zlib.crc32(self.name.encode())), self.n), dtype=np.float64)

    def __repr__(self):
        return self.name


def two_point(n, k, c):
    """k particles at 0, n - k at -c"""
    ll = np.full(n, -float(c))
    ll[:k] = 0.0
    return ll


def two_point_root(n, k, c, target, beta=0.0):
    """closed form of ESS(b) = target for two_point(n, k, c): with m = n - k and r = exp(-(b - beta) c), ESS = (k + m r)^2 / (k + m r^2),
    so (m^2 - T m) r^2 + 2 k m r + k^2 - T k = 0; the root r in (0, 1)"""
    with mpmath.workdps(DPS):
        m, k, T = mpmath.mpf(n - k), mpmath.mpf(k), mpmath.mpf(target)
        a, bq, cq = m * m - T * m, 2 * k * m, k * k - T * k
        disc = mpmath.sqrt(bq * bq - 4 * a * cq)
        rs = [r for r in ((-bq + disc) / (2 * a), (-bq - disc) / (2 * a)) if 0 < r < 1]
        assert len(rs) == 1, rs
        return mpmath.mpf(beta) - mpmath.log(rs[0]) / c


def _smooth(sigma, grid):
    def make(rng, n):
        z = rng.standard_normal(n)
        if grid:
            z = np.round(z * 256.0) / 256.0
        return -3.0 + sigma * z
    return make


def _two_point_at(db_root, thr, k_frac=0.5):
    """two-point ll whose exact root lies db_root above beta (c from the closed form)"""
    def make(rng, n):
        k = max(1, int(n * k_frac))
        r = two_point_root(n, k, 1.0, thr * n)          # root in units of c = 1: (b - beta) = -ln r
        return two_point(n, k, float(r) / db_root)
    return make


def step_cases(max_n=None):
    out = []

    def add(name, n, make, beta, thr, kind):
        if max_n is None or n <= max_n:
            out.append(StepCase(f"{name}-n{n}-b{beta!r}-t{thr}", n, make, beta, thr, kind))
    for n in SIZES:
        add("smooth1", n, _smooth(1.0, n > GRID_ABOVE), 0.3, 0.5, "smooth")
        add("twopoint", n, lambda rng, n: two_point(n, max(1, n // 3), 2.0), 0.0, 0.5, "tie")
    for n in FULL_SIZES:
        for sigma in SIGMAS:
            for beta in BETAS:
                for thr in THRS:
                    add(f"smooth{sigma:g}", n, _smooth(sigma, False), beta, thr, "smooth")
        for beta in (0.0, 0.3):
            add("twopoint1", n, lambda rng, n: two_point(n, 1, 5.0), beta, 0.5, "tie")
            add("three", n, lambda rng, n: rng.choice(np.array([-1.0, -2.5, -7.0]), n), beta, 0.5, "tie")
            add("block64", n, lambda rng, n: np.resize(rng.normal(-3.0, 2.0, 64), n), beta, 0.5, "tie")
            add("equal", n, lambda rng, n: np.full(n, -2.0), beta, 0.999, "tie")
            add("ninety", n, lambda rng, n: (lambda v: np.where(rng.random(n) < 0.9, v.max(), v))(rng.normal(-3.0, 1.0, n)), beta, 0.5, "tie")
            # both ends of the bisection: the bracket reaches adjacent doubles before the 64th halving when the root lies above about
            # (1 - beta) 2^-12 (the `fixed` exit / `mid == lo || mid == hi`); far below that all 64 halvings run
            edge = (1.0 - beta) * 2.0 ** -12
            for f in (8.0, 1.0 / 64.0, 1e-4):
                add(f"root{f:g}edge", n, _two_point_at(edge * f, 0.5), beta, 0.5, "tie")
            add("steep1e9", n, _smooth(1e9, False), beta, 0.5, "steep")
            add("onefinite", n, lambda rng, n: np.where(np.arange(n) == n // 2, -3.0, -np.inf), beta, 0.5, "steep")
        add("allneginf", n, lambda rng, n: np.full(n, -np.inf), 0.0, 0.5, "nonfinite")
        add("halfneginf", n, lambda rng, n: np.where(np.arange(n) % 2 == 0, rng.normal(-3.0, 1.0, n), -np.inf), 0.0, 0.5, "smooth")
        add("oneposinf", n, lambda rng, n: np.where(np.arange(n) == 7, np.inf, rng.normal(-3.0, 1.0, n)), 0.0, 0.5, "nonfinite")
        add("onenan", n, lambda rng, n: np.where(np.arange(n) == 5, np.nan, rng.normal(-3.0, 1.0, n)), 0.3, 0.5, "nonfinite")
        add("pm1e300", n, lambda rng, n: rng.uniform(-1e300, 1e300, n), 0.0, 0.5, "nonfinite")
    return out
