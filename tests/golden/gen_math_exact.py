#!/usr/bin/env python3
"""Generates tests/golden/math_exact.json and math_exact.bin: exact expectations for the device's arithmetic (tests/test_gpu_math_exact.py,
tests/test_math_exact_cpu.py).  Needs mpmath and numpy; reads nothing but this file.  `python tests/golden/gen_math_exact.py` rewrites
the fixture; `generate()` returns the two files' contents, which tests/test_math_exact_cpu.py compares with the committed files.

Log-density cases.  Each of the 13 formulas of fg_logpdf (fugue_amd/csrc/fg_math.h) is restated term by term.  Whatever the formula
computes with +, -, *, / on doubles before it calls a function -- `1.0 - x`, `z * z / p0`, `xf / p1`, `(p0 + 1.0) / 2.0`,
`(double)(n - k) + 1.0`, and z itself -- is computed here in double, exactly as written (IEEE arithmetic: the same bits everywhere).
Every elementary function is then evaluated with mpmath (60 digits) on that double argument, every term's product and the sum of the
terms are exact.  The one function value that feeds further arithmetic, LogNormal's ln x inside z, enters z as the correctly rounded
double.  A case's budget is B = sum |term| + (number of lgamma calls): an implementation whose functions are good to F ulp, with one
rounding per product and per in-order addition, lies within (2F + 6) 2^-53 B of the exact value.

Ranges (log-uniform, seed 7): sigma / scale / rate 1e-6..1e6; Beta a, b 1e-3..1e6 with x from 1e-300 to 1 - 2^-53; Gamma and
InverseGamma shape 1e-3..1e6; Binomial n to 1e12; Poisson lambda 1e-3..1e12 with k within +-3 sd; StudentT nu 1e-2..1e12 with
Cauchy-tailed x; Weibull shape 0.05..50; ChiSquared k 1e-2..1e6; and the shapes 1 +- 2^-e, 2 +- 2^-e (e = 1..52) as the argument of
lgamma in Beta, Gamma, StudentT, ChiSquared and InverseGamma (Binomial and Poisson call lgamma on k + 1, n - k + 1: their zeros are the
counts 0 and 1, which are cases too).  Two ranges are narrower than they could be, on purpose:
  * LogNormal's mu lies within +-sigma.  z = (ln x - mu) / sigma carries ln x's rounding error divided by sigma, which the budget
    does not hold: with |mu| <= sigma that share stays below z^2 + 1, i.e. inside the budget's own terms.
  * LogNormal's sigma z and Weibull's x keep exp and pow finite.
Only cases with a finite value are kept.  The project's oracle (oracle/orc_numerics.c with the host's libm) is evaluated on every case:
its K = |oracle - exact| / (2^-53 B) must be <= 4, or generation fails -- no case is dropped for it.

Storage: doubles as 16 hex digits of their bits, concatenated per column; an exact value as a double-double (hi = the nearest double,
lo = the rest as a float32, 8 hex digits: 2^-24 of half an ulp); integers (Binomial's and Poisson's value) as the int64's bits; a case's
family as one hex digit, its index in `families`.  On disk every such column is the bytes its hex digits spell, in math_exact.bin, and
math_exact.json holds {"@": offset, "n": bytes} in its place (`pack` / `unpack`): a third of a megabyte of digits is nothing a reader
of a diff can check, and half the size as bytes.  tests/math_exact_fixture.py reads the two back into the columns of hex digits.
"""
import json
import math
import os
import struct
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "math_exact.json")
OUT_BIN = os.path.join(HERE, "math_exact.bin")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

FAMILIES = ["Normal", "LogNormal", "Exponential", "Beta", "Gamma", "Binomial", "Poisson", "StudentT", "Cauchy", "Laplace", "Weibull",
            "ChiSquared", "InverseGamma"]
INT_FAMILIES = ("Binomial", "Poisson")
NPARAMS = {"Normal": 2, "LogNormal": 2, "Exponential": 1, "Beta": 2, "Gamma": 2, "Binomial": 2, "Poisson": 1, "StudentT": 3, "Cauchy": 2,
           "Laplace": 2, "Weibull": 2, "ChiSquared": 1, "InverseGamma": 2}
LN_2PI, LN_PI, LN_2 = 1.8378770664093456, 1.1447298858494002, 0.6931471805599453          # the constants of fg_math.h, as doubles
N_RANDOM = 64                                                                             # per family
K_ORACLE_MAX = 4.0
REFUSED_H = float.fromhex("0x1.f86664b036c57p-12")                                        # tests/test_gpu_div2.py
MODEL_SIGMAS = [0.5, 0.7, 2.0, 3.0, 0.8, 5.0, 1.3, 0.85, 1.2, 0.75, 0.25]                 # tests/models.py
DIV_FIXED = [2e-5, 0.8, 2.5, 3.0, 0.7, 0.3, 1.0 / 3.0, 0.1, 1e-3, 7.0, 1e5]               # tests/cpp/test_div_const.cpp


def bits(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(u: int) -> float:
    return struct.unpack("<d", struct.pack("<Q", u & 0xFFFFFFFFFFFFFFFF))[0]


def hex64(values) -> str:
    return "".join("%016x" % bits(float(v)) for v in values)


def hexu64(values) -> str:
    return "".join("%016x" % (int(v) & 0xFFFFFFFFFFFFFFFF) for v in values)


def hex32(values) -> str:
    return "".join("%08x" % struct.unpack("<I", struct.pack("<f", float(v)))[0] for v in values)


# --------------------------------------------------------------------------------------------------------------------------------------
# the 13 formulas, term by term.  F: the exact functions (mpmath) or the recorder of the arguments; returns (terms, lgamma calls)
# --------------------------------------------------------------------------------------------------------------------------------------
class Exact:
    def __init__(self, mp):
        self.mp, self.calls = mp, []

    def _f(self, name, fn, *args):
        self.calls.append((name,) + tuple(float(a) for a in args))
        return fn(*[self.mp.mpf(float(a)) for a in args])

    def log(self, a): return self._f("log", self.mp.log, a)
    def log1p(self, a): return self._f("log1p", self.mp.log1p, a)
    def lgamma(self, a): return self._f("lgamma", self.mp.loggamma, a)
    def pow(self, a, b): return self._f("pow", self.mp.power, a, b)

    def rn(self, v) -> float:
        return float(v)                                  # mpmath rounds to nearest

    def c(self, v):
        return self.mp.mpf(float(v))


def terms_of(fam, p, x, F):
    """p: the double parameters, x: the value (a double, or an int for the integer families).  None: outside the finite formula."""
    c = F.c
    if fam == "Normal":
        z = (x - p[0]) / p[1]
        return [c(-0.5) * c(z) * c(z), -F.log(p[1]), c(-0.5) * c(LN_2PI)], 0
    if fam == "LogNormal":
        lxm = F.log(x)
        z = (F.rn(lxm) - p[0]) / p[1]
        return [c(-0.5) * c(z) * c(z), -lxm, -F.log(p[1]), c(-0.5) * c(LN_2PI)], 0
    if fam == "Exponential":
        return [F.log(p[0]), -c(p[0]) * c(x)], 0
    if fam == "Beta":
        if not (0.0 < x < 1.0):
            return None
        return [c(p[0] - 1.0) * F.log(x), c(p[1] - 1.0) * F.log(1.0 - x), -F.lgamma(p[0]), -F.lgamma(p[1]), F.lgamma(p[0] + p[1])], 3
    if fam == "Gamma":
        return [c(p[0]) * F.log(p[1]), c(p[0] - 1.0) * F.log(x), -c(p[1]) * c(x), -F.lgamma(p[0])], 1
    if fam == "Binomial":
        n, k = int(p[0]), int(x)
        if not (0 <= k <= n) or not (0.0 < p[1] < 1.0):
            return None
        return [F.lgamma(float(n) + 1.0), -F.lgamma(float(k) + 1.0), -F.lgamma(float(n - k) + 1.0), c(float(k)) * F.log(p[1]),
                c(float(n - k)) * F.log(1.0 - p[1])], 3
    if fam == "Poisson":
        k = int(x)
        if k < 0:
            return None
        if p[0] > 700.0 and k == 0:
            return [-c(p[0])], 0
        return [c(float(k)) * F.log(p[0]), -c(p[0]), -F.lgamma(float(k) + 1.0)], 1
    if fam == "StudentT":
        z = (x - p[1]) / p[2]
        return [F.lgamma((p[0] + 1.0) / 2.0), -F.lgamma(p[0] / 2.0), c(-0.5) * F.log(p[0]), c(-0.5) * c(LN_PI), -F.log(p[2]),
                -c(0.5 * (p[0] + 1.0)) * F.log1p(z * z / p[0])], 2
    if fam == "Cauchy":
        z = (x - p[0]) / p[1]
        return [-c(LN_PI), -F.log(p[1]), -F.log1p(z * z)], 0
    if fam == "Laplace":
        return [-F.log(2.0 * p[1]), -c(abs(x - p[0]) / p[1])], 0
    if fam == "Weibull":
        if not x > 0.0:
            return None
        return [F.log(p[0]), -c(p[0]) * F.log(p[1]), c(p[0] - 1.0) * F.log(x), -F.pow(x / p[1], p[0])], 0
    if fam == "ChiSquared":
        hk = p[0] / 2.0
        return [-c(hk) * c(LN_2), -F.lgamma(hk), c(hk - 1.0) * F.log(x), -c(x / 2.0)], 1
    if fam == "InverseGamma":
        return [c(p[0]) * F.log(p[1]), -F.lgamma(p[0]), -c(p[0] + 1.0) * F.log(x), -c(p[1] / x)], 1
    raise ValueError(fam)


# --------------------------------------------------------------------------------------------------------------------------------------
# the cases
# --------------------------------------------------------------------------------------------------------------------------------------
def lgamma_zero_shapes():
    out = []
    for e in range(1, 53):
        for base in (1.0, 2.0):
            for sg in (-1.0, 1.0):
                out.append((base + sg * 2.0 ** -e, e))
    return out


def draw_cases():
    rng = np.random.default_rng(7)
    lu = lambda lo, hi: float(10.0 ** rng.uniform(math.log10(lo), math.log10(hi)))
    loc = lambda: float(rng.normal() * 10.0 ** rng.uniform(-2.0, 2.0))
    wide = lambda: float(rng.choice([-1.0, 1.0]) * 10.0 ** rng.uniform(-3.0, 1.5))
    cauchy = lambda: float(math.tan(math.pi * (rng.uniform() - 0.5)))
    cases = []                                                                     # (family, params, x, tag)
    for _ in range(N_RANDOM):
        s, m = lu(1e-6, 1e6), loc()
        cases.append(("Normal", [m, s], m + s * wide(), "r"))
        s = lu(1e-6, 1e6)
        m, z = min(s, 300.0) * float(rng.uniform(-1.0, 1.0)), wide()
        z = math.copysign(min(abs(z), 300.0 / s), z)
        cases.append(("LogNormal", [m, s], math.exp(m + s * z), "r"))
        r = lu(1e-6, 1e6)
        cases.append(("Exponential", [r], lu(1e-3, 1e2) / r, "r"))
        a, b = lu(1e-3, 1e6), lu(1e-3, 1e6)
        which = rng.integers(0, 4)
        if which <= 1:
            mean, sd = a / (a + b), math.sqrt(a * b / ((a + b) ** 2 * (a + b + 1.0)))
            x = min(max(mean + 2.0 * sd * float(rng.normal()), 1e-300), 1.0 - 2.0 ** -53)
        elif which == 2:
            x = float(10.0 ** rng.uniform(-300.0, 0.0))
        else:
            x = 1.0 - 2.0 ** -int(rng.integers(1, 54))
        cases.append(("Beta", [a, b], x, "r"))
        for fam in ("Gamma", "InverseGamma"):
            sh, rt = lu(1e-3, 1e6), lu(1e-6, 1e6)
            g = sh * lu(0.1, 10.0) if rng.integers(0, 2) else lu(1e-6, 1e3)
            cases.append((fam, [sh, rt], g / rt if fam == "Gamma" else rt / g, "r"))
        n = int(lu(1.0, 1e12))
        pr = lu(1e-6, 0.5)
        pr = pr if rng.integers(0, 2) else 1.0 - pr
        k = int(round(n * pr + 3.0 * math.sqrt(n * pr * (1.0 - pr)) * float(rng.uniform(-1.0, 1.0))))
        cases.append(("Binomial", [float(n), pr], min(max(k, 0), n), "r"))
        lam = lu(1e-3, 1e12)
        cases.append(("Poisson", [lam], max(0, int(round(lam + 3.0 * math.sqrt(lam) * float(rng.uniform(-1.0, 1.0))))), "r"))
        nu, m, s = lu(1e-2, 1e12), loc(), lu(1e-6, 1e6)
        cases.append(("StudentT", [nu, m, s], m + s * cauchy(), "r"))
        m, s = loc(), lu(1e-6, 1e6)
        cases.append(("Cauchy", [m, s], m + s * cauchy(), "r"))
        m, s = loc(), lu(1e-6, 1e6)
        u = float(rng.uniform()) - 0.5
        cases.append(("Laplace", [m, s], m - s * math.copysign(1.0, u) * math.log(1.0 - 2.0 * abs(u)), "r"))
        sh, sc = lu(0.05, 50.0), lu(1e-6, 1e6)
        cases.append(("Weibull", [sh, sc], sc * (-math.log(1.0 - float(rng.uniform()))) ** (1.0 / sh), "r"))
        kk = lu(1e-2, 1e6)
        cases.append(("ChiSquared", [kk], kk * lu(0.1, 10.0) if rng.integers(0, 2) else lu(1e-6, 1e3), "r"))
    # lgamma next to its zeros at 1 and 2
    for s, e in lgamma_zero_shapes():
        x01, xp = float(rng.uniform(0.05, 0.95)), lu(0.1, 10.0)
        cases.append(("Beta", [s, lu(0.5, 4.0)] if e % 2 else [lu(0.5, 4.0), s], x01, "z"))
        cases.append(("Gamma", [s, lu(0.1, 10.0)], xp, "z"))
        cases.append(("StudentT", [2.0 * s - 1.0 if (e % 2 and s > 0.5) else 2.0 * s, 0.25, lu(0.1, 10.0)], 0.25 + float(rng.normal()), "z"))
        cases.append(("ChiSquared", [2.0 * s], xp, "z"))
        cases.append(("InverseGamma", [s, lu(0.1, 10.0)], xp, "z"))
    for n, k in [(1, 0), (1, 1), (2, 1), (5, 0), (5, 1), (5, 4), (5, 5), (1000000007, 0), (1000000007, 1), (10 ** 12, 10 ** 12 - 1), (10 ** 12, 10 ** 12)]:
        cases.append(("Binomial", [float(n), 0.3], k, "z"))
    for lam, k in [(0.5, 0), (0.5, 1), (3.0, 0), (3.0, 1), (3.0, 2), (699.0, 0), (701.0, 0), (701.0, 1), (1e12, 10 ** 12)]:
        cases.append(("Poisson", [lam], k, "z"))
    return cases


# --------------------------------------------------------------------------------------------------------------------------------------
# primitive points
# --------------------------------------------------------------------------------------------------------------------------------------
def div_const_ok(b: float) -> bool:
    u = bits(b)
    e = (u >> 52) & 0x7FF
    return 1023 - 400 < e < 1023 + 400 and (u & 0xFFFFFFFFFFFFF) != 0xFFFFFFFFFFFFF


def rnd_double(rng, emin, emax) -> float:
    u = ((int(rng.integers(emin, emax + 1)) + 1023) << 52) | int(rng.integers(0, 1 << 52))
    return from_bits(u | (int(rng.integers(0, 2)) << 63))


def div_points():
    rng = np.random.default_rng(71)
    divisors = DIV_FIXED + [2.0 * 1e-5, REFUSED_H, 2.0 * REFUSED_H] + MODEL_SIGMAS
    while len(divisors) < 150:
        b = rnd_double(rng, -399, 399)
        if div_const_ok(b):
            divisors.append(b)
    a, bb = [], []
    for b in divisors:
        assert div_const_ok(b)
        nums = [b * (float(int(rng.integers(0, 1 << 48))) + 0.5) for _ in range(2)]                 # quotient next to a midpoint
        for _ in range(2):                                                                            # quotient with 20 low one-bits
            nums.append(from_bits(bits(rnd_double(rng, -30, 30)) | 0xFFFFF) * b)
        nums += [rnd_double(rng, -1022, 1023) for _ in range(2)]                                      # the whole exponent range
        nums += [rnd_double(rng, -1022, -969), rnd_double(rng, -968, -940), 0.0]                      # below and at the window's lower edge
        for x in nums:
            a.append(x); bb.append(b)
    return a, bb


def halving_significands():
    """(m - 1) for the first 53-bit significand that fg_fast_log halves (high word 0x6a09c of the fraction) and the one before, in every
    binade from 2^-53 to 1: tests/test_gpu_rng_identity.py's _forced_words."""
    out = [0, 2 ** 53 - 1]
    for k in range(0, 53):
        mb = (0x16a09c << (k - 20)) if k >= 20 else ((0x16a09c + (1 << (20 - k)) - 1) >> (20 - k))
        for m in (mb - 1, mb):
            if 1 <= m <= 2 ** 53:
                out.append(m - 1)
    return out


def log_points():
    rng = np.random.default_rng(72)
    ks = sorted(set([0, 1, 2, 3, 1998, 1999] + [int(v) for v in rng.integers(0, 2000, 150)]))
    pts = [(k + 1) * 2.0 ** -53 for k in ks]
    pts += [1.0 - k * 2.0 ** -53 for k in range(0, 40)] + [1.0 + k * 2.0 ** -52 for k in range(1, 40)]
    pts += [(a + 1) * 2.0 ** -53 for a in halving_significands()]
    pts += [1e-10]
    pts += [float(10.0 ** v) for v in rng.uniform(-3.0, 2.0, 600)]                                   # fg_cold_mh_adapt's range
    return pts


def sincos_points():
    rng = np.random.default_rng(73)
    us = [int(v) for v in rng.integers(0, 1 << 53, 400)]
    for q in range(0, 5):                                                                            # u2 = q / 4 -+ steps of 2^-53
        for d in [0, 1, 2, 3, 4095, 4096] + [int(v) for v in rng.integers(4, 4096, 20)]:
            for u in (q * 2 ** 51 - d, q * 2 ** 51 + d):
                if 0 <= u < 2 ** 53:
                    us.append(u)
    us = sorted(set(us))
    return [2.0 * math.pi * (u * 2.0 ** -53) for u in us]


def pair_words():
    rng = np.random.default_rng(74)
    wa = [int(v) for v in rng.integers(0, 1 << 64, 500, dtype=np.uint64)]
    wb = [int(v) for v in rng.integers(0, 1 << 64, 500, dtype=np.uint64)]
    b = [0, 2 ** 53 - 1]
    for k in (1, 2, 3):
        b += [k * 2 ** 51 - 1, k * 2 ** 51, k * 2 ** 51 + 1]
    hs = halving_significands()
    for i, a in enumerate(hs):                                                                        # each forced u1 with three of the forced u2
        for j in range(3):
            low = 0x7FF if (i + j) % 2 else 0
            wa.append((a << 11) | low); wb.append((b[(i + 4 * j) % len(b)] << 11) | low)
    return wa, wb


def digamma_points():
    rng = np.random.default_rng(75)
    pts = [float(10.0 ** v) for v in rng.uniform(-8.0, 10.0, 250)]
    x = 6.0
    lo = hi = x
    for _ in range(4):
        lo, hi = math.nextafter(lo, 0.0), math.nextafter(hi, 10.0)
        pts += [lo, hi]
    pts += [6.0, 5.0, 1.0, 2.0, 1.4616321449683623, math.nextafter(1.4616321449683623, 0.0), math.nextafter(1.4616321449683623, 2.0)]
    return pts


# --------------------------------------------------------------------------------------------------------------------------------------
HEX = set("0123456789abcdef")


def pack(tree):
    """-> (the index as JSON text, the blob): every column of hex digits moves into the blob"""
    blob = bytearray()

    def walk(v):
        if isinstance(v, dict):
            return {k: walk(w) for k, w in v.items()}
        if isinstance(v, str) and len(v) >= 64 and len(v) % 2 == 0 and set(v) <= HEX:
            at = len(blob)
            blob.extend(bytes.fromhex(v))
            return {"@": at, "n": len(v) // 2}
        return v
    index = walk(tree)
    return json.dumps(index, indent=1) + "\n", bytes(blob)


def unpack(text: str, blob: bytes):
    def walk(v):
        if isinstance(v, dict):
            if set(v) == {"@", "n"}:
                assert 0 <= v["@"] and v["@"] + v["n"] <= len(blob)
                return blob[v["@"]:v["@"] + v["n"]].hex()
            return {k: walk(w) for k, w in v.items()}
        return v
    return walk(json.loads(text))


LAST_K_ORACLE = {}                                       # per family, the oracle's worst K of the last generate()


def generate():
    import mpmath
    from oracle import oracle as orc
    mp = mpmath.mp
    mp.dps = 60
    orc.build()
    dd = lambda v: (float(v), float(v - mp.mpf(float(v))))

    F = Exact(mp)
    rows, k_oracle = [], {f: 0.0 for f in FAMILIES}
    for fam, p, x, tag in draw_cases():
        t = terms_of(fam, p, x, F)
        if t is None:
            continue
        terms, n_lg = t
        exact = mp.fsum(terms)
        budget = float(mp.fsum([abs(v) for v in terms]) + n_lg)
        hi, lo = dd(exact)
        if not (math.isfinite(hi) and math.isfinite(budget)):
            continue
        o = orc.logpdf(fam, x, p)
        K = float(abs(mp.mpf(o) - exact) / (mp.mpf(2) ** -53 * budget)) if math.isfinite(o) else math.inf
        if K > K_ORACLE_MAX:
            raise SystemExit(f"the oracle is loose on {fam} {p} {x}: K = {K}; change the ranges, do not drop the case")
        k_oracle[fam] = max(k_oracle[fam], K)
        rows.append((fam, p + [0.0] * (3 - len(p)), x, hi, lo, budget, tag))
    out = {"_about": "exact values for the device's arithmetic; written by gen_math_exact.py, which documents the layout",
           "families": FAMILIES}
    LAST_K_ORACLE.update(k_oracle)
    out["logpdf"] = {
        "family": "".join("%x" % FAMILIES.index(r[0]) for r in rows), "tag": "".join(r[6] for r in rows),
        "p0": hex64(r[1][0] for r in rows), "p1": hex64(r[1][1] for r in rows), "p2": hex64(r[1][2] for r in rows),
        "x": "".join(("%016x" % (int(r[2]) & 0xFFFFFFFFFFFFFFFF)) if r[0] in INT_FAMILIES else "%016x" % bits(float(r[2])) for r in rows),
        "hi": hex64(r[3] for r in rows), "lo": hex32(r[4] for r in rows), "budget": hex64(r[5] for r in rows)}

    # FG_OP_NORMAL_FAST edges: literal results
    edges = []
    for s in (0.3, 0.7, 2.5):
        ls = float(mp.log(mp.mpf(s)))
        assert ls == math.log(s)
        edges.append({"mu": 0.25, "sigma": s, "x": 1e308, "expected": "-inf"})
        edges.append({"mu": 0.0, "sigma": s, "x": 1e-300, "expected": "%016x" % bits(-0.0 - ls - 0.5 * LN_2PI)})
    out["normal_fast_edges"] = edges

    # ocml: every argument the cases feed, and the samplers' exp / tan
    rng = np.random.default_rng(76)
    calls = sorted(set(F.calls))
    for u in rng.uniform(0.0, 1.0, 60):
        calls.append(("tan", math.pi * (float(u) - 0.5)))
    for lam in 10.0 ** rng.uniform(-3.0, math.log10(30.0), 60):
        calls.append(("exp", -float(lam)))
    fn = {"log": mp.log, "log1p": mp.log1p, "lgamma": mp.loggamma, "pow": mp.power, "exp": mp.exp, "tan": mp.tan}
    out["ocml"] = {}
    for name in ("log", "log1p", "lgamma", "exp", "pow", "tan"):
        sel = [c for c in calls if c[0] == name]
        vals = [dd(fn[name](*[mp.mpf(a) for a in c[1:]])) for c in sel]
        out["ocml"][name] = {"a": hex64(c[1] for c in sel), "hi": hex64(v[0] for v in vals), "lo": hex32(v[1] for v in vals)}
        if name == "pow":
            out["ocml"][name]["b"] = hex64(c[2] for c in sel)

    a, b = div_points()
    out["div"] = {"a": hex64(a), "b": hex64(b)}
    pts = log_points()
    vals = [dd(mp.log(mp.mpf(x))) for x in pts]
    out["log"] = {"a": hex64(pts), "hi": hex64(v[0] for v in vals), "lo": hex32(v[1] for v in vals)}
    pts = sincos_points()
    sn, cs = [dd(mp.sin(mp.mpf(x))) for x in pts], [dd(mp.cos(mp.mpf(x))) for x in pts]
    out["sincos"] = {"a": hex64(pts), "sin_hi": hex64(v[0] for v in sn), "sin_lo": hex32(v[1] for v in sn),
                     "cos_hi": hex64(v[0] for v in cs), "cos_lo": hex32(v[1] for v in cs)}
    wa, wb = pair_words()
    z0, z1, gz = [], [], []
    for ua, ub in zip(wa, wb):
        u1, u2 = (float(ua >> 11) + 1.0) * 2.0 ** -53, float(ub >> 11) * 2.0 ** -53                  # the doubles the code forms
        th = mp.mpf(2.0 * math.pi * u2)
        r = mp.sqrt(-2 * mp.log(mp.mpf(u1)))
        z0.append(dd(r * mp.cos(th))); z1.append(dd(r * mp.sin(th)))
        g1 = max(float(ua >> 11) * 2.0 ** -53, 1e-10)                                                # fg_gaussian_z_of: u1 in [0, 1), clamped
        gz.append(dd(mp.sqrt(-2 * mp.log(mp.mpf(g1))) * mp.cos(th)))
    out["pair"] = {"wa": hexu64(wa), "wb": hexu64(wb), "z0_hi": hex64(v[0] for v in z0), "z0_lo": hex32(v[1] for v in z0),
                   "z1_hi": hex64(v[0] for v in z1), "z1_lo": hex32(v[1] for v in z1), "gz_hi": hex64(v[0] for v in gz), "gz_lo": hex32(v[1] for v in gz)}
    pts = digamma_points()
    vals = [dd(mp.digamma(mp.mpf(x))) for x in pts]
    out["digamma"] = {"a": hex64(pts), "hi": hex64(v[0] for v in vals), "lo": hex32(v[1] for v in vals)}
    if len(rows) % 2:                                   # (a column of single digits packs as whole bytes)
        raise SystemExit("an odd number of cases")
    text, blob = pack(out)
    assert unpack(text, blob) == out
    return text, blob


if __name__ == "__main__":
    text, blob = generate()
    with open(OUT, "w") as f:
        f.write(text)
    with open(OUT_BIN, "wb") as f:
        f.write(blob)
    d = unpack(text, blob)
    print(len(d["logpdf"]["family"]), "log-density cases,", {k: len(v["a"]) // 16 for k, v in d["ocml"].items()}, "ocml arguments,",
          len(text), "+", len(blob), "bytes; oracle K:", {k: round(v, 2) for k, v in LAST_K_ORACLE.items()})
