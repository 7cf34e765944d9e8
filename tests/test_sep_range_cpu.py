"""fg_sep_range.h: the host proof that lets k_hmc_sep_steps's folded trajectory loop drop the range test of its quotient by 2h.

The arithmetic of one step of the folded loop (fg_hmc_sep.hip: FG_SEP_DUALS, FG_SEP_LPF, FG_SEP_LPF_U, n = tp - tm, g = fma(n, Ch, n Cl))
is restated here in exact rational arithmetic -- every rounding is one float(Fraction), which CPython rounds correctly -- and checked
against the three parts of the argument ("The range test leaves the step"):

1. every term is a multiple of 2^-54 and never -0, so n is +0 or |n| >= 2^-54, and the quotient of n = +0 is +0 whatever the sign of Cl;
2. when q + h == q - h the two sides are the same bits (n is +0 or NaN), and that is so for every |q| >= 2^55 h;
3. otherwise |n| <= fg_sep_range_bound, formed by the C++ header (tests/cpp/sep_range_driver.cpp, also built with
   -fsanitize=address,undefined and run as its own program).

The verdicts: accepted for the headline model (x_i ~ N(0, 1), y_i ~ N(x_i, 0.5), h = 1e-5), refused for an observation of 1.5 * 2^510
and for any bound that is not finite."""
import math
import os
import random
import struct
import subprocess
from fractions import Fraction

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 0.5 * 1.8378770664093454835606594728112          # 0.5 * FG_LN_2PI as the kernels form it
GRID = Fraction(1, 2 ** 54)
H = 1e-5


def bits(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


def unbits(s):
    return struct.unpack("<d", struct.pack("<Q", int(s, 16)))[0]


def _rn(x: Fraction) -> float:
    try:
        return float(x)
    except OverflowError:
        return math.inf if x > 0 else -math.inf


def _mul(a, b):
    if not (math.isfinite(a) and math.isfinite(b)):
        return a * b
    r = _rn(Fraction(a) * Fraction(b))
    return math.copysign(r, math.copysign(1.0, a) * math.copysign(1.0, b)) if r == 0.0 else r


def _fma(a, b, c):
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    x = Fraction(a) * Fraction(b) + Fraction(c)
    if x == 0:                                           # exact zero: the sign rule of an addition of the product and c
        return _mul(a, b) + c
    return _rn(x)


def _sub(a, b):                                          # a - b is one correctly rounded IEEE operation in CPython; kept as a name
    return a - b


def term_folded(x, c, s, lns):                           # FG_SEP_DUALS: s = 1 / sigma a power of two, nhs2 = -0.5 s^2
    d = _sub(x, c)
    return _sub(_fma(-0.5 * s * s, _mul(d, d), -lns), K)


def term_fused(x, c, sigma, lns):                        # FG_SEP_LPF with z = RN((x - c) / sigma)
    d = _sub(x, c)
    z = _rn(Fraction(d) / Fraction(sigma)) if math.isfinite(d) else d
    return _sub(_fma(-0.5, _mul(z, z), -lns), K)


def term_u0(x):                                          # FG_SEP_LPF_U
    return _fma(-0.5, _mul(x, x), -K)


def side(x, recs, u0):
    """recs: [(c, s, lns, sigma or None)]; sigma None: a power-of-two record (folded), else the fused form."""
    def term(k):
        c, s, lns, sigma = recs[k]
        return term_folded(x, c, s, lns) if sigma is None else term_fused(x, c, sigma, lns)
    terms = [term_u0(x) if u0 else term(0)] + [term(k) for k in range(1, len(recs))]
    t = terms[0]
    if len(recs) > 1:
        sp = terms[1]
        for k in range(2, len(recs)):
            sp = sp + terms[k]
        t = t + sp
    return t, terms


def numerator(q, h, recs, u0):
    (tp, terms_p), (tm, terms_m) = side(q + h, recs, u0), side(q - h, recs, u0)
    return tp - tm, terms_p + terms_m + [tp, tm]


def on_grid(v):
    return math.isfinite(v) and (Fraction(v) / GRID).denominator == 1 and not (v == 0.0 and math.copysign(1.0, v) < 0)


def p2rec(c, k):
    """sigma = 2^k"""
    sigma = math.ldexp(1.0, k)
    return (c, 1.0 / sigma, math.log(sigma), None)


def rec(c, sigma):
    return (c, 1.0 / sigma, math.log(sigma), sigma)


def check_step(q, h, recs, u0):
    """The lower side and zero on one step.  Returns n."""
    n, parts = numerator(q, h, recs, u0)
    if all(math.isfinite(p) for p in parts):
        assert all(on_grid(p) for p in parts), (q, h, recs, parts)
    if math.isfinite(n):
        assert on_grid(n), (q, n)
        assert n == 0.0 or abs(n) >= 2.0 ** -54, (q, n)
        if q + h == q - h:
            assert n == 0.0, (q, n)
    else:
        assert q + h != q - h or not all(math.isfinite(p) for p in parts)
    return n


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    def build(name, extra=()):
        exe = str(tmp_path_factory.mktemp(name) / name)
        subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-mfma", "-ffp-contract=off", *extra, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "sep_range_driver.cpp"), "-o", exe], check=True)

        def run(lines):
            r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
            assert r.returncode == 0, r.stdout + r.stderr
            return [ln.split() for ln in r.stdout.splitlines()]
        run.exe = exe
        return run
    return build("sep_range_driver"), build("sep_range_driver_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _recline(recs):
    return " ".join("%s %s %s" % (bits(c), bits(s), bits(lns)) for c, s, lns, _ in recs)


def bound(run, h, recs):
    (v, b), = run(["bound %s %d %s" % (bits(h), len(recs), _recline(recs))])
    return bool(int(v)), unbits(b)


def test_rounded_difference_with_k_is_on_the_grid():
    """RN(r - K) for any double r, and the U0 form fma(-0.5, m, -K) for m >= 0: multiples of 2^-54, never -0."""
    rng = random.Random(1)
    rs = [0.0, -0.0, K, -K, 0.5, -0.5, math.nextafter(0.5, 0.0), math.nextafter(0.5, 1.0), math.nextafter(K, 0.0), math.nextafter(K, 1.0),
          5e-324, -5e-324, 2.0 ** -1022, 2.0 ** -54, 2.0 ** -55, 1.0, 2.0 ** 52, 2.0 ** 53, 2.0 ** 54 + 2.0, 1.7976931348623157e308]
    rs += [s * math.ldexp(1.0 + rng.random(), rng.randrange(-1074, 1023)) for s in (1.0, -1.0) for _ in range(4000)]
    rs += [K + s * math.ldexp(rng.random(), rng.randrange(-60, 0)) for s in (1.0, -1.0) for _ in range(2000)]
    for r in rs:
        assert on_grid(r - K), r
        if r >= 0.0:
            v = _fma(-0.5, r, -K)
            assert on_grid(v) and v <= -K, r
    assert (K - K) == 0.0 and math.copysign(1.0, K - K) > 0          # a root gives +0


def _adversarial_steps():
    rng = random.Random(2)
    for k in (0, 1, -1, 2, -2, 7, -30, 200, -200, 480, -480):
        for c in (0.0, 0.3, -1.0, 1.5 * 2.0 ** 40):
            recs = [p2rec(c, k)]
            _, s, lns, _ = recs[0]
            qs = [0.0, c, c + H, c - H, 1.0, -0.7, 2.0 ** 55 * H, math.nextafter(2.0 ** 55 * H, 0.0), -(2.0 ** 55 * H), 2.0 ** 300, 2.0 ** 510, -(2.0 ** 510),
                  math.nextafter(-H, 0.0), math.nextafter(H, 0.0), c + math.ldexp(1.0, -30)]
            if -lns - K > 0.0:                            # roots of the term: -0.5 s^2 d^2 - ln sigma - K = 0, at q + h and at q - h
                root = math.sqrt(2.0 * (-lns - K)) / s
                for x in (c + root, c - root):
                    for y in (math.nextafter(x, -math.inf), x, math.nextafter(x, math.inf)):
                        qs += [y - H, y + H]
            qs += [rng.gauss(0.0, 1.0) * 10.0 ** rng.uniform(-6, 6) for _ in range(12)]
            for q in qs:
                yield q, H, recs, False
    # several records, a U0 prior, ln sigma = 0 records away from 0, sigmas that are not powers of two
    shapes = [([p2rec(0.0, 0), p2rec(-1.0, -1)], True), ([p2rec(0.0, 0), p2rec(0.2, 0)], True), ([p2rec(0.4, 0), p2rec(0.2, 0), p2rec(-3.0, 0)], False),
              ([p2rec(0.0, 0), p2rec(1.0, -2), p2rec(-1.0, 2), p2rec(0.5, -1)], True), ([rec(0.2, 0.3), p2rec(1.0, 1), rec(-1.0, 1.7)], False),
              ([rec(0.0, 1.0 / 3.0)], False), ([rec(1e-3, 0.39), rec(0.0, 0.01)], False), ([p2rec(2.0 ** 510, 0), p2rec(2.0 ** 510, -1)], False)]
    for recs, u0 in shapes:
        for h in (H, 2.0 ** -20, 1e-3, 0.7 * 2.0 ** -69):
            qs = [0.0, 1.0, -1.0, 0.25, 2.0 ** 55 * h, math.nextafter(2.0 ** 55 * h, 0.0), -math.nextafter(2.0 ** 55 * h, 0.0), 2.0 ** 56 * h, 2.0 ** 510, 1e300]
            qs += [rng.gauss(0.0, 1.0) * 10.0 ** rng.uniform(-8, 8) for _ in range(40)]
            for q in qs:
                yield q, h, recs, u0


def test_terms_and_numerators_stay_on_the_grid_and_zero_is_plus_zero():
    zeros = steps = 0
    for q, h, recs, u0 in _adversarial_steps():
        n = check_step(q, h, recs, u0)
        steps += 1
        if n == 0.0:
            zeros += 1
            assert math.copysign(1.0, n) > 0
            for ch, cl in ((1.0 / (2 * h), 1e-13), (1.0 / (2 * h), -1e-13), (1.0 / (2 * h), 0.0), (1.0 / (2 * h), -0.0)):
                g = _fma(n, ch, _mul(n, cl))                 # the two-instruction quotient of +0
                assert g == 0.0 and math.copysign(1.0, g) > 0 and (n / (2 * h)) == 0.0 and math.copysign(1.0, n / (2 * h)) > 0
    assert steps > 1500 and zeros > 100


def test_term_level_grid_with_subnormal_squares():
    """The term itself at operand differences the step cannot always reach: d^2 subnormal or 0, d at the roots, huge d."""
    rng = random.Random(3)
    for k in (0, 1, -1, 3, -3, 100, -100, 480, -480):
        c, s, lns, _ = p2rec(0.0, k)
        ds = [0.0, -0.0, 5e-324, 2.0 ** -540, 2.0 ** -537.5, 2.0 ** -511, 2.0 ** -512 * 1.3, 1.0, 2.0 ** 400, 2.0 ** 511, 2.0 ** 512]
        ds += [math.ldexp(1.0 + rng.random(), rng.randrange(-1074, 520)) for _ in range(200)]
        for d in ds:
            for x in (d, -d):
                t = term_folded(x, 0.0, s, lns)
                if math.isfinite(t):
                    assert on_grid(t), (k, x, t)
    for sigma in (0.3, 1.7, 1.0 / 3.0, 0.39, 123.456, 1e-9):
        for d in [0.0, 5e-324, 2.0 ** -540, 1e-3, 1.0, 1e9, 2.0 ** 500] + [math.ldexp(1.0 + rng.random(), rng.randrange(-1074, 500)) for _ in range(200)]:
            t = term_fused(d, 0.0, sigma, math.log(sigma))
            if math.isfinite(t):
                assert on_grid(t), (sigma, d, t)


def test_restatement_is_the_drivers_arithmetic(drivers):
    """The C++ driver forms the folded step with the host's doubles and fma: the same bits as the Fraction restatement."""
    run, _ = drivers
    cases = [(q, h, recs, u0) for q, h, recs, u0 in _adversarial_steps() if all(r[3] is None for r in recs)][::3]
    got = run(["n %s %s %d %d %s" % (bits(h), bits(q), 1 if u0 else 0, len(recs), _recline(recs)) for q, h, recs, u0 in cases])
    for (q, h, recs, u0), (g,) in zip(cases, got):
        n, _ = numerator(q, h, recs, u0)
        assert bits(n) == g or (math.isnan(n) and math.isnan(unbits(g))), (q, h, recs, n, unbits(g))


def test_bound_dominates_the_exact_numerator(drivers):
    run, _ = drivers
    rng = random.Random(4)
    cases = list(_adversarial_steps())
    for _ in range(1500):                                 # random (q, c, s, h), q up to the largest magnitude at which q + h != q - h
        h = math.ldexp(1.0 + rng.random(), rng.randrange(-71, 0))
        nrec = rng.randrange(1, 5)
        u0 = nrec > 1 and rng.random() < 0.3
        recs = [p2rec(0.0, 0)] if u0 else []
        while len(recs) < nrec:
            c = rng.choice([0.0, rng.gauss(0, 1), rng.gauss(0, 1) * 10.0 ** rng.uniform(-10, 100)])
            recs.append(p2rec(c, rng.randrange(-60, 61)) if rng.random() < 0.7 else rec(c, math.exp(rng.uniform(-20, 20))))
        qmax = math.nextafter(2.0 ** 55 * h, 0.0)
        q = rng.choice([qmax, -qmax, qmax * rng.random(), rng.gauss(0, 1), rng.gauss(0, 1) * 10.0 ** rng.uniform(-8, 8)])
        cases.append((q, h, recs, u0))
    lines = ["bound %s %d %s" % (bits(h), len(recs), _recline(recs)) for _, h, recs, _ in cases]
    nonzero = 0
    for (q, h, recs, u0), (v, b) in zip(cases, run(lines)):
        n, _ = numerator(q, h, recs, u0)
        b = unbits(b)
        if abs(q) >= 2.0 ** 55 * h:
            assert q + h == q - h and (n == 0.0 or math.isnan(n)), (q, h, n)
        if math.isfinite(n) and n != 0.0:
            nonzero += 1
            assert abs(n) <= b, (q, h, recs, n, b)
            assert int(v) == (1 if b < 2.0 ** 953 else 0)
    assert nonzero > 1500


def _headline(n=32):
    return [[p2rec(0.0, 0), p2rec(0.2 * i - 1.0, -1)] for i in range(n)]


def _prove(run, h, coords):
    line = "prove %s %d " % (bits(h), len(coords)) + " ".join("%d %s" % (len(r), _recline(r)) for r in coords)
    (v, w), = run([line])
    return bool(int(v)), unbits(w)


@pytest.mark.parametrize("san", [False, True])
def test_verdicts(drivers, san):
    """Also under -fsanitize=address,undefined (its own program: a finding ends the run with a non-zero status)."""
    run = drivers[1 if san else 0]
    ok, worst = _prove(run, H, _headline())
    assert ok and 2.0 ** 76 < worst < 2.0 ** 84            # "about 2^80"
    big = 1.5 * 2.0 ** 510
    refused = _headline()
    refused[17] = [p2rec(0.0, 0), p2rec(big, 2)]           # sigma = 4: the bound is finite, about 2^1017
    ok, worst = _prove(run, H, refused)
    assert not ok and worst >= 2.0 ** 953 and math.isfinite(worst)
    refused[17] = [p2rec(0.0, 0), p2rec(big, -2)]          # sigma = 1/4: the bound itself overflows
    ok, worst = _prove(run, H, refused)
    assert not ok and worst == math.inf
    for bad in ([p2rec(math.inf, 0)], [p2rec(math.nan, 0)], [p2rec(1e300, -400)], [(0.0, 1.0, math.nan, None)], [(0.0, math.inf, 0.0, None)]):
        ok, worst = _prove(run, H, _headline(3) + [bad])
        assert not ok and not math.isfinite(worst), bad
    for h in (0.0, -1e-5, math.inf, math.nan):
        assert not _prove(run, h, _headline(2))[0]
    assert not _prove(run, H, [])[0]
    assert _prove(run, 0.7 * 2.0 ** 148, _headline(2))[0]  # the largest h the short quotient admits: 2^55 h = 2^203, bound about 2^410
    assert bound(run, H, [p2rec(0.0, 0)])[0]
    if san:
        r = subprocess.run([run.exe, "--self-check"], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0 and "self-check ok" in r.stdout, r.stdout + r.stderr
