"""fg_div2_prove (fugue_amd/csrc/fg_div2.h): the host proof that a / b is fma(a, Ch, RN(a Cl)) for a fixed divisor b, against exact
rational arithmetic.

`form2` restates the two-instruction quotient with Fractions (every rounding is one float(Fraction), which CPython rounds correctly);
`near_midpoint` enumerates, for both scalings of the quotient's significand and every odd |delta| <= 2000, the numerators whose
quotient lies delta / (2 B) ulp from a midpoint between two doubles (B: the odd part of b's significand).  The verdict of the C++
proof must be the verdict of that enumeration; accepted divisors must be exact everywhere the kernels may use them.
"""
import math
import os
import random
import struct
import subprocess
from fractions import Fraction

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAILING = [float.fromhex(x) for x in ("0x1.f86664b036c57p-11", "0x1.adff816a7d897p-6", "0x1.7a243b2332317p-22", "0x1.b555b9e69c5a7p-14",
                                      "0x1.ab9b08cf72eafp-15")]
DIVISORS = [2e-5, 2e-4, 2e-6, 2e-3, 6e-5, 0.8, 2.5, 0.7, 1.0 / 3.0] + FAILING
# both ends of the admitted exponent window of b, [-70, 147] (an a * Cl that underflows at the upper end)
EDGE_DIVISORS = [math.ldexp(0.7, -69), math.ldexp(0.7, 148), math.ldexp(0.8, -69), math.ldexp(0.8, 148)]
LO, HI = math.ldexp(1.0, -823), math.ldexp(1.0, 953)          # fg_sep_trajectory's window on |n|


def bits(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", x))[0]


def unbits(s):
    return struct.unpack("<d", struct.pack("<Q", int(s, 16)))[0]


def constants(b):
    fb = Fraction(b)
    ch = float(1 / fb)
    cl = float(1 / fb - Fraction(ch))
    return ch, cl


def form2(a, b, c=None):
    ch, cl = c or constants(b)
    return float(Fraction(a) * Fraction(ch) + Fraction(float(Fraction(a) * Fraction(cl))))


def exact(a, b):
    return float(Fraction(a) / Fraction(b))


def near_midpoint(b, dmax=2000, per_class=6):
    """[(delta, a)]: a in [1, 2) with a / b exactly delta / (2 B) ulp from a midpoint.  A class with many solutions (small B) gives
    its first and last per_class / 2."""
    m, _ = math.frexp(b)
    B, z = int(m * 2 ** 53), 0
    while B % 2 == 0:
        B, z = B // 2, z + 1
    out = []
    if B == 1:
        return out
    for s in (52 - z, 53 - z):
        inv = pow(2, -s, B)
        for delta in range(-dmax + (dmax + 1) % 2, dmax + 1, 2):      # odd: X 2^(s+1) is even and B is odd
            if abs(delta) >= B:
                continue
            x0 = ((B + delta) // 2 % B) * inv % B
            x0 += (2 ** 52 - x0 + B - 1) // B * B
            count = (2 ** 53 - 1 - x0) // B + 1 if x0 < 2 ** 53 else 0
            ks = range(count) if count <= per_class else list(range(per_class // 2)) + list(range(count - per_class // 2, count))
            for k in ks:
                X = x0 + k * B
                assert (X * 2 ** (s + 1) - delta) % B == 0 and (X * 2 ** (s + 1) - delta) // B % 2 == 1
                out.append((delta, math.ldexp(float(X), -52)))
    return out


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("div2") / "div2_driver")
    subprocess.run(["g++", "-std=c++17", "-O2", "-mfma", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "div2_driver.cpp"), "-o", exe], check=True)

    def run(lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        return [ln.split() for ln in r.stdout.splitlines()]
    return run


@pytest.fixture(scope="module")
def enumerated():
    """Per divisor: its near-midpoint numerators and those on which the two-instruction form is not RN(a / b)."""
    out = {}
    for b in DIVISORS + EDGE_DIVISORS:
        c = constants(b)
        cand = near_midpoint(b)
        out[b] = (cand, [(d, a) for d, a in cand if form2(a, b, c) != exact(a, b)])
    return out


def prove(driver, bs):
    return [(int(v), unbits(hi), unbits(lo)) for v, hi, lo in driver(["prove " + bits(b) for b in bs])]


def test_verdict_is_the_enumerations(driver, enumerated):
    """(i) the C++ verdict == no near-midpoint numerator with |delta| <= 2000 fails; an accepted divisor comes with RN(1 / b) and
    RN(1 / b - Ch)."""
    for b, (v, hi, lo) in zip(DIVISORS + EDGE_DIVISORS, prove(driver, DIVISORS + EDGE_DIVISORS)):
        cand, wrong = enumerated[b]
        assert bool(v) == (not wrong), (b.hex(), v, wrong[:3])
        assert (hi, lo) == (constants(b) if v else (0.0, 0.0)), b.hex()
        assert cand, b.hex()
    assert len(enumerated[2e-5][0]) > 3000          # 2000 odd deltas, two scalings, 2^52 / B = 0.76 solutions per class


def test_default_is_accepted_and_the_failing_divisors_are_refused(driver, enumerated):
    """(ii) with a witness numerator for every refused divisor, which the C++ form gets wrong in the same way."""
    assert prove(driver, [2e-5])[0][0] == 1
    for b, (v, _, _) in zip(FAILING, prove(driver, FAILING)):
        assert v == 0, b.hex()
        wrong = enumerated[b][1]
        assert wrong and all(abs(d) <= 4 for d, _ in wrong), (b.hex(), wrong[:3])
        d, a = wrong[0]
        (got, ref), = driver(["eval %s %s" % (bits(b), bits(a))])
        assert unbits(ref) == exact(a, b) and unbits(got) == form2(a, b) and got != ref


def test_accepted_divisors_are_exact(driver, enumerated):
    """(iii) the form == RN(a / b) in exact arithmetic on the enumerated numerators, on 20 000 random numerators over the binades of
    [2^-823, 2^953) and at both ends of that window; the C++ form computes the Fraction form's bits."""
    everyone = DIVISORS + EDGE_DIVISORS
    accepted = [b for b, (v, _, _) in zip(everyone, prove(driver, everyone)) if v]
    assert set(accepted) >= set(DIVISORS) - set(FAILING) and math.ldexp(0.7, 148) in accepted and math.ldexp(0.7, -69) in accepted
    rng = random.Random(20)
    ends = [LO, math.nextafter(LO, 1.0), math.nextafter(HI, 0.0), math.nextafter(math.nextafter(HI, 0.0), 0.0), LO * 1.5, HI * 0.75]
    for b in accepted:
        c = constants(b)
        nums = [a for _, a in enumerated[b][0]]
        nums += [math.ldexp(a, e) for (_, a), e in zip(enumerated[b][0][:400], (rng.randrange(-823, 952) for _ in range(400)))]
        nums += [s * math.ldexp(1.0 + rng.random(), rng.randrange(-823, 953)) for s in (1.0, -1.0) for _ in range(10000)]
        nums += ends + [-a for a in ends]
        got = [form2(a, b, c) for a in nums]
        assert got == [exact(a, b) for a in nums], b.hex()
        assert all(LO <= abs(a) < HI for a in nums)
        cpp = driver(["eval %s %s" % (bits(b), bits(a)) for a in nums[::7]])
        assert [unbits(g) for g, _ in cpp] == got[::7] and [unbits(r) for _, r in cpp] == got[::7], b.hex()


def test_two_instruction_quotient_matches_ieee_division(tmp_path):
    """tests/cpp/test_div2.cpp: fg_div2 == a / b bit for bit on 2e7 random and near-midpoint quotients over accepted divisors."""
    exe = str(tmp_path / "test_div2")
    subprocess.run(["g++", "-std=c++17", "-O2", "-mfma", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_div2.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checked 2" in r.stdout and "mismatches 0" in r.stdout


def test_refused_inputs(driver):
    """(iv) zero, an all-ones significand, exponents outside [-70, 147], negative and non-finite divisors."""
    ones = unbits("3fefffffffffffff")
    bad = [0.0, -0.0, ones, math.ldexp(ones, 10), math.ldexp(1.0, -71), math.ldexp(1.999, -71), math.ldexp(1.0, 148), 1e200, 1e-200, 5e-324,
           -2e-5, math.inf, -math.inf, math.nan]
    assert [v for v, _, _ in prove(driver, bad)] == [0] * len(bad)
    ok = [math.ldexp(1.0, -70), math.ldexp(1.5, 147), 1.0, 0.5, 3.0]          # (powers of two: Cl = 0, the product alone is exact)
    res = prove(driver, ok)
    assert [v for v, _, _ in res] == [1] * len(ok)
    assert res[2][1:] == (1.0, 0.0) and res[3][1:] == (2.0, 0.0)
