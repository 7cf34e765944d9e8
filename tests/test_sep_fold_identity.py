"""The two identities behind the folded trajectory loop of k_hmc_sep_steps (fg_hmc_sep.hip, FG_SEP_DUALS and the deferred range
test), checked on the host in exact rational arithmetic:

1. for sigma = 2^-k (1 / sigma = s = 2^k, k <= 480) the folded density RN(RN(-0.5 s^2 RN(d^2) - ln sigma) - 0.5 ln 2 pi) equals the
   reference's RN(RN(RN(RN(-0.5 z) z) - ln sigma) - 0.5 ln 2 pi) with z = RN(d s) whenever it is finite, and is -inf only when
   RN(d^2) or the reference overflows; and it equals the fused loop's value RN(RN(-0.5 RN(z z) - ln sigma) - 0.5 ln 2 pi) wherever both are finite;
2. the 32-bit test 2 |hi(n)| - 0x19000000 < 0xde000000 (mod 2^32) holds exactly for 2^-823 <= |n| < 2^953, so it flags every n
   the per-step test |n| in [2^-823, 2^953] flags."""
import math
import struct
from fractions import Fraction

import numpy as np

LN_2PI = 1.8378770664093454835606594728112


def _rn(x: Fraction) -> float:
    """x rounded to the nearest double (ties to even), overflow to +-inf."""
    try:
        return float(x)                                  # int / int true division: correctly rounded, subnormals included
    except OverflowError:
        return math.inf if x > 0 else -math.inf


def _fma(a: float, b: float, c: float) -> float:
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c
    return _rn(Fraction(a) * Fraction(b) + Fraction(c))


def _ref(d, s, lns):                                     # FG_SEP_LP: -0.5 * z * z - ln sigma - 0.5 ln 2 pi, unfused
    z = d * s
    return ((-0.5 * z) * z - lns) - 0.5 * LN_2PI


def _fused(d, s, lns):                                   # FG_SEP_LPF
    z = d * s
    return _fma(-0.5, z * z, -lns) - 0.5 * LN_2PI


def _folded(d, s, lns):                                  # FG_SEP_DUALS (nhs2 = -0.5 s^2, as the host stores it)
    return _fma(-0.5 * s * s, d * d, -lns) - 0.5 * LN_2PI


def _cases(rng):
    ks = [0, 1, 2, -1, -2, 5, -5, 30, -30, 200, -200, 400, -400, 480, -498] + [int(k) for k in rng.integers(-498, 481, 12)]
    for k in ks:
        s = math.ldexp(1.0, k)
        lns = math.log(1.0 / s)                          # the host's ln(sigma)
        ds = [0.0, -0.0, 1.0, 0.3, math.ldexp(1.0, -1074), math.ldexp(1.0, -1022), math.ldexp(1.0, 511), math.ldexp(1.0, 512),
              math.ldexp(1.5, 511), math.ldexp(1.0, -511), math.ldexp(1.0, -537), math.ldexp(1.0, -530) * (1 + 2.0 ** -52)]
        ds += [math.ldexp(1.0, 511 - k) * f for f in (0.7, 0.99999999, 1.0, 1.0000001, 1.4142135623730951, 1.5)]   # (d s)^2 at the overflow threshold
        ds += [math.ldexp(1.0, -511 - k) * f for f in (0.5, 0.99999999, 1.0, 1.3)]                                  # (d s)^2 at the subnormal boundary
        ds += [math.ldexp(float(m), int(e)) for m, e in zip(rng.uniform(0.5, 1.0, 40), rng.integers(-1080, 520, 40))]
        ds += list(rng.normal(size=20) * 10.0 ** rng.uniform(-5, 5, 20))
        for d in ds:
            for x in (d, -d):
                yield x, s, lns


def test_folded_density_matches_reference_and_fused_form():
    rng = np.random.default_rng(5)
    n = 0
    for d, s, lns in _cases(rng):
        if not math.isfinite(d * s):
            continue
        new, ref, fused = _folded(d, s, lns), _ref(d, s, lns), _fused(d, s, lns)
        if math.isfinite(new):
            assert new == ref, (d, s, new, ref)          # a finite folded value is the reference's
        else:
            assert math.isinf(d * d) or not math.isfinite(ref), (d, s, new, ref)   # d^2 or the reference overflowed: the checked re-run
        if math.isfinite(fused) and math.isfinite(new):
            assert new == fused, (d, s, new, fused)      # the same bits as the loop it replaces (-inf: the re-run gives them)
        n += 1
    assert n > 3000


def _hi(x: float) -> int:
    return struct.unpack("<Q", struct.pack("<d", x))[0] >> 32


def _int_in_range(n: float) -> bool:
    return ((_hi(n) << 1) - 0x19000000) % (1 << 32) < 0xde000000


def test_deferred_range_test_is_exact():
    rng = np.random.default_rng(6)
    lo, hi = math.ldexp(1.0, -823), math.ldexp(1.0, 953)
    vals = [0.0, -0.0, math.inf, -math.inf, math.nan, lo, hi, math.nextafter(lo, 0.0), math.nextafter(lo, 1.0),
            math.nextafter(hi, 0.0), math.nextafter(hi, math.inf), math.ldexp(1.0, -1074), 1.7976931348623157e308, 1.0]
    vals += [math.ldexp(float(m), int(e)) for m, e in zip(rng.uniform(0.5, 1.0, 4000), rng.integers(-1080, 1025, 4000))]
    vals += list(np.frombuffer(rng.integers(0, 2 ** 63, 4000, dtype=np.int64).tobytes(), dtype=np.float64))
    for v in vals:
        for n in (float(v), -float(v)):
            a = abs(n)
            assert _int_in_range(n) == (lo <= a < hi), n
            if not (a >= lo and a <= hi):                # the per-step test's flags are a subset
                assert not _int_in_range(n), n
