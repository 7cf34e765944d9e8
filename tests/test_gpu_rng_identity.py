"""The momentum draw of the samplers in its present form (scalar Philox keys, one three-input xor per round output, polynomial
coefficients from SGPRs, fg_sqrt_pos) against the form it replaced (vector keys, two xors, the compiler's constant operands, ocml's
sqrt), which the library keeps behind the debug entry point fg_debug_rng_pairs (fg_rng_debug.hip).  Every comparison is bit for bit:
the change removes instructions, it changes no number that is drawn."""
import ctypes as C

import numpy as np
import pytest

from fugue_amd import engine as E

pytestmark = pytest.mark.gpu

ROWS = 12
RNG_HMC, RNG_SMC_REJUV = 2, 6                 # fg_ir.h
SEEDS = (0x9E3779B97F4A7C15, 0x00000000DEADBEEF)   # the second: a zero high word (k1 = 0)
U64 = C.POINTER(C.c_uint64)


def _call(mode, n, seed=0, chain0=0, block=0, it=0, purpose=RNG_HMC, wa=None, wb=None):
    L = E.lib()
    L.fg_debug_rng_pairs.argtypes = [C.c_int, C.c_longlong, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, U64, U64, U64]
    L.fg_debug_rng_pairs.restype = C.c_int
    out = np.zeros((ROWS, n), dtype=np.uint64)
    pa = np.ascontiguousarray(wa, dtype=np.uint64) if wa is not None else None
    pb = np.ascontiguousarray(wb, dtype=np.uint64) if wb is not None else None
    rc = L.fg_debug_rng_pairs(mode, n, seed, chain0, block, it, purpose, pa.ctypes.data_as(U64) if pa is not None else None,
                              pb.ctypes.data_as(U64) if pb is not None else None, out.ctypes.data_as(U64))
    assert rc == 0
    return out


def _same_pairs(o):
    assert np.array_equal(o[0], o[2]) and np.array_equal(o[1], o[3])          # the normal pair, bits


@pytest.mark.parametrize("seed", SEEDS)
def test_counters_old_and_new_agree_bit_for_bit(seed):
    """65 536 consecutive chain ids x 3 blocks x 3 iterations x 2 purposes: the normal pair, the Philox words and the two uniforms."""
    n, chain0 = 65536, 5
    seen = set()
    for block in (0, 1, 17):
        for it in (0, 1, 1234567):
            for purpose in (RNG_HMC, RNG_SMC_REJUV):
                o = _call(0, n, seed, chain0, block, it, purpose)
                _same_pairs(o)
                assert np.array_equal(o[4], o[6]) and np.array_equal(o[5], o[7])      # Philox words
                assert np.array_equal(o[8], o[10]) and np.array_equal(o[9], o[11])    # uniforms of fg_cold_u01_pair
                z = o[:2].view(np.float64)
                assert np.isfinite(z).all() and 0.95 < z.std() < 1.05 and len(np.unique(o[6])) == n
                seen.add(int(o[6][0]))
    assert len(seen) == 18                                                             # every counter word and the key take part


def test_partial_waves_agree_with_full_ones():
    """A chain count that is no multiple of 64: the last wave runs the scalar-key form with inactive lanes."""
    seed = SEEDS[1]
    full = _call(0, 4160, seed, 9, 3, 7, RNG_HMC)
    for n in (100, 4133, 1):
        o = _call(0, n, seed, 9, 3, 7, RNG_HMC)
        _same_pairs(o)
        assert np.array_equal(o, full[:, :n])


def _forced_words():
    """a, b: the 53-bit values after the shift (u1 = (a + 1) 2^-53, u2 = b 2^-53)."""
    a = [0, 2**53 - 1]                                   # u1 = 2^-53; u1 = 1: ln = +0, -0 into the root, r = -0
    for k in range(0, 53):                               # m = a + 1 in [2^k, 2^(k+1)): the first significand fg_fast_log halves (0x95f64), and the one before
        mb = (0x16a09c << (k - 20)) if k >= 20 else ((0x16a09c + (1 << (20 - k)) - 1) >> (20 - k))
        for m in (mb - 1, mb):
            if 1 <= m <= 2**53: a.append(m - 1)
    b = [0, 2**53 - 1]
    for k in (1, 2, 3):                                  # the quadrant changes of sincos
        b += [k * 2**51 - 1, k * 2**51, k * 2**51 + 1]
    aa, bb = np.meshgrid(np.array(a, dtype=np.uint64), np.array(b, dtype=np.uint64), indexing="ij")
    low = np.uint64(0x7ff)                               # the 11 bits the shift drops: both all ones and all zeros
    wa = np.concatenate([aa.ravel() << np.uint64(11), (aa.ravel() << np.uint64(11)) | low])
    wb = np.concatenate([bb.ravel() << np.uint64(11), (bb.ravel() << np.uint64(11)) | low])
    return wa, wb


def test_forced_words_agree_bit_for_bit():
    wa, wb = _forced_words()
    o = _call(1, len(wa), wa=wa, wb=wb)
    _same_pairs(o)
    x, got = o[4].view(np.float64), o[5].view(np.float64)
    assert np.array_equal(np.sqrt(x).view(np.uint64), got.view(np.uint64))            # fg_sqrt_pos == the correctly rounded root, -0 -> -0
    assert np.array_equal(o[5], o[6])                                                  # ... == ocml's sqrt
    one = (wa >> np.uint64(11)) == np.uint64(2**53 - 1)                                # u1 = 1
    assert one.any() and (o[4][one] == np.uint64(0x8000000000000000)).all() and (o[5][one] == np.uint64(0x8000000000000000)).all()
    zero = (wa >> np.uint64(11)) == np.uint64(0)                                       # u1 = 2^-53: the largest radius
    assert np.allclose(x[zero], 2 * 53 * np.log(2.0), rtol=1e-15)


def test_sqrt_pos_is_the_correctly_rounded_root():
    rng = np.random.default_rng(11)
    x = np.exp2(rng.uniform(-60.0, 7.0, 100_000))
    x = np.concatenate([x, [2.0**-60, 2.0**7, 2.2e-16, 73.5, 1.0, 4.0, 0.0, -0.0, np.inf]])
    o = _call(2, len(x), wa=x.view(np.uint64))
    assert np.array_equal(o[0], np.sqrt(x).view(np.uint64))
    assert np.array_equal(o[0], o[1])
