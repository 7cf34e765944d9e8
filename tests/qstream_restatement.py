"""A numpy restatement of the streamed quantile selection (fugue_amd/csrc/fg_diag_qstream_plan.h), slot by slot, and the plain
reference it must equal: sort by the order-preserving key, take index round((len - 1) p) (summarize_f64_parameter,
diagnostics.rs:355-371).

A slot (one coordinate, one probability) holds b decided leading key bits, their prefix, the rank r among the elements matching
the prefix and their count m; start b = 0, m = len, r = round((len - 1) p) half away from zero.  Every pass sees the whole column:
  collect    (m <= capacity)  the answer is the r-th smallest matching key;
  histogram  (otherwise)      count the next w = min(digit_bits, 64 - b) bits of the matching keys; if their min == max that key is
                              the answer; else walk to the digit holding r, r -= counts below, extend the prefix, b += w, m = that
                              digit's count; b == 64 makes the prefix the answer.
The matching count of a pass must equal the m the previous pass left (ReplayDiverged otherwise).

Also the seeded inputs shared by tests/test_diag_qstream_cpu.py and tests/test_gpu_diag_qstream.py."""
import math

import numpy as np

DEFAULT_PROBS = (0.025, 0.25, 0.5, 0.75, 0.975)
PROBS8 = (0.0, 0.001, 0.025, 0.25, 0.5, 0.75, 0.999, 1.0)
U64 = np.uint64
TOP = U64(1) << U64(63)


class ReplayDiverged(Exception):
    pass


def key(x: np.ndarray) -> np.ndarray:
    """Ascending in the double's order: -0.0 just below +0.0, positive-sign NaN above +inf."""
    u = np.ascontiguousarray(x, dtype=np.float64).view(U64)
    return np.where((u >> U64(63)) != 0, ~u, u | TOP)


def unkey(k) -> np.ndarray:
    k = np.asarray(k, dtype=U64)
    return np.where((k >> U64(63)) != 0, k & ~TOP, ~k).astype(U64).view(np.float64)


def rank(length: int, p: float) -> int:
    """round((len - 1) p), half away from zero (f64::round); the product is one f64 multiplication."""
    v = float(length - 1) * float(p)
    f = math.floor(v)
    return int(f) + (1 if v - f >= 0.5 else 0)


def bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.float64).view(U64)


def reference(column: np.ndarray, probs) -> np.ndarray:
    """The elements a sort by key puts at the ranks: [len(probs)] doubles."""
    k = np.sort(key(np.asarray(column).ravel()))
    return unkey(np.array([k[rank(k.size, p)] for p in probs], dtype=U64))


def select(column: np.ndarray, probs, digit_bits: int, capacity: int, replays=None):
    """(values [len(probs)], passes per slot [len(probs)]) of one column (any shape: all its elements).  `replays`: the columns
    presented in pass 2, 3, ... (the last one again when more passes follow); default: the same column every pass."""
    presented = [np.asarray(column)] + [np.asarray(c) for c in (replays or [])]
    keys = [key(c.ravel()) for c in presented]
    length = keys[0].size
    values, passes = [], []
    for p in probs:
        b, prefix, r, m, n_pass = 0, 0, rank(length, p), length, 0
        while True:
            k = keys[min(n_pass, len(keys) - 1)]
            n_pass += 1
            match = k if b == 0 else k[(k >> U64(64 - b)) == U64(prefix >> (64 - b))]
            if match.size != m:
                raise ReplayDiverged(f"pass {n_pass}: {match.size} elements match where {m} did")
            if m <= capacity:
                answer = int(np.sort(match)[r])
                break
            w = min(digit_bits, 64 - b)
            lo, hi = int(match.min()), int(match.max())
            if lo == hi:
                answer = lo
                break
            digit = (match >> U64(64 - b - w)) & U64((1 << w) - 1)
            hist = np.bincount(digit.astype(np.int64), minlength=1 << w)
            cum, dg = 0, 0
            while dg < (1 << w) - 1 and cum + int(hist[dg]) <= r:
                cum += int(hist[dg])
                dg += 1
            r -= cum
            prefix |= dg << (64 - b - w)
            b += w
            m = int(hist[dg])
            if b == 64:
                answer = prefix
                break
        values.append(answer)
        passes.append(n_pass)
    return unkey(np.array(values, dtype=U64)), np.array(passes, dtype=np.int32)


def select_all(x: np.ndarray, probs, digit_bits: int, capacity: int):
    """select over every coordinate of x [n][d][C]: (values [d][len(probs)], slot passes [d][len(probs)], passes of the stream)."""
    out = [select(x[:, i, :], probs, digit_bits, capacity) for i in range(x.shape[1])]
    values, sp = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    return values, sp, int(sp.max())


def reference_all(x: np.ndarray, probs) -> np.ndarray:
    return np.stack([reference(x[:, i, :], probs) for i in range(x.shape[1])])


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------
SPECIALS = np.array([-np.inf, -1.5, -0.0, 0.0, 5e-324, -5e-324, 1.0, 1.0 + 2.0 ** -52, np.inf, np.nan])


def normal_input() -> np.ndarray:
    """[97][3][70] iid N(0, 1): 6 790 elements per coordinate."""
    return np.random.default_rng(97).standard_normal((97, 3, 70))


def last_bits_column(n: int = 97, C: int = 70) -> np.ndarray:
    """1 + k 2^-52, k < 16: the values differ in the last four bits only, so no histogram pass before the sixth (12-bit digits)
    separates them and min != max throughout."""
    return 1.0 + np.random.default_rng(5).integers(0, 16, (n, C)) * 2.0 ** -52


def constant_column(n: int = 97, C: int = 70) -> np.ndarray:
    return np.full((n, C), 2.5)


def specials_column(n: int = 97, C: int = 70) -> np.ndarray:
    """Draws from {-inf, -1.5, -0.0, +0.0, +-5e-324, 1, 1 + 2^-52, +inf, NaN}: every ordering rule of the key, heavy ties."""
    return SPECIALS[np.random.default_rng(11).integers(0, SPECIALS.size, (n, C))]


def adversarial_input(C: int = 70) -> np.ndarray:
    """[97][3][C]: specials, last bits, constant."""
    return np.ascontiguousarray(np.stack([specials_column(97, C), last_bits_column(97, C), constant_column(97, C)], axis=1))
