"""How the reference's model language turns an observed expression into the value a discrete density is evaluated at, restated in plain
Python integers from crates/fugue-wasm/src/dsl.rs -- and sharing nothing with oracle/ or fg_math.h:

  Value::as_index (:71-77)    Int(i) -> Some(i);  F64(x) if x.fract() == 0.0 && x.is_finite() -> Some(x as i64);  otherwise None
  Value::as_bool  (:79-84)    as_f64() != 0.0  (NaN is true)
  Stmt::Observe   (:985-998)  U64 / Usize: as_index().unwrap_or(0).max(0);  I64: as_index().unwrap_or(0);  Bool: as_bool()
  build_dist      (:843-851)  Binomial: `a[0] < 0.0 || a[0].fract() != 0.0` is an error (the statement becomes factor(-inf), :1002-1006),
                              otherwise `a[0] as u64`

`as i64` / `as u64` of a float saturate and send NaN to 0 (Rust reference, "Numeric cast").  f64::fract is `x - x.trunc()`: NaN for NaN
and for +-inf, which is why an infinite Binomial n is an error without an `is_finite` test.

The expected log-density of an observe statement is then `oracle.logpdf(family, observed_int(vtype, x), params)`: the oracle's density
functions take the integer itself and are pinned by tests/test_oracle_kats.py, so the expectation does not pass through the conversion
under test."""
import math
import struct

I64_MIN, I64_MAX, U64_MAX = -(1 << 63), (1 << 63) - 1, (1 << 64) - 1
VTYPES = {"bool": 1, "u64": 2, "usize": 3, "i64": 4}                      # ChoiceValue tags of fugue_amd.model
FAMILY_VTYPE = {"Bernoulli": "bool", "Binomial": "u64", "Poisson": "u64", "Categorical": "usize", "DiscreteUniform": "i64"}   # dsl.rs:842-856


def from_bits(hex16: str) -> float:
    return struct.unpack("<d", struct.pack("<Q", int(hex16, 16)))[0]


def to_bits(x: float) -> int:
    """the f64 as a signed 64-bit cell"""
    return struct.unpack("<q", struct.pack("<d", x))[0]


def _fract_is_zero(x: float) -> bool:
    """x.fract() == 0.0 (fract = x - x.trunc(): NaN for a non-finite x)"""
    if math.isnan(x) or math.isinf(x):
        return False
    return math.modf(x)[0] == 0.0


def as_i64(x: float) -> int:
    """Rust `x as i64`"""
    if math.isnan(x):
        return 0
    if math.isinf(x):
        return I64_MAX if x > 0 else I64_MIN
    return min(max(int(x), I64_MIN), I64_MAX)                             # int() of a finite float is exact


def as_u64(x: float) -> int:
    """Rust `x as u64`"""
    if math.isnan(x):
        return 0
    if math.isinf(x):
        return U64_MAX if x > 0 else 0
    return min(max(int(x), 0), U64_MAX)


def as_index(x: float):
    """dsl.rs:71-77 for Value::F64"""
    return as_i64(x) if _fract_is_zero(x) and math.isfinite(x) else None


def as_bool(x: float) -> bool:
    """dsl.rs:79-84"""
    return x != 0.0


def observed_int(vtype: str, x: float) -> int:
    """dsl.rs:985-998"""
    if vtype == "bool":
        return int(as_bool(x))
    i = as_index(x)
    i = 0 if i is None else i
    return i if vtype == "i64" else max(i, 0)


def binomial_n(x: float):
    """dsl.rs:843-851 -> (valid, n)"""
    if x < 0.0 or not _fract_is_zero(x):
        return False, None
    return True, as_u64(x)


def expected_logpdf(oracle, family: str, x: float, params) -> float:
    """The reference's log-weight of `observe(_, family(params), x)`; Binomial's n goes through build_dist's test first."""
    if family == "Binomial":
        ok, n = binomial_n(float(params[0]))
        if not ok:
            return -math.inf
        params = [float(n), params[1]]                                    # (exact below 2^53; u64::MAX rounds to 2^64, which `as u64` takes back to u64::MAX)
    if family == "DiscreteUniform":
        return oracle.logpdf_discrete_uniform(observed_int("i64", x), as_i64(float(params[0])), as_i64(float(params[1])))   # bounds `as i64`, dsl.rs:854-856
    return oracle.logpdf(family, observed_int(FAMILY_VTYPE[family], x), params)
