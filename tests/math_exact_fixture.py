"""Reader of tests/golden/math_exact.json and math_exact.bin (written by tests/golden/gen_math_exact.py, which documents the layout) for
tests/test_math_exact_cpu.py and tests/test_gpu_math_exact.py.  numpy only; the arrays are read-only."""
import json
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "math_exact.json")
PATH_BIN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "math_exact.bin")
INT_FAMILIES = ("Binomial", "Poisson")
NPARAMS = {"Normal": 2, "LogNormal": 2, "Exponential": 1, "Beta": 2, "Gamma": 2, "Binomial": 2, "Poisson": 1, "StudentT": 3, "Cauchy": 2,
           "Laplace": 2, "Weibull": 2, "ChiSquared": 1, "InverseGamma": 2}
LGAMMA_FAMILIES = ("Beta", "Gamma", "Binomial", "Poisson", "StudentT", "ChiSquared", "InverseGamma")
EPS = 2.0 ** -53


def u64(hexes: str) -> np.ndarray:
    assert len(hexes) % 16 == 0
    a = np.array([int(hexes[i:i + 16], 16) for i in range(0, len(hexes), 16)], dtype=np.uint64)
    a.setflags(write=False)
    return a


def f64(hexes: str) -> np.ndarray:
    return u64(hexes).view(np.float64)


def f32(hexes: str) -> np.ndarray:
    assert len(hexes) % 8 == 0
    a = np.array([int(hexes[i:i + 8], 16) for i in range(0, len(hexes), 8)], dtype=np.uint32).view(np.float32).astype(np.float64)
    a.setflags(write=False)
    return a


def err(got: np.ndarray, hi: np.ndarray, lo: np.ndarray) -> np.ndarray:
    """|got - exact| for exact = hi + lo (got - hi is exact wherever got is near hi)"""
    return np.abs((np.asarray(got, dtype=np.float64) - hi) - lo)


def ulp(x: np.ndarray) -> np.ndarray:
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)))


def _unpack(v, blob: bytes):
    """{"@": offset, "n": bytes} -> the hex digits of those bytes of math_exact.bin (gen_math_exact.py: `pack`)"""
    if isinstance(v, dict):
        if set(v) == {"@", "n"}:
            assert 0 <= v["@"] and v["@"] + v["n"] <= len(blob)
            return blob[v["@"]:v["@"] + v["n"]].hex()
        return {k: _unpack(w, blob) for k, w in v.items()}
    return v


class Fixture:
    def __init__(self, path: str = PATH, path_bin: str = PATH_BIN):
        with open(path) as f, open(path_bin, "rb") as fb:
            d = _unpack(json.load(f), fb.read())
        self.raw = d
        self.families = d["families"]
        L = d["logpdf"]
        self.fam = np.array([int(c, 16) for c in L["family"]], dtype=np.int64)
        self.tag = L["tag"]
        self.p = np.stack([f64(L["p0"]), f64(L["p1"]), f64(L["p2"])])            # [3][N]
        self.x_bits = u64(L["x"])                                                # a double's bits, or the int64 of an integer family
        self.hi, self.lo, self.budget = f64(L["hi"]), f32(L["lo"]), f64(L["budget"])
        self.n = len(self.fam)
        for a in (self.fam, self.p):
            a.setflags(write=False)

    def family_name(self, i: int) -> str:
        return self.families[int(self.fam[i])]

    def value(self, i: int):
        """the case's value as the number a model holds: an int for the integer families, else a float"""
        if self.family_name(i) in INT_FAMILIES:
            return int(self.x_bits[i:i + 1].view(np.int64)[0])
        return float(self.x_bits[i:i + 1].view(np.float64)[0])

    def params(self, i: int):
        return [float(v) for v in self.p[:NPARAMS[self.family_name(i)], i]]

    def K(self, got: np.ndarray, idx=None) -> np.ndarray:
        """|got - exact| in units of 2^-53 B"""
        idx = np.arange(self.n) if idx is None else np.asarray(idx)
        return err(got, self.hi[idx], self.lo[idx]) / (EPS * self.budget[idx])

    def column(self, group: str, name: str) -> np.ndarray:
        h = self.raw[group][name]
        return f32(h) if name.endswith("lo") else f64(h)


_CACHE = {}


def fixture() -> Fixture:
    if "f" not in _CACHE:
        _CACHE["f"] = Fixture()
    return _CACHE["f"]
