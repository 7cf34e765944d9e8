"""tests/golden/math_exact.json and math_exact.bin without a device: the fixture is well-formed, the oracle lies within 4 units of every case's budget (the
condition under which a case may hold the device to 16), the committed files are what their generator writes, and the host build of the
primitives meets the assertions that tests/test_gpu_math_exact.py makes of the device build (tests/cpp/test_math_exact_host.cpp)."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import math_exact_fixture as MF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_is_well_formed():
    fx = MF.fixture()
    assert 1500 <= fx.n <= 2100 and len(fx.tag) == fx.n and set(fx.tag) == {"r", "z"}
    assert fx.families == list(MF.NPARAMS) and set(fx.fam.tolist()) == set(range(13))
    for a in (fx.hi, fx.lo, fx.budget, fx.x_bits):
        assert len(a) == fx.n
    assert fx.p.shape == (3, fx.n) and np.isfinite(fx.p).all() and np.isfinite(fx.hi).all() and (fx.budget > 0).all() and np.isfinite(fx.budget).all()
    assert (np.abs(fx.lo) <= 0.5 * MF.ulp(fx.hi) * (1 + 2.0 ** -20)).all()                  # hi is the nearest double
    assert (np.abs(fx.hi) <= fx.budget * (1 + 1e-15)).all()                                  # |sum| <= sum of |terms|
    for k, name in enumerate(fx.families):
        sel = fx.fam == k
        assert sel.sum() >= 60, name
        zeros = sum(1 for i in np.nonzero(sel)[0] if fx.tag[i] == "z")
        assert (zeros >= 200 if name in ("Beta", "Gamma", "StudentT", "ChiSquared", "InverseGamma") else zeros >= 9 if name in MF.INT_FAMILIES else zeros == 0), name
    # the ranges the cases must reach
    top = lambda name, row: fx.p[row, fx.fam == fx.families.index(name)].max()
    assert top("Binomial", 0) > 1e11 and top("Poisson", 0) > 1e11 and top("StudentT", 0) > 1e10 and top("Beta", 0) > 3e5 and top("Gamma", 0) > 3e5
    raw = fx.raw
    n_prim = 0
    for g, cols in (("div", ("a", "b")), ("log", ("a", "hi", "lo")), ("sincos", ("a", "sin_hi", "sin_lo", "cos_hi", "cos_lo")),
                    ("pair", ("wa", "wb", "z0_hi", "z0_lo", "z1_hi", "z1_lo", "gz_hi", "gz_lo")), ("digamma", ("a", "hi", "lo"))):
        assert set(raw[g]) == set(cols), g
        n = len(raw[g][cols[0]]) // 16
        n_prim += n
        for c in cols:
            assert len(raw[g][c]) == n * (8 if c.endswith("lo") else 16), (g, c)
    assert 3000 <= n_prim <= 4500
    for name in ("log", "log1p", "lgamma", "exp", "pow", "tan"):
        o = raw["ocml"][name]
        n = len(o["a"]) // 16
        assert n >= 60 and len(o["hi"]) == 16 * n and len(o["lo"]) == 8 * n and (("b" in o) == (name == "pow"))
    assert len(raw["normal_fast_edges"]) == 6
    assert os.path.getsize(MF.PATH) < 1 << 14 and os.path.getsize(MF.PATH_BIN) < 1 << 19


def test_oracle_is_within_four_units_of_every_budget(oracle):
    """no mpmath: the oracle against the committed exact values"""
    fx = MF.fixture()
    got = np.array([oracle.logpdf(fx.family_name(i), fx.value(i), fx.params(i)) for i in range(fx.n)])
    K = fx.K(got)
    worst = {name: float(K[fx.fam == k].max()) for k, name in enumerate(fx.families)}
    print("oracle, worst K per family:", {k: round(v, 2) for k, v in worst.items()})
    assert np.isfinite(got).all() and K.max() <= 4.0, worst
    for e in fx.raw["normal_fast_edges"]:
        o = oracle.logpdf("Normal", e["x"], [e["mu"], e["sigma"]])
        if e["expected"] == "-inf":
            assert o == -math.inf
        else:
            assert np.array([o]).view(np.uint64)[0] == int(e["expected"], 16)


def test_committed_fixture_is_what_the_generator_writes():
    pytest.importorskip("mpmath")
    from tests.golden import gen_math_exact as G
    text, blob = G.generate()
    with open(MF.PATH) as f, open(MF.PATH_BIN, "rb") as fb:
        assert f.read() == text and fb.read() == blob


def test_host_build_of_the_primitives(tmp_path):
    """fg_div_const's window and fg_digamma's bound on the host build of fg_math.h"""
    raw = MF.fixture().raw["digamma"]
    n = len(raw["a"]) // 16
    pts = tmp_path / "digamma.txt"
    pts.write_text("".join(f"{raw['a'][16 * i:16 * i + 16]} {raw['hi'][16 * i:16 * i + 16]} {raw['lo'][8 * i:8 * i + 8]}\n" for i in range(n)))
    exe = str(tmp_path / "test_math_exact_host")
    subprocess.run(["g++", "-std=c++17", "-O2", "-mfma", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_math_exact_host.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, str(pts)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "math exact host ok" in r.stdout and f"digamma: {n} points" in r.stdout
