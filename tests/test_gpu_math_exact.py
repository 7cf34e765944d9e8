"""The device's arithmetic against exact values (tests/golden/math_exact.json and .bin, written with mpmath by tests/golden/gen_math_exact.py).

Primitives, through the debug entry point fg_debug_math (fg_rng_debug.hip): fg_div_const against IEEE division inside the window of
its bitwise claim, fg_fast_log / fg_fast_sincos / the normal pair / gaussian_z / fg_digamma against exact values, and ocml's log,
log1p, lgamma, exp, pow and tan measured (not asserted) at every argument the log-density cases feed them.

Log-densities: every case of the fixture on every path that computes a density -- the interpreter with site-fed and with constant
(hoisted) parameters, the score-stream records in both forms, the unit compiled at run time -- held to
    |device - exact| <= 16 * 2^-53 * B,        B = sum |term| + (number of lgamma calls),
the case's budget.  16 is derived, not measured: a term is at most one function value (F ulp = 2F 2^-53 relative), one product rounding
and one rounding per in-order addition of at most six terms, (2F + 6) 2^-53 B, with F = 5 allowed to ocml.  The oracle is within 4 on
the same cases (tests/test_math_exact_cpu.py).

fg_div_const below its window (|a| < 2^-968): the result is finite and within 2^-1022 of a / b where |a / b| < 2^-970; for larger
quotients that absolute bound cannot hold of any faithful quotient (on the host build 12 488 of 2 000 000 quotients with a in
2^[-1022, -969] and b in 2^[-399, -60] miss it, the worst by 2^-671, one ulp of that quotient), and the assertion is two ulps of a / b.

Measured on an MI355X (records, not thresholds; worst K = |device - exact| / (2^-53 B) per family and path, the oracle's next to it):

  family        oracle  site/interp  site/stream  const/interp  const/stream  compiled unit (sum of 13)
  Normal         1.54         1.54         1.54          1.54          1.54           3.22
  LogNormal      1.52         1.52         1.52          1.52          1.52           1.95
  Exponential    1.19         1.19         1.19          1.04          1.04           1.79
  Beta           1.98         1.98         1.98          1.38          1.38           1.74
  Gamma          1.46         1.46         1.46          1.46          1.46           3.27
  Binomial       1.34         1.34         1.34          1.34             -           1.34
  Poisson        1.28         1.30         1.30          1.28          1.28           1.30
  StudentT       1.34         1.02         1.02          1.02          1.02           0.78
  Cauchy         1.65         1.49         1.49          1.49          1.49           0.58
  Laplace        1.41         1.41         1.41          1.41          1.41           0.89
  Weibull        2.01         2.01         2.01          1.35          1.35           0.65
  ChiSquared     1.79         1.79         1.79          1.79          1.79           3.51
  InverseGamma   1.61         1.61         1.61          1.59          1.59           1.76
  (1 892 cases; the constant forms run the 1 320-case subset: every case next to a zero of lgamma and 20 wide cases per family; hoisted
  Binomial has no stream record.  The cap on every path is 16.)

  ocml, worst error in ulps of the exact value (lgamma: of max(1, |exact|)), at the arguments the cases feed:
    log    0.619 at 1.0625 (2 760 arguments)          log1p  0.545 at 0.2430656990965424 (336)
    lgamma 1.576 at 10.796083340161106 (1 546)        exp    0.524 at -2.992443025422494 (60)
    pow    0.829 at (1808.9306121285633, 0.08832761349197792) (64)      tan 0.576 at -0.5899766181847166 (60)
  primitives: fg_div_const 0 mismatches with the device's `/` and with IEEE division on 116 619 quotients inside the window (5 of 1 285
    below it misrounded); fg_fast_log 0.648 ulp at 2.721057825267751 (ocml log 0.590 on the same 940 points); fg_fast_sincos sin 0.576 /
    cos 0.601 ulp, absolute 6.4e-17 / 6.7e-17; normal pair |z - exact| <= 2.08e-16 r, gaussian_z 2.29e-16 r; fg_digamma 1.33e-13
    max(1, |psi|) at x = 1 (the host build: the same).
"""
import ctypes as C
import math
import os

import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import model as M
from tests import math_exact_fixture as MF
from tests import test_gpu_golden as TG

pytestmark = pytest.mark.gpu

OP_DIV, OP_LOG, OP_SINCOS, OP_PAIR, OP_OCML, OP_DIGAMMA = range(6)
ROWS, MAX_LAUNCH = 6, 65536
K_CAP = 16.0
DP, U64P = C.POINTER(C.c_double), C.POINTER(C.c_uint64)


def _math(op, a, b=None, c=None):
    """fg_debug_math on the arrays (doubles; PAIR: the words' bits), in launches of at most 65 536 elements -> [ROWS][n] uint64"""
    L = E.lib()
    L.fg_debug_math.argtypes = [C.c_int, C.c_longlong, DP, DP, DP, U64P]
    L.fg_debug_math.restype = C.c_int
    arrs = [None if v is None else np.ascontiguousarray(v).view(np.float64) for v in (a, b, c)]
    n = len(arrs[0])
    out = np.zeros((ROWS, n), dtype=np.uint64)
    for s in range(0, n, MAX_LAUNCH):
        part = [None if v is None else np.ascontiguousarray(v[s:s + MAX_LAUNCH]) for v in arrs]
        m = len(part[0])
        o = np.zeros((ROWS, m), dtype=np.uint64)
        rc = L.fg_debug_math(op, m, *[None if v is None else v.ctypes.data_as(DP) for v in part], o.ctypes.data_as(U64P))
        assert rc == 0
        out[:, s:s + m] = o
    return out


def _col(group, name):
    return MF.fixture().column(group, name)


def _ulps(got, hi, lo):
    return MF.err(got, hi, lo) / MF.ulp(hi)


# ---------------------------------------------------------------------------------------------------------------------------------
# primitives
# ---------------------------------------------------------------------------------------------------------------------------------
def _div_const_ok(b):
    u = np.ascontiguousarray(b).view(np.uint64)
    e = (u >> np.uint64(52)) & np.uint64(0x7FF)
    return (e > 1023 - 400) & (e < 1023 + 400) & ((u & np.uint64(0xFFFFFFFFFFFFF)) != np.uint64(0xFFFFFFFFFFFFF))


def _rnd(rng, n, emin, emax):
    u = ((rng.integers(emin, emax + 1, n) + 1023).astype(np.uint64) << np.uint64(52)) | rng.integers(0, 1 << 52, n).astype(np.uint64)
    return (u | (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(63))).view(np.float64)


def test_div_const_is_ieee_division_inside_its_window():
    """The fixture's divisors and numerators, and 120 000 random quotients more (numpy's `/` is the expectation: no exact value needed)."""
    a, b = _col("div", "a"), _col("div", "b")
    rng = np.random.default_rng(5)
    n = 60000
    fixed = np.unique(b)
    rb = np.where(rng.integers(0, 4, 2 * n) == 0, fixed[rng.integers(0, len(fixed), 2 * n)], _rnd(rng, 2 * n, -399, 399))
    ra = np.concatenate([_rnd(rng, n, -1022, 1023), _rnd(rng, n, -60, 60)])
    mid = rng.integers(0, 3, 2 * n) == 0                                        # a quotient next to a rounding boundary
    ra = np.where(mid, rb * (rng.integers(0, 1 << 48, 2 * n).astype(np.float64) + 0.5), ra)
    a, b = np.concatenate([a, ra]), np.concatenate([b, rb])
    keep = _div_const_ok(b) & np.isfinite(a)                                    # a refused divisor is not passed
    a, b = a[keep], b[keep]
    assert _div_const_ok(_col("div", "b")).all() and len(a) > 100000
    with np.errstate(all="ignore"):
        q = a / b
        o = _math(OP_DIV, a, b, 1.0 / b)
    got = o[0].view(np.float64)
    qb = q.view(np.uint64)
    inside = np.isfinite(q) & (np.abs(q) >= 2.0 ** -1022) & (np.abs(a) >= 2.0 ** -968) & (np.abs(q) < 2.0 ** 1020)
    over = np.isinf(q)
    below = np.abs(a) < 2.0 ** -968
    assert inside.sum() > 80000 and over.sum() > 100 and below.sum() > 500
    print(f"DIV: {inside.sum()} quotients inside the window, mismatches with the device's `/` {(o[0] != o[1])[inside].sum()}, with numpy's "
          f"{(o[0] != qb)[inside].sum()}; below the window {below.sum()}, misrounded {(o[0] != qb)[below].sum()}")
    assert np.array_equal(o[0][inside], o[1][inside]) and np.array_equal(o[0][inside], qb[inside])     # zero mismatches
    assert np.array_equal(o[1][inside], qb[inside])
    assert not np.isfinite(got[over]).any()
    assert np.isfinite(got[below]).all()
    e = np.abs(got[below] - q[below])
    small = np.abs(q[below]) < 2.0 ** -970
    assert small.sum() > 200 and (e[small] <= 2.0 ** -1022).all()
    assert (e <= 2.0 * np.spacing(np.abs(q[below]))).all()
    zero = a == 0.0
    assert zero.any() and (got[zero] == 0.0).all()


def _log_extra():
    rng = np.random.default_rng(6)
    k = np.arange(2000, dtype=np.float64)
    return np.concatenate([(k + 1.0) * 2.0 ** -53, 1.0 - k * 2.0 ** -53, 1.0 + k * 2.0 ** -52, 10.0 ** rng.uniform(-3.0, 2.0, 20000)])


def test_fast_log_is_within_one_ulp_of_the_exact_logarithm():
    a, hi, lo = _col("log", "a"), _col("log", "hi"), _col("log", "lo")
    o = _math(OP_LOG, a)
    assert np.array_equal(o[0], o[1])                                           # constants from SGPRs or not: the same bits
    u = np.where(hi == 0.0, np.where(o[0].view(np.float64) == 0.0, 0.0, 1e9), _ulps(o[0].view(np.float64), hi, np.where(hi == 0.0, 0.0, lo)))
    uo = _ulps(o[2].view(np.float64), hi, lo)[hi != 0.0]
    w = int(np.argmax(u))
    print(f"LOG: fg_fast_log worst {u.max():.3f} ulp at {a[w]!r}; ocml log worst {uo.max():.3f} ulp ({len(a)} points)")
    assert u.max() < 1.0
    one = a == 1.0
    assert one.any() and (o[0][one] == 0).all()                                 # fg_fast_log(1.0) == +0
    x = _log_extra()                                                            # 26 000 points more: the two forms, bit for bit
    o = _math(OP_LOG, x)
    assert np.array_equal(o[0], o[1])
    ref = np.log(x)                                                             # a sanity check only: numpy's log is itself within an ulp
    assert (np.abs(o[0].view(np.float64) - ref) <= 3.0 * np.spacing(np.abs(ref))).all()


def test_fast_sincos_is_within_one_ulp_of_the_exact_sine_and_cosine():
    a = _col("sincos", "a")
    o = _math(OP_SINCOS, a)
    assert np.array_equal(o[0], o[2]) and np.array_equal(o[1], o[3])
    for row, name in ((0, "sin"), (1, "cos")):
        hi, lo = _col("sincos", name + "_hi"), _col("sincos", name + "_lo")
        got = o[row].view(np.float64)
        err = MF.err(got, hi, lo)
        big = np.abs(hi) > 1e-8
        u = err[big] / MF.ulp(hi[big])
        print(f"SINCOS: {name} worst {u.max():.3f} ulp where |exact| > 1e-8, worst absolute error {err.max():.3g} ({len(a)} points)")
        assert u.max() < 1.0 and err.max() < 2.3e-16
    rng = np.random.default_rng(8)                                              # 50 000 angles more: the two forms, bit for bit
    x = 2.0 * math.pi * (rng.integers(0, 1 << 53, 50000).astype(np.float64) * 2.0 ** -53)
    o = _math(OP_SINCOS, x)
    assert np.array_equal(o[0], o[2]) and np.array_equal(o[1], o[3])
    assert np.abs(o[0].view(np.float64) - np.sin(x)).max() < 4e-16 and np.abs(o[1].view(np.float64) - np.cos(x)).max() < 4e-16


def test_normal_pair_and_gaussian_z_against_the_exact_box_muller_values():
    """|z - exact| <= 1e-15 r, r = sqrt(-2 ln u1): the logarithm within one ulp, a correctly rounded root, a cosine with absolute error
    <= 2.3e-16 and one product rounding make 5e-16 r; doubled."""
    fx = MF.fixture()
    wa, wb = MF.u64(fx.raw["pair"]["wa"]), MF.u64(fx.raw["pair"]["wb"])
    o = _math(OP_PAIR, wa, wb)
    assert np.array_equal(o[0], o[2]) and np.array_equal(o[1], o[3])
    u1 = ((wa >> np.uint64(11)).astype(np.float64) + 1.0) * 2.0 ** -53
    r = np.sqrt(-2.0 * np.log(u1))
    worst = 0.0
    for row, name in ((0, "z0"), (1, "z1")):
        err = MF.err(o[row].view(np.float64), _col("pair", name + "_hi"), _col("pair", name + "_lo"))
        assert (err <= 1e-15 * r).all(), name
        worst = max(worst, float((err[r > 0] / r[r > 0]).max()))
    g1 = np.maximum((wa >> np.uint64(11)).astype(np.float64) * 2.0 ** -53, 1e-10)
    rg = np.sqrt(-2.0 * np.log(g1))
    err = MF.err(o[4].view(np.float64), _col("pair", "gz_hi"), _col("pair", "gz_lo"))
    print(f"PAIR: normal pair worst |z - exact| / r {worst:.3g}; gaussian_z {float((err / rg).max()):.3g} ({len(wa)} word pairs)")
    assert (err <= 1e-15 * rg).all()
    assert (u1 == 1.0).any() and (u1 == 2.0 ** -53).any()
    rng = np.random.default_rng(9)                                              # 50 000 random word pairs more: the two forms, bit for bit
    xa, xb = rng.integers(0, 1 << 64, 50000, dtype=np.uint64), rng.integers(0, 1 << 64, 50000, dtype=np.uint64)
    o = _math(OP_PAIR, xa, xb)
    assert np.array_equal(o[0], o[2]) and np.array_equal(o[1], o[3])
    z = o[:2].view(np.float64)
    assert np.isfinite(z).all() and np.isfinite(o[4].view(np.float64)).all()


def test_digamma_is_within_1e12_relative_to_max_1_psi():
    a, hi, lo = _col("digamma", "a"), _col("digamma", "hi"), _col("digamma", "lo")
    got = _math(OP_DIGAMMA, a)[0].view(np.float64)
    rel = MF.err(got, hi, lo) / np.maximum(1.0, np.abs(hi))
    w = int(np.argmax(rel))
    print(f"DIGAMMA: worst |err| / max(1, |psi|) {rel.max():.3g} at {a[w]!r} ({len(a)} points)")
    assert rel.max() <= 1e-12


def test_ocml_functions_measured_against_exact_values():
    """Nothing fixed in advance: the worst error of each ocml function the log-densities and samplers call, in ulps of the exact value
    (lgamma: of max(1, |exact|)), at every argument the fixture's cases feed it.  The table is what a log-density case that leaves its
    budget is explained with."""
    raw = MF.fixture().raw["ocml"]
    for row, name in enumerate(("log", "log1p", "lgamma", "exp", "pow", "tan")):
        a, hi, lo = MF.f64(raw[name]["a"]), MF.f64(raw[name]["hi"]), MF.f32(raw[name]["lo"])
        b = MF.f64(raw[name]["b"]) if name == "pow" else np.ones_like(a)
        got = _math(OP_OCML, a, b)[row].view(np.float64)
        unit = MF.ulp(np.maximum(1.0, np.abs(hi))) if name == "lgamma" else MF.ulp(hi)
        exact_zero = hi == 0.0
        u = np.where(exact_zero, np.where(got == 0.0, 0.0, np.inf), MF.err(got, hi, lo) / np.where(exact_zero, 1.0, unit))
        w = int(np.argmax(u))
        arg = f"{a[w]!r}" + (f", {b[w]!r}" if name == "pow" else "")
        print(f"OCML: {name:6s} worst {u.max():.3f} ulp at ({arg}) over {len(a)} arguments")
        assert np.isfinite(got).all() and np.isfinite(u).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# log-densities
# ---------------------------------------------------------------------------------------------------------------------------------
def _report(path, fx, K, idx):
    worst = {}
    for k, name in enumerate(fx.families):
        sel = fx.fam[idx] == k
        if sel.any():
            worst[name] = float(K[sel].max())
    print(f"K {path}: " + ", ".join(f"{n} {v:.2f}" for n, v in worst.items()))
    return worst


def _assert_within_cap(path, fx, got, idx):
    idx = np.asarray(idx)
    got = np.asarray(got, dtype=np.float64)
    assert np.isfinite(got).all(), (path, [(fx.family_name(i), fx.params(i), fx.value(i)) for i in idx[~np.isfinite(got)][:5]])
    K = fx.K(got, idx)
    _report(path, fx, K, idx)
    bad = np.nonzero(K > K_CAP)[0]
    assert len(bad) == 0, (path, len(bad), [(fx.family_name(idx[j]), fx.params(idx[j]), fx.value(idx[j]), float(got[j]), float(K[j])) for j in bad[:8]])


def _cell(value, is_int):
    return int(value) if is_int else int(np.array([float(value)], dtype=np.float64).view(np.int64)[0])


def test_site_fed_densities_in_the_interpreter_and_the_stream_records():
    """One program, one statement per family whose parameters and value are all sample sites; chain c holds case c of every family, so one
    engine and one launch of each kernel cover the fixture (the non-hoisted arm of fg_logpdf; FG_G_GEN records with slot operands)."""
    fx = MF.fixture()
    P = M.Program()
    by_family, p_handles, v_handles, v_stmt = [], [], [], []
    for k, name in enumerate(fx.families):
        by_family.append(np.nonzero(fx.fam == k)[0])
        ps = [P.sample(M.addr(f"p{j}", k), M.Normal(0.0, 1.0)) for j in range(MF.NPARAMS[name])]
        p_handles.append([e.a for e in ps])
        v_stmt.append(len(P.stmts))
        v_handles.append(P.sample(M.addr("v", k), M.Dist(name, ps)).a)
    cp = E.compile_model(P)
    n_chains = max(len(ix) for ix in by_family)
    n_chains += 1 if n_chains % 64 == 0 else 0
    assert n_chains % 64 != 0 and n_chains > 64
    cells = np.zeros((cp.S, n_chains), dtype=np.int64)
    for k, name in enumerate(fx.families):
        ix = by_family[k]
        jv = cp.site_of_handle(v_handles[k])
        assert (cp.site_vtypes[jv] != 0) == (name in MF.INT_FAMILIES)
        for c in range(n_chains):
            i = ix[c % len(ix)]
            cells[jv, c] = _cell(fx.value(i), name in MF.INT_FAMILIES)
            for h, p in zip(p_handles[k], fx.params(i)):
                cells[cp.site_of_handle(h), c] = _cell(p, False)
    eng = E.Engine(cp, n_chains, seed=1)
    eng.set_values(cells)
    _, logp = eng.log_joint(want_logp=True)
    assert cp.stream_records[1] == len(P.stmts), cp.stream_records
    _, rec = eng.log_joint_stream(want_records=True)
    assert np.array_equal(eng.get_values(), cells)
    eng.close()
    idx = np.concatenate(by_family)
    interp = np.concatenate([logp[cp.site_of_handle(v_handles[k])][:len(ix)] for k, ix in enumerate(by_family)])
    stream = np.concatenate([rec[v_stmt[k]][:len(ix)] for k, ix in enumerate(by_family)])
    assert len(idx) == fx.n
    _assert_within_cap("site / interpreter", fx, interp, idx)
    _assert_within_cap("site / stream", fx, stream, idx)


def _const_subset(fx):
    """every case next to a zero of lgamma, and 20 of the wide cases of every family"""
    idx = [i for i in range(fx.n) if fx.tag[i] == "z"]
    for k in range(len(fx.families)):
        idx += [i for i in np.nonzero(fx.fam == k)[0] if fx.tag[i] == "r"][:20]
    return sorted(idx)


def test_constant_parameter_densities_in_the_interpreter_and_the_stream_records():
    """Batches of 96 statements with literal parameters: fg_hoist's constants (evaluated by the host's libm), FG_F_RCPSCALE / the
    power-of-two scale, FG_OP_NORMAL_FAST, and the hoisted score-stream records (every family but Binomial has one)."""
    fx = MF.fixture()
    idx = _const_subset(fx)
    assert len(idx) >= 300
    got_i, got_s, idx_s = {}, [], []
    for want_stream in (True, False):
        sel = [i for i in idx if TG._streamable(fx.family_name(i), fx.params(i), "const") == want_stream]
        for s in range(0, len(sel), 96):
            part = sel[s:s + 96]
            interp, stream = TG._run_batch([(fx.family_name(i), fx.params(i), fx.value(i)) for i in part], "const", want_stream)
            for j, i in enumerate(part):
                got_i[i] = interp[j]
                if stream is not None:
                    got_s.append(stream[j]); idx_s.append(i)
    assert len(got_i) == len(idx) and len(idx_s) >= len(idx) - 40
    _assert_within_cap("const / interpreter", fx, [got_i[i] for i in idx], idx)
    _assert_within_cap("const / stream", fx, got_s, idx_s)


def test_normal_fast_edges_give_their_literal_results():
    """FG_OP_NORMAL_FAST with a constant sigma that is no power of two (fg_div_const): x - mu = 1e308 makes the quotient's sequence
    NaN, which must score -inf; x - mu = 1e-300 makes z^2 underflow, which must leave -ln sigma - ln(2 pi) / 2 exactly."""
    edges = MF.fixture().raw["normal_fast_edges"]
    interp, stream = TG._run_batch([("Normal", [e["mu"], e["sigma"]], e["x"]) for e in edges], "const", True)
    for e, a, b in zip(edges, interp, stream):
        for got in (a, b):
            if e["expected"] == "-inf":
                assert got == -math.inf, (e, got)
            else:
                assert int(np.array([got]).view(np.uint64)[0]) == int(e["expected"], 16), (e, got)


def _dd_sum(parts):
    s = math.fsum(parts)
    return s, math.fsum(list(parts) + [-s])


def test_densities_in_the_unit_compiled_at_run_time(monkeypatch):
    """`log_joint_compiled` returns sums: one program with one observe per family, parameters and observed value from sites.  Chain c gives
    case c to its family and a benign case (the family's smallest budget) to the twelve others; acc[likelihood] is compared with the exact
    sum under the summed budget.  The call launches the compiled unit or fails -- with FG_JIT=0 it must fail."""
    fx = MF.fixture()
    P = M.Program()
    handles = []
    for k, name in enumerate(fx.families):
        ps = [P.sample(M.addr(f"p{j}", k), M.Normal(0.0, 1.0)) for j in range(MF.NPARAMS[name])]
        v = P.sample(M.addr("v", k), M.Normal(0.0, 1.0))
        P.observe(M.addr("o", k), M.Dist(name, ps), v)
        handles.append([e.a for e in ps] + [v.a])
    cp = E.compile_model(P)
    benign = []
    for k in range(len(fx.families)):
        ix = np.nonzero((fx.fam == k) & (np.array(list(fx.tag)) == "r"))[0]
        benign.append(int(ix[np.argmin(fx.budget[ix])]))
    n_chains = fx.n + (1 if fx.n % 64 == 0 else 0)
    assert n_chains % 64 != 0
    cells = np.zeros((cp.S, n_chains), dtype=np.int64)
    hi, lo, budget = np.zeros(n_chains), np.zeros(n_chains), np.zeros(n_chains)
    for c in range(n_chains):
        wild = c % fx.n
        use = [wild if fx.fam[wild] == k else benign[k] for k in range(len(fx.families))]
        for k, i in enumerate(use):
            for h, p in zip(handles[k], fx.params(i) + [float(fx.value(i))]):
                cells[cp.site_of_handle(h), c] = _cell(p, False)
        hi[c], lo[c] = _dd_sum([float(fx.hi[i]) for i in use] + [float(fx.lo[i]) for i in use])
        budget[c] = float(fx.budget[use].sum())
    monkeypatch.setenv("FG_JIT", "0")
    eng = E.Engine(cp, n_chains, seed=1)
    with pytest.raises(E.EngineError):
        eng.log_joint_compiled()
    eng.close()
    monkeypatch.setenv("FG_JIT", "1")
    eng = E.Engine(cp, n_chains, seed=1)
    eng.set_values(cells)
    acc = eng.log_joint_compiled()                      # raises where no compiled unit ran
    eng.close()
    lik = acc[1]
    assert np.isfinite(lik).all() and (acc[2] == 0.0).all()
    K = MF.err(lik, hi, lo) / (MF.EPS * budget)
    wild = np.arange(n_chains) % fx.n
    _report("site / compiled unit (sums of 13)", fx, K, wild)
    bad = np.nonzero(K > K_CAP)[0]
    assert len(bad) == 0, (len(bad), [(fx.family_name(wild[j]), fx.params(wild[j]), fx.value(wild[j]), float(lik[j]), float(K[j])) for j in bad[:8]])
