"""MCSE / ESS of the mean, the sd and quantiles without a GPU: the rule of fugue_amd/csrc/fg_diag_mcse_plan.h through the
stand-alone tests/cpp/mcse_driver.cpp (built a second time with AddressSanitizer / UBSan and run directly) against
tests/mcse_restatement.py; the Beta inverse against mpmath at 50 digits (scipy as a second opinion); the positions against positions
computed from the mpmath values; the law of the reported errors over seeds; the argument codes; the ABI; the Python layer.  Every
compared figure is printed before it is asserted."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import abi_check
from tests import mcse_restatement as M
from tests import rank_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FG_E_BAD_ARG = -3
NEW = ["fg_diag_mcse_words", "fg_mcse_quantile_ranks", "fg_diag_mcse_transform", "fg_diag_mcse"]
SIZES = ((1, 1), (2, 2), (21, 3), (777, 7), (9000, 8))             # (S, chains): 9 000 is three radix tiles
PROBS3 = (0.05, 0.5, 0.95)
PROBS8 = (0.0, 0.01, 0.25, 0.5, 0.5000001, 0.75, 0.99, 1.0)


def _build(out_dir, name, extra=()):
    assert shutil.which("g++"), "g++ builds the driver"
    exe = os.path.join(str(out_dir), name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", *extra, os.path.join(ROOT, "tests", "cpp", "mcse_driver.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("mcse"), "mcse_driver")


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("mcse_san"), "mcse_driver_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-3000:])
    return r


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


@pytest.fixture(scope="module")
def beta_grid():
    """the issue's grid: (ess, p, y) -> alpha, beta and mpmath's inverse at 50 digits, computed once"""
    import mpmath as mp
    mp.mp.dps = 50
    out = []
    for ess in M.BETA_ESS:
        for p in M.BETA_P:
            a, b = ess * p + 1.0, ess * (1.0 - p) + 1.0
            for y in (M.Y_LO, M.Y_HI):
                out.append(dict(ess=ess, p=p, y=y, a=a, b=b, truth=M.mp_betaincinv(a, b, y, M.betaincinv(a, b, y))))
    return out


def test_beta_inverse_against_mpmath(driver, beta_grid):
    """fg_mcse_betaincinv over ess in {0.7, 9.3, 211.7, 3 100.2, 80 000.5, 2.1e9} x p in {0, 0.05, 0.5, 0.95, 1} x both levels against
    mpmath at 50 digits (mpmath's betainc, and where both parameters are large the integral of the density in mpmath: mcse_restatement.
    mp_betainc), the root refined by Newton steps in mpmath.

    Measured: the rule in C++ deviates by at most 2.25e-15 relative (alpha = 1, beta = 212.7, the upper level); the restatement's port
    by the same; scipy.special.betaincinv by at most 1.39e-12 (alpha = 1.05e8, beta = 1.995e9).  The tolerance is four times the
    measurement: mcse_restatement.BETA_TOL = 9.2e-15."""
    import mpmath as mp
    from scipy.special import betaincinv as sp_inv
    mp.mp.dps = 50
    r = _run(driver, ["beta"] + [repr(v) for g in beta_grid for v in (g["a"], g["b"], g["y"])])
    lines = [l for l in r.stdout.splitlines() if l.startswith("beta | ")]
    assert r.returncode == 0 and len(lines) == len(beta_grid) == 60
    worst = dict(driver=0.0, restatement=0.0, scipy=0.0)
    for g, line in zip(beta_grid, lines):
        got = dict(driver=float(line.split("|")[1]), restatement=M.betaincinv(g["a"], g["b"], g["y"]), scipy=float(sp_inv(g["a"], g["b"], g["y"])))
        dev = {k: float(abs(mp.mpf(v) - g["truth"]) / g["truth"]) for k, v in got.items()}
        print(f"ess {g['ess']:g} p {g['p']:g} y {g['y']:.4f}: x {got['driver']!r}; relative deviation from mpmath: " + ", ".join(f"{k} {v:.3e}" for k, v in dev.items()))
        for k in worst:
            worst[k] = max(worst[k], dev[k])
        assert 0.0 < got["driver"] < 1.0
    print("largest:", worst, "measured", M.BETA_MEASURED_DEV, "tolerance", M.BETA_TOL)
    assert worst["driver"] <= M.BETA_TOL and worst["restatement"] <= M.BETA_TOL


def test_quantile_positions_against_mpmath(driver, beta_grid):
    """fg_mcse_quantile_ranks (the library's entry and the rule through the driver) over the same grid x S in {1, 21, 600, 12 707,
    309 300, 2^31 - 1} against i_lo = max(floor(a1 S), 1) - 1, i_hi = min(ceil(a2 S), S) - 1 evaluated in mpmath on mpmath's a1, a2:
    equal as integers.  A grid point is left out only where mpmath's a S lies within S x BETA_TOL of an integer (there a deviation the
    Beta test allows could move the floor or the ceiling); the grid is chosen so that this never happens: checked here on the mpmath
    values alone, at most 1 % may be left out.  Measured: none is left out; the nearest approach of a S to an integer is 680 times that margin."""
    import mpmath as mp
    from fugue_amd import engine as E
    mp.mp.dps = 50
    by = {(g["ess"], g["p"], g["y"]): g["truth"] for g in beta_grid}
    cases, left_out, nearest = [], 0, float("inf")
    for S in M.RANK_S:
        for ess in M.BETA_ESS:
            for p in M.BETA_P:
                a1, a2 = by[(ess, p, M.Y_LO)] * S, by[(ess, p, M.Y_HI)] * S
                margin = min(abs(v - mp.nint(v)) for v in (a1, a2))
                if margin <= S * M.BETA_TOL:
                    left_out += 1
                    continue
                nearest = min(nearest, float(margin / (S * M.BETA_TOL)))
                cases.append((S, p, ess, max(int(mp.floor(a1)), 1) - 1, min(int(mp.ceil(a2)), S) - 1))
    total = len(M.RANK_S) * len(M.BETA_ESS) * len(M.BETA_P)
    print(f"{total} grid points, {left_out} left out; the nearest approach of a S to an integer among the kept is {nearest:.4g} times the margin S x BETA_TOL")
    assert total == 180 and left_out <= total // 100
    r = _run(driver, ["ranks"] + [repr(v) for c in cases for v in c[:3]])
    lines = [l for l in r.stdout.splitlines() if l.startswith("ranks | ")]
    assert r.returncode == 0 and len(lines) == len(cases)
    for (S, p, ess, lo, hi), line in zip(cases, lines):
        got = [int(v) for v in line.split("|")[1].split()]
        lib = E.mcse_quantile_ranks(S, p, ess)
        if got != [0, lo, hi] or lib != (lo, hi):
            print(f"S {S} p {p} ess {ess}: driver {got}, library {lib}, mpmath {(lo, hi)}")
        assert got == [0, lo, hi] and lib == (lo, hi), (S, p, ess)
        assert 0 <= lo <= hi < S
        assert M.quantile_ranks(S, p, ess) == (lo, hi), (S, p, ess)


def _law(make, K, S_chains=(1000, 4)):
    n, C = S_chains
    rep = {k: [] for k in ("mcse_mean", "mcse_sd", "mcse_quantile")}
    est = {k: [] for k in ("mean", "sd", "quantile")}
    for seed in range(K):
        f = M.law_figures(make(np.random.default_rng(10_000 + seed), n, C))
        for k in rep:
            rep[k].append(f[k])
        for k in est:
            est[k].append(f[k])
    return {k: np.array(v) for k, v in rep.items()}, {k: np.array(v) for k, v in est.items()}


def test_law_of_the_reported_errors():
    """The restatement alone, 200 seeds of S = 4 000 draws in 4 chains.  What a reported standard error claims is the seed-to-seed
    standard deviation of its estimate.  The yardstick: the standard deviation s of K estimates has the standard error s / sqrt(2 (K - 1))
    (normal estimates), the average of K reported errors the standard error sd(reported) / sqrt(K); the two are independent enough to add
    in quadrature, and the average reported error must lie within four of that of s.

    iid N(0, 1): mcse_mean against the seeds' sd of the mean, mcse_sd against that of the sd, mcse_quantile(0.5) against that of the
    median.  AR(1) with phi = 0.7 and unit innovations (started in the stationary law): mcse_mean against the analytic
    sd sqrt((1 + phi) / ((1 - phi) S)), sd = 1 / sqrt(1 - phi^2), with the same yardstick (the standard error a seed-to-seed estimate of
    that value would have), and against the seeds' own value.

    Measured (K = 200): iid mean 0.01607 reported / 0.01559 seen, sd 0.01135 / 0.01182, median 0.02015 / 0.01934, each less than one
    standard error apart; AR(1) mean 0.05313 reported / 0.05270 analytic / 0.05203 seen."""
    K = 200
    rep, est = _law(lambda rng, n, C: rng.normal(size=(n, C)), K)
    misses = []
    for r_name, e_name in (("mcse_mean", "mean"), ("mcse_sd", "sd"), ("mcse_quantile", "quantile")):
        seen, told = float(est[e_name].std(ddof=1)), float(rep[r_name].mean())
        se = math.hypot(seen / math.sqrt(2.0 * (K - 1)), float(rep[r_name].std(ddof=1)) / math.sqrt(K))
        print(f"iid {r_name}: reported on average {told:.5f}, the seeds' sd of the {e_name} {seen:.5f}, standard error {se:.5f}: {abs(told - seen) / se:.2f} of them apart")
        if not abs(told - seen) <= 4.0 * se:
            misses.append((r_name, told, seen, se))
    phi = 0.7

    def ar1(rng, n, C):
        e = rng.normal(size=(n, C))
        x = np.empty((n, C))
        x[0] = e[0] / math.sqrt(1.0 - phi * phi)
        for t in range(1, n):
            x[t] = phi * x[t - 1] + e[t]
        return x

    rep, est = _law(ar1, K)
    S = 4000
    analytic = (1.0 / math.sqrt(1.0 - phi * phi)) * math.sqrt((1.0 + phi) / ((1.0 - phi) * S))
    seen, told = float(est["mean"].std(ddof=1)), float(rep["mcse_mean"].mean())
    se_rep = float(rep["mcse_mean"].std(ddof=1)) / math.sqrt(K)
    for label, target in (("analytic", analytic), ("seen", seen)):
        se = math.hypot(target / math.sqrt(2.0 * (K - 1)), se_rep)
        print(f"AR(1) mcse_mean: reported on average {told:.5f}, {label} {target:.5f}, standard error {se:.5f}: {abs(told - target) / se:.2f} of them apart")
        if not abs(told - target) <= 4.0 * se:
            misses.append(("ar1 " + label, told, target, se))
    assert not misses, misses


def _params(t, probs):
    """the parameter file of the driver's `coord` from a restatement's coordinate: the combination's figures as the oracle gave them"""
    comb = [M.combination(t["rows"][:, i, :]) for i in range(t["rows"].shape[1])]
    raw = t["raw"]
    return np.array([len(probs), *probs, raw["mean"], raw["std"], raw["rhat"], raw["ess"], *[c["ess"] for c in comb], *[c["mean"] for c in comb], *[c["std"] for c in comb]], dtype=np.float64)


def _coordinate_with_raw(x, C, probs):
    n = x.size // C
    draws = np.ascontiguousarray(x.reshape(n, 1, C))
    t = M.coordinate(draws, 0, probs)
    t["raw"] = M.combination(draws[:, 0, :])
    return t


def _driver_coord(exe, tmp, x, t, probs):
    src, par, dst = (os.path.join(str(tmp), f) for f in ("x.f64", "par.f64", "out.f64"))
    np.ascontiguousarray(x, dtype=np.float64).tofile(src)
    _params(t, probs).tofile(par)
    r = _run(exe, ["coord", src, par, dst])
    assert r.returncode == 0 and r.stdout.strip().endswith("| ok"), r.stdout
    o, S, Rw = np.fromfile(dst, dtype=np.float64), x.size, 2 + len(probs)
    nw = 10 + 6 * len(probs)
    return dict(rows=o[:Rw * S].reshape(Rw, S), sorted=o[Rw * S:Rw * S + S], words=o[Rw * S + S:Rw * S + S + nw], counts=o[Rw * S + S + nw:].astype(np.int64))


def _compare(got, x, C, t, probs, label):
    n = x.size // C
    want_rows = t["rows"].transpose(1, 0, 2).reshape(2 + len(probs), -1)
    assert _bits_equal(got["rows"], want_rows), (label, "rows")
    assert _bits_equal(got["sorted"], M.sorted_values(t["stats"])), (label, "sorted")
    fixed = [t["words"][k] for k in M.WORD_NAMES]
    per = [t["prob_words"][k][i] for i in range(len(probs)) for k in M.PROB_WORD_NAMES]
    print(f"{label}: words {got['words'].tolist()} / {fixed + per}")
    assert _bits_equal(got["words"], np.array(fixed + per, dtype=np.float64)), (label, "words")
    want_counts = [t["counts"][k] for k in M.COUNT_NAMES[:5]] + [0] + [t["prob_counts"][k][i] for i in range(len(probs)) for k in M.PROB_COUNT_NAMES]
    print(f"{label}: counts {got['counts'].tolist()} / {want_counts}")
    assert got["counts"].tolist() == want_counts, (label, "counts")
    assert n * C == x.size


@pytest.mark.parametrize("S,C", SIZES)
def test_driver_and_restatement_agree_on_every_input(driver, tmp_path, S, C):
    """rows, sorted cells, every word (order statistics, q7, the formulas on the combination's figures handed to both) and every count
    (positions included) bit-equal, on normal, Cauchy, tied, constant, signed-zero / denormal, +-inf and NaN columns"""
    for name, x in R.inputs(S, seed=5 * S + 2).items():
        for probs in (PROBS3, PROBS8):
            t = _coordinate_with_raw(x, C, probs)
            _compare(_driver_coord(driver, tmp_path, x, t, probs), x, C, t, probs, f"S = {S} {name} {len(probs)} probabilities")
            if name == "nans":
                assert t["counts"]["n_nan"] > 0 and all(math.isnan(v) for v in t["words"].values())
            if name == "constant":
                assert t["words"]["mad"] == 0.0 and t["words"]["median"] == -2.75 and all(v == -2.75 for v in t["prob_words"]["q7"])


def test_driver_under_address_and_ub_sanitizers(driver_san, tmp_path):
    """the stand-alone program itself runs under the sanitizers: no Python process does"""
    for S, C in ((1, 1), (2, 1), (4100, 4)):
        for name, x in R.inputs(S, seed=S).items():
            t = _coordinate_with_raw(x, C, PROBS8)
            _compare(_driver_coord(driver_san, tmp_path, x, t, PROBS8), x, C, t, PROBS8, f"sanitized S = {S} {name}")
    assert _run(driver_san, ["refusals"]).returncode == 0
    x = np.r_[np.full(40, np.inf), np.arange(30.0)]                  # more than half the cells +inf: the median is +inf, the folded cells there NaN
    t = _coordinate_with_raw(x, 2, PROBS3)
    _compare(_driver_coord(driver_san, tmp_path, x, t, PROBS3), x, 2, t, PROBS3, "median +inf")
    assert t["words"]["median"] == np.inf and math.isnan(t["words"]["mad"]) and t["counts"]["n_nan_folded"] == 40 and t["counts"]["n_nan"] == 0
    r = _run(driver_san, ["beta"] + [repr(v) for ess in M.BETA_ESS for p in M.BETA_P for v in (ess * p + 1.0, ess * (1.0 - p) + 1.0, M.Y_HI)])
    assert r.returncode == 0 and r.stdout.count("beta | ") == 30


def test_plan_and_refusals(driver):
    assert _run(driver, ["refusals"]).returncode == 0
    shapes = [(1, 1, 1, 0, 1, 1, 0), (7, 3, 2, 1, 1, 3, 0), (61, 200, 3, 0, 3, 3, 0), (300, 1031, 1, 0, 1, 8, 0), (1000, 65536, 4, 0, 4, 3, 0), (200, 8192, 64, 3, 61, 3, 1 << 28),
              (4, 4, 65535, 0, 65535, 8, 0)]
    r = _run(driver, ["plan"] + [v for s in shapes for v in s])
    lines = [l for l in r.stdout.splitlines() if l.startswith("plan ")]
    assert r.returncode == 0 and len(lines) == len(shapes) and all(l.endswith("| ok") for l in lines)
    for (n, C, d, j0, nj, npb, mob), line in zip(shapes, lines):
        got = [int(v) for v in line.split("|")[1].split()]
        S, rows = n * C, 2 + npb
        budget = mob if mob > 0 else 1 << 30
        assert got == [0, S, rows, 10 + 6 * npb, 6 + 3 * npb, max(1, min(d, 65535 // rows, budget // (8 * S * (rows + 1))))], line


def test_argument_codes_need_no_device():
    """every argument is checked before the engine and the device are looked at; FG_E_LIMIT needs the engine's chain count and is
    checked where it is decided, in fg_mcse_plan through the driver (test_plan_and_refusals)"""
    from fugue_amd import engine as E
    import ctypes as C
    L = E.lib()
    assert [L.fg_diag_mcse_words(k) for k in (1, 3, 8)] == [16, 28, 58] and L.fg_diag_mcse_words(0) == FG_E_BAD_ARG and L.fg_diag_mcse_words(9) == FG_E_BAD_ARG
    assert tuple(E.MCSE_WORD_NAMES) == M.WORD_NAMES and tuple(E.MCSE_PROB_WORD_NAMES) == M.PROB_WORD_NAMES
    assert tuple(E.MCSE_COUNT_NAMES) == M.COUNT_NAMES and tuple(E.MCSE_PROB_COUNT_NAMES) == M.PROB_COUNT_NAMES and E.MCSE_MAX_PROBS == 8
    words, one, counts, pr = np.zeros(28), np.zeros(1), np.zeros(15, dtype=np.int64), np.array(PROBS3)
    cp, dp = counts.ctypes.data_as(C.POINTER(C.c_int64)), E._dp
    bad = lambda *v: dp(np.array(v, dtype=np.float64))
    fig = lambda draws=8, n=4, d=1, p=dp(pr), k=3, mob=0, w=dp(words), c=cp: L.fg_diag_mcse(None, draws, n, d, p, k, mob, w, c)
    tr = lambda draws=8, n=4, d=2, j0=0, nj=1, m=dp(one), p=dp(pr), k=3, out=8, med=dp(one), mad=dp(one), c=cp: L.fg_diag_mcse_transform(None, draws, n, d, j0, nj, m, p, k, out, None, med, mad, c)
    cases = [fig(), fig(draws=None), fig(p=None), fig(w=None), fig(c=None), fig(n=0), fig(d=0), fig(d=65536), fig(k=0), fig(k=9), fig(p=bad(0.5, -0.1, 0.9)), fig(p=bad(0.5, 1.5, 0.9)),
             fig(p=bad(float("nan"), 0.5, 0.9)), fig(mob=-1), tr(), tr(out=None), tr(m=None), tr(p=None), tr(med=None), tr(mad=None), tr(c=None), tr(n=-3), tr(d=0), tr(j0=2), tr(j0=-1),
             tr(nj=0), tr(j0=1, nj=2), tr(k=0), tr(k=9), tr(p=bad(2.0, 0.5, 0.9))]
    assert cases == [FG_E_BAD_ARG] * len(cases), cases
    for call, word in ((lambda: fig(n=0), "n must"), (lambda: tr(j0=2), "block"), (lambda: fig(), "null engine"), (lambda: fig(k=9), "n_probs"), (lambda: fig(p=bad(0.5, 1.5, 0.9)), "probabilities"),
                       (lambda: fig(mob=-1), "max_out_bytes"), (lambda: fig(d=65536), "d outside")):
        assert call() == FG_E_BAD_ARG and word in E.last_error(), (word, E.last_error())
    lo, hi = C.c_int64(), C.c_int64()
    ranks = lambda S=10, p=0.5, ess=10.0, a=C.byref(lo), b=C.byref(hi): L.fg_mcse_quantile_ranks(S, p, ess, a, b)
    assert [ranks(S=0), ranks(p=-0.1), ranks(p=1.1), ranks(ess=0.0), ranks(ess=-1.0), ranks(ess=float("nan")), ranks(ess=float("inf")), ranks(a=None), ranks(b=None)] == [FG_E_BAD_ARG] * 9
    assert ranks() == 0 and 0 <= lo.value <= hi.value < 10
    with pytest.raises(E.EngineError):
        E.mcse_quantile_ranks(10, 0.5, float("nan"))


def test_abi_check_passes_with_the_new_entries():
    from fugue_amd import engine as E
    header = open(os.path.join(ROOT, "include", "fugue_amd.h")).read()
    rust = open(os.path.join(ROOT, "rust", "fugue-gpu", "src", "ffi.rs")).read()
    H, Rs = abi_check.parse_header(header), abi_check.parse_rust(rust)
    for f in NEW:
        assert f in H["fns"] and f in Rs["fns"] and f in E.ABI_SYMBOLS, f
    assert abi_check.compare_header_rust(header, rust) == []
    assert abi_check.compare_header_ctypes(header, E.lib()) == []
    for line in ("#define FG_MCSE_MAX_PROBS 8", "#define FG_MCSE_FIXED_WORDS 10", "#define FG_MCSE_PROB_WORDS 6", "#define FG_MCSE_FIXED_COUNTS 6", "#define FG_MCSE_PROB_COUNTS 3"):
        assert line in header, line


def test_python_layer_without_a_device():
    import fugue_amd as F
    from fugue_amd import diagnostics as D
    z, zp = np.zeros(2), np.zeros((2, 3))
    mq = np.array([[0.1, 0.2, 0.3], [0.4, 0.5, 0.6]])
    md = D.McseDiagnostics(names=["a", "b"], n_draws=100, probs=np.array(PROBS3), mean=np.array([1.0, 2.0]), sd=z, rhat=z, ess_mean=z, mcse_mean=z, ess_sd=z, ess_sq=z, mcse_sd=z,
                           median=z, mad=z, q=zp, q7=zp, ess_quantile=zp, mcse_quantile=mq, th_lo=zp, th_hi=zp,
                           counts={k: np.zeros(2, dtype=np.int64) for k in M.COUNT_NAMES + M.PROB_COUNT_NAMES})
    assert md.d == 2 and md.of("b")["mean"] == 2.0 and set(md.of("a")) == set(M.WORD_NAMES + M.PROB_WORD_NAMES) and md.of("b")["mcse_quantile"].tolist() == [0.4, 0.5, 0.6]
    assert md.at("mcse_quantile", 0.5).tolist() == [0.2, 0.5]
    for name in ("McseDiagnostics", "mcse_diagnostics", "mcse_mean", "mcse_sd", "mcse_quantile", "mcse_median", "ess_mean", "ess_sd", "ess_quantile", "ess_median", "mad", "summarise_draws"):
        assert getattr(F, name) is getattr(D, name), name
    assert D.SUMMARY_COLUMNS == ("mean", "median", "sd", "mad", "q5", "q95", "rhat", "ess_bulk", "ess_tail", "mcse_mean", "mcse_sd", "mcse_q5", "mcse_median", "mcse_q95")
    with pytest.raises(ValueError, match=r"\[n\]\[d\]\[C\]"):
        D.mcse_diagnostics(np.zeros((3, 4)))
    with pytest.raises(KeyError):
        md.of("c")
    with pytest.raises(KeyError):
        md.at("mcse_quantile", 0.3)
