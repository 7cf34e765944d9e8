"""The summary of a weighted population without a GPU: tests/cpp/wpop_driver.cpp (fg_wpop_plan.h's units, pools, selection step and
read-outs, with host loops for the kernels) against the Python restatement, bit for bit, and under AddressSanitizer / UBSan (a
stand-alone binary); the restatement against independent definitions (a brute-force sort, collections.Counter, the exact weighted mean in
Fractions, mpmath) within derived bounds; the integrity check of the selection; every argument limit; the ABI of the new entry points; SMCResult.weighted_mean.  Every compared figure is
printed before it is asserted."""
import math
import os
from fractions import Fraction
import shutil
import subprocess

import numpy as np
import pytest

from tests import abi_check
from tests import wpop_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FG_E_BAD_ARG, FG_E_STATE = -3, -5
F64, BOOL, U64, USIZE, I64 = range(5)
EPS = 2.0 ** -52
NS = (1, 2, 3, 64, 65, 257, 600)
NEW = ["fg_wpop_new", "fg_wpop_units", "fg_wpop_moments", "fg_wpop_quantiles", "fg_wpop_counts", "fg_wpop_free"]


def _build(out_dir, name, extra=()):
    assert shutil.which("g++"), "g++ builds the driver"
    exe = os.path.join(str(out_dir), name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", *extra, os.path.join(ROOT, "tests", "cpp", "wpop_driver.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("wpop"), "wpop_driver")


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("wpop_san"), "wpop_driver_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _csv(v):
    return ",".join(repr(float(a)) if isinstance(a, float) else str(int(a)) for a in v)


def driver_args(work_dir, x, w, probs, digit_bits, capacity, tables=None):
    d, N = x.shape
    px, pw = os.path.join(str(work_dir), "x.f64"), os.path.join(str(work_dir), "w.f64")
    np.ascontiguousarray(x, dtype=np.float64).tofile(px)
    np.ascontiguousarray(w, dtype=np.float64).tofile(pw)
    args = [str(N), str(d), px, pw, _csv([float(p) for p in probs]), str(digit_bits), str(capacity)]
    if tables is not None:
        cells, vt, lo, bins = tables
        pc = os.path.join(str(work_dir), "cells.u64")
        np.ascontiguousarray(cells, dtype=np.uint64).tofile(pc)
        args += [str(len(vt)), pc, _csv(vt), _csv(lo), _csv(bins)]
    return args


def run_driver(exe, args, env=None):
    """-> dict(units, q, moments [d][6] bits, quant [d][np] bits, passes, table) or (rc, message)"""
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=None if env is None else dict(os.environ, **env))
    if r.returncode == 2:
        _, rc, msg = r.stdout.strip().splitlines()[-1].split(" ", 2)            # an error of the selection comes after the units and moments
        return int(rc), msg
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = dict(moments={}, quant={}, passes={}, table={})
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "units":
            out["units"] = tuple(int(v) for v in w[1:])
        elif w[0] == "q":
            out["q"] = [int(v, 16) for v in w[1:]]
        elif w[0] in ("moments", "quant"):
            out[w[0]][int(w[1])] = [int(v, 16) for v in w[2:]]
        elif w[0] == "passes":
            out["passes"][int(w[1])] = [int(v) for v in w[2:]]
        elif w[0] == "table":
            out["table"][int(w[1])] = dict(below=int(w[2]), above=int(w[3]), min=int(w[4]), max=int(w[5]), units=[int(v) for v in w[6:]])
    return out


def table_rows(N, seed=0):
    """one row per value type, with cells outside the bins: (typed values [4][N] as Python ints, vtypes, lo, bins)"""
    rng = np.random.default_rng(3000 + seed)
    vals = [[int(v) for v in rng.integers(0, 2, N)],
            [int(v) for v in rng.integers(0, 12, N)],
            [int(v) for v in rng.integers(2, 9, N)],
            [int(v) for v in rng.integers(-6, 7, N)]]
    vals[1][0] = 2 ** 63 + 5                     # a u64 above the signed range: `above`, and the largest cell
    return vals, [BOOL, U64, USIZE, I64], [0, 1, 2, -4], [2, 8, 9, 4096]


def check_driver(exe, tmp_path, kinds, wkind, N, plan, label, seed=0):
    x = R.rows(kinds, N, seed)
    if wkind == "bad":
        w, n_bad = R.bad_weights(N, seed)
    else:
        w, n_bad = R.weights(wkind, N, seed), 0
    vals, vt, lo, bins = table_rows(N, seed)
    cells = np.stack([R.encode(v, t == U64) for v, t in zip(vals, vt)])
    got = run_driver(exe, driver_args(tmp_path, x, w, R.PROBS, plan[0], plan[1], (cells, vt, lo, bins)))
    q, T, nb, nz = R.units(w)
    print(f"{label}: units {got['units']} / {(T, nb, nz)}; q equal {got['q'] == [int(v) for v in q]}")
    assert got["units"] == (T, nb, nz) and nb == n_bad
    assert got["q"] == [int(v) for v in q]
    for k, kind in enumerate(kinds):
        m = R.moments(x[k], w)
        qv, qp = R.quantiles(x[k], q, T, R.PROBS, *plan)
        print(f"  {kind}: moments {[f'{v:.6g}' for v in m]} equal {got['moments'][k] == [R.bits(v) for v in m]}; quantiles {[f'{v:.6g}' for v in qv]} equal "
              f"{got['quant'][k] == [R.bits(v) for v in qv]}; passes {got['passes'][k]} / {qp}")
        assert got["moments"][k] == [R.bits(v) for v in m]
        assert got["quant"][k] == [R.bits(v) for v in qv]
        assert got["passes"][k] == qp
    for k in range(len(vt)):
        t = R.table(vals[k], q, T, lo[k], bins[k])
        want = dict(t, min=0 if t["min"] is None else t["min"], max=0 if t["max"] is None else t["max"])
        g = dict(got["table"][k])
        if vt[k] == U64:
            g["min"], g["max"] = g["min"] & (2 ** 64 - 1), g["max"] & (2 ** 64 - 1)
        print(f"  table {k}: below {g['below']} above {g['above']} min {g['min']} max {g['max']} equal {g == want}")
        assert g == want
    return got


@pytest.mark.parametrize("plan", R.PLANS)
@pytest.mark.parametrize("N", NS)
def test_driver_equals_the_restatement_bit_for_bit(driver, tmp_path, N, plan):
    """Every kind of row under every kind of weights, bad ones included: units, T, the six moments words, quantiles, passes, tables."""
    for wkind in R.WEIGHT_KINDS + ("bad",):
        got = check_driver(driver, tmp_path, R.ROW_KINDS, wkind, N, plan, f"N {N} plan {plan} weights {wkind}", seed=N)
        if wkind == "tiny":
            assert got["units"] == (0, 0, N)
            for k in got["quant"]:
                assert all((b & 0x7ff0000000000000) == 0x7ff0000000000000 and b & 0xfffffffffffff for b in got["quant"][k]), "T == 0: every quantile is NaN"
                assert got["passes"][k] == [0] * len(R.PROBS)


def test_driver_under_address_and_ub_sanitizers(driver_san, tmp_path):
    """One shape of each kind: a single particle, a partial block, two tree levels; every plan; every kind of weights."""
    for N, plan in ((1, (12, 65536)), (65, (3, 0)), (600, (5, 4))):
        for wkind in R.WEIGHT_KINDS + ("bad",):
            check_driver(driver_san, tmp_path, R.ROW_KINDS, wkind, N, plan, f"sanitizers N {N} plan {plan} weights {wkind}", seed=N)


def test_the_passes_are_what_the_plans_are_meant_to_force(driver, tmp_path):
    """(3, 0) never collects: a row of distinct values is decided bit by bit, 22 passes of 3 bits (the last of 1), unless the bucket
    shrinks to one value first; (5, 4) crosses from histogram to collect; (12, 65536) collects at once."""
    N = 600
    x, w = R.rows(("normal", "constant"), N, 7), R.weights("dirichlet", N, 7)
    p = {plan: run_driver(driver, driver_args(tmp_path, x, w, R.PROBS, *plan))["passes"] for plan in R.PLANS}
    print(p)
    assert p[(12, 65536)] == {0: [1] * 5, 1: [1] * 5}
    assert p[(3, 0)][1] == [1] * 5 and all(2 <= v <= 22 for v in p[(3, 0)][0])
    assert all(2 <= v < 13 for v in p[(5, 4)][0])


def test_a_pass_that_does_not_reproduce_the_previous_one_is_an_error_never_a_quantile(driver, driver_san, tmp_path):
    """One unit too many in a histogram of pass 1 or 2, one cursor step too many in a collect pass: FG_E_STATE with the row named."""
    x, w = R.rows(("normal",), 600, 3), R.weights("dirichlet", 600, 3)
    for exe in (driver, driver_san):
        for plan, k in (((3, 0), 1), ((3, 0), 2), ((12, 65536), 1), ((5, 4), 3)):
            got = run_driver(exe, driver_args(tmp_path, x, w, R.PROBS, *plan), env=dict(WPOP_DRIVER_CORRUPT_PASS=str(k)))
            print(plan, k, got)
            assert isinstance(got, tuple) and got[0] == FG_E_STATE and f"pass {k} did not reproduce the previous one: row 0" in got[1]
        assert isinstance(run_driver(exe, driver_args(tmp_path, x, w, R.PROBS, 12, 65536), env=dict(WPOP_DRIVER_CORRUPT_PASS="2")), dict)    # no second pass: nothing spoilt


# ---- the restatement against independent definitions -------------------------------------------------------------------------
@pytest.mark.parametrize("N", NS)
def test_quantiles_equal_a_brute_force_sort_and_cumulative_sum(N):
    for wkind in R.WEIGHT_KINDS + ("bad",):
        w = R.bad_weights(N, N)[0] if wkind == "bad" else R.weights(wkind, N, N)
        q, T, _, _ = R.units(w)
        for kind in R.ROW_KINDS:
            x = R.row(kind, N, N)
            want = [R.quantile_brute(x, q, T, p) for p in R.PROBS]
            for plan in R.PLANS:
                got, _ = R.quantiles(x, q, T, R.PROBS, *plan)
                if plan == R.PLANS[0]:
                    print(f"N {N} {wkind} {kind}: {got} / {want}")
                assert [R.bits(v) for v in got] == [R.bits(v) for v in want], (wkind, kind, plan)
            if T == 0:
                assert all(v != v for v in want)


@pytest.mark.parametrize("N", NS)
def test_tables_equal_a_counter_of_the_units(N):
    vals, vt, lo, bins = table_rows(N, N)
    for wkind in R.WEIGHT_KINDS:
        q, T, _, _ = R.units(R.weights(wkind, N, N))
        for k in range(len(vt)):
            t, c = R.table(vals[k], q, T, lo[k], bins[k]), R.table_counter(vals[k], q)
            inside = {v: u for v, u in c.items() if lo[k] <= v < lo[k] + bins[k]}
            print(f"N {N} {wkind} row {k}: {len(inside)} values inside, below {t['below']}, above {t['above']}, T {T}")
            assert {lo[k] + j: u for j, u in enumerate(t["units"]) if u} == inside
            assert t["below"] == sum(u for v, u in c.items() if v < lo[k]) and t["above"] == sum(u for v, u in c.items() if v >= lo[k] + bins[k])
            assert sum(t["units"]) + t["below"] + t["above"] == T
            assert (t["min"], t["max"]) == ((min(c), max(c)) if c else (None, None))


@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("kind", ("normal", "constant", "three", "zeros"))
def test_moments_are_within_the_derived_bounds(kind, N):
    """mean against the exact weighted mean within (N + 8) 2^-52 max|x - mean| -- the sums math.fsum would give, but of exact products
    (Fractions): a product w x rounded to a double first puts an error of the reference's own on a constant row, 2.5000000000000004 for
    2.5, where the bound is 0; var and mcse^2 against mpmath at 50 digits within (N + 8) 2^-52
    relative, var with the factor (1 + mean^2 / var) of a variance computed about a leaf's value."""
    import mpmath
    mpmath.mp.dps = 50
    x = [float(v) for v in R.row(kind, N, N)]
    for wkind in R.WEIGHT_KINDS:
        w = [float(v) for v in R.weights(wkind, N, N)]
        W, mean, var, std, mcse, n_used = R.moments(x, w)
        bound = (N + 8) * EPS
        used = [(a, b) for a, b in zip(w, x) if a > 0.0]
        assert n_used == len(used)
        if not used:                                 # every weight is zero (quarter_zero at N = 1): W = 0, the rest NaN
            print(f"{kind} N {N} {wkind}: no particle with weight: W {W!r}, mean {mean!r}")
            assert W == 0.0 and all(v != v for v in (mean, var, std, mcse))
            continue
        exact = sum(Fraction(a) * Fraction(b) for a, b in used) / sum(Fraction(a) for a, _ in used)
        want_mean = float(exact)
        spread = float(max(abs(Fraction(b) - exact) for _, b in used))
        print(f"{kind} N {N} {wkind}: W {W!r}, mean {mean!r} / {want_mean!r}: err {abs(mean - want_mean):.3e}, bound {bound * spread:.3e}")
        assert abs(W - math.fsum(a for a, _ in used)) <= bound * W
        assert abs(mean - want_mean) <= bound * spread
        ws, xs = [mpmath.mpf(a) for a, _ in used], [mpmath.mpf(b) for _, b in used]
        Wm = sum(ws)
        m = sum(a * b for a, b in zip(ws, xs)) / Wm
        v = sum(a * (b - m) ** 2 for a, b in zip(ws, xs)) / Wm
        e2 = sum(a * a * (b - m) ** 2 for a, b in zip(ws, xs)) / (Wm * Wm)
        if v == 0:
            print(f"  var {var!r}, mcse {mcse!r}: exact 0")
            assert var == 0.0 and mcse == 0.0 and std == 0.0
            continue
        rel_v = float(abs(mpmath.mpf(var) - v) / v)
        rel_e = float(abs(mpmath.mpf(mcse) ** 2 - e2) / e2)
        bound_v = bound * float(1 + m * m / v)
        print(f"  var {var!r}: rel err {rel_v:.3e}, bound {bound_v:.3e}; mcse^2 {mcse * mcse!r}: rel err {rel_e:.3e}, bound {bound:.3e}")
        assert rel_v <= bound_v
        assert rel_e <= bound
        assert std == math.sqrt(var)


def test_non_finite_cells_and_dead_weights_stay_out_of_the_moments():
    N = 65
    x, (w, n_bad) = R.row("non_finite", N, 1), R.bad_weights(N, 1)
    W, mean, var, std, mcse, n_used = R.moments(x, w)
    keep = [i for i in range(N) if math.isfinite(x[i]) and 0.0 < w[i] <= 1.0]
    W2, mean2, *_ = R.moments([x[i] for i in keep], [w[i] for i in keep])
    print(n_used, len(keep), mean, mean2)
    assert n_used == len(keep) < N - n_bad and math.isfinite(mean) and abs(mean - mean2) <= (N + 8) * EPS * max(abs(x[i] - mean2) for i in keep)
    assert R.moments(x, np.zeros(N)) [5] == 0.0 and R.moments(x, np.zeros(N))[0] == 0.0


# ---- argument errors ---------------------------------------------------------------------------------------------------------
def test_every_argument_limit_returns_its_code_with_a_message(driver, tmp_path):
    x, w = R.rows(("normal",), 4, 0), R.weights("uniform", 4)
    cells = np.zeros((1, 4), dtype=np.uint64)

    def args(N=4, d=1, probs=(0.5,), digit_bits=12, capacity=16, tables=None):
        a = driver_args(tmp_path, x, w, probs, digit_bits, capacity, tables)
        a[0], a[1] = str(N), str(d)
        return a

    def tab(vt=(I64,), lo=(0,), bins=(4,), n_rows=None):
        a = driver_args(tmp_path, x, w, (0.5,), 12, 16, (cells, list(vt), list(lo), list(bins)))
        if n_rows is not None:
            a[7] = str(n_rows)
        return a

    cases = [(args(N=0), "fg_wpop_new: n < 1"), (args(d=0), "fg_wpop_moments: d must lie in [1, 65535]"), (args(d=65536), "d must lie in [1, 65535]"),
             (args(probs=()), "n_probs must lie in [1, 8]"), (args(probs=(0.1,) * 9), "n_probs must lie in [1, 8]"),
             (args(probs=(1.5,)), "probabilities must lie in [0, 1]"), (args(probs=(float("nan"),)), "probabilities must lie in [0, 1]"),
             (args(digit_bits=0), "digit_bits must lie in [1, 12]"), (args(digit_bits=13), "digit_bits must lie in [1, 12]"),
             (args(capacity=-1), "capacity < 0"), (tab(bins=(0,)), "bins must lie in [1, 4096]"), (tab(bins=(4097,)), "bins must lie in [1, 4096]"),
             (tab(n_rows=0), "n_rows must lie in [1, 65535]"), (tab(n_rows=65536), "n_rows must lie in [1, 65535]"),
             (tab(vt=(F64,)), "an f64 row has no frequency table"), (tab(vt=(7,)), "unknown value type 7"),
             (tab(vt=(U64,), lo=(-1,)), "lo of an unsigned row must not be negative"), (tab(lo=(2 ** 63 - 2,), bins=(3,)), "overflows")]
    for a, text in cases:
        got = run_driver(driver, a)
        print(got)
        assert isinstance(got, tuple) and got[0] == FG_E_BAD_ARG and text in got[1] and got[1].startswith("fg_wpop_"), (text, got)
    for a in (args(probs=(0.0, 1.0)), args(capacity=0), args(digit_bits=1), tab(bins=(4096,))):          # the limits themselves pass
        assert isinstance(run_driver(driver, a), dict)


def test_weights_that_are_not_normalised_are_refused(driver, tmp_path):
    """T >= 2^53: 4 096 weights of 1 would wrap a 64-bit sum of units; two of 1 reach 2^53."""
    for N in (2, 4096):
        got = run_driver(driver, driver_args(tmp_path, R.rows(("normal",), N, 0), np.ones(N), (0.5,), 12, 16))
        print(N, got)
        assert got[0] == FG_E_BAD_ARG and "not normalised" in got[1]
    got = run_driver(driver, driver_args(tmp_path, R.rows(("normal",), 1, 0), np.ones(1), (0.5,), 12, 16))
    assert got["units"] == (2 ** 52, 0, 0)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_abi_check_passes_with_the_new_entries():
    from fugue_amd import engine as E
    header = open(os.path.join(ROOT, "include", "fugue_amd.h")).read()
    rust = open(os.path.join(ROOT, "rust", "fugue-gpu", "src", "ffi.rs")).read()
    H, Rs = abi_check.parse_header(header), abi_check.parse_rust(rust)
    for f in NEW:
        assert f in H["fns"] and f in Rs["fns"] and f in E.ABI_SYMBOLS, f
    assert abi_check.compare_header_rust(header, rust) == []
    assert abi_check.compare_header_ctypes(header, E.lib()) == []
    assert set(H["fns"]) == set(E.ABI_SYMBOLS)


# ---- SMCResult.weighted_mean ----------------------------------------------------------------------------------------------------
def test_smc_result_weighted_mean_on_a_hand_made_result():
    from fugue_amd.inference import SMCResult
    xs, ws = [1.0, 2.0, 4.0], [0.25, 0.25, 0.5]
    cells = np.stack([np.array(xs).view(np.int64), np.array([3, 1, 2], dtype=np.int64)])
    r = SMCResult(["mu", "k"], [F64, U64], cells, np.array(ws), np.log(np.array(ws)), -1.0)
    num = den = 0.0
    for v, w in zip(xs, ws):
        num += w * v
        den += w
    print(r.weighted_mean("mu"), num / den)
    assert r.weighted_mean("mu") == num / den == 2.75
    assert r.weighted_mean("k") is None and r.weighted_mean("absent") is None
    r.weights = np.zeros(3)
    assert r.weighted_mean("mu") is None
    from fugue_amd import adaptive_smc_summary
    assert callable(adaptive_smc_summary)
