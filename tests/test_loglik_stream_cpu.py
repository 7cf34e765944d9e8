"""The log-likelihood stream without a GPU: tests/cpp/loglik_stream_driver.cpp (fg_loglik_stream_plan.h's update / merge / finish
functions, launch cuts and tree schedule, with host loops for the kernels) against the Python restatement, bit for bit, over
several chunkings and under AddressSanitizer / UBSan (a stand-alone binary); the restatement against the two-pass textbook formulas
within derived bounds; the ABI of the new entry points; compare_models on hand-made tables.  Every compared figure is printed
before it is asserted."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import abi_check
from tests import loglik_stream_restatement as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FG_E_BAD_ARG, FG_E_STATE = -3, -5
EPS = 2.0 ** -52
CS, NSELS = (1, 2, 3, 64, 65), (1, 3)
NEW = ["fg_loglik_stream_new", "fg_loglik_stream_update", "fg_loglik_stream_count", "fg_loglik_stream_pooled", "fg_loglik_stream_result",
       "fg_loglik_stream_free"]


def _build(out_dir, name, extra=()):
    assert shutil.which("g++"), "g++ builds the driver"
    exe = os.path.join(str(out_dir), name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", *extra, os.path.join(ROOT, "tests", "cpp", "loglik_stream_driver.cpp"), "-o", exe],
                   check=True)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("llstream"), "loglik_stream_driver")


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("llstream_san"), "loglik_stream_driver_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def run_driver(exe, work_dir, x, chunks, grid=(), expect_rc=0):
    """x [n][n_sel][C] -> (pooled bits [n_sel][8], counts [n_sel][3], figure bits [n_sel][8], (launches, levels, slices)), or (rc, message)."""
    n, n_sel, C = x.shape
    path = os.path.join(str(work_dir), "table.f64")
    np.ascontiguousarray(x, dtype=np.float64).tofile(path)
    r = subprocess.run([exe, str(n), str(n_sel), str(C), path, ",".join(str(c) for c in chunks)] + [str(g) for g in grid], capture_output=True, text=True)
    if r.returncode == 2:
        _, rc, msg = r.stdout.strip().split(" ", 2)
        assert expect_rc and int(rc) == expect_rc, r.stdout
        return int(rc), msg
    assert r.returncode == 0 and not expect_rc, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    pooled, counts, figs, shape = {}, {}, {}, None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "pooled":
            pooled[int(w[1])] = [int(v, 16) for v in w[2:]]
        elif w[0] == "counts":
            counts[int(w[1])] = [int(v) for v in w[2:]]
        elif w[0] == "figures":
            figs[int(w[1])] = [int(v, 16) for v in w[2:]]
        elif w[0] == "launches":
            shape = (int(w[1]), int(w[3]), int(w[5]))
    return [pooled[k] for k in range(n_sel)], [counts[k] for k in range(n_sel)], [figs[k] for k in range(n_sel)], shape


def chunkings(n):
    out = [(n,), (1,) * n]
    if n > 8:
        out.append((1, 7, n - 8))
    return out


def kinds_for(n_sel, group):
    return [L.ROW_KINDS[(group * 3 + j) % len(L.ROW_KINDS)] for j in range(n_sel)]


def check_driver(exe, tmp_path, x, label, grid=()):
    want_e, want_f = L.stream(x)
    n = x.shape[0]
    for chunks in chunkings(n):
        pooled, counts, figs, shape = run_driver(exe, tmp_path, x, chunks, grid)
        for k in range(x.shape[1]):
            wp = [L.bits(v) for v in want_e[k][:L.POOLED]]
            wf = [L.bits(v) for v in want_f[k]]
            ok = pooled[k] == wp and counts[k] == list(want_e[k][8:]) and figs[k] == wf
            if not ok or len(chunks) == 1:
                print(f"{label} chunks {chunks if len(chunks) < 4 else '(1,)*n'} k {k}: pooled equal {pooled[k] == wp}, counts {counts[k]} / {want_e[k][8:]}, "
                      f"figures equal {figs[k] == wf}: {[f'{v:.6g}' for v in want_f[k]]}")
            assert ok
    return shape


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("n_sel", NSELS)
def test_driver_equals_the_restatement_bit_for_bit(driver, tmp_path, C, n_sel):
    """Every row kind at every shape, n_total = 23, chunkings (N,), (1, 1, ...), (1, 7, rest)."""
    groups = range(4) if n_sel == 3 else range(len(L.ROW_KINDS))
    for g in groups:
        kinds = kinds_for(n_sel, g) if n_sel == 3 else [L.ROW_KINDS[g]]
        check_driver(driver, tmp_path, L.table(kinds, 23, C, seed=C), f"C {C} {kinds}")


def test_a_single_cell(driver, tmp_path):
    """n_total x C = 1: p_waic is NaN (no N - 1), lppd = elpd_loo = mean_ll = the cell, is_ess = max_weight = 1."""
    for v in (-2.5, -np.inf, np.inf, np.nan):
        x = np.full((1, 1, 1), v)
        check_driver(driver, tmp_path, x, f"single {v}")
    _, f = L.stream(np.full((1, 1, 1), -2.5))
    print(f[0])
    assert f[0][0] == -2.5 and f[0][1] == -2.5 and f[0][2] != f[0][2] and f[0][4] == -2.5 and f[0][6] == 1.0 and f[0][7] == 1.0


def test_launch_cuts_and_slices_change_nothing(driver, tmp_path):
    """Grid limits of 1 block per update launch and 2 statements per pool launch: more launches, the same bits (the restatement knows
    no launch).  C = 600 spans three blocks of a tree level, so the tree has two levels."""
    x = L.table(["normal", "far", "neg_inf"], 9, 600, seed=5)
    base = check_driver(driver, tmp_path, x, "default grid")
    cut = check_driver(driver, tmp_path, x, "cut grid", grid=(1, 2))
    print("launches, levels, slices:", base, cut)
    assert base == (1, 2, 1) and cut == (math.ceil(3 * 600 / 256), 2, 2)


def test_a_tree_of_three_levels(driver, tmp_path):
    """C = 65 537 chains: 65 537 -> 257 -> 2 -> 1, the last block of every level partial.  One statement, one draw, the default grid;
    the -inf cell's counter crosses the three levels with the finite words."""
    shape = check_driver(driver, tmp_path, L.table(["neg_inf"], 1, 65537, seed=3), "C 65537")
    print("launches, levels, slices:", shape)
    assert shape == (1, 3, 1)


def test_driver_under_address_and_ub_sanitizers(driver_san, tmp_path):
    for C in (1, 3, 65):
        check_driver(driver_san, tmp_path, L.table(["normal", "far", "both_inf"], 23, C, seed=C), f"sanitizers C {C}")
        check_driver(driver_san, tmp_path, L.table(["increasing", "all_neg_inf", "nan"], 23, C, seed=C), f"sanitizers C {C}")
    check_driver(driver_san, tmp_path, L.table(["normal", "decreasing", "pos_inf"], 9, 600, seed=1), "sanitizers C 600, cut", grid=(1, 2))
    check_driver(driver_san, tmp_path, np.full((1, 1, 1), -2.5), "sanitizers single")


def test_protocol_errors_of_the_plan(driver, tmp_path):
    x = L.table(["normal"], 10, 3)
    for shape in ((0, 1, 3), (10, 0, 3), (10, 1, 0)):
        r = subprocess.run([driver, *[str(v) for v in shape], os.path.join(str(tmp_path), "none"), "1"], capture_output=True, text=True)
        print(shape, r.stdout.strip())
        assert r.returncode == 2 and r.stdout.startswith(f"error {FG_E_BAD_ARG} ")
    rc, msg = run_driver(driver, tmp_path, x, (9, 2), expect_rc=FG_E_STATE)
    print(rc, msg)
    assert "pass n_total" in msg
    rc, msg = run_driver(driver, tmp_path, x, (4, 0, 5), expect_rc=FG_E_STATE)
    print(rc, msg)
    assert "9 of 10" in msg
    a = run_driver(driver, tmp_path, x, (4, 0, 6))                # an empty chunk is a no-op
    b = run_driver(driver, tmp_path, x, (10,))
    assert a == b


# ---- the restatement against the two-pass formulas --------------------------------------------------------------------------
@pytest.mark.parametrize("C", CS)
def test_non_finite_rows_have_the_class_the_two_pass_formulas_give(C):
    kinds = [k for k in L.ROW_KINDS if k not in L.FINITE_KINDS]
    x = L.table(kinds, 23, C, seed=C)
    elems, figs = L.stream(x)
    for k, kind in enumerate(kinds):
        want = L.two_pass(x[:, k, :])
        print(f"C {C} {kind}: restatement {figs[k]}\n        two-pass    {want}")
        for name, a, b in zip(L.FIGURE_NAMES, figs[k], want):
            assert L.same_class(a, b), (kind, name, a, b)
        row = x[:, k, :]
        assert elems[k][8:] == [int(np.isneginf(row).sum()), int(np.isposinf(row).sum()), int(np.isnan(row).sum())]


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("kind", L.FINITE_KINDS)
def test_finite_rows_are_within_the_derived_bounds_of_the_two_pass_formulas(kind, C):
    """lppd, elpd_loo absolute and is_ess relative within (N + 8) 2^-52 (a sequential sum of N positive terms, each within an ulp or
    two); mean_ll within (N + 8) 2^-52 max|x - pivot|; p_waic against mpmath at 50 digits within (N + 8) 2^-52 (1 + mu^2 / var), mu
    measured from the pivot."""
    import mpmath
    n = 23
    x = L.table([kind], n, C, seed=C)
    elems, figs = L.stream(x)
    f, row = dict(zip(L.FIGURE_NAMES, figs[0])), x[:, 0, :].ravel()
    want = dict(zip(L.FIGURE_NAMES, L.two_pass(row)))
    N = row.size
    bound = (N + 8) * EPS
    pivot = float(x[0, 0, 0])
    err = {k: abs(f[k] - want[k]) for k in ("lppd", "elpd_loo", "mean_ll")}
    err["is_ess"] = abs(f["is_ess"] - want["is_ess"]) / want["is_ess"]
    mean_bound = bound * max(float(np.max(np.abs(row - pivot))), 0.0)
    print(f"{kind} C {C} N {N}: bound {bound:.3e}; lppd err {err['lppd']:.3e}, elpd_loo err {err['elpd_loo']:.3e}, is_ess rel err {err['is_ess']:.3e}, "
          f"mean_ll err {err['mean_ll']:.3e} (bound {mean_bound:.3e})")
    assert err["lppd"] <= bound
    assert err["elpd_loo"] <= bound
    assert err["is_ess"] <= bound
    assert err["mean_ll"] <= mean_bound
    if N > 1:
        mpmath.mp.dps = 50
        xs = [mpmath.mpf(float(v)) for v in row]
        m = sum(xs) / N
        var = sum((v - m) ** 2 for v in xs) / (N - 1)
        if var == 0:
            print(f"  p_waic {f['p_waic']!r}, exact 0")
            assert f["p_waic"] == 0.0
        else:
            mu = m - mpmath.mpf(pivot)
            rel_bound = bound * float(1 + mu * mu / var)
            rel = float(abs(mpmath.mpf(f["p_waic"]) - var) / var)
            print(f"  p_waic {f['p_waic']!r}, exact {float(var)!r}: rel err {rel:.3e}, bound {rel_bound:.3e}")
            assert rel <= rel_bound
    assert f["elpd_waic"] == f["lppd"] - f["p_waic"] or N == 1
    assert f["p_loo"] == f["lppd"] - f["elpd_loo"]
    mw = abs(f["max_weight"] - want["max_weight"]) / want["max_weight"]
    print(f"  max_weight rel err {mw:.3e}")
    assert mw <= bound                               # 1 / the same sum


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_abi_check_passes_with_the_new_entries():
    from fugue_amd import engine as E
    header = open(os.path.join(ROOT, "include", "fugue_amd.h")).read()
    rust = open(os.path.join(ROOT, "rust", "fugue-gpu", "src", "ffi.rs")).read()
    H, R = abi_check.parse_header(header), abi_check.parse_rust(rust)
    for f in NEW:
        assert f in H["fns"] and f in R["fns"] and f in E.ABI_SYMBOLS, f
    assert abi_check.compare_header_rust(header, rust) == []
    assert abi_check.compare_header_ctypes(header, E.lib()) == []
    assert set(H["fns"]) == set(E.ABI_SYMBOLS)


# ---- compare_models ---------------------------------------------------------------------------------------------------------
def _hand_made(names, elpd_loo, elpd_waic):
    from fugue_amd.comparison import PointwiseComparison
    O = len(names)
    z = np.zeros(O)
    return PointwiseComparison(names=list(names), n_draws=10, lppd=z.copy(), mean_ll=z.copy(), p_waic=z.copy(), elpd_waic=np.array(elpd_waic, dtype=np.float64),
                               elpd_loo=np.array(elpd_loo, dtype=np.float64), p_loo=z.copy(), is_ess=z + 10.0, max_weight=z + 0.1,
                               n_neg_inf=np.zeros(O, dtype=np.int64), n_pos_inf=np.zeros(O, dtype=np.int64), n_nan=np.zeros(O, dtype=np.int64))


def test_compare_models_on_hand_made_tables():
    from fugue_amd.comparison import compare_models
    names = ["y0", "y1", "y2", "y3"]
    a = _hand_made(names, [-1.0, -2.0, -3.5, -0.25], [-1.5, -2.0, -3.0, -0.5])
    b = _hand_made(names, [-1.25, -1.0, -4.0, -0.75], [-1.0, -2.5, -3.5, -0.25])
    for which in ("elpd_loo", "elpd_waic"):
        diff, se = compare_models(a, b, which)
        pa, pb = getattr(a, which), getattr(b, which)
        tot_a, tot_b = 0.0, 0.0
        for v in pa.tolist():
            tot_a += v
        for v in pb.tolist():
            tot_b += v
        d = (pa - pb).tolist()
        m = sum(d) / 4
        want_se = math.sqrt(4 * sum((v - m) ** 2 for v in d) / 3)
        print(which, diff, se, tot_a - tot_b, want_se)
        assert diff == tot_a - tot_b == getattr(a, which + "_total") - getattr(b, which + "_total")
        assert abs(se - want_se) <= 4 * EPS * want_se
        assert abs(a.se(which) - math.sqrt(4 * np.var(pa, ddof=1))) <= 4 * EPS * a.se(which)
    with pytest.raises(ValueError):
        compare_models(a, _hand_made(["y0", "y1", "y2", "other"], [0, 0, 0, 0], [0, 0, 0, 0]))
    with pytest.raises(ValueError):
        compare_models(a, _hand_made(names[:3], [0, 0, 0], [0, 0, 0]))
    with pytest.raises(ValueError):
        compare_models(a, b, which="lppd_nonsense")
