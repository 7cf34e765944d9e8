"""Predictive checks and WAIC / IS-LOO of a weighted population without a GPU: tests/cpp/wpop_eval_driver.cpp
(fg_wpop_eval_plan.h's categories, slices, integrity rule and finish step over the plan headers' pools and tree, with host loops for the
kernels) against tests/wpop_eval_restatement.py -- integers and every double no transcendental touches bit for bit -- and under
AddressSanitizer / UBSan (a stand-alone binary); the exp-based figures against mpmath at 50 digits within the bound derived in
`wpop_eval_restatement.bounds`; equal weights against the restatements of the chain streams; the corners; slicing; every argument limit;
the ABI.  Every compared figure is printed before it is asserted."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import abi_check
from tests import loglik_stream_restatement as LR
from tests import ppc_restatement as PR
from tests import wpop_eval_restatement as R
from tests import wpop_restatement as WR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FG_E_BAD_ARG, FG_E_STATE = -3, -5
EPS = 2.0 ** -52
NS = (1, 2, 63, 64, 65, 257, 600)
NEW = ["fg_wpop_checks_n_slots", "fg_wpop_checks", "fg_wpop_loglik"]
EXACT_WORDS = ("W", "W_fin", "W2", "mean", "ssd", "n_used", "mx", "mn")          # no transcendental touches them
EXACT_FIGURES = ("mean_ll", "p_waic")


def _build(out_dir, name, extra=()):
    assert shutil.which("g++"), "g++ builds the driver"
    exe = os.path.join(str(out_dir), name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", *extra, os.path.join(ROOT, "tests", "cpp", "wpop_eval_driver.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("wpe"), "wpop_eval_driver")


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("wpe_san"), "wpop_eval_driver_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _csv(v):
    return ",".join(repr(float(a)) if isinstance(a, float) else str(int(a)) for a in v)


def masks_of(checks):
    return [int(m) for _, m, _ in checks]


def driver_args(work_dir, w, cells=None, vtypes=(), checks=(), ll=None, slices=None, N=None, n_rows=None, n_sel=None):
    pw = os.path.join(str(work_dir), "w.f64")
    np.ascontiguousarray(w, dtype=np.float64).tofile(pw)
    args = [str(len(w) if N is None else N), pw]
    offsets, members, observed = [0], [], []
    for rows, _, obs in checks:
        members += list(rows)
        observed += [float(v) for v in obs]
        offsets.append(len(members))
    pc = "-"
    if cells is not None:
        pc = os.path.join(str(work_dir), "cells.u64")
        np.ascontiguousarray(cells, dtype=np.uint64).tofile(pc)
    args += [str((0 if cells is None else len(cells)) if n_rows is None else n_rows), pc, _csv(vtypes), _csv(offsets), _csv(members), _csv(masks_of(checks)), _csv(observed)]
    pl = "-"
    if ll is not None:
        pl = os.path.join(str(work_dir), "ll.f64")
        np.ascontiguousarray(ll, dtype=np.float64).tofile(pl)
    args += [str((0 if ll is None else len(ll)) if n_sel is None else n_sel), pl]
    if slices is not None:
        args += [str(slices[0]), str(slices[1])]
    return args


def run_driver(exe, args, env=None):
    """-> dict(units, slot {k: dict}, ll {k: dict}, text) or (rc, message)"""
    r = subprocess.run([exe] + args, capture_output=True, text=True, env=None if env is None else dict(os.environ, **env))
    if r.returncode == 2:
        _, rc, msg = r.stdout.strip().splitlines()[-1].split(" ", 2)
        return int(rc), msg
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    out = dict(slot={}, ll={}, text=r.stdout)
    for line in r.stdout.splitlines():
        t = line.split()
        if t[0] == "units":
            out["units"] = tuple(int(v) for v in t[1:])
        elif t[0] == "slot":
            out["slot"][int(t[1])] = dict(t_obs=int(t[2], 16), units=[int(v) for v in t[3:7]], counts=[int(v) for v in t[7:11]], moments=[int(v, 16) for v in t[11:17]],
                                          p=[int(v, 16) for v in t[17:20]])
        elif t[0] == "ll":
            out["ll"][int(t[1])] = dict(figures=[int(v, 16) for v in t[2:10]], words=[int(v, 16) for v in t[10:22]], counts=[int(v) for v in t[22:26]], arg=int(t[26]))
    return out


def unbits(b):
    return np.array([b], dtype=np.uint64).view(np.float64)[0].item()


def same_class(a, b):
    return LR.same_class(a, b)


def check_slots(got, want, label):
    """units, counts, t_obs, the six moment words and the p-values of every slot, bit for bit"""
    assert len(got["slot"]) == len(want["t_obs"])
    for k, ob in enumerate(want["t_obs"]):
        g = got["slot"][k]
        ok = (g["t_obs"] == R.bits(ob) and g["units"] == want["units"][k] and g["counts"] == want["counts"][k] and g["moments"] == [R.bits(v) for v in want["moments"][k]] and
              g["p"] == [R.bits(v) for v in want["p"][k]])
        print(f"{label} slot {k}: units {g['units']} counts {g['counts']} p {[f'{unbits(b):.6g}' for b in g['p']]} mean {unbits(g['moments'][1]):.6g} equal {ok}")
        assert ok, (label, k, g, want["units"][k], want["counts"][k], want["moments"][k], want["p"][k])


def check_ll(got, want, ll, w, label, e_exp=R.E_EXP):
    """counters, the transcendental-free words and figures, mx, mn and tmax's argument bit for bit; the exp-based within the bound"""
    worst = 0.0
    for k in range(len(ll)):
        g, words, counts, figs = got["ll"][k], want["words"][k], want["counts"][k], want["figures"][k]
        assert g["counts"] == counts, (label, k, g["counts"], counts)
        for name in EXACT_WORDS:
            j = R.WORD_NAMES.index(name)
            assert g["words"][j] == R.bits(words[j]) or (words[j] != words[j] and unbits(g["words"][j]) != unbits(g["words"][j])), (label, k, name, unbits(g["words"][j]), words[j])
        for name in EXACT_FIGURES:
            j = R.FIGURE_NAMES.index(name)
            a = unbits(g["figures"][j])
            assert g["figures"][j] == R.bits(figs[j]) or (a != a and figs[j] != figs[j]), (label, k, name, a, figs[j])
        assert g["arg"] == (-1 if want["arg_tmax"][k] is None else want["arg_tmax"][k]), (label, k, g["arg"], want["arg_tmax"][k])
        got_f = {n: unbits(g["figures"][j]) for j, n in enumerate(R.FIGURE_NAMES)}
        for j, n in enumerate(R.FIGURE_NAMES):
            assert same_class(got_f[n], figs[j]), (label, k, n, got_f[n], figs[j])
        if counts[0] == 0 or counts[3] > 0:
            print(f"{label} row {k}: counters {counts}, every figure NaN")
            assert all(v != v for v in got_f.values())
            continue
        exact = R.exact_row(ll[k], w)
        bound = R.bounds(ll[k], w, exact, e_exp)
        for n in R.EXP_FIGURES:
            if not math.isfinite(got_f[n]):
                continue
            err = abs(got_f[n] - exact[n])
            worst = max(worst, err / bound[n])
            print(f"{label} row {k} {n}: {got_f[n]!r} / exact {exact[n]!r}: err {err:.3e} bound {bound[n]:.3e}")
            assert err <= bound[n], (label, k, n, got_f[n], exact[n])
    return worst


@pytest.mark.parametrize("N", NS)
def test_driver_equals_the_restatement(driver, tmp_path, N):
    """Every kind of weights, bad ones included (the C level gives them no units and no leaf); every check and every kind of row."""
    for wkind in R.WEIGHT_KINDS:
        w, n_bad = R.weights(wkind, N, N)
        cells, vt, chk = R.check_table(N, N)
        ll = R.ll_table(R.LL_KINDS, N, w, N)
        got = run_driver(driver, driver_args(tmp_path, w, cells, vt, chk, ll))
        q, T, nb, nz = WR.units(w)
        assert got["units"] == (T, nb, nz) and nb == n_bad
        check_slots(got, R.checks(cells, vt, chk, w), f"N {N} {wkind}")
        worst = check_ll(got, R.loglik(ll, w), ll, w, f"N {N} {wkind}")
        print(f"N {N} {wkind}: largest error / bound {worst:.3f}")


def test_driver_under_address_and_ub_sanitizers(driver_san, tmp_path):
    for N, slices in ((1, None), (65, (1, 1)), (600, (3, 2))):
        for wkind in R.WEIGHT_KINDS:
            w, _ = R.weights(wkind, N, N)
            cells, vt, chk = R.check_table(N, N)
            ll = R.ll_table(R.LL_KINDS, N, w, N)
            got = run_driver(driver_san, driver_args(tmp_path, w, cells, vt, chk, ll, slices))
            check_slots(got, R.checks(cells, vt, chk, w), f"sanitizers N {N} {wkind}")
            check_ll(got, R.loglik(ll, w), ll, w, f"sanitizers N {N} {wkind}")


def test_the_bound_is_no_looser_than_the_chain_streams():
    """(N + 8) 2^-52 is what tests/test_gpu_loglik_stream.py holds the chain figures to.  At every N and under every kind of weights of
    these tests, the bound of every exp-based figure of every finite row is no looser (relative for is_ess and max_weight, relative to
    max(1, |figure|) for lppd and elpd_loo): where the derivation gives more -- small N, through the D terms -- `bounds` returns the
    ceiling.  A test of the restatement's own bound, not of the library: it is the one new test that passes without the feature."""
    for N in NS:
        for wkind in R.WEIGHT_KINDS:
            w, _ = R.weights(wkind, N, N)
            for kind in R.LL_FINITE:
                x = R.ll_row(kind, N, w, N)
                if not any(R.weight(float(a)) > 0.0 for a in w):
                    continue
                exact = R.exact_row(x, w)
                b, top = R.bounds(x, w, exact), R.ceiling(N, exact)
                print(N, wkind, kind, {k: f"{b[k] / top[k]:.3f} of the ceiling" for k in b}, f"(N + 8) = {N + 8}")
                assert all(0.0 <= b[k] <= top[k] for k in b)
                assert top["is_ess"] == (N + 8) * EPS * exact["is_ess"] and top["lppd"] == (N + 8) * EPS * max(1.0, abs(exact["lppd"]))


@pytest.mark.parametrize("N", (1, 2, 64, 256, 1024))
def test_equal_weights_are_the_chain_streams_of_one_draw(driver, tmp_path, N):
    """w = 1 / N with N a power of two, so q_i = 2^52 / N exactly.  The unit sums are tests/ppc_restatement.py's counters of the table
    read as 1 draw x N chains times 2^52 / N, and the p-values equal checks.py's quotients of those counters bit for bit (a common
    power of two leaves a quotient's bits alone).  The figures equal tests/loglik_stream_restatement.py's within the two derived bounds
    added, and no more than (N + 8) 2^-52.  p_waic: the weighted merges are the counted ones scaled by 2^-k exactly, so ssd_w = ssd / N bit for bit; then
    ssd_w / (1 - 1 / N) against ssd / (N - 1): one rounding of the denominator and one more division, 3 x 2^-53 relative: 3 ulps."""
    from fugue_amd import checks as CK
    w = np.full(N, 1.0 / N)
    cells, vt, chk = R.check_table(N, N)
    ll = R.ll_table(R.LL_KINDS, N, w, N)
    got = run_driver(driver, driver_args(tmp_path, w, cells, vt, chk, ll))
    S = PR.stream(np.ascontiguousarray(cells)[None], vt, chk)
    unit = 2 ** 52 // N
    for k, (n_lt, n_eq, n_gt, n_nan, _) in enumerate(S["counts"]):
        g = got["slot"][k]
        p = CK._p_values([n_lt], [n_eq], [n_gt])
        want_p = [R.bits(p[name][0]) for name in CK.P_VALUES]
        print(f"N {N} slot {k}: units {g['units']} = {unit} x {[n_lt, n_eq, n_gt, n_nan]}; p {[unbits(b) for b in g['p']]}")
        assert g["units"] == [unit * n_lt, unit * n_eq, unit * n_gt, unit * n_nan] and g["counts"] == [n_lt, n_eq, n_gt, n_nan]
        assert all(a == b or (unbits(a) != unbits(a) and unbits(b) != unbits(b)) for a, b in zip(g["p"], want_p))
    _, figs = LR.stream(np.ascontiguousarray(ll)[None])
    for k, kind in enumerate(R.LL_KINDS):
        gf = {n: unbits(got["ll"][k]["figures"][j]) for j, n in enumerate(R.FIGURE_NAMES)}
        if got["ll"][k]["counts"][0] == 0:           # no finite cell: the weighted form reports NaN figures, the chain form an infinity
            assert all(v != v for v in gf.values())
            continue
        wf = dict(zip(LR.FIGURE_NAMES, figs[k]))
        for n in R.FIGURE_NAMES:
            assert same_class(gf[n], wf[n]), (N, kind, n, gf[n], wf[n])
        if not math.isfinite(gf["lppd"]) or not math.isfinite(gf["elpd_loo"]):
            continue
        exact = R.exact_row(ll[k], w)
        b = R.bounds(ll[k], w, exact)
        for n in R.EXP_FIGURES:
            err = abs(gf[n] - wf[n])
            tol = min(2 * b[n], R.ceiling(N, exact)[n])
            print(f"N {N} {kind} {n}: {gf[n]!r} / {wf[n]!r}: err {err:.3e}, the two bounds under the ceiling {tol:.3e}")
            assert err <= tol
        assert gf["mean_ll"] == wf["mean_ll"]
        if N > 1:
            err = abs(gf["p_waic"] - wf["p_waic"])
            print(f"N {N} {kind} p_waic: {gf['p_waic']!r} / {wf['p_waic']!r}: {err / (abs(wf['p_waic']) * 2.0 ** -53) if wf['p_waic'] else 0.0:.2f} x 2^-53")
            assert err <= 3 * 2.0 ** -53 * abs(wf["p_waic"])
        else:
            assert gf["p_waic"] != gf["p_waic"]


def test_corners(driver, tmp_path):
    """N = 1; one weight about 1; a weight below 2^-53 is a leaf of the figures and the moments and in no unit sum; zero-weight
    particles with -inf / NaN cells change nothing; a far row stays finite; the K = 1 variance and the NaN T_obs slots are all nan."""
    N = 65
    w, _ = R.weights("below_unit", N, 5)
    i_small, i_zero = N // 3, (N // 3 + 1) % N
    assert WR.units(w)[0][i_small] == 0 and w[i_small] > 0.0
    cells, vt, chk = R.check_table(N, 5)
    ll = R.ll_table(("normal", "far", "dead_cells"), N, w, 5)
    ll[0][i_small] = 50.0                            # the largest cell by far: it must be mx
    ll[2][i_zero] = np.nan
    got = run_driver(driver, driver_args(tmp_path, w, cells, vt, chk, ll))
    want = R.loglik(ll, w)
    check_ll(got, want, ll, w, "corners")
    assert unbits(got["ll"][0]["words"][R.WORD_NAMES.index("mx")]) == 50.0 and got["ll"][0]["counts"][0] == N - 1
    assert got["ll"][2]["counts"] == [N - 1, 0, 0, 0]
    far = {n: unbits(got["ll"][1]["figures"][j]) for j, n in enumerate(R.FIGURE_NAMES)}
    print("far", far)
    assert all(math.isfinite(v) for v in far.values()) and -1.1e4 < far["lppd"] < -0.9e4
    # the same row with the dead particles' cells finite: the same words
    ll2 = ll.copy()
    ll2[2][[i for i in range(N) if R.weight(float(w[i])) == 0.0]] = -3.0
    got2 = run_driver(driver, driver_args(tmp_path, w, None, (), (), ll2))
    assert got2["ll"][2] == got["ll"][2]
    # units: the small particle is in the element counts of no category, and in the moments' n_used
    wantc = R.checks(cells, vt, chk, w)
    check_slots(got, wantc, "corners")
    labels = PR.slots_of(chk)
    k8 = labels.index((3, PR.MEAN))                  # the mean of row 0 alone: no NaN replicate
    assert sum(got["slot"][k8]["counts"]) == N - 2 and unbits(got["slot"][k8]["moments"][5]) == N - 1
    for k, (q, st) in enumerate(labels):
        if (q == 3 and st == PR.VAR) or q == 5:
            print("all-nan slot", k, got["slot"][k]["units"])
            assert got["slot"][k]["units"][:3] == [0, 0, 0] and got["slot"][k]["units"][3] == got["units"][0]
            assert all(unbits(b) != unbits(b) for b in got["slot"][k]["p"])
    # N = 1 and one heavy weight
    for N1, kind in ((1, "uniform"), (257, "one_heavy")):
        w1, _ = R.weights(kind, N1, 2)
        c1, vt1, chk1 = R.check_table(N1, 2)
        l1 = R.ll_table(R.LL_KINDS, N1, w1, 2)
        g1 = run_driver(driver, driver_args(tmp_path, w1, c1, vt1, chk1, l1))
        check_slots(g1, R.checks(c1, vt1, chk1, w1), f"{kind} N {N1}")
        check_ll(g1, R.loglik(l1, w1), l1, w1, f"{kind} N {N1}")
        if N1 == 1:
            f = {n: unbits(g1["ll"][0]["figures"][j]) for j, n in enumerate(R.FIGURE_NAMES)}
            assert f["p_waic"] != f["p_waic"] and f["is_ess"] == 1.0 and f["max_weight"] == 1.0 and f["lppd"] == l1[0][0] == f["elpd_loo"]


def test_non_finite_cells_follow_the_table(driver, tmp_path):
    N = 64
    w, _ = R.weights("dirichlet", N, 9)
    ll = R.ll_table(R.LL_KINDS, N, w, 9)
    got = run_driver(driver, driver_args(tmp_path, w, None, (), (), ll))
    f = {kind: {n: unbits(got["ll"][k]["figures"][j]) for j, n in enumerate(R.FIGURE_NAMES)} for k, kind in enumerate(R.LL_KINDS)}
    c = {kind: got["ll"][k]["counts"] for k, kind in enumerate(R.LL_KINDS)}
    print(f, c)
    assert c["neg_inf"] == [N - 1, 1, 0, 0] and c["pos_inf"] == [N - 1, 0, 1, 0] and c["nan"] == [N - 1, 0, 0, 1] and c["both_inf"] == [N - 2, 1, 1, 0] and c["all_neg_inf"] == [0, N, 0, 0]
    assert all(v != v for v in f["nan"].values()) and all(v != v for v in f["all_neg_inf"].values())
    a = f["neg_inf"]
    assert math.isfinite(a["lppd"]) and a["elpd_loo"] == -math.inf and a["mean_ll"] == -math.inf and a["p_waic"] != a["p_waic"] and a["is_ess"] != a["is_ess"] and a["max_weight"] != a["max_weight"] and a["p_loo"] == math.inf
    b = f["pos_inf"]
    assert b["lppd"] == math.inf and math.isfinite(b["elpd_loo"]) and b["mean_ll"] == math.inf and b["p_waic"] != b["p_waic"] and math.isfinite(b["is_ess"])
    ab = f["both_inf"]
    assert ab["lppd"] == math.inf and ab["elpd_loo"] == -math.inf and ab["mean_ll"] != ab["mean_ll"]


@pytest.mark.parametrize("N", (65, 600))
def test_the_result_does_not_depend_on_the_slicing(driver, tmp_path, N):
    w, _ = R.weights("quarter_zero", N, 4)
    cells, vt, chk = R.check_table(N, 4)
    ll = R.ll_table(R.LL_KINDS, N, w, 4)
    whole = run_driver(driver, driver_args(tmp_path, w, cells, vt, chk, ll))["text"]
    for slices in ((1, 1), (2, 4), (7, 3)):
        assert run_driver(driver, driver_args(tmp_path, w, cells, vt, chk, ll, slices))["text"] == whole, slices
    # rows and checks one at a time
    one = run_driver(driver, driver_args(tmp_path, w, cells, vt, chk[:1], ll[3:4]))
    full = run_driver(driver, driver_args(tmp_path, w, cells, vt, chk, ll))
    assert one["ll"][0] == full["ll"][3] and all(one["slot"][k] == full["slot"][k] for k in range(5))


def test_units_that_do_not_add_up_are_an_error(driver, tmp_path):
    w, _ = R.weights("dirichlet", 65, 1)
    cells, vt, chk = R.check_table(65, 1)
    got = run_driver(driver, driver_args(tmp_path, w, cells, vt, chk, None), env=dict(WPOP_EVAL_DRIVER_CORRUPT="1"))
    print(got)
    assert isinstance(got, tuple) and got[0] == FG_E_STATE and "slot 0 counted" in got[1]


def test_every_argument_limit_returns_its_code_with_a_message(driver, tmp_path):
    N = 4
    w = np.full(N, 0.25)
    cells = np.zeros((2, N), dtype=np.uint64)
    ll = np.zeros((1, N))
    ok = [([0, 1], PR.ALL, [0.0, 1.0])]

    def chk_args(checks=ok, vtypes=(PR.F64, PR.I64), **kw):
        return driver_args(tmp_path, w, cells, vtypes, checks, None, **kw)

    many = [([0], PR.ALL, [0.0])] * 13108              # 65540 slots
    cases = [(chk_args(N=0), "fg_wpop_new: n < 1"), (chk_args(n_rows=0), "n_rows must lie in [1, 65535]"), (chk_args(n_rows=65536), "n_rows must lie in [1, 65535]"),
             (chk_args(checks=()), "no check"), (chk_args(checks=[([0], 0, [0.0])]), "no statistic"), (chk_args(checks=[([0], 32, [0.0])]), "mask bit beyond"),
             (chk_args(checks=[([], PR.ALL, [])]), "is empty"), (chk_args(checks=[([2], PR.ALL, [0.0])]), "outside [0, n_rows)"), (chk_args(vtypes=(PR.F64, 9)), "unknown value type 9"),
             (chk_args(checks=many), "n_slots must lie in [1, 65535]"),
             (driver_args(tmp_path, w, None, (), (), ll, n_sel=0), "n_sel must lie in [1, 65535]"), (driver_args(tmp_path, w, None, (), (), ll, n_sel=65536), "n_sel must lie in [1, 65535]")]
    for a, text in cases:
        got = run_driver(driver, a)
        print(got)
        assert isinstance(got, tuple) and got[0] == FG_E_BAD_ARG and text in got[1] and got[1].startswith("fg_wpop_"), (text, got)
    assert isinstance(run_driver(driver, chk_args(checks=[([0], PR.ALL, [0.0])] * 13107)), dict)          # 65535 slots pass
    got = run_driver(driver, driver_args(tmp_path, np.ones(2), None, (), (), np.zeros((1, 2))))
    assert got[0] == FG_E_BAD_ARG and "not normalised" in got[1]


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


def test_python_refuses_bad_weights_and_keeps_the_old_refusals():
    """`weighted_predictive_check` / `weighted_model_comparison` raise ValueError on a NaN weight before any device is touched;
    `posterior_predictive_check` still refuses an SMCResult with the word "weighted"."""
    from fugue_amd import checks as CK
    from fugue_amd import comparison as CM
    from fugue_amd.inference import SMCResult
    cells = np.zeros((1, 3), dtype=np.int64)
    r = SMCResult(["mu"], [0], cells, np.array([0.5, np.nan, 0.5]), np.zeros(3), -1.0)
    r.predictive, r.predictive_names, r.predictive_vtypes, r.observe_values = cells, ["y"], [0], {"y": 0.0}
    r.log_likelihood = np.zeros((1, 3))
    for fn in (CK.weighted_predictive_check, CM.weighted_model_comparison):
        with pytest.raises(ValueError, match="n_bad"):
            fn(r)
    with pytest.raises(ValueError, match="weighted"):
        CK.posterior_predictive_check(r)
