"""Pareto-smoothed LOO without a GPU: the plan's integers through the library's own `fg_psis_tail_len` and through
tests/cpp/psis_plan_driver.cpp (stand-alone, also under AddressSanitizer / UBSan), the error codes that need no device, the law of the
estimator and the conventions on tests/psis_restatement.py, and the ABI.  Of `fg_psis_loo`'s own codes only the null engine is reached
here -- an engine needs a device -- so FG_E_LIMIT and the other FG_E_BAD_ARG cases are checked where they are decided: `fg_psis_tail_len`
and `fg_psis_plan` through the driver.  Every compared figure is printed before it is asserted."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import abi_check
from tests import psis_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FG_E_BAD_ARG, FG_E_LIMIT = -3, -7
NEW = ["fg_psis_words", "fg_psis_tail_len", "fg_psis_loo"]


def _build(out_dir, name, extra=()):
    assert shutil.which("g++"), "g++ builds the driver"
    exe = os.path.join(str(out_dir), name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", *extra, os.path.join(ROOT, "tests", "cpp", "psis_plan_driver.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("psis_san"), "psis_plan_driver_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    print(r.stdout[-3000:], r.stderr[-3000:])
    return r


# ---- the plan --------------------------------------------------------------------------------------------------------------------------
def rule_tail_len(S):
    """step 2 of the rule, written independently of the restatement: integers only"""
    b = 0
    while b * b < 9 * S:
        b += 1
    return min(-(-S // 5), b)


def test_tail_len_follows_the_rule_for_every_small_S_and_at_the_limit():
    from fugue_amd import engine as E
    L = E.lib()
    b = 0
    for S in range(1, 5001):
        while b * b < 9 * S:
            b += 1
        want = min(-(-S // 5), b)
        assert L.fg_psis_tail_len(S) == want == R.tail_len(S), S
    top = 2 ** 31 - 1
    assert L.fg_psis_tail_len(top) == R.tail_len(top) == min(-(-top // 5), math.isqrt(9 * top - 1) + 1) == 139023
    assert 139022 ** 2 < 9 * top <= 139023 ** 2
    assert [S for S in range(1, 200) if L.fg_psis_tail_len(S) < 5] == list(range(1, 21))            # M < 5 exactly for S <= 20
    assert [L.fg_psis_tail_len(S) for S in range(21, 26)] == [5] * 5 and L.fg_psis_tail_len(26) == 6
    # ceil(S / 5) up to S = 225, where both branches give 45; the square-root branch from there on
    assert all(L.fg_psis_tail_len(S) == -(-S // 5) for S in range(1, 226)) and L.fg_psis_tail_len(225) == 45 == 3 * 15
    assert L.fg_psis_tail_len(226) == 46 == -(-226 // 5) == rule_tail_len(226) and L.fg_psis_tail_len(231) == 46 < -(-231 // 5)
    assert L.fg_psis_words() == len(R.WORD_NAMES) == len(E.PSIS_WORD_NAMES) and E.PSIS_COUNTS == len(R.COUNT_NAMES)
    assert tuple(E.PSIS_WORD_NAMES) == R.WORD_NAMES and tuple(E.PSIS_COUNT_NAMES) == R.COUNT_NAMES


def test_error_codes_need_no_device():
    from fugue_amd import engine as E
    import ctypes as C
    L = E.lib()
    assert L.fg_psis_tail_len(0) == FG_E_BAD_ARG and L.fg_psis_tail_len(-5) == FG_E_BAD_ARG
    assert L.fg_psis_tail_len(2 ** 31) == FG_E_LIMIT and L.fg_psis_tail_len(2 ** 40) == FG_E_LIMIT
    words, counts = np.zeros(R.WORD_NAMES.__len__()), np.zeros(len(R.COUNT_NAMES), dtype=np.int64)
    rc = L.fg_psis_loo(None, 8, 1, 1, E._dp(words), counts.ctypes.data_as(C.POINTER(C.c_int64)), None)
    print(rc, E.last_error())
    assert rc == FG_E_BAD_ARG and "null engine" in E.last_error()


def test_plan_driver_under_address_and_ub_sanitizers(driver_san, tmp_path):
    """M, G, the t* index, the padded sort length, the passes, the blocks, the ownership of every cell and tail term, the buffer sizes
    and the slicing of the statements at every shape of the GPU tests, both benchmark shapes, the largest S and a statement count
    above the grid's y; the refusals; the select by host loops on tables with ties, signed zeros and non-finite cells."""
    shapes = [(n, C, k) for n, C in R.GPU_SHAPES for k in (1, 3)] + [(64, 65536, 16), (16, 4096, 1024), (1024, 65536, 70000), (32767, 65536, 1), (0, 3, 1), (2 ** 16, 2 ** 15, 1)]
    r = _run(driver_san, ["plan"] + [v for s in shapes for v in s])
    assert r.returncode == 0
    lines = [l for l in r.stdout.splitlines() if l.startswith("plan ")]
    assert len(lines) == len(shapes) and all(l.endswith("| ok") for l in lines)
    for (n, C, k), line in zip(shapes, lines):
        got = [int(v) for v in line.split("|")[1].split()]
        if n < 1:
            assert got[0] == FG_E_BAD_ARG
            continue
        if n * C >= 2 ** 31:
            assert got[0] == FG_E_LIMIT
            continue
        S, M = n * C, R.tail_len(n * C)
        assert got[:10] == [0, S, M, R.profile_points(M), R.quartile_index(M), R.sort_len(M), min(M + 1, S), R.blocks(S), R.pow2(R.blocks(S)), 6], (line, M)
    assert _run(driver_san, ["refusals"]).returncode == 0
    r = _run(driver_san, ["dd"])                        # the double-double functions of the fit against long double
    assert r.returncode == 0 and r.stdout.strip().endswith("| ok")
    rng = np.random.default_rng(5)
    cases = [rng.normal(size=1351), np.zeros(300), np.r_[np.full(60, -2.0), rng.normal(size=197)], np.r_[-0.0, 0.0, rng.normal(size=98)],
             np.r_[np.nan, -np.inf, np.inf, -np.nan, rng.normal(size=40)], np.array([1.5]), rng.normal(size=20), np.repeat(rng.normal(size=50), 9)]
    paths = []
    for i, x in enumerate(cases):
        paths.append(os.path.join(str(tmp_path), f"x{i}.f64"))
        np.ascontiguousarray(x, dtype=np.float64).tofile(paths[-1])
    r = _run(driver_san, ["select"] + paths)
    assert r.returncode == 0
    for x, line in zip(cases, [l for l in r.stdout.splitlines() if l.startswith("select ")]):
        want = R.psis_statement(x)
        key, below, equal = line.split("|")[1].split()
        ky = np.sort(R.keys(x))
        assert line.endswith("| ok") and int(key, 16) == int(ky[min(want["M"] + 1, x.size) - 1]) and (int(below), int(equal)) == (want["n_below"], want["n_equal"]), (line, want["M"])


# ---- the law (the restatement only; the device never enters) -----------------------------------------------------------------------------
# k-hat of the restatement over the seeds 0 ... 199 at S = 40 000 (M = 600): mean and standard deviation (ddof = 1).  The band is four
# standard deviations: a property of the estimator at this S, which covers its bias (below a fifth of a standard deviation everywhere).
#   r = U^(-k):          k = 0.2: 0.2088, 0.0475    k = 0.5: 0.5034, 0.0609    k = 0.9: 0.8962, 0.0787
#   k = -0.3: U^(0.3) is bounded by 1 and its density stays positive there, so its tail has shape -1 (after the prior adjustment
#   (-M + 5) / (M + 10) = -0.975), not -0.3: measured -0.9452, 0.0348.  The generalised Pareto law of shape -0.3 itself,
#   r = 1 + (U^(-k) - 1) / k: -0.2837, 0.0294.  Both are checked.
LAW_SEEDS = (1001, 1002, 1003)
LAW = ((R.pareto_ratios, 0.2, 0.2, 0.0475), (R.pareto_ratios, 0.5, 0.5, 0.0609), (R.pareto_ratios, 0.9, 0.9, 0.0787), (R.pareto_ratios, -0.3, -0.975, 0.0348),
       (R.gpd_ratios, -0.3, -0.3, 0.0294))


@pytest.mark.parametrize("gen,k,expect,sd", LAW)
def test_khat_recovers_the_shape_of_an_exact_pareto_tail(gen, k, expect, sd):
    for seed in LAW_SEEDS:
        r = R.psis_statement(gen(k, 40000, seed))
        print(gen.__name__, k, seed, "khat", float(r["khat"]), "expected", expect, "band", 4 * sd, "sigma", float(r["sigma"]), "n_capped", r["n_capped"])
        assert r["status"] == R.FITTED and r["tail_len"] == 600
        assert abs(float(r["khat"]) - expect) <= 4 * sd


# The conjugate Normal model y_i ~ N(mu, 1), mu ~ N(0, 2) on these seven observations (the last one far out): S = 4 000 exact posterior
# draws.  The Monte Carlo standard error of elpd_loo_psis per observation is the replicate spread of the restatement over the seeds
# 1000 ... 1199 (ddof = 1); over those 200 replicates the mean sits within 0.18 standard errors of the exact value at every observation.
NORMAL_Y = (-1.1, -0.3, 0.2, 0.4, 0.9, 1.6, 3.5)
NORMAL_SE = (0.01703455916884995, 0.008473006484178263, 0.00446828139482621, 0.003136287298739524, 0.002000298878916051, 0.006200115312735649, 0.03060255847451785)
NORMAL_SEEDS = (5001, 5002, 5003)


def test_elpd_loo_psis_of_the_conjugate_normal_model_is_the_exact_leave_one_out_density():
    y = np.array(NORMAL_Y)
    mean, sd, exact = R.normal_loo_exact(y, 1.0, 2.0)
    for seed in NORMAL_SEEDS:
        mu = np.random.default_rng(seed).normal(mean, sd, size=4000)
        ll = -0.5 * (y[None, :] - mu[:, None]) ** 2 - 0.5 * math.log(2.0 * math.pi)
        for i in range(y.size):
            r = R.psis_statement(ll[:, i])
            err = abs(float(r["elpd_loo_psis"]) - exact[i])
            print(f"seed {seed} y {y[i]}: elpd_loo_psis {float(r['elpd_loo_psis'])!r} exact {exact[i]!r}: {err / NORMAL_SE[i]:.2f} standard errors, khat {float(r['khat']):.3f}")
            assert r["status"] == R.FITTED and err <= 4.0 * NORMAL_SE[i]


# ---- conventions -----------------------------------------------------------------------------------------------------------------------
def test_non_finite_cells():
    x = R.table(4, 60, 1, 3)[:, 0, :].reshape(-1)
    base = R.psis_statement(x)
    a = x.copy(); a[17] = np.nan
    r = R.psis_statement(a)
    assert r["status"] == R.NONFINITE and r["n_nan"] == 1 and all(math.isnan(float(r[k])) for k in R.WORD_NAMES if k != "khat_threshold")
    b = x.copy(); b[17] = -np.inf
    r = R.psis_statement(b)
    assert r["status"] == R.NONFINITE and r["n_neg_inf"] == 1 and float(r["elpd_loo_psis"]) == -np.inf and float(r["khat"]) == np.inf and math.isfinite(float(r["lppd"]))
    c = x.copy(); c[int(np.argmax(x))] = np.inf            # ratio 0: it lies in the body and adds nothing to its sum
    r = R.psis_statement(c)
    assert r["status"] == R.FITTED and r["n_pos_inf"] == 1 and float(r["lppd"]) == np.inf and np.array_equal(r["tail"], base["tail"]) and float(r["khat"]) == float(base["khat"])
    assert float(r["body_sum"]) <= float(base["body_sum"]) and math.isfinite(float(r["elpd_loo_psis"]))


def test_the_two_statuses_without_a_fit_give_the_raw_estimate():
    rng = np.random.default_rng(2)
    for x, status in ((rng.normal(size=20), R.TOO_FEW), (np.full(400, -1.25), R.DEGENERATE), (np.r_[np.full(R.tail_len(400) + 3, -3.0), rng.normal(size=400 - R.tail_len(400) - 3)], R.DEGENERATE)):
        r = R.psis_statement(x)
        raw = -(math.log(np.sum(np.exp(-x - np.max(-x)))) + np.max(-x) - math.log(x.size))           # -ln((1/N) sum exp(-x)), DESIGN 3.16
        print(status, float(r["elpd_loo_psis"]), raw, float(r["khat"]))
        assert r["status"] == status and float(r["khat"]) == np.inf and r["n_capped"] == 0 and float(r["tail_num"]) == r["tail_len"]
        assert abs(float(r["elpd_loo_psis"]) - raw) <= 64 * R.EPS * max(1.0, abs(raw))
    assert R.psis_statement(rng.normal(size=21))["status"] == R.FITTED and R.tail_len(21) == 5 and R.tail_len(20) == 4


def test_a_tail_heavier_than_one_is_capped():
    r = R.psis_statement(R.pareto_ratios(1.5, 4000, 3))
    print(float(r["khat"]), r["n_capped"])
    assert r["status"] == R.FITTED and float(r["khat"]) > 1.0 and r["n_capped"] > 0


def test_the_plan_sums_are_sums():
    rng = np.random.default_rng(0)
    for S in (1, 63, 257, 4097, 70001):
        v = rng.uniform(size=S)
        assert abs(float(R.cell_sum(v)) - math.fsum(v)) <= R.cell_depth(S) * R.EPS * math.fsum(v)
        assert abs(float(R.tail_sum(v)) - math.fsum(v)) <= R.tail_depth(S) * R.EPS * math.fsum(v)
        assert float(R.cell_sum(np.ones(S))) == S == float(R.tail_sum(np.ones(S)))


# ---- the ABI and the Python layer --------------------------------------------------------------------------------------------------------
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
    assert "#define FG_ABI_VERSION 1" in header


def test_python_layer_without_a_device():
    import fugue_amd as F
    from fugue_amd import comparison as CM
    z = np.zeros(2)
    ps = CM.PsisLoo(names=["a", "b"], n_draws=100, elpd_loo_psis=np.array([-1.0, -2.5]), p_loo_psis=np.array([0.1, 0.2]), khat=np.array([0.3, np.inf]), sigma=z,
                    khat_threshold=np.array([0.5, 0.5]), lppd=z, tail_len=z, status=np.array([0, 2]), n_capped=z, n_neg_inf=z, n_pos_inf=z, n_nan=z)
    assert ps.elpd_loo_psis_total == -3.5 and abs(ps.p_loo_psis_total - 0.3) < 1e-15 and ps.n_bad_k() == 1 and ps.n_sel == 2
    assert ps.se() == math.sqrt(2 * np.var([-1.0, -2.5], ddof=1)) and ps.status_words() == ["fitted", "degenerate tail"]
    with pytest.raises(ValueError, match="no pointwise figure"):
        ps.se("tail_len")
    f8 = {k: np.array([-1.0, -2.0]) for k in CM.POINTWISE}
    mk = lambda psis: CM.PointwiseComparison(names=["a", "b"], n_draws=100, n_neg_inf=z, n_pos_inf=z, n_nan=z, psis=psis, **f8)
    assert mk(None).psis is None
    with pytest.raises(ValueError, match="carry .psis"):
        CM.compare_models(mk(ps), mk(None), which="elpd_loo_psis")
    d, se = CM.compare_models(mk(ps), mk(ps), which="elpd_loo_psis")
    assert d == 0.0 and se == 0.0
    with pytest.raises(ValueError, match="elpd_loo_psis"):
        CM.compare_models(mk(ps), mk(ps), which="khat")
    assert F.PsisLoo is CM.PsisLoo and F.psis_loo is CM.psis_loo
    with pytest.raises(ValueError, match=r"\[n\]\[n_sel\]\[C\]"):
        CM.psis_loo(np.zeros((3, 4)))
