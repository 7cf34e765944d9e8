"""tests/diag_reference.py pinned on the CPU: its high-precision forms against the oracle on well-conditioned inputs, its
in-order forms against its high-precision forms, and -- from the reference alone -- that every adversarial input of
tests/test_gpu_diag_edges.py reaches the path it is named for."""
import math

import numpy as np
import pytest

from tests import diag_reference as R


def _chains(col):                          # [n][C] -> [m][n] for the oracle
    return np.ascontiguousarray(np.asarray(col).T)


def test_extended_precision_is_available():
    """The high-precision forms lean on an x87-style long double (64-bit significand)."""
    assert np.finfo(np.longdouble).nmant >= 63


@pytest.mark.parametrize("n", [7, 50, 401])
def test_high_precision_forms_match_the_oracle(oracle, n):
    """Same inputs and tolerances as test_rhat_and_ess_match_oracle (tests/test_diagnostics_cpu.py)."""
    rng = np.random.default_rng(n)
    draws = np.stack([R.ar1(rng, n, 12, 0.6), rng.standard_normal((n, 12)) * 3 + 1, R.ar1(rng, n, 12, 0.95)], axis=1)
    for i in range(3):
        col, ch = draws[:, i, :], _chains(draws[:, i, :])
        hp, s = R.stats_hp(col), oracle.summarize(ch)
        assert hp["r_hat"] == pytest.approx(oracle.split_rhat(ch), rel=1e-11)
        assert hp["ess"] == pytest.approx(oracle.ess_multichain(ch), rel=1e-9)
        assert hp["mean"] == pytest.approx(s["mean"], rel=1e-11, abs=1e-12)
        assert hp["std"] == pytest.approx(s["std"], rel=1e-10)
        z, _ = R.geweke_hp(ch[0])
        assert z == pytest.approx(oracle.geweke(ch[0]), rel=1e-9, nan_ok=True)


def test_in_order_forms_agree_with_the_high_precision_forms():
    x = R.three_columns(3, 65, 9)
    n = x.shape[0]
    half = n // 2
    mom = R.chain_moments_inorder(x)
    xl = x.astype(np.longdouble)
    for k, (a, b) in enumerate(((0, n), (0, half), (half, 2 * half))):
        mean = xl[a:b].sum(axis=0) / (b - a)
        np.testing.assert_allclose(mom[:, 2 * k], mean.astype(np.float64), rtol=1e-14, atol=1e-15)
        np.testing.assert_allclose(mom[:, 2 * k + 1], ((xl[a:b] - mean) ** 2).sum(axis=0).astype(np.float64), rtol=1e-13)
    c = xl - xl.sum(axis=0) / n
    for lag in (0, 1, 31, 32, 64):
        want = ((c[:n - lag] * c[lag:]).sum(axis=0) / n).astype(np.float64)
        np.testing.assert_allclose(R.chain_autocov_inorder(x, lag), want, rtol=1e-12, atol=1e-13 * np.abs(want).max())
    one = R.chain_moments_inorder(x[:1])
    assert np.isnan(one[:, 2]).all() and np.isnan(one[:, 4]).all() and (one[:, [1, 3, 5]] == 0.0).all()
    assert np.array_equal(one[:, 0], x[0])


def test_in_order_moments_are_the_oracles_sums(oracle):
    """The in-order moments reproduce the oracle's pooled mean bit for bit when the oracle's sum visits one chain (m = 1):
    the same additions in the same order."""
    x = R.three_columns(5, 33, 1)
    mom = R.chain_moments_inorder(x)
    for i in range(3):
        assert mom[i, 0, 0] == oracle.summarize(_chains(x[:, i, :]))["mean"]


@pytest.mark.parametrize("name", R.RHAT_ESS_CASES)
def test_rhat_ess_inputs_reach_their_paths(oracle, name):
    x = R.rhat_ess_case(name)
    n, d, C = x.shape
    assert d == 3
    for i in range(3):
        col, ch = x[:, i, :], _chains(x[:, i, :])
        e = R.ess_hp(col)
        want = oracle.ess_multichain(ch)
        print(f"{name}[{i}] n={n} C={C} max_t={e['max_t']} corrected={e['corrected']} tau={e['tau']:.6g} ess_hp={e['ess']:.9g} oracle={want:.9g}")
        if name != "h_constant":
            assert e["ess"] == pytest.approx(want, rel=1e-8)
            rh, rw = R.split_rhat_hp(col), oracle.split_rhat(ch)
            assert (math.isnan(rh) and math.isnan(rw)) or rh == pytest.approx(rw, rel=1e-10)
        if name == "a_multiblock":
            assert C > 2 * 256 and (i != 0 or e["max_t"] >= 65)                 # three blocks of chains; column 0: three chunks of lags
        elif name == "b_deep_window":
            assert e["max_t"] > 64 and e["max_t"] < min(n - 1, 2048)          # truncates beyond lag 64: at least three chunks of lags
        elif name == "c_cap_2048":
            assert n - 1 > 2048 and e["max_t"] == 2047 and min(e["rho"]) > 0.0
        elif name == "d_monotone":
            assert e["corrected"] >= 1
        elif name.startswith("e_n"):
            assert e["max_t"] == (n - 1 if n % 2 == 0 else n - 2) and min(e["rho"]) > 0.0      # lags come in pairs: the last odd lag <= n - 1
        elif name.startswith("f_n"):
            assert e["ess"] == float(C * n) if n < 4 else 1.0 <= e["ess"] <= C * n
        elif name == "g_antithetic":
            assert e["tau"] < 1.0 and e["ess"] == float(C * n) == want
        elif name == "h_constant":
            assert e["ess"] == float(C * n) == want and math.isnan(oracle.split_rhat(ch)) and math.isnan(R.split_rhat_hp(col))


def test_monotone_correction_changes_the_answer():
    """The d_monotone input is one where dropping the correction gives another ESS: the branch matters."""
    col = R.rhat_ess_case("d_monotone")[:, 0, :]
    e = R.ess_hp(col)
    uncorrected = col.size / max(-1.0 + 2.0 * math.fsum(e["rho"]), 1.0)
    assert abs(uncorrected - e["ess"]) > 1e-3 * e["ess"]


def test_geweke_inputs_reach_their_paths(oracle):
    x = R.geweke_cap_input()
    n, d, C = x.shape
    for i in range(d):
        for c in range(C):
            z, lags = R.geweke_hp(x[:, i, c])
            z_free, lags_free = R.geweke_hp(x[:, i, c], lag_cap=None)
            print(f"geweke cap [{i}][{c}] n={n} lags={lags} z={z:.12g}; cap lifted: lags={lags_free} z={z_free:.12g}")
            assert lags[1] == 1024 and lags[0] < 1024 and lags_free[1] > 1024      # the last segment sums exactly the cap
            assert abs(z - z_free) > 1e-6 * abs(z)                                # ... and the cap binds
            assert z == pytest.approx(oracle.geweke(np.ascontiguousarray(x[:, i, c])), rel=1e-9, abs=1e-12)
    for n in (19, 20, 21, 39, 40):
        x = R.geweke_input(n, 5)
        for i in range(3):
            for c in range(5):
                z, lags = R.geweke_hp(x[:, i, c])
                assert z == pytest.approx(oracle.geweke(np.ascontiguousarray(x[:, i, c])), rel=1e-9, abs=1e-12, nan_ok=True)
                assert math.isnan(z) == (n < 20)
                if n >= 20:
                    assert (i != 2 or z == 0.0) and (i != 1 or lags[0] == 0) and (i == 2 or z != 0.0)
    assert 20 // 10 == 2 and 39 // 10 == 3                                         # segments of 2 and of 3 draws


def test_conditioning_input_and_the_oracles_own_deviation(oracle):
    """1e8 + 1e-3 N(0, 1): the oracle's float64 sums lose digits here; the figure is what the GPU test scales its tolerance by."""
    x = R.conditioning_input()
    assert x.shape == (200, 3, 300) and abs(x.mean() - 1e8) < 100 and x[:, 0].std() == pytest.approx(1e-3, rel=0.05)
    tol = R.conditioning_tolerance(oracle, x)
    for i, row in enumerate(tol):
        for k, (t, dev) in row.items():
            print(f"conditioning[{i}] {k}: oracle deviation {dev:.3e}, tolerance {t:.3e}")
            assert t == max(R.FIGURE_TOL[k], 4.0 * dev) and dev < 1e-3           # deviations of a float64 path, not of a wrong formula
    well = R.oracle_deviation(oracle, R.three_columns(11, 200, 30))
    assert all(v < R.FIGURE_TOL[k] for row in well for k, v in row.items())        # well-conditioned: below the usual tolerances


def test_nonfinite_input_classes(oracle):
    clean, bad = R.nonfinite_input()
    assert np.array_equal(clean[:, 2], bad[:, 2]) and np.isnan(bad[:, 0]).sum() == 1 and np.isinf(bad[:, 1]).sum() == 1
    m_n = float(bad.shape[0] * bad.shape[2])
    for i in (0, 1):
        ch = _chains(bad[:, i, :])
        assert oracle.ess_multichain(ch) == m_n == R.ess_hp(bad[:, i, :])["ess"] and math.isnan(oracle.split_rhat(ch))
    s0, s1 = oracle.summarize(_chains(bad[:, 0, :])), oracle.summarize(_chains(bad[:, 1, :]))
    assert math.isnan(s0["mean"]) and math.isnan(s0["std"]) and s1["mean"] == math.inf and math.isnan(s1["std"])


def test_pooled_autocov_bound_counts_the_tree():
    assert R.pooled_autocov_bound(65, np.array([1.0]))[0] == 10 * 2.0 ** -52
    assert R.pooled_autocov_bound(257, np.array([1.0]))[0] == 11 * 2.0 ** -52
    assert R.pooled_autocov_bound(600, np.array([2.0]))[0] == 12 * 2.0 ** -51
