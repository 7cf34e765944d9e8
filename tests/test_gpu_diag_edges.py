"""GPU parity of the diagnostics kernels (fg_diag.hip, fg_diag_host.cpp) at the shapes where they can go wrong: several blocks
of chains, wave and block boundaries, one chain, deep Geyer windows, the lag caps, ill-conditioned and non-finite draws.

Synthetic draws from seeded numpy generators (tests/diag_reference.py) are uploaded into a device buffer; the `d` handed to the
diagnostics calls is independent of the engine's model.  Every input has d = 3 visibly different columns (offset, scale,
autocorrelation), so a coordinate-stride mix-up shows.  There is no knife-edge allowance: every decision in these formulas is
continuous in its inputs, or is pinned on the CPU by tests/test_diag_reference_cpu.py.  Every compared figure is printed.

A constant column of 0.1 is deliberately NOT among the inputs: 0.1 is not exactly summable, so the reference's own sums of
squared deviations there are rounding noise (R-hat and ESS switch between the degenerate rule and a ratio of two roundings
depending on the summation order), and there is nothing to be equal to.  The constant columns used here hold 2.5, -4.0,
1024.5 and -50.0, whose sums and means are exact in every order."""
import math

import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import workloads as W
from tests import diag_reference as R

pytestmark = pytest.mark.gpu

FIGURES = ("r_hat", "ess", "mean", "std")
ABS_TOL = dict(r_hat=0.0, ess=0.0, mean=1e-12, std=0.0)          # test_native_rhat_ess_entry_point_and_geweke's abs on the mean
MODES = [pytest.param(E.DIAG_REDUCE, id="reduce"), pytest.param(E.DIAG_GATHER, id="gather")]


class _Engines:
    """One engine per chain count for the whole module (the model does not matter to the diagnostics calls)."""

    def __init__(self):
        self.cp, self.by_c = E.compile_model(W.normal_sites(1)), {}

    def get(self, C: int):
        if C not in self.by_c:
            self.by_c[C] = E.Engine(self.cp, C, seed=1)
        return self.by_c[C]

    def close(self):
        for e in self.by_c.values():
            e.close()


@pytest.fixture(scope="module")
def engines():
    pool = _Engines()
    yield pool
    pool.close()


class _Draws:
    """x [n][d][C] in a device buffer of the engine with C chains."""

    def __init__(self, engines, x):
        self.x = np.ascontiguousarray(x, dtype=np.float64)
        self.n, self.d, self.C = self.x.shape
        self.eng = engines.get(self.C)
        self.ptr = self.eng.device_alloc(self.x.nbytes)
        E._check(E.lib().fg_device_upload(self.eng.h, self.ptr, self.x.ctypes.data, self.x.nbytes))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.eng.device_free(self.ptr)

    def moments_ptr(self):
        p = self.eng.device_alloc(self.d * 6 * self.C * 8)
        self.eng.diag_chain_moments(self.ptr, self.n, self.d, p)
        return p


def _chains(col):
    return np.ascontiguousarray(np.asarray(col).T)


_oracle_cache = {}


def _oracle_figures(oracle, key, x):
    """The oracle's four figures per column of x, computed once per input and shared by both exchange modes."""
    if key not in _oracle_cache:
        rows = []
        for i in range(x.shape[1]):
            ch = _chains(x[:, i, :])
            s = oracle.summarize(ch)
            rows.append(dict(r_hat=oracle.split_rhat(ch), ess=oracle.ess_multichain(ch), mean=s["mean"], std=s["std"]))
        _oracle_cache[key] = rows
    return _oracle_cache[key]


def _same(got: float, want: float, rel: float, abs_: float = 0.0) -> bool:
    """The class of `want` (NaN, +inf, -inf) and, where finite, its value within max(rel |want|, abs_)."""
    if math.isnan(want) or math.isinf(want):
        return (math.isnan(got) and math.isnan(want)) or got == want
    return math.isfinite(got) and abs(got - want) <= max(rel * abs(want), abs_)


# ---- per-chain moments ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [1, 63, 64, 65, 255, 256, 257, 600])
def test_chain_moments_are_the_in_order_sums_bit_for_bit(engines, C):
    """fg_diag_chain_moments == the in-order float64 forms, every bit, at one chain, around the wave (64) and block (256)
    boundaries and over three blocks; n = 1 (NaN half means), the smallest halves, odd n (the last draw outside both halves), and
    n past a lag chunk."""
    full = R.three_columns(100 + C, 64, C)
    for n in (1, 2, 3, 4, 5, 33, 64):
        with _Draws(engines, full[:n]) as D:
            p = D.moments_ptr()
            got = D.eng.download(p, (3, 6, C))
            D.eng.device_free(p)
        want = R.chain_moments_inorder(full[:n])
        diff = np.nanmax(np.abs(got - want))
        print(f"moments C={C} n={n}: max |engine - in-order| = {diff:.3e}, NaN entries {int(np.isnan(got).sum())}")
        assert np.array_equal(got, want, equal_nan=True)
        assert np.isnan(got[:, [2, 4]]).all() == (n == 1) and not np.isnan(got[:, [0, 1, 3, 5]]).any()


# ---- pooled lag sums -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [33, 65, 100])
def test_single_chain_lag_sums_are_the_in_order_autocovariance_bit_for_bit(engines, n):
    """C = 1: every other lane adds +0.0, so fg_diag_autocov_sums must return the chain's in-order autocovariance itself, at every
    lag 0 ... n - 1 -- across the chunk edges at 32, 64 and 96, including last chunks that hold one, one and four lags."""
    x = R.three_columns(200 + n, n, 1)
    with _Draws(engines, x) as D:
        p = D.moments_ptr()
        got = D.eng.diag_autocov_sums(D.ptr, n, 3, p, 0, n)
        tail = D.eng.diag_autocov_sums(D.ptr, n, 3, p, n - 1, 1)             # a chunk that starts at the last lag
        D.eng.device_free(p)
    want = np.stack([R.chain_autocov_inorder(x, lag)[:, 0] for lag in range(n)], axis=1)
    print(f"lag sums C=1 n={n}: max |engine - in-order| = {np.abs(got - want).max():.3e} over {got.size} values; lag 0 {got[:, 0]}, lag n-1 {got[:, -1]}")
    assert np.array_equal(got, want) and np.array_equal(tail[:, 0], want[:, -1])


@pytest.mark.parametrize("C", [65, 257, 600])
def test_pooled_lag_sums_stay_within_the_bound_of_the_summation_tree(engines, C):
    """C > 1: the per-chain values are the in-order ones (pinned above); they are added in a fixed tree with at most 6 shuffle adds,
    3 wave adds and nblk block adds on any path.  So the result lies within (9 + nblk) 2^-52 sum_c |acov_c| of the exact (fsum) sum
    of the in-order values -- a bound from that count, with nblk = 1, 2, 3 here."""
    n = 40
    x = R.three_columns(300 + C, n, C, phis=(0.9, 0.5, -0.6))
    with _Draws(engines, x) as D:
        p = D.moments_ptr()
        got = D.eng.diag_autocov_sums(D.ptr, n, 3, p, 0, n)
        D.eng.device_free(p)
    worst = 0.0
    for lag in range(n):
        centre, scale = R.pooled_autocov_fsum(x, lag)
        bound = R.pooled_autocov_bound(C, scale)
        ratio = np.abs(got[:, lag] - centre) / bound
        worst = max(worst, ratio.max())
        assert (ratio <= 1.0).all(), (lag, got[:, lag], centre, bound)
    print(f"pooled lag sums C={C} (nblk={(C + 255) // 256}) n={n}: worst |engine - fsum| / bound = {worst:.3f}")


# ---- fg_diag_rhat_ess against the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("exchange", MODES)
@pytest.mark.parametrize("name", R.RHAT_ESS_CASES)
def test_rhat_ess_edge_inputs_match_the_oracle(oracle, engines, name, exchange):
    """Cases a-h of tests/diag_reference.rhat_ess_case (what each reaches is proven in tests/test_diag_reference_cpu.py): multi-block
    sums, a window many chunks deep, the cap of 2 048 lags, the monotone correction, n - 1 = 31 / 32 / 33, the n < 4 rule and one
    chain, tau clamped at 1, constant columns.  Tolerances of test_native_rhat_ess_entry_point_and_geweke."""
    x = R.rhat_ess_case(name)
    n, d, C = x.shape
    want = _oracle_figures(oracle, name, x)
    with _Draws(engines, x) as D:
        r = D.eng.diag_rhat_ess(D.ptr, n, d, exchange=exchange)
    assert r["chains"] == C
    for i in range(d):
        for k in FIGURES:
            print(f"{name}[{i}] {k}: engine {r[k][i]!r} oracle {want[i][k]!r}")
    for i in range(d):
        for k in FIGURES:
            assert _same(float(r[k][i]), want[i][k], R.FIGURE_TOL[k], ABS_TOL[k]), (name, i, k, r[k][i], want[i][k])
        if name in ("g_antithetic", "h_constant") or n < 4:
            assert r["ess"][i] == float(C * n)                                  # tau clamped to 1 / every draw counts: exactly m n
        if name == "h_constant":
            assert math.isnan(r["r_hat"][i]) and r["mean"][i] == x[0, i, 0] and r["std"][i] == 0.0


# ---- conditioning -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exchange", MODES)
@pytest.mark.parametrize("figure", FIGURES)
def test_rhat_ess_on_ill_conditioned_draws(oracle, engines, figure, exchange):
    """Draws 1e8 + 1e-3 N(0, 1), C = 300, n = 200, against the high-precision forms.  Tolerance per figure: the larger of the usual
    one and 4 x the oracle's own deviation from the high-precision value on the same input (measured on the CPU, from the oracle
    alone): the oracle is another rounding path of the same conditioning -- the engine pools chain means where the reference
    sums every value, and the reduce mode sums per block, hence the small margin.

    This input found a loss in the pooled std: sqrt((sum_j ssd_j + n sum_j (mean_j - mean)^2) / (m n - 1)) is an identity only for exact
    chain means, and the in-order mean of 200 values near 1e8 is off by ~8e-8, a thousandth of the spread of the chain means.  Without
    the cross term 2 sum_j (mean_j - mean) sum_t (x_t - mean_j) the std deviated 2.6e-7 / 2.3e-7 / 1.6e-7 per column (oracle 2.8e-8 /
    8.4e-8 / 3.4e-9); fg_diag_rhat_ess now adds it (k_diag_std_cross) and lands within 1e-9."""
    x = R.conditioning_input()
    n, d, C = x.shape
    tol = R.conditioning_tolerance(oracle, x)
    with _Draws(engines, x) as D:
        r = D.eng.diag_rhat_ess(D.ptr, n, d, exchange=exchange)
    bad = []
    for i in range(d):
        hp = R.stats_hp(x[:, i, :])[figure]
        t, odev = tol[i][figure]
        dev = abs(float(r[figure][i]) - hp) / abs(hp)
        print(f"conditioning[{i}] {figure}: engine {r[figure][i]!r} high-precision {hp!r}; engine deviation {dev:.3e}, oracle deviation {odev:.3e}, tolerance {t:.3e}")
        if not dev <= t:
            bad.append((i, dev, t))
    assert not bad, bad


# ---- non-finite draws -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exchange", MODES)
def test_one_non_finite_draw_follows_the_reference(oracle, engines, exchange):
    """One NaN in one chain of column 0, one +inf in one chain of column 1, column 2 clean: column 2 does not change a bit, and
    columns 0 and 1 have the oracle's values by class and, where finite, by value -- in particular ESS = m n: f64::max(NaN, 1.0) is
    1.0 (mcmc_utils.rs:337)."""
    clean, dirty = R.nonfinite_input()
    n, d, C = dirty.shape
    want = _oracle_figures(oracle, "nonfinite", dirty)
    with _Draws(engines, clean) as D:
        r0 = D.eng.diag_rhat_ess(D.ptr, n, d, exchange=exchange)
    with _Draws(engines, dirty) as D:
        r = D.eng.diag_rhat_ess(D.ptr, n, d, exchange=exchange)
    for i in range(d):
        for k in FIGURES:
            print(f"nonfinite[{i}] {k}: engine {r[k][i]!r} oracle {want[i][k]!r} (clean input: {r0[k][i]!r})")
    for k in FIGURES:
        assert r[k][2] == r0[k][2] and math.isfinite(r[k][2])
        for i in (0, 1):
            assert _same(float(r[k][i]), want[i][k], R.FIGURE_TOL[k], ABS_TOL[k]), (i, k, r[k][i], want[i][k])
    assert r["ess"][0] == r["ess"][1] == float(C * n)
    assert math.isnan(r["mean"][0]) and r["mean"][1] == math.inf and math.isnan(r["std"][0]) and math.isnan(r["std"][1])


# ---- Geweke -------------------------------------------------------------------------------------------------------------------
def _assert_geweke(oracle, x, z, label):
    n, d, C = x.shape
    want = np.array([[oracle.geweke(np.ascontiguousarray(x[:, i, c])) for c in range(C)] for i in range(d)])
    assert np.array_equal(np.isnan(z), np.isnan(want)), label
    err = np.abs(z - want)
    ok = np.isnan(want) | (err <= np.maximum(1e-9 * np.abs(want), 1e-12))
    finite = err[~np.isnan(err)]
    print(f"geweke {label}: {want.size} columns, NaN {int(np.isnan(want).sum())}, max |engine - oracle| = {finite.max() if finite.size else 0.0:.3e},"
          f" chain 0: engine {z[:, 0]} oracle {want[:, 0]}")
    assert ok.all(), (label, np.argwhere(~ok)[:5], z[~ok][:5], want[~ok][:5])
    return want


@pytest.mark.parametrize("C", [1, 65, 257])
def test_geweke_at_its_boundaries(oracle, engines, C):
    """fg_diag_geweke on EVERY (coordinate, chain) column: n = 19 (NaN) / 20 / 21 (segments of 2 draws), 39 / 40 (3 -> 4 draws);
    a column constant on its first 10 % only (that segment's variance term is 0, z is not); a fully constant column (se = 0: z = 0)."""
    for n in (19, 20, 21, 39, 40):
        x = R.geweke_input(n, C)
        with _Draws(engines, x) as D:
            z = D.eng.diag_geweke(D.ptr, n, 3)
        want = _assert_geweke(oracle, x, z, f"C={C} n={n}")
        assert np.isnan(z).all() == (n < 20)
        if n >= 20:
            assert (z[2] == 0.0).all() and (z[:2] != 0.0).all() and np.isfinite(want).all()


def test_geweke_lag_cap(oracle, engines):
    """A ramp plus small noise, n = 7 200: the last segment's autocorrelation is still positive at lag 1 024, so
    fg_spectral_var_of_mean's cap ends the sum (proven for this input in test_geweke_inputs_reach_their_paths: summing on changes z
    by 2 %)."""
    x = R.geweke_cap_input()
    n, d, C = x.shape
    with _Draws(engines, x) as D:
        z = D.eng.diag_geweke(D.ptr, n, d)
    _assert_geweke(oracle, x, z, f"cap C={C} n={n}")
    print(f"geweke cap z: {z.tolist()}")


# ---- quantiles ----------------------------------------------------------------------------------------------------------------
def _host_quantiles(col, probs):
    v = np.sort(np.asarray(col).ravel())
    return np.array([v[int(math.floor((len(v) - 1) * p + 0.5))] for p in probs])


PROBS8 = (0.0, 0.001, 0.025, 0.25, 0.5, 0.75, 0.975, 1.0)


def test_quantiles_beyond_one_grid_trip(engines):
    """n = 257, C = 4 100, d = 1: 1 053 700 elements, more than the 4 096 x 256 threads of k_diag_qhist's grid, so the grid-stride
    loop takes a second trip; eight probabilities (the most the kernel holds) against a host sort, bit for bit; nine are refused."""
    rng = np.random.default_rng(257)
    x = rng.standard_normal((257, 1, 4100)) * 3.0 - 1.0
    assert x.size > 4096 * 256
    with _Draws(engines, x) as D:
        q = D.eng.diag_quantiles(D.ptr, 257, 1, PROBS8)
        with pytest.raises(E.EngineError) as err:
            D.eng.diag_quantiles(D.ptr, 257, 1, PROBS8 + (0.9,))
    want = _host_quantiles(x, PROBS8)
    print(f"quantiles 257 x 4100: engine {q[0].tolist()} host sort {want.tolist()}")
    assert err.value.code == E.FG_E_BAD_ARG
    assert q[0].view(np.uint64).tolist() == want.view(np.uint64).tolist()


def test_quantiles_decided_in_the_last_key_byte(engines):
    """Column 0: 1.0 + k 2^-52, k = 0 ... 255 repeated -- the values share the seven upper key bytes, ranks are decided in pass 7
    only.  Column 1: all negative (the inverted keys).  Column 2: an ordinary column next to them."""
    n, C = 97, 130
    rng = np.random.default_rng(97)
    x = np.empty((n, 3, C))
    x[:, 0] = 1.0 + (np.arange(n * C) % 256).reshape(n, C) * 2.0 ** -52
    x[:, 1] = -np.abs(rng.standard_normal((n, C))) - 1e-3
    x[:, 2] = rng.standard_normal((n, C)) * 20.0 - 50.0
    assert len(np.unique(x[:, 0])) == 256 and (x[:, 1] < 0).all()
    with _Draws(engines, x) as D:
        q = D.eng.diag_quantiles(D.ptr, n, 3, PROBS8)
    for i in range(3):
        want = _host_quantiles(x[:, i], PROBS8)
        print(f"quantiles column {i}: engine {[v.hex() for v in q[i].tolist()]} host sort {[v.hex() for v in want.tolist()]}")
        assert q[i].view(np.uint64).tolist() == want.view(np.uint64).tolist()
    assert len(set(q[0].tolist())) == len(PROBS8) - 1       # seven values that differ in the last byte only (ranks 0 and 13 both fall on the ~50 copies of 1.0)
