"""GPU tests of the chunked diagnostics (fg_diag_stream.hip): the device state against its numpy restatement bit for bit and under
every chunking, the figures against the oracle in both exchange modes, the lag limit as an error, ill-conditioned draws against
the high-precision forms, the edges, and the two summary drivers against the stored-draws drivers.

Synthetic draws are uploaded once with Engine.upload; a chunk is a slice [n_c][d][C] of that buffer.  Every compared figure is
printed before it is asserted."""
import ctypes
import math

import numpy as np
import pytest

from fugue_amd import diagnostics as D
from fugue_amd import engine as E
from fugue_amd import inference as I
from fugue_amd import workloads as W
from tests import diag_reference as R
from tests.stream_diag_restatement import ar1_input, oracle_figures, restate

pytestmark = pytest.mark.gpu

FIGURES = ("r_hat", "ess", "mean", "std")
ABS_TOL = dict(r_hat=0.0, ess=0.0, mean=1e-12, std=0.0)          # tests/test_gpu_diag.py's abs on the mean
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


class _Streamed:
    """x [n][d][C] uploaded once and fed to a stream of K lags in `chunks` (lengths; default: one chunk)."""

    def __init__(self, engines, x, K, chunks=None):
        self.x = np.ascontiguousarray(x, dtype=np.float64)
        self.n, self.d, self.C = self.x.shape
        self.eng = engines.get(self.C)
        self.ptr = self.eng.upload(self.x)
        self.stream = self.eng.diag_stream(self.n, self.d, K)
        at = 0
        for nc in (chunks or [self.n]):
            assert at + nc <= self.n
            self.stream.update(self.ptr + at * self.d * self.C * 8, nc)
            at += nc
            assert self.stream.count == at

    def __enter__(self):
        return self.stream

    def __exit__(self, *exc):
        self.eng.synchronize()
        self.stream.close()
        self.eng.device_free(self.ptr)


def _same(got: float, want: float, rel: float, abs_: float = 0.0) -> bool:
    """The class of `want` (NaN, +inf, -inf) and, where finite, its value within max(rel |want|, abs_)."""
    if math.isnan(want) or math.isinf(want):
        return (math.isnan(got) and math.isnan(want)) or got == want
    return math.isfinite(got) and abs(got - want) <= max(rel * abs(want), abs_)


def _assert_figures(label, got, want, figures=FIGURES):
    for i, row in enumerate(want):
        for k in figures:
            print(f"{label}[{i}] {k}: stream {got[k][i]!r} reference {row[k]!r}")
    for i, row in enumerate(want):
        for k in figures:
            assert _same(float(got[k][i]), row[k], R.FIGURE_TOL[k], ABS_TOL[k]), (label, i, k, got[k][i], row[k])


CHUNKINGS = {"one": [97], "mixed": [5, 31, 1, 60], "ones": [1] * 97}


# ---- 1. the state, bit for bit -------------------------------------------------------------------------------------------
def test_state_equals_the_restatement_under_every_chunking(engines):
    """n = 97 (odd: halves of 48, draw 96 in neither), d = 3, C = 70 (a full wave and a partial one), K = 32, iid normal draws, cut
    as one chunk, as [5, 31, 1, 60] (a chunk below K, a chunk of one, one across draw 48, one ending on the dropped draw) and as 97
    chunks of one.  moments() must be the restatement's bits and autocov_sums(0, 32) one set of bits under all three; the pooled
    lag sums lie within the summation tree's bound (9 + nblk) 2^-52 sum_c |acov_c| of the fsum of the restated columns."""
    x = np.random.default_rng(97).standard_normal((97, 3, 70))
    want = restate(x, 32)
    mom, acov = {}, {}
    for name, chunks in CHUNKINGS.items():
        with _Streamed(engines, x, 32, chunks) as s:
            mom[name], acov[name] = s.moments(), s.autocov_sums(0, 32)
        print(f"chunking {name}: max |moments - restatement| = {np.abs(mom[name] - want.moments()).max():.3e}")
    for name in CHUNKINGS:
        assert np.array_equal(mom[name], want.moments()), name
        assert np.array_equal(acov[name], acov["one"]), name
    worst = 0.0
    for lag in range(32):
        cols = want.chain_autocov(lag)
        centre = np.array([math.fsum(row) for row in cols])
        bound = R.pooled_autocov_bound(70, np.array([math.fsum(np.abs(row)) for row in cols]))
        ratio = np.abs(acov["one"][:, lag] - centre) / bound
        worst = max(worst, ratio.max())
        assert (ratio <= 1.0).all(), (lag, acov["one"][:, lag], centre, bound)
    print(f"pooled lag sums C=70: worst |stream - fsum| / bound = {worst:.3f}")


def test_single_chain_lag_sums_equal_the_restatement_bit_for_bit(engines):
    """C = 1: every other lane adds +0.0, so autocov_sums(0, 32) is the column's own value -- the restatement's bits, under every
    chunking."""
    x = np.random.default_rng(971).standard_normal((97, 3, 1))
    want = np.stack([restate(x, 32).chain_autocov(lag)[:, 0] for lag in range(32)], axis=1)
    for name, chunks in CHUNKINGS.items():
        with _Streamed(engines, x, 32, chunks) as s:
            got = s.autocov_sums(0, 32)
        print(f"C=1 chunking {name}: max |stream - restatement| = {np.abs(got - want).max():.3e}; lag 0 {got[:, 0]}, lag 31 {got[:, 31]}")
        assert np.array_equal(got, want), name


# ---- 2. against the oracle -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exchange", MODES)
def test_figures_match_the_oracle(oracle, engines, exchange):
    """AR(1) phi = 0.5, n = 200, 5 chains, 2 coordinates, seeds 0-4, K = 32, chunks of 37: rhat_ess() in both exchange modes, and
    the same stream through ChainDiagnostics(StreamMoments), against the oracle at the project's tolerances."""
    for seed in range(5):
        x = ar1_input(seed, 200, 5, 2, 0.5)
        want = oracle_figures(oracle, x)
        with _Streamed(engines, x, 32, [37] * 5 + [15]) as s:
            r = s.rhat_ess(exchange=exchange)
            cd = D.ChainDiagnostics(D.StreamMoments(s), exchange="reduce" if exchange == E.DIAG_REDUCE else "gather").summary()
        assert r["chains"] == 5 and r["exchange_bytes"] == 0
        _assert_figures(f"seed {seed} rhat_ess", r, want)
        _assert_figures(f"seed {seed} ChainDiagnostics", cd, want)
        _assert_figures(f"seed {seed} ChainDiagnostics vs rhat_ess", cd, [{k: float(r[k][i]) for k in FIGURES} for i in range(2)])


# ---- 3. the lag limit ----------------------------------------------------------------------------------------------------
def test_a_lag_beyond_K_is_an_error_never_a_figure(oracle, engines):
    """AR(1) phi = 0.99, n = 400, 4 chains, seeds 0-4: Geyer's sequence runs to lag >= 97 (tests/test_diag_stream_cpu.py).  K = 32:
    rhat_ess() and the ChainDiagnostics path raise FG_E_LIMIT naming K, and without the ESS the other three figures come back;
    K = 416 holds every lag and the ESS matches the oracle."""
    for seed in range(5):
        x = ar1_input(seed, 400, 4, 1, 0.99)
        want = oracle_figures(oracle, x)
        with _Streamed(engines, x, 32, [64] * 6 + [16]) as s:
            with pytest.raises(E.EngineError) as err:
                s.rhat_ess()
            assert err.value.code == E.FG_E_LIMIT and "K = 32" in str(err.value), str(err.value)
            with pytest.raises(E.EngineError) as err:
                D.ChainDiagnostics(D.StreamMoments(s)).ess()
            assert err.value.code == E.FG_E_LIMIT
            with pytest.raises(E.EngineError) as err:
                s.autocov_sums(0, 33)
            assert err.value.code == E.FG_E_LIMIT
            r = s.rhat_ess(want_ess=False)
        assert r["ess"] is None
        _assert_figures(f"seed {seed} K=32 without ESS", r, want, ("r_hat", "mean", "std"))
        with _Streamed(engines, x, 416, [64] * 6 + [16]) as s:
            assert s.K == 416
            r = s.rhat_ess()
            tail = s.autocov_sums(399, 3)
        _assert_figures(f"seed {seed} K=416", r, want)
        assert tail[0, 0] != 0.0 and tail[0, 1] == 0.0 and tail[0, 2] == 0.0          # lags >= n_total are 0


# ---- 4. conditioning -----------------------------------------------------------------------------------------------------
_cond = {}


@pytest.mark.parametrize("exchange", MODES)
def test_ill_conditioned_draws(oracle, engines, exchange):
    """Draws 1e8 + 1e-3 N(0, 1), C = 300, n = 200 -- the input and the per-figure tolerances of
    test_rhat_ess_on_ill_conditioned_draws (the larger of the usual one and 4 x the oracle's own deviation from the high-precision
    forms).  The pivot takes the 1e8 out before anything is squared; the pooled std gets the residual row of k_diag_stream_moments
    (zeros would leave column 2 at 1.7e-8 against a tolerance of 1.4e-8, tests/test_diag_stream_cpu.py)."""
    x = R.conditioning_input()
    n, d, C = x.shape
    if not _cond:
        _cond["tol"] = R.conditioning_tolerance(oracle, x)
        _cond["hp"] = [R.stats_hp(x[:, i, :]) for i in range(d)]
    with _Streamed(engines, x, 224, [64, 64, 64, 8]) as s:
        r = s.rhat_ess(exchange=exchange)
    bad = []
    for i in range(d):
        for k in FIGURES:
            hp = _cond["hp"][i][k]
            t, odev = _cond["tol"][i][k]
            dev = abs(float(r[k][i]) - hp) / abs(hp)
            print(f"conditioning[{i}] {k}: stream {r[k][i]!r} high-precision {hp!r}; stream deviation {dev:.3e}, oracle deviation {odev:.3e}, tolerance {t:.3e}")
            if not dev <= t:
                bad.append((i, k, dev, t))
    assert not bad, bad


# ---- 5. edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["f_n3_c2", "f_n4_c2", "f_n3_c1", "f_n5_c2", "h_constant"])
def test_small_runs_and_constant_columns(oracle, engines, name):
    """n_total = 3 (the small-sample rule ESS = m n), 4 and 5 (the first lengths with a Geyer loop), one chain, and exactly summable
    constant columns (mean_var <= 0: ESS = m n, R-hat NaN as the oracle gives); one draw per chunk."""
    x = R.rhat_ess_case(name)
    n, d, C = x.shape
    want = oracle_figures(oracle, x)
    with _Streamed(engines, x, 32, [1] * n) as s:
        r = s.rhat_ess()
    _assert_figures(name, r, want)
    if name == "h_constant" or n < 4:
        assert (r["ess"] == float(C * n)).all()
    if name == "h_constant":
        assert np.isnan(r["r_hat"]).all() and np.array_equal(r["mean"], x[0, :, 0]) and (r["std"] == 0.0).all()


def test_one_non_finite_draw_stays_in_its_coordinate(oracle, engines):
    """One NaN in one chain of column 0, one +inf in one chain of column 1, column 2 clean (tests/diag_reference.nonfinite_input):
    column 2 does not change a bit; R-hat, mean and std of columns 0 and 1 are non-finite.  Their ESS is the oracle's m n: the
    combination is the stored-draws one, and there f64::max(NaN, 1.0) = 1.0 clamps tau (mcmc_utils.rs:337), so that one figure is
    finite by the reference's own rule.  K = 96 >= n - 1: a NaN never ends Geyer's sequence, every lag is asked for."""
    clean, dirty = R.nonfinite_input()
    n, d, C = dirty.shape
    want = oracle_figures(oracle, dirty)
    with _Streamed(engines, clean, 96, [40, 56]) as s:
        r0 = s.rhat_ess()
    with _Streamed(engines, dirty, 96, [40, 56]) as s:
        r = s.rhat_ess()
    for i in range(d):
        for k in FIGURES:
            print(f"nonfinite[{i}] {k}: stream {r[k][i]!r} oracle {want[i][k]!r} (clean input: {r0[k][i]!r})")
    for k in FIGURES:
        assert r[k][2] == r0[k][2] and math.isfinite(r[k][2])
    for i in (0, 1):
        for k in ("r_hat", "mean", "std"):
            assert not math.isfinite(r[k][i]), (i, k, r[k][i])
        assert r["ess"][i] == want[i]["ess"] == float(C * n)


def test_call_order_and_arguments_are_checked(engines):
    eng = engines.get(70)
    x = np.random.default_rng(5).standard_normal((10, 2, 70))
    ptr = eng.upload(x)
    s = eng.diag_stream(10, 2, 32)
    try:
        s.update(ptr, 6)
        for call in (s.moments, lambda: s.autocov_sums(0, 4), s.rhat_ess):          # read-outs before the end
            with pytest.raises(E.EngineError) as err:
                call()
            assert err.value.code == E.FG_E_STATE, str(err.value)
        with pytest.raises(E.EngineError) as err:                                    # an update that would pass n_total
            s.update(ptr, 5)
        assert err.value.code == E.FG_E_STATE and s.count == 6
        with pytest.raises(E.EngineError) as err:
            s.update(ptr, 0)
        assert err.value.code == E.FG_E_BAD_ARG
        s.update(ptr + 6 * 2 * 70 * 8, 4)
        assert s.count == 10 and s.moments().shape == (2, 6, 70)
        with pytest.raises(E.EngineError) as err:
            s.update(ptr, 1)
        assert err.value.code == E.FG_E_STATE
    finally:
        eng.synchronize()
        s.close()
        eng.device_free(ptr)
    out = ctypes.c_void_p()
    for args in ((0, 2, 32), (10, 0, 32), (10, 70000, 32), (10, 2, 0), (10, 2, 2049)):   # the library's own checks, below the Python ones
        assert E.lib().fg_diag_stream_new(eng.h, *args, ctypes.byref(out)) == E.FG_E_BAD_ARG and not out.value, args


# ---- 6. the drivers --------------------------------------------------------------------------------------------------------
def _stored_figures(chains, sites):
    draws = np.ascontiguousarray(np.stack([chains.get_f64(a) for a in sites], axis=1))         # [n][d][C]
    s = D.ChainDiagnostics(D.HostMoments(draws)).summary()
    return [{k: float(s[k][i]) for k in FIGURES} for i in range(len(sites))]


def test_hmc_chain_summary_matches_the_stored_run():
    """hmc_chain_summary in chunks of 16 (16 + 16 + 16 + 12) against hmc_chain with the same arguments: the same transitions, so
    the sampler's statistics are equal exactly, and the four figures agree with ChainDiagnostics(HostMoments) over the stored draws."""
    a = dict(seed=7, model_fn=W.normal_sites(4), n_samples=60, n_warmup=20, n_chains=128)
    chains = I.hmc_chain(**a)
    summ = I.hmc_chain_summary(chunk=16, **a)
    assert summ.sites == [s for s, v in zip(chains.sites, chains.vtypes) if v == 0] and (summ.n_samples, summ.n_chains) == (60, 128)
    print(f"hmc: accept_rate {summ.accept_rate!r} / {chains.accept_rate!r}, step size {summ.mean_step_size!r} / {chains.mean_step_size!r}, divergent {summ.n_divergent} / {chains.n_divergent}")
    assert (summ.accept_rate, summ.mean_step_size, summ.n_divergent) == (chains.accept_rate, chains.mean_step_size, chains.n_divergent)
    _assert_figures("hmc_chain_summary", dict(r_hat=summ.r_hat, ess=summ.ess, mean=summ.mean, std=summ.std), _stored_figures(chains, summ.sites))


def test_adaptive_mcmc_chain_summary_matches_the_stored_run():
    """The same for adaptive_mcmc_chain_summary on reference_model(4), f64 sites only."""
    a = dict(seed=7, model_fn=W.reference_model(4), n_samples=60, n_warmup=20, n_chains=128)
    chains = I.adaptive_mcmc_chain(**a)
    summ = I.adaptive_mcmc_chain_summary(chunk=16, **a)
    assert summ.sites == [s for s, v in zip(chains.sites, chains.vtypes) if v == 0] and (summ.n_samples, summ.n_chains) == (60, 128)
    print(f"mh: accept_rate {summ.accept_rate!r} / {chains.accept_rate!r}")
    assert summ.accept_rate == chains.accept_rate and math.isnan(summ.mean_step_size) and summ.n_divergent == 0
    _assert_figures("adaptive_mcmc_chain_summary", dict(r_hat=summ.r_hat, ess=summ.ess, mean=summ.mean, std=summ.std), _stored_figures(chains, summ.sites))
