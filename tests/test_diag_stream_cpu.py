"""The chunked diagnostics state without a GPU: its numpy restatement (tests/stream_diag_restatement.py) fed through the existing
combination must give the oracle's figures, the state must not depend on the chunking, and the Python surface must refuse bad
arguments before it touches a device."""
import numpy as np
import pytest

import fugue_amd
from fugue_amd import diagnostics as D
from fugue_amd import engine as E
from fugue_amd import inference as I
from fugue_amd import workloads as W
from tests import diag_reference as R
from tests.stream_diag_restatement import RestatementMoments, ar1_input, oracle_figures, restate

TOL = dict(r_hat=(1e-10, 0.0), ess=(1e-8, 0.0), mean=(1e-11, 1e-12), std=(1e-10, 0.0))       # tests/test_gpu_diag.py


@pytest.mark.parametrize("exchange", ["reduce", "gather"])
@pytest.mark.parametrize("seed", range(5))
def test_restated_state_gives_the_oracles_figures(oracle, seed, exchange):
    """AR(1) phi = 0.5, n = 200, 5 chains, 2 coordinates: Geyer's sequence ends by lag 25 at the latest (by 15 in the first
    coordinate; asserted from the high-precision form) and the pair after its end is the last one asked for, so K = 32 holds every
    lag the combination wants."""
    x = ar1_input(seed, 200, 5, 2, 0.5)
    assert R.ess_hp(x[:, 0, :])["max_t"] <= 15 and max(R.ess_hp(x[:, i, :])["max_t"] for i in range(2)) + 2 < 32
    st = restate(x, 32, [37] * 5 + [15])
    got = D.ChainDiagnostics(RestatementMoments(st), exchange=exchange).summary()
    want = oracle_figures(oracle, x)
    for i in range(2):
        for k, (rel, abs_) in TOL.items():
            print(f"seed {seed} [{i}] {k}: restatement {got[k][i]!r} oracle {want[i][k]!r}")
            assert got[k][i] == pytest.approx(want[i][k], rel=rel, abs=abs_)


def test_the_deep_input_needs_more_than_32_lags():
    """AR(1) phi = 0.99, n = 400, 4 chains: the sequence runs to lag >= 97 for every seed (what tests/test_gpu_diag_stream.py's
    lag-limit test relies on)."""
    for seed in range(5):
        assert R.ess_hp(ar1_input(seed, 400, 4, 1, 0.99)[:, 0, :])["max_t"] >= 97


def test_restated_state_does_not_depend_on_the_chunking():
    x = np.random.default_rng(97).standard_normal((97, 3, 7))
    a, b, c = restate(x, 32), restate(x, 32, [5, 31, 1, 60]), restate(x, 32, [1] * 97)
    for k in ("pivot", "s1", "s2", "P", "head", "ring"):
        assert np.array_equal(getattr(a, k), getattr(b, k)) and np.array_equal(getattr(a, k), getattr(c, k)), k
    assert np.array_equal(a.ring[96 % 32], x[96] - x[0]) and np.array_equal(a.head[31], x[31] - x[0])
    np.testing.assert_allclose(a.moments(), R.chain_moments_inorder(x), rtol=1e-11, atol=1e-13)
    for lag in (0, 1, 31):
        np.testing.assert_allclose(a.chain_autocov(lag), R.chain_autocov_inorder(x, lag), rtol=0, atol=1e-13)
    assert not a.chain_autocov(97).any()                                     # lags >= n are 0


def test_pivoted_sums_survive_an_offset_of_1e8():
    """1e8 + 1e-3 N(0, 1): the restated moments land on the high-precision forms, and the residual row carries what the rounding
    of pivot + mu leaves over (the pooled std needs it: without it column 2 misses the tolerance of
    test_rhat_ess_on_ill_conditioned_draws)."""
    x = R.conditioning_input()
    n, d, C = x.shape
    st = restate(x, 32)
    mom, res = st.moments(), st.resid()
    for i in range(d):
        hp = R.pooled_mean_std_hp(x[:, i, :])[1]
        gm = mom[i, 0].sum() / C
        total = mom[i, 1].sum() + n * ((mom[i, 0] - gm) ** 2).sum()
        plain, crossed = np.sqrt(total / (C * n - 1.0)), np.sqrt((total + 2.0 * ((mom[i, 0] - gm) * res[i]).sum()) / (C * n - 1.0))
        print(f"column {i}: std deviation without the cross term {abs(plain - hp) / hp:.3e}, with it {abs(crossed - hp) / hp:.3e}")
        assert abs(crossed - hp) / hp < 1e-10 < abs(plain - hp) / hp


class _NoEngine:
    h, C = None, 4


@pytest.mark.parametrize("args", [(0, 1, 64), (10, 0, 64), (10, 70000, 64), (10, 1, 0), (10, 1, 2049)])
def test_stream_handle_refuses_bad_arguments_before_the_device(args):
    with pytest.raises(ValueError):
        E.DiagStream(_NoEngine(), *args)
    with pytest.raises(TypeError):
        E.DiagStream(_NoEngine(), 10.5, 1, 64)


@pytest.mark.parametrize("kw", [dict(n_samples=0), dict(chunk=0), dict(max_lag=0), dict(max_lag=4096)])
def test_summary_drivers_refuse_bad_arguments_before_the_device(kw):
    a = dict(n_samples=10, n_warmup=5, n_chains=4)
    a.update(kw)
    with pytest.raises(ValueError):
        I.hmc_chain_summary(1, W.normal_sites(2), **a)
    with pytest.raises(ValueError):
        I.adaptive_mcmc_chain_summary(1, W.normal_sites(2), **a)


def test_new_names_are_exported():
    for name in ("ChainSummary", "StreamMoments", "hmc_chain_summary", "adaptive_mcmc_chain_summary"):
        assert hasattr(fugue_amd, name), name
    assert hasattr(E.Engine, "diag_stream") and E.DiagStream.__init__.__defaults__ == (64,)
    assert {"sites", "mean", "std", "r_hat", "ess", "n_samples", "n_chains", "accept_rate", "mean_step_size", "n_divergent"} <= set(I.ChainSummary.__dataclass_fields__)
