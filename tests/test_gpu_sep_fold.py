"""The folded trajectory loop of k_hmc_sep_steps (-0.5 / sigma^2 folded into the density's fma, the quotient's range test deferred to
the trajectory's end) against the same kernels without it (FG_HMC_SEP_FOLD=0): every draw, position, info row, step size,
log-joint, mass matrix and value row BIT FOR BIT -- resident and plain 64-chain tiles, half and quarter tiles, 0..3 observations per
site, power-of-two sigmas from 1/4 to 4, and inputs that drive the corners of the fold (squares that overflow only once scaled,
quotients of exactly 0, huge step sizes)."""
import numpy as np
import pytest

import fugue_amd as F
from fugue_amd import engine as E
from fugue_amd import workloads as W

pytestmark = pytest.mark.gpu


def _sites(stm):
    """stm: per site (prior mu, prior sigma, [(y, sigma), ...]): x_i ~ N(mu, sigma), y_ij ~ N(x_i, sigma_ij)."""
    def model():
        m = F.pure(None)
        for i, (mu0, s0, obs) in enumerate(stm):
            def site(i=i, mu0=mu0, s0=s0, obs=obs):
                return F.sample(F.addr("x", i), F.Normal(mu0, s0)).bind(lambda x: F.sequence_vec(
                    [F.observe(F.addr("y", 10 * i + j), F.Normal(x, s), yv) for j, (yv, s) in enumerate(obs)]))
            m = m.bind(lambda _, site=site: site())
        return m
    return model


def _shaped(d, nobs, sig, prior=(0.0, 1.0), y0=-1.0):
    return _sites([(prior[0], prior[1], [(y0 + 0.2 * i + 0.7 * j, sig[(i + j) % len(sig)]) for j in range(nobs)]) for i in range(d)])


def _session(monkeypatch, fold, prog, C, half, resident=True, waves=0, adapt_mass=False, L=7, eps=None, nw=20, launches=(7, 3, 11), n_draws=5):
    monkeypatch.setenv("FG_JIT", "0")
    monkeypatch.setenv("FG_HMC_SEP", "1")
    monkeypatch.setenv("FG_HMC_SEP_HALF", str(half))
    monkeypatch.setenv("FG_HMC_SEP_RESIDENT", "1" if resident else "0")
    monkeypatch.setenv("FG_HMC_SEP_FOLD", "1" if fold else "0")
    if waves: monkeypatch.setenv("FG_HMC_WAVES", str(waves))
    else: monkeypatch.delenv("FG_HMC_WAVES", raising=False)
    cp = E.compile_model(prog)
    eng = E.Engine(cp, C, seed=29, chain_offset=5)
    out, kernels = [], []
    try:
        eng.hmc_init(E.hmc_config(n_leapfrog=L, adapt_mass=adapt_mass, init_step_size=eps), nw)
        for n in launches:                                   # warmup (and past it) in launches of uneven length
            pos, info = eng.hmc_step_info(n)
            kernels.append(eng.hmc_last_kernel())
            out += [pos, info["accepted"], info["divergent"], info["accept_prob"], info["step_size"], eng.get_values(),
                    eng.hmc_step_sizes(), eng.hmc_log_joint()]
            if adapt_mass: out.append(eng.hmc_mass())
        d = eng.device_alloc(n_draws * cp.d * C * 8)
        eng.hmc_step(n_draws, d)
        kernels.append(eng.hmc_last_kernel())
        out += [eng.download(d, (n_draws, cp.d, C)), eng.get_values(), eng.hmc_log_joint()]
        eng.device_free(d)
        st = eng.hmc_stats()
        out += [np.array([st.accept_rate, st.n_divergent])]
    finally:
        eng.close()
    return out, kernels


def _check(monkeypatch, expect_fold=True, **kw):
    a, ka = _session(monkeypatch, True, **kw)
    b, kb = _session(monkeypatch, False, **kw)
    assert all("k_hmc_sep_steps" in k and ("(folded)" in k) == expect_fold for k in ka), ka
    assert all("k_hmc_sep_steps" in k and "(folded)" not in k for k in kb), kb
    assert [k.replace("(folded) ", "") for k in ka] == kb
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), f"output {k} differs"
    return a, ka


# tile forms: (FG_HMC_SEP_HALF, resident, kernel-name tag)
TILES = [(0, True, "(resident)"), (0, False, "k_hmc_sep_steps (folded) W="), (1, True, "half tiles"), (2, True, "quarter tiles")]


@pytest.mark.parametrize("half,resident,tag", TILES)
@pytest.mark.parametrize("nobs", [0, 1, 2, 3])
def test_fold_is_bit_identical_per_record_shape(nobs, half, resident, tag, monkeypatch):
    """U0 prior (nobs = 0: a sigma-2 prior instead) and nobs observations with sigmas 1/4, 1/2, 2, 4."""
    prior = (0.0, 1.0) if nobs else (0.4, 2.0)
    prog = _shaped(8, nobs, [0.25, 0.5, 2.0, 4.0], prior=prior)
    out, kern = _check(monkeypatch, prog=prog, C=150, half=half, resident=resident, waves=2 if half == 0 else 0)
    assert all(tag in k for k in kern), kern
    assert np.isfinite(out[0]).all()


@pytest.mark.parametrize("sig", [0.25, 0.5, 2.0, 4.0])
@pytest.mark.parametrize("adapt_mass", [False, True])
def test_fold_is_bit_identical_per_sigma(sig, adapt_mass, monkeypatch):
    """A non-U0 sigma-1 prior and one observation of sigma `sig`, resident (NC = 4) and plain 64-chain tiles."""
    prog = _shaped(8, 1, [sig], prior=(0.3, 1.0))
    for resident in (True, False):
        _check(monkeypatch, prog=prog, C=150, half=0, resident=resident, waves=2, adapt_mass=adapt_mass)


def test_fold_mixed_records_is_bit_identical(monkeypatch):
    """Records of different shapes and sigmas that are not powers of two (0.3, 1.7: no resident form, unfolded densities) next to
    folded ones: the deferred range test alone."""
    stm = [(0.0, 1.0, [(0.5, 0.5)]), (0.2, 0.3, [(1.0, 2.0), (-1.0, 1.7)]), (0.0, 4.0, []), (-0.3, 0.25, [(0.1, 0.25), (0.2, 4.0), (0.3, 0.5)])] * 2
    out, kern = _check(monkeypatch, prog=_sites(stm), C=150, half=0, resident=True, waves=2)
    assert all("(resident)" not in k for k in kern)


@pytest.mark.parametrize("half,resident,tag", TILES)
def test_fold_corners_are_bit_identical(half, resident, tag, monkeypatch):
    """Observations near 2^510 (d^2 finite, (d / sigma)^2 past the overflow threshold: FG_SEP_LPF's -inf, the fold's finite value)
    and coordinates near 2^510 (q +- h == q: every quotient exactly 0), each with a pinned first step of 1e150 and of a sane size."""
    big = 2.0 ** 510
    progs = [_shaped(8, 1, [0.25, 4.0], y0=1.5 * big), _shaped(8, 2, [0.5, 0.25], prior=(big, 1.0), y0=big)]
    for prog in progs:
        for eps in (1e150, 0.05):
            _check(monkeypatch, prog=prog, C=150, half=half, resident=resident, waves=2 if half == 0 else 0, eps=eps, nw=0, launches=(4, 3))


def test_fold_huge_step_is_bit_identical(monkeypatch):
    """The headline model with a first step so large that trajectories overflow: the checked re-run."""
    out, _ = _check(monkeypatch, prog=W.normal_sites(32), C=150, half=0, resident=True, waves=8, eps=1e150)
    assert out[2].any()


def test_fold_headline_shape_is_bit_identical(monkeypatch):
    """The benchmark's shape: 65 536 chains, L = 16, the host's own layout (8 waves per tile)."""
    _, kern = _check(monkeypatch, prog=W.normal_sites(32), C=65536, half=0, resident=True, waves=0, L=16, nw=10, launches=(7, 3, 11), n_draws=7)
    assert all("(resident) (folded) W=8" in k for k in kern), kern


def test_fold_8192_half_tiles_is_bit_identical(monkeypatch):
    """The hmc_8192 leg's shape: half tiles."""
    _check(monkeypatch, prog=W.normal_sites(32), C=8192, half=1, resident=True, waves=0, L=16, nw=10, launches=(5, 4), n_draws=3)
