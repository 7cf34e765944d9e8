"""k_hmc_sep_steps's folded trajectory loop WITHOUT the range test of its quotient (the host bounded every numerator for the program and
h: fg_sep_range.h, fg_hmc_range_proved) against the same loop with the test (FG_HMC_SEP_RANGE=0) against the kernels without the folded
loop (FG_HMC_SEP_FOLD=0): every draw, position, info row, step size, log-joint and value row BIT FOR BIT, on resident and plain 64-chain
tiles, half and quarter tiles.

150 chains, d = 8, L = 7, launches of 7 / 3 / 11 transitions as in tests/test_gpu_sep_fold.py.  Cases: the four record shapes; priors so
far out that q + h == q - h and every numerator is exactly +0 (at 2^40 the bound is accepted and no coordinate is run again; at 2^510
the bound itself overflows, so that program is refused and keeps the test); a first step of 1e150 (non-finite exits: the checked
re-run); a refused program (observations of 1.5 * 2^510); the headline shape with 8 waves per tile."""
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


ARMS = [("proved", "1", "1"), ("tested", "0", "1"), ("unfolded", "1", "0")]      # (name, FG_HMC_SEP_RANGE, FG_HMC_SEP_FOLD)


def _session(monkeypatch, rng_switch, fold, prog, C, half, resident=True, waves=0, L=7, eps=None, nw=20, launches=(7, 3, 11), n_draws=5):
    monkeypatch.setenv("FG_JIT", "0")
    monkeypatch.setenv("FG_HMC_SEP", "1")
    monkeypatch.setenv("FG_HMC_SEP_HALF", str(half))
    monkeypatch.setenv("FG_HMC_SEP_RESIDENT", "1" if resident else "0")
    monkeypatch.setenv("FG_HMC_SEP_FOLD", fold)
    monkeypatch.setenv("FG_HMC_SEP_RANGE", rng_switch)
    if waves: monkeypatch.setenv("FG_HMC_WAVES", str(waves))
    else: monkeypatch.delenv("FG_HMC_WAVES", raising=False)
    cp = E.compile_model(prog)
    eng = E.Engine(cp, C, seed=29, chain_offset=5)
    out, kernels = [], []
    try:
        eng.hmc_init(E.hmc_config(n_leapfrog=L, init_step_size=eps), nw)
        proved = eng.hmc_range_proved()
        for n in launches:
            pos, info = eng.hmc_step_info(n)
            kernels.append(eng.hmc_last_kernel())
            out += [pos, info["accepted"], info["divergent"], info["accept_prob"], info["step_size"], eng.get_values(),
                    eng.hmc_step_sizes(), eng.hmc_log_joint()]
        d = eng.device_alloc(n_draws * cp.d * C * 8)
        eng.hmc_step(n_draws, d)
        kernels.append(eng.hmc_last_kernel())
        out += [eng.download(d, (n_draws, cp.d, C)), eng.get_values(), eng.hmc_step_sizes(), eng.hmc_log_joint()]
        eng.device_free(d)
    finally:
        eng.close()
    return out, kernels, proved


def _check(monkeypatch, expect_proved, tag, **kw):
    runs = {name: _session(monkeypatch, r, f, **kw) for name, r, f in ARMS}
    a, ka, _ = runs["proved"]
    assert [p for _, _, p in runs.values()] == [expect_proved] * 3      # the verdict depends on neither switch
    assert all("k_hmc_sep_steps" in k and "(folded)" in k and tag in k for k in ka), ka
    assert runs["tested"][1] == ka                                       # kernel names do not change
    assert runs["unfolded"][1] == [k.replace("(folded) ", "") for k in ka]
    for name in ("tested", "unfolded"):
        b = runs[name][0]
        assert len(a) == len(b)
        for k, (x, y) in enumerate(zip(a, b)):
            assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), f"{name}: output {k} differs"
    return a


# tile forms: (FG_HMC_SEP_HALF, resident, kernel-name tag)
TILES = [(0, True, "(resident)"), (0, False, "k_hmc_sep_steps (folded) W="), (1, True, "half tiles"), (2, True, "quarter tiles")]


def _waves(half):
    return 2 if half == 0 else 0


@pytest.mark.parametrize("half,resident,tag", TILES)
@pytest.mark.parametrize("nobs", [0, 1, 2, 3])
def test_range_proved_is_bit_identical_per_record_shape(nobs, half, resident, tag, monkeypatch):
    """U0 prior (nobs = 0: a sigma-2 prior instead) and nobs observations with sigmas 1/4, 1/2, 2, 4."""
    prior = (0.0, 1.0) if nobs else (0.4, 2.0)
    out = _check(monkeypatch, True, tag, prog=_shaped(8, nobs, [0.25, 0.5, 2.0, 4.0], prior=prior), C=150, half=half, resident=resident, waves=_waves(half))
    assert np.isfinite(out[0]).all()


@pytest.mark.parametrize("half,resident,tag", TILES)
@pytest.mark.parametrize("big,proved", [(2.0 ** 40, True), (2.0 ** 510, False)])
def test_numerators_of_exactly_zero(big, proved, half, resident, tag, monkeypatch):
    """Coordinates near `big` with h = 1e-5: q + h == q - h, both sides are the same bits and every n is +0 -- the quotient of +0 is +0
    without a test.  2^40 > 2^55 h is accepted (bound about 2^85); at 2^510 the bound overflows: refused, the tested step."""
    prog = _shaped(8, 2, [0.5, 0.25], prior=(big, 1.0), y0=big)
    for eps in (1e150, 0.05):
        _check(monkeypatch, proved, tag, prog=prog, C=150, half=half, resident=resident, waves=_waves(half), eps=eps, nw=0, launches=(4, 3))


@pytest.mark.parametrize("half,resident,tag", TILES)
def test_non_finite_exits_take_the_checked_rerun(half, resident, tag, monkeypatch):
    """A first step of 1e150: positions overflow, n is huge-but-zero or not finite; a non-finite momentum is never finite again and the
    coordinate runs through the checked instance."""
    out = _check(monkeypatch, True, tag, prog=_shaped(8, 1, [0.5, 2.0]), C=150, half=half, resident=resident, waves=_waves(half), eps=1e150, nw=0,
                 launches=(7, 3, 11))
    assert out[2].any()                                       # divergent transitions were recorded


@pytest.mark.parametrize("half,resident,tag", TILES)
def test_refused_program_keeps_the_tested_step(half, resident, tag, monkeypatch):
    """Observations of 1.5 * 2^510 (tests/test_gpu_sep_fold.py's corner): the bound is refused, the launch still takes a "(folded)" kernel."""
    prog = _shaped(8, 1, [0.25, 4.0], y0=1.5 * 2.0 ** 510)
    for eps in (1e150, 0.05):
        _check(monkeypatch, False, tag, prog=prog, C=150, half=half, resident=resident, waves=_waves(half), eps=eps, nw=0, launches=(4, 3))


def test_headline_shape_is_bit_identical(monkeypatch):
    """The benchmark's model and kernel form (resident, 8 waves per tile, L = 16) at 150 chains."""
    out = _check(monkeypatch, True, "(resident) (folded) W=8", prog=W.normal_sites(32), C=150, half=0, resident=True, waves=8, L=16)
    assert np.isfinite(out[0]).all()
