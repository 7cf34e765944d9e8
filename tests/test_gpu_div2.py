"""The two-instruction quotient by 2h of k_hmc_sep_steps's folded trajectory loop (g = fma(n, Ch, n * Cl), proved exact for the run's h
by fg_div2_prove on the host) against the same kernels without the folded loop (FG_HMC_SEP_FOLD=0: fg_div_const's five instructions
and the per-step range test): every draw, position, info row, step size, log-joint, mass matrix and value row BIT FOR BIT.

The short quotient is part of the folded loop itself ("The short quotient"), so the switched-off arm is FG_HMC_SEP_FOLD=0.
The Normal-sites model at d = 4 (two coordinates per wave: the NC = 2 resident form) and d = 5 (two and three: NC = 4), L = 3, 2 warmup
and 4 sampling transitions, on every tile form; a program whose records keep the unfolded density; a step size that drives n out of
the quotient's window (the checked re-run); and an h whose 2h the proof refuses (no folded loop at all)."""
import numpy as np
import pytest

import fugue_amd as F
from fugue_amd import engine as E
from fugue_amd import workloads as W

pytestmark = pytest.mark.gpu

REFUSED_H = float.fromhex("0x1.f86664b036c57p-12")          # 2h = 0x1.f86664b036c57p-11 fails at |delta| = 1


def _session(monkeypatch, fold, prog, C, half, resident=True, adapt_mass=False, nw=2, eps=None, h=1e-5):
    monkeypatch.setenv("FG_JIT", "0")
    monkeypatch.setenv("FG_HMC_SEP", "1")
    monkeypatch.setenv("FG_HMC_SEP_HALF", str(half))
    monkeypatch.setenv("FG_HMC_SEP_RESIDENT", "1" if resident else "0")
    monkeypatch.setenv("FG_HMC_SEP_FOLD", "1" if fold else "0")
    monkeypatch.delenv("FG_HMC_WAVES", raising=False)
    cp = E.compile_model(prog)
    eng = E.Engine(cp, C, seed=31, chain_offset=3)
    out, kernels = [], []
    try:
        eng.hmc_init(E.hmc_config(n_leapfrog=3, adapt_mass=adapt_mass, init_step_size=eps, finite_diff_eps=h), nw)
        short = eng.hmc_short_quotient()
        for n in ((nw, 2) if nw else (2,)):                  # the warmup, then two sampling transitions with their info rows
            pos, info = eng.hmc_step_info(n)
            kernels.append(eng.hmc_last_kernel())
            out += [pos, info["accepted"], info["divergent"], info["accept_prob"], info["step_size"], eng.get_values(),
                    eng.hmc_step_sizes(), eng.hmc_log_joint()]
            if adapt_mass: out.append(eng.hmc_mass())
        d = eng.device_alloc(2 * cp.d * C * 8)               # and two more into a draws buffer
        eng.hmc_step(2, d)
        kernels.append(eng.hmc_last_kernel())
        out += [eng.download(d, (2, cp.d, C)), eng.get_values(), eng.hmc_step_sizes(), eng.hmc_log_joint()]
        eng.device_free(d)
    finally:
        eng.close()
    return out, kernels, short


def _check(monkeypatch, expect_short=True, **kw):
    a, ka, sa = _session(monkeypatch, True, **kw)
    b, kb, sb = _session(monkeypatch, False, **kw)
    assert sa == expect_short and sb == expect_short          # the proof's verdict does not depend on the switch
    assert all("k_hmc_sep_steps" in k and ("(folded)" in k) == expect_short for k in ka), ka
    assert all("k_hmc_sep_steps" in k and "(folded)" not in k for k in kb), kb
    assert [k.replace("(folded) ", "") for k in ka] == kb
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True), f"output {k} differs"
    return a, ka


# tile forms: (FG_HMC_SEP_HALF, resident, chains, kernel-name tag)
TILES = [(0, True, 128, "(resident)"), (0, False, 65, "k_hmc_sep_steps (folded) W="), (1, True, 32, "half tiles"), (2, True, 16, "quarter tiles")]


@pytest.mark.parametrize("half,resident,C,tag", TILES)
@pytest.mark.parametrize("adapt_mass", [False, True])
@pytest.mark.parametrize("d", [4, 5])
def test_short_quotient_is_bit_identical(d, adapt_mass, half, resident, C, tag, monkeypatch):
    """With 2 warmup transitions adapt_mass leaves the identity mass (the mass matrix needs 4: hmc.rs:704-708), so the mass arm
    also runs with 4, where the MASS instantiations take the launch."""
    for nw in ((2, 4) if adapt_mass else (2,)):
        out, kern = _check(monkeypatch, prog=W.normal_sites(d), C=C, half=half, resident=resident, adapt_mass=adapt_mass, nw=nw)
        assert all(tag in k for k in kern), kern
        assert np.isfinite(out[0]).all()


def test_short_quotient_with_unfolded_densities(monkeypatch):
    """Sigmas 0.3 and 1.7 next to powers of two: no resident form, FG_SEP_DUALF's densities, the short quotient and the deferred range test."""
    def model():
        stm = [(0.0, 1.0, [(0.5, 0.5)]), (0.2, 0.3, [(1.0, 2.0), (-1.0, 1.7)]), (0.0, 4.0, []), (-0.3, 0.25, [(0.1, 0.25), (0.2, 4.0), (0.3, 0.5)])]
        m = F.pure(None)
        for i, (mu0, s0, obs) in enumerate(stm):
            def site(i=i, mu0=mu0, s0=s0, obs=obs):
                return F.sample(F.addr("x", i), F.Normal(mu0, s0)).bind(lambda x: F.sequence_vec(
                    [F.observe(F.addr("y", 10 * i + j), F.Normal(x, s), yv) for j, (yv, s) in enumerate(obs)]))
            m = m.bind(lambda _, site=site: site())
        return m
    _, kern = _check(monkeypatch, prog=model, C=65, half=0, resident=True)
    assert all("(resident)" not in k and "tiles" not in k for k in kern), kern


@pytest.mark.parametrize("half,resident,C,tag", TILES)
def test_short_quotient_out_of_window_takes_the_checked_rerun(half, resident, C, tag, monkeypatch):
    """A first step of 1e150: positions overflow, n leaves [2^-823, 2^953) or is not finite, and the coordinate runs again through the
    checked instance (fg_div_const / true division)."""
    out, kern = _check(monkeypatch, prog=W.normal_sites(5), C=C, half=half, resident=resident, eps=1e150, nw=0)
    assert all(tag in k for k in kern), kern
    assert out[2].any()                                       # divergent transitions were recorded


def test_refused_divisor_runs_without_the_folded_loop(monkeypatch):
    """2h = 0x1.f86664b036c57p-11 is one of the divisors the two-instruction form gets wrong: fg_hmc_short_quotient is 0 and the launch
    takes the kernels of the switched-off arm, with its bits."""
    for half, resident, C, _ in TILES:
        _check(monkeypatch, expect_short=False, prog=W.normal_sites(5), C=C, half=half, resident=resident, h=REFUSED_H)


def test_default_h_is_accepted(monkeypatch):
    _, kern, short = _session(monkeypatch, True, W.normal_sites(4), 64, 0)
    assert short and all("(folded)" in k for k in kern)
