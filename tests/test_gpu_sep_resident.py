"""The resident form of k_hmc_sep_steps (64-chain sparse tiles, a wave's coordinates in registers for a whole launch) against
the same kernel without it (FG_HMC_SEP_RESIDENT=0) and against the gradient-stream kernel (FG_HMC_SEP=0): every draw, position,
info row, step size, log-joint, mass matrix and value row BIT FOR BIT, after every launch of a session whose launches have uneven
lengths, span the end of warmup and meet a state export / import."""
import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import workloads as W

pytestmark = pytest.mark.gpu

FORMS = (("resident", {"FG_HMC_SEP": "1", "FG_HMC_SEP_RESIDENT": "1"}),
         ("plain", {"FG_HMC_SEP": "1", "FG_HMC_SEP_RESIDENT": "0"}),
         ("stream", {"FG_HMC_SEP": "0", "FG_HMC_SEP_RESIDENT": "1"}))


def _session(monkeypatch, env, prog, C, waves, adapt_mass, L=7, eps=None, nw=20, launches=(7, 3, 11), n_draws=5):
    monkeypatch.setenv("FG_JIT", "0")
    monkeypatch.setenv("FG_HMC_SEP_HALF", "0")
    if waves: monkeypatch.setenv("FG_HMC_WAVES", str(waves))
    else: monkeypatch.delenv("FG_HMC_WAVES", raising=False)
    for k, v in env.items(): monkeypatch.setenv(k, v)
    cp = E.compile_model(prog)
    eng = E.Engine(cp, C, seed=13, chain_offset=3)
    out, kernels = [], []
    try:
        eng.hmc_init(E.hmc_config(n_leapfrog=L, adapt_mass=adapt_mass, init_step_size=eps), nw)
        for n in launches:                                   # warmup (and past it) in launches of uneven length
            pos, info = eng.hmc_step_info(n)
            kernels.append(eng.hmc_last_kernel())
            out += [pos, info["accepted"], info["divergent"], info["accept_prob"], info["step_size"], eng.get_values(),
                    eng.hmc_step_sizes(), eng.hmc_log_joint()]
            if adapt_mass: out.append(eng.hmc_mass())
        blob = eng.state_export()                            # a state round trip between launches
        eng.state_import(blob)
        d = eng.device_alloc(n_draws * cp.d * C * 8)
        eng.hmc_step(n_draws, d)
        kernels.append(eng.hmc_last_kernel())
        out += [eng.download(d, (n_draws, cp.d, C)), eng.get_values(), eng.hmc_log_joint()]
        eng.device_free(d)
        pos, info = eng.hmc_step_info(2)
        out += [pos, info["accept_prob"], eng.get_values(), eng.hmc_step_sizes()]
        st = eng.hmc_stats()
        out += [np.array([st.accept_rate, st.n_divergent])]
    finally:
        eng.close()
    return out, kernels


def _check_forms(monkeypatch, expect_resident, **kw):
    res = {}
    for name, env in FORMS:
        res[name] = _session(monkeypatch, env, **kw)
    out0, kern0 = res["resident"]
    assert all(("(resident)" in k) == expect_resident and "k_hmc_sep_steps" in k for k in kern0), kern0
    assert all("(resident)" not in k for k in res["plain"][1])
    assert all("k_hmc_sep_steps" not in k for k in res["stream"][1])
    for name in ("plain", "stream"):
        out = res[name][0]
        assert len(out) == len(out0)
        for k, (a, b) in enumerate(zip(out0, out)):
            assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), f"{name}: output {k} differs"
    return out0


# (d, waves): 4 coordinates per wave (NC = 4), 2 per wave (NC = 2), an odd d (a wave with 3, the last pair half used)
@pytest.mark.parametrize("d,waves", [(8, 2), (8, 4), (32, 8), (32, 16), (7, 2)])
@pytest.mark.parametrize("adapt_mass", [False, True])
def test_sep_resident_is_bit_identical(d, waves, adapt_mass, monkeypatch):
    out = _check_forms(monkeypatch, True, prog=W.normal_sites(d), C=150, waves=waves, adapt_mass=adapt_mass)
    assert np.isfinite(out[0]).all()


def test_sep_resident_checked_rerun_is_bit_identical(monkeypatch):
    """A first step size so large that trajectories overflow: non-finite forces send coordinates through the checked re-run."""
    out = _check_forms(monkeypatch, True, prog=W.normal_sites(32), C=150, waves=8, adapt_mass=False, eps=1e150)
    assert out[2].any()                                     # some transitions of the first launch diverged


def test_sep_resident_headline_shape_is_bit_identical(monkeypatch):
    """The benchmark's shape: 65 536 chains, L = 16, the host's own layout (8 waves per tile), about 30 transitions."""
    _check_forms(monkeypatch, True, prog=W.normal_sites(32), C=65536, waves=0, adapt_mass=False, L=16, nw=10,
                 launches=(7, 3, 11), n_draws=7)
