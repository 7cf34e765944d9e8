"""The tail of k_hmc_sep_steps's transition -- the endpoint score terms, whose NaN -> -inf replacement sits behind a wave-uniform
test, and the Welford count, loaded and converted only while the mass adapts -- against the gradient-stream kernel (FG_HMC_SEP=0),
bit for bit: draws, committed values, log-joint, step sizes, divergence counts, acceptance and the adapted mass.  Few chains, few
transitions: the shapes are the smallest that reach each form of the kernel the change touches."""
import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import workloads as W
from fugue_amd.model import Normal, Program, addr

pytestmark = pytest.mark.gpu

C_CHAINS, N_WARM, N_SAMP = 100, 3, 5          # one full and one partial 64-chain tile
N_WARM_MASS = 12                              # the mass resets at n_warmup / 2 from the Welford sums, and keeps 1 below two pushes or while
                                              # every proposal was rejected: 3 warmup transitions never show the sums; 12 reset it from six


def _two_obs(d):
    """A prior with sigma != 1 and two observations per coordinate (power-of-two sigmas: the resident form takes it)."""
    P = Program()
    for i in range(d):
        x = P.sample(addr("x", i), Normal(0.5, 2.0))
        P.observe(addr("y", i), Normal(x, 0.5), 0.2 * i - 1.0)
        P.observe(addr("w", i), Normal(x, 0.25), 0.1 * i)
    return P


SHAPES = {"headline": W.normal_sites, "two_obs": _two_obs}
# name: (d, environment, what the kernel's name must hold; None: the plain 64-chain form, no tag but "(folded)")
LAYOUTS = {
    "resident_nc4": (8, {"FG_HMC_WAVES": "2", "FG_HMC_SEP_HALF": "0"}, "(resident)"),
    "resident_nc2": (4, {"FG_HMC_WAVES": "2", "FG_HMC_SEP_HALF": "0"}, "(resident)"),
    "plain_odd_d": (5, {"FG_HMC_SEP_RESIDENT": "0", "FG_HMC_SEP_HALF": "0"}, None),
    "half_tiles": (8, {"FG_HMC_SEP_HALF": "1"}, "(half tiles)"),
    "quarter_tiles": (8, {"FG_HMC_SEP_HALF": "2"}, "(quarter tiles)"),
}
ENV_KEYS = ("FG_HMC_SEP", "FG_HMC_WAVES", "FG_HMC_SEP_HALF", "FG_HMC_SEP_RESIDENT")
_compiled, _reference = {}, {}


def _run(monkeypatch, cp, env, adapt_mass, eps, split, n_warm=N_WARM):
    for k in ENV_KEYS: monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("FG_JIT", "0")          # the hand-written kernels
    for k, v in env.items(): monkeypatch.setenv(k, v)
    eng = E.Engine(cp, C_CHAINS, seed=77, chain_offset=3)
    d_draws = eng.device_alloc(N_SAMP * cp.d * C_CHAINS * 8)
    eng.hmc_init(E.hmc_config(n_leapfrog=6, adapt_mass=adapt_mass, init_step_size=eps), n_warm)
    if split:                                  # two launches, the second across the end of the warmup
        eng.hmc_step(2, d_draws)
        eng.hmc_step(n_warm + N_SAMP - 2, d_draws)
    else:
        eng.hmc_step(n_warm + N_SAMP, d_draws)
    st = eng.hmc_stats()
    out = dict(draws=eng.download(d_draws, (N_SAMP, cp.d, C_CHAINS)), values=eng.get_values(), lj=eng.hmc_log_joint(), eps=eng.hmc_step_sizes(),
               n_div=int(st.n_divergent), accept=float(st.accept_rate), mass=eng.hmc_mass() if adapt_mass else None, kernel=eng.hmc_last_kernel())
    eng.device_free(d_draws)
    eng.close()
    return out


def _cp(shape, d):
    if (shape, d) not in _compiled: _compiled[(shape, d)] = E.compile_model(SHAPES[shape](d))
    return _compiled[(shape, d)]


def _ref(monkeypatch, shape, d, adapt_mass, eps, n_warm=N_WARM):
    key = (shape, d, adapt_mass, eps, n_warm)
    if key not in _reference:
        r = _run(monkeypatch, _cp(shape, d), {"FG_HMC_SEP": "0"}, adapt_mass, eps, False, n_warm)
        assert "k_hmc_sep_steps" not in r["kernel"], r["kernel"]
        _reference[key] = r
    return _reference[key]


def _check_kernel(name, tag):
    if tag is None: assert name.replace(" (folded)", "").startswith("k_hmc_sep_steps W="), name
    else: assert "k_hmc_sep_steps" in name and tag in name, name


def _same(a, b):
    for k in ("draws", "values", "lj", "eps", "mass"):
        assert (a[k] is None and b[k] is None) or np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k
    assert a["n_div"] == b["n_div"] and a["accept"] == b["accept"]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_sep_transition_tail_is_bit_identical_to_the_stream_kernel(layout, shape, monkeypatch):
    d, env, tag = LAYOUTS[layout]
    cp = _cp(shape, d)
    for adapt_mass, n_warm in ((False, N_WARM), (True, N_WARM), (True, N_WARM_MASS)):
        ref = _ref(monkeypatch, shape, d, adapt_mass, None, n_warm)
        assert np.isfinite(ref["draws"]).all() and ref["n_div"] == 0 and 0.3 < ref["accept"] <= 1.0
        if n_warm == N_WARM_MASS: assert np.isfinite(ref["mass"]).all() and (ref["mass"] != 1.0).any()      # the Welford sums reached the mass
        for split in (False, True):
            got = _run(monkeypatch, cp, env, adapt_mass, None, split, n_warm)
            _check_kernel(got["kernel"], tag)
            _same(got, ref)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_overflowing_step_size_diverges_on_both_sides(layout, shape, monkeypatch):
    """Step size 1e160: q overflows in the first drift, z is NaN at the endpoint, the score term must come out -inf (not NaN) and
    the transition divergent -- for every chain, in every transition while the step size stands (the mass reset finds a new one)."""
    d, env, tag = LAYOUTS[layout]
    cp = _cp(shape, d)
    for adapt_mass in (False, True):
        ref = _ref(monkeypatch, shape, d, adapt_mass, 1e160)
        if adapt_mass: assert ref["n_div"] >= C_CHAINS
        else: assert ref["n_div"] == (N_WARM + N_SAMP) * C_CHAINS and ref["accept"] == 0.0
        for split in (False, True):
            got = _run(monkeypatch, cp, env, adapt_mass, 1e160, split)
            _check_kernel(got["kernel"], tag)
            _same(got, ref)
