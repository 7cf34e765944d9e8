"""The resident form of k_hmc_sep_steps reads its uniform scalars -- pointers, strides, h, L, the plan's flags, the warmup and Welford
conditions -- again from the kernarg segment at the head of each phase of a transition instead of holding them for the launch.  A wrong
offset, a scalar that is stale after a call or a condition read in the wrong phase changes a draw, a step size or a count: everything is
compared bit for bit with the gradient-stream kernel (FG_HMC_SEP=0) -- draws, committed values, log-joint, step sizes, divergence
count, acceptance, adapted mass -- on 100 chains (one full and one partial tile), L = 6, 3 warmup + 5 sampling transitions, in one launch
and in two launches split across the end of the warmup.  The shapes are the smallest that take each path: a wave with fewer coordinates
than the instantiation holds (NC = 4 and NC = 2), the five record shapes, with and without an adapting mass, the plan's switches, the
tested and unfolded twins of the same source, the recording calls, and a step size that overflows."""
import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import workloads as W
from fugue_amd.model import Normal, Program, addr

pytestmark = pytest.mark.gpu

C_CHAINS, N_WARM, N_SAMP, L = 100, 3, 5, 6
N_WARM_MASS = 12                              # the mass resets at n_warmup / 2 from the Welford sums: 12 warmup transitions reset it from six pushes


def _obs(n_obs):
    """A prior with sigma != 1 and n_obs observations per coordinate (power-of-two sigmas: the resident form takes it)."""
    def make(d):
        P = Program()
        for i in range(d):
            x = P.sample(addr("x", i), Normal(0.5, 2.0))
            for k, (name, sigma) in enumerate((("y", 0.5), ("w", 0.25), ("v", 1.0))[:n_obs]):
                P.observe(addr(name, i), Normal(x, sigma), 0.2 * i - 1.0 + 0.3 * k)
        return P
    return make


# the five record shapes of the resident instantiations: 0 .. 3 observations, and the headline's (N(0, 1) prior, one observation)
SHAPES = {"obs0": _obs(0), "obs1": _obs(1), "obs2": _obs(2), "obs3": _obs(3), "u0": W.normal_sites}
# name: (d, waves per tile): the coordinates per wave the plan deals out (fg_hmc_sep_plan.h: whole pairs, floor(pairs * w / W))
LAYOUTS = {
    "nc4_short_wave": (6, 2),         # waves own 2 and 4 coordinates: the NC = 4 instantiation with a wave that holds two
    "nc2_short_wave": (3, 2),         # waves own 2 and 1: the NC = 2 instantiation, odd d
    "nc4_eight_waves": (30, 8),       # 2, 4, 4, ...: eight waves -- priority turns, and enough waves for the four-wave sums
}
SWITCHES = {
    "predraw_off": {"FG_HMC_PREDRAW": "0"}, "predraw_on": {"FG_HMC_PREDRAW": "1"}, "sum4": {"FG_HMC_SUM4": "1"},
    "sum4_no_predraw": {"FG_HMC_SUM4": "1", "FG_HMC_PREDRAW": "0"}, "prio_off": {"FG_HMC_PRIO": "0"}, "prio_on": {"FG_HMC_PRIO": "1"},
    "range_tested": {"FG_HMC_SEP_RANGE": "0"}, "unfolded": {"FG_HMC_SEP_FOLD": "0"},
}
ENV_KEYS = ("FG_HMC_SEP", "FG_HMC_WAVES", "FG_HMC_SEP_HALF", "FG_HMC_SEP_RESIDENT", "FG_HMC_PREDRAW", "FG_HMC_SUM4", "FG_HMC_PRIO", "FG_HMC_SEP_RANGE",
            "FG_HMC_SEP_FOLD", "FG_HMC_STAGGER")
_compiled, _reference = {}, {}


def _cp(shape, d):
    if (shape, d) not in _compiled: _compiled[(shape, d)] = E.compile_model(SHAPES[shape](d))
    return _compiled[(shape, d)]


def _engine(monkeypatch, cp, env, adapt_mass, eps, n_warm):
    for k in ENV_KEYS: monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("FG_JIT", "0")          # the hand-written kernels
    for k, v in env.items(): monkeypatch.setenv(k, v)
    eng = E.Engine(cp, C_CHAINS, seed=77, chain_offset=3)
    eng.hmc_init(E.hmc_config(n_leapfrog=L, adapt_mass=adapt_mass, init_step_size=eps), n_warm)
    return eng


def _state(eng, adapt_mass):
    st = eng.hmc_stats()
    return dict(values=eng.get_values(), lj=eng.hmc_log_joint(), eps=eng.hmc_step_sizes(), n_div=int(st.n_divergent), accept=float(st.accept_rate),
                mass=eng.hmc_mass() if adapt_mass else None, kernel=eng.hmc_last_kernel())


def _run(monkeypatch, cp, env, adapt_mass, eps, split, n_warm):
    eng = _engine(monkeypatch, cp, env, adapt_mass, eps, n_warm)
    d_draws = eng.device_alloc(N_SAMP * cp.d * C_CHAINS * 8)
    if split:                                  # two launches, the second across the end of the warmup
        eng.hmc_step(2, d_draws)
        eng.hmc_step(n_warm + N_SAMP - 2, d_draws)
    else:
        eng.hmc_step(n_warm + N_SAMP, d_draws)
    out = _state(eng, adapt_mass)
    out["draws"] = eng.download(d_draws, (N_SAMP, cp.d, C_CHAINS))
    eng.device_free(d_draws)
    eng.close()
    return out


def _sep_env(waves, extra=None):
    env = {"FG_HMC_WAVES": str(waves), "FG_HMC_SEP_HALF": "0"}
    env.update(extra or {})
    return env


def _ref(monkeypatch, shape, d, adapt_mass, eps, n_warm, split):
    """The stream kernel over the same launches: a launch adds ITS sum of acceptance probabilities to the chain's, so the last place of
    the acceptance rate belongs to the split (every other output is the same for both splits, which the callers check)."""
    key = (shape, d, adapt_mass, eps, n_warm, split)
    if key not in _reference:
        r = _run(monkeypatch, _cp(shape, d), {"FG_HMC_SEP": "0"}, adapt_mass, eps, split, n_warm)
        assert "k_hmc_sep_steps" not in r["kernel"], r["kernel"]
        _reference[key] = r
    return _reference[key]


def _check_kernel(name, waves, folded=None):
    assert name.startswith("k_hmc_sep_steps (resident)") and name.endswith(f" W={waves}"), name
    if folded is not None: assert ("(folded)" in name) == folded, name


def _same_state(a, b, keys=("draws", "values", "lj", "eps", "mass")):
    for k in keys:
        assert (a[k] is None and b[k] is None) or np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k
    assert a["n_div"] == b["n_div"]


def _same(a, b, keys=("draws", "values", "lj", "eps", "mass")):
    _same_state(a, b, keys)
    assert a["accept"] == b["accept"]


def _compare(monkeypatch, shape, d, waves, extra=None, folded=None):
    cp = _cp(shape, d)
    for adapt_mass, n_warm in ((False, N_WARM), (True, N_WARM_MASS)):
        ref1 = _ref(monkeypatch, shape, d, adapt_mass, None, n_warm, False)
        assert np.isfinite(ref1["draws"]).all() and ref1["n_div"] == 0 and 0.3 < ref1["accept"] <= 1.0
        if adapt_mass: assert np.isfinite(ref1["mass"]).all() and (ref1["mass"] != 1.0).any()      # the Welford sums reached the mass
        for split in (False, True):
            ref = _ref(monkeypatch, shape, d, adapt_mass, None, n_warm, split)
            _same_state(ref, ref1)
            got = _run(monkeypatch, cp, _sep_env(waves, extra), adapt_mass, None, split, n_warm)
            _check_kernel(got["kernel"], waves, folded)
            _same(got, ref)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_resident_form_is_bit_identical_to_the_stream_kernel(layout, shape, monkeypatch):
    d, waves = LAYOUTS[layout]
    _compare(monkeypatch, shape, d, waves)


@pytest.mark.parametrize("shape", ["u0", "obs2"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("switch", list(SWITCHES))
def test_plan_switches_and_twins_are_bit_identical(switch, layout, shape, monkeypatch):
    d, waves = LAYOUTS[layout]
    _compare(monkeypatch, shape, d, waves, SWITCHES[switch], folded=False if switch == "unfolded" else None)


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_overflowing_step_size_diverges_on_both_sides(layout, shape, monkeypatch):
    """Step size 1e160: the fast trajectory ends with a non-finite momentum, the checked one runs again, the endpoint's score terms are
    -inf and the transition divergent -- for every chain, in every transition while the step size stands (the mass reset finds a new one)."""
    d, waves = LAYOUTS[layout]
    cp = _cp(shape, d)
    for adapt_mass in (False, True):
        ref1 = _ref(monkeypatch, shape, d, adapt_mass, 1e160, N_WARM, False)
        if adapt_mass: assert ref1["n_div"] >= C_CHAINS
        else: assert ref1["n_div"] == (N_WARM + N_SAMP) * C_CHAINS and ref1["accept"] == 0.0
        for split in (False, True):
            ref = _ref(monkeypatch, shape, d, adapt_mass, 1e160, N_WARM, split)
            _same_state(ref, ref1)
            got = _run(monkeypatch, cp, _sep_env(waves), adapt_mass, 1e160, split, N_WARM)
            _check_kernel(got["kernel"], waves)
            _same(got, ref)


def _recorded(monkeypatch, cp, env, adapt_mass):
    """Five transitions, each through hmc_step_recorded (two chains' trajectories, then the transition), then more through hmc_step_info:
    positions and HmcStepInfo of every transition -- the kernel's pos_all / info arguments.  Without mass adaptation the recorded ones
    cross the end of a 3-transition warmup; with it they are warmup, and the others cross the mass reset at 6 and the warmup's end at 12."""
    eng = _engine(monkeypatch, cp, env, adapt_mass, None, N_WARM_MASS if adapt_mass else N_WARM)
    rec = [eng.hmc_step_recorded([1, 70], L) for _ in range(5)]
    kernel_rec = eng.hmc_last_kernel()
    pos, info = eng.hmc_step_info(10 if adapt_mass else 4)
    out = _state(eng, adapt_mass)
    out.update(traj=np.stack([r[0] for r in rec]), ham=np.stack([r[1] for r in rec]), npts=np.stack([r[2] for r in rec]), pos=pos,
               kernel_rec=kernel_rec, **{"info_" + k: v for k, v in info.items()})
    eng.close()
    return out


@pytest.mark.parametrize("shape", ["u0", "obs3"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_recorded_and_info_paths_are_bit_identical(layout, shape, monkeypatch):
    d, waves = LAYOUTS[layout]
    cp = _cp(shape, d)
    keys = ("values", "lj", "eps", "mass", "traj", "ham", "npts", "pos", "info_accepted", "info_divergent", "info_accept_prob", "info_step_size")
    for adapt_mass in (False, True):
        ref = _recorded(monkeypatch, cp, {"FG_HMC_SEP": "0"}, adapt_mass)
        assert "k_hmc_sep_steps" not in ref["kernel"] and np.isfinite(ref["pos"]).all() and ref["info_accepted"].any()
        got = _recorded(monkeypatch, cp, _sep_env(waves), adapt_mass)
        _check_kernel(got["kernel_rec"], waves)
        _check_kernel(got["kernel"], waves)
        _same(got, ref, keys)
