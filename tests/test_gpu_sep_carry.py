"""The resident forms of k_hmc_sep_steps carry the gradient at the committed position from one transition to the next inside a launch
(fg_hmc_sep.hip, fg_sep_carries): the first step of a trajectory takes it instead of computing it, the last step hands its own back, the
commit selects it with the position, a launch's first comes from checked arithmetic in the prologue and a checked re-run replaces the
proposal's.  A gradient committed with the wrong position, kept across a rejected proposal's re-run or stale at a launch boundary moves
every later draw: everything is compared bit for bit with the gradient-stream kernel (FG_HMC_SEP=0), which computes all L + 1 gradients
of every trajectory, over the same launch split -- positions and HmcStepInfo rows of every transition, draws, committed values,
log-joint, step sizes, divergence count and acceptance.

100 chains (one full and one partial tile), L = 6, FG_JIT=0.  The fixed step sizes were chosen on the CPU oracle
(oracle.OracleModel(prog).hmc_run(77, 100, 0, 12, HmcConfig.default(n_leapfrog=6, init_step_size=eps), chain0=3)) for an acceptance rate
between 0.3 and 0.7, where accepted and rejected transitions follow each other in every order:
    W.normal_sites, eps 0.75: 0.546 at d = 6, 0.617 at d = 3       three observations, eps 0.35: 0.464 at d = 6, 0.545 at d = 3
(eps 0.6 / 0.3 accept 0.78 .. 0.96 of the proposals, 0.85 / 0.44 under 0.26)."""
import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import workloads as W
from fugue_amd.model import Normal, Program, addr

pytestmark = pytest.mark.gpu

C_CHAINS, L, N_T = 100, 6, 12


def _obs3(d):
    """A prior with sigma != 1 and three observations per coordinate (power-of-two sigmas: the resident form takes it)."""
    P = Program()
    for i in range(d):
        x = P.sample(addr("x", i), Normal(0.5, 2.0))
        for k, (name, sigma) in enumerate((("y", 0.5), ("w", 0.25), ("v", 1.0))):
            P.observe(addr(name, i), Normal(x, sigma), 0.2 * i - 1.0 + 0.3 * k)
    return P


def _far(d):
    """tests/test_gpu_sep_range.py's prior at 2^40 (two observations, sigmas 1/2 and 1/4): q + h == q - h at h = 1e-5, every numerator is +0."""
    big, sig = 2.0 ** 40, [0.5, 0.25]
    P = Program()
    for i in range(d):
        x = P.sample(addr("x", i), Normal(big, 1.0))
        for j in range(2):
            P.observe(addr("y", 10 * i + j), Normal(x, sig[(i + j) % 2]), big + 0.2 * i + 0.7 * j)
    return P


SHAPES = {"u0": (W.normal_sites, 0.75), "obs3": (_obs3, 0.35), "far": (_far, 0.05)}          # name: (program of d coordinates, fixed step size)
# name: (d, waves per tile): the coordinates per wave the plan deals out (fg_hmc_sep_plan.h: whole pairs, floor(pairs * w / W))
LAYOUTS = {"nc4": (6, 2),             # waves own 2 and 4 coordinates: the NC = 4 instantiation, one wave with two coordinates
           "nc2": (3, 2)}             # waves own 2 and 1: the NC = 2 instantiation, odd d
SPLITS = {"one": (12,), "ones": (1,) * 12, "five_seven": (5, 7)}
ENV_KEYS = ("FG_HMC_SEP", "FG_HMC_WAVES", "FG_HMC_SEP_HALF", "FG_HMC_SEP_RESIDENT", "FG_HMC_PREDRAW", "FG_HMC_SUM4", "FG_HMC_PRIO", "FG_HMC_SEP_RANGE",
            "FG_HMC_SEP_FOLD", "FG_HMC_STAGGER")
INFO = ("accepted", "divergent", "accept_prob", "step_size")
_compiled, _reference = {}, {}


def _cp(shape, d):
    if (shape, d) not in _compiled: _compiled[(shape, d)] = E.compile_model(SHAPES[shape][0](d))
    return _compiled[(shape, d)]


def _session(monkeypatch, cp, env, split, eps, n_warm=0, adapt_mass=False, then=None, recorded=0):
    """Launches of split[0], split[1], ... transitions through hmc_step_info (positions and HmcStepInfo of every transition), then two more
    through hmc_step with a draws buffer.  then = (eps, split): the step size is set anew and more launches follow in the same engine.
    recorded: that many transitions through hmc_step_recorded first."""
    for k in ENV_KEYS: monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("FG_JIT", "0")          # the hand-written kernels
    for k, v in env.items(): monkeypatch.setenv(k, v)
    eng = E.Engine(cp, C_CHAINS, seed=77, chain_offset=3)
    out, kernels = {}, []
    try:
        eng.hmc_init(E.hmc_config(n_leapfrog=L, adapt_mass=adapt_mass, init_step_size=eps), n_warm)
        if recorded:
            rec = [eng.hmc_step_recorded([1, 70], L) for _ in range(recorded)]
            kernels.append(eng.hmc_last_kernel())
            out.update(traj=np.stack([r[0] for r in rec]), ham=np.stack([r[1] for r in rec]), npts=np.stack([r[2] for r in rec]))
        pos, info = [], []
        for leg in ((eps, split),) + ((then,) if then else ()):
            if leg is then: eng.hmc_set_step_size(leg[0])
            for n in leg[1]:
                p, i = eng.hmc_step_info(n)
                kernels.append(eng.hmc_last_kernel())
                pos.append(p); info.append(i)
        out["pos"] = np.concatenate(pos)
        for k in INFO: out[k] = np.concatenate([i[k] for i in info])
        d_draws = eng.device_alloc(2 * cp.d * C_CHAINS * 8)
        eng.hmc_step(2, d_draws)
        kernels.append(eng.hmc_last_kernel())
        st = eng.hmc_stats()
        out.update(draws=eng.download(d_draws, (2, cp.d, C_CHAINS)), values=eng.get_values(), lj=eng.hmc_log_joint(), eps=eng.hmc_step_sizes(),
                   n_div=int(st.n_divergent), accept=float(st.accept_rate), mass=eng.hmc_mass() if adapt_mass else None)
        eng.device_free(d_draws)
    finally:
        eng.close()
    return out, kernels


def _same(a, b, but=()):
    assert a.keys() == b.keys()
    for k in a:
        if k in but: continue
        assert (a[k] is None and b[k] is None) or np.array_equal(np.asarray(a[k]), np.asarray(b[k]), equal_nan=True), k


def _compare(monkeypatch, shape, layout, split, extra=None, folded=None, **kw):
    """The resident form against the stream kernel over the same launches; returns the stream kernel's outputs."""
    d, waves = LAYOUTS[layout]
    cp = _cp(shape, d)
    kw.setdefault("eps", SHAPES[shape][1])
    key = (shape, d, split, tuple(sorted(kw.items())))
    if key not in _reference:
        ref, kref = _session(monkeypatch, cp, {"FG_HMC_SEP": "0"}, split, **kw)
        assert not any("k_hmc_sep_steps" in k for k in kref), kref
        _reference[key] = ref
    ref = _reference[key]
    env = {"FG_HMC_WAVES": str(waves), "FG_HMC_SEP_HALF": "0"}
    env.update(extra or {})
    got, kernels = _session(monkeypatch, cp, env, split, **kw)
    for name in kernels:
        assert name.startswith("k_hmc_sep_steps (resident)") and name.endswith(f" W={waves}"), name
        if folded is not None: assert ("(folded)" in name) == folded, name
    _same(got, ref)
    return ref


def _pairs(accepted):
    """chains in which accept->accept, accept->reject, reject->accept and reject->reject each occur among consecutive transitions"""
    a, b = accepted[:-1], accepted[1:]
    return [int(((a == x) & (b == y)).any(axis=0).sum()) for x, y in ((True, True), (True, False), (False, True), (False, False))]


@pytest.mark.parametrize("shape", ["u0", "obs3"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_accept_and_reject_sequences_over_every_launch_split(layout, shape, monkeypatch):
    """No warmup, a fixed step size, 12 transitions: in one launch, in 12 launches of one (every start gradient is then the prologue's) and
    as 5 + 7 with accepted and rejected chains at the boundary.  The carried gradient has to follow the position through every order of
    accepted and rejected transitions: each of the four orders must occur in at least 10 of the 100 chains."""
    one = _compare(monkeypatch, shape, layout, SPLITS["one"])
    acc = one["accepted"][:N_T]
    assert acc.shape == (N_T, C_CHAINS) and one["n_div"] == 0 and np.isfinite(one["pos"]).all()
    assert 0.3 < acc.mean() < 0.7, acc.mean()
    assert min(_pairs(acc)) >= 10, _pairs(acc)
    assert 10 <= int(acc[4].sum()) <= C_CHAINS - 10              # the 5 + 7 split: both kinds of chain stand at the boundary
    for name in ("ones", "five_seven"):
        ref = _compare(monkeypatch, shape, layout, SPLITS[name])
        _same(ref, one, but=("accept",))                         # (a launch adds ITS sum of acceptance probabilities: the last place belongs to the split)


@pytest.mark.parametrize("switch", [{"FG_HMC_SEP_RANGE": "0"}, {"FG_HMC_SEP_FOLD": "0"}], ids=["range_tested", "unfolded"])
@pytest.mark.parametrize("shape", ["u0", "obs3"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_twins_carry_the_same_bits(layout, shape, switch, monkeypatch):
    """The folded loop with its range test and the unfolded loop: other instantiations of the same source (unfolded, NC = 4, three
    observations is the one resident form without a mass that does not take the carry)."""
    for name in ("five_seven", "ones"):
        ref = _compare(monkeypatch, shape, layout, SPLITS[name], switch, folded="FG_HMC_SEP_FOLD" not in switch)
        assert min(_pairs(ref["accepted"][:N_T])) >= 10


def test_checked_rerun_hands_its_last_gradient_on(monkeypatch):
    """The prior at 2^40 under the tested twin, NC = 2: every numerator is +0, which the running maximum of the range test counts as out of
    range, so EVERY trajectory ends with a NaN momentum and runs again through the checked instance -- and is a sound proposal (g = +0: the
    momentum never changes) that is accepted or rejected on its merits.  The next transition's start gradient is then the re-run's last."""
    for name in ("one", "five_seven"):
        ref = _compare(monkeypatch, "far", "nc2", SPLITS[name], {"FG_HMC_SEP_RANGE": "0"}, folded=True)
        assert ref["n_div"] == 0 and np.isfinite(ref["pos"]).all()
        acc = ref["accepted"][:N_T]
        assert acc.any(axis=0).sum() >= 90 and acc.mean() > 0.3, acc.mean()     # accepted proposals: the re-run's gradient is committed


@pytest.mark.parametrize("shape", ["u0", "obs3"])
def test_adapting_mass_nc2(shape, monkeypatch):
    """NC = 2 with an adapting mass: 12 warmup transitions (the mass is reset at 6 from the Welford sums) in launches of 5 + 9, and as 14 x 1."""
    for split in ((5, 9), (1,) * 14):
        ref = _compare(monkeypatch, shape, "nc2", split, eps=None, n_warm=12, adapt_mass=True)
        assert np.isfinite(ref["mass"]).all() and (ref["mass"] != 1.0).any() and ref["accepted"].any()


@pytest.mark.parametrize("shape", ["u0", "obs3"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_warmup_across_a_launch_boundary(layout, shape, monkeypatch):
    """Six warmup transitions in launches of 4 + 8: the step size changes from transition to transition and freezes inside the second
    launch, while the carried gradient depends on none of it."""
    ref = _compare(monkeypatch, shape, layout, (4, 8), eps=None, n_warm=6)
    assert len(np.unique(ref["step_size"][:7, 0])) > 3 and ref["accepted"].any() and not ref["accepted"].all()


@pytest.mark.parametrize("shape", ["u0", "obs3"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_overflowing_step_size_then_a_sane_one(layout, shape, monkeypatch):
    """Step size 1e160: every fast trajectory ends with a non-finite momentum, the checked one runs again and the transition is divergent
    -- for every chain in 2 + 1 transitions.  No proposal is accepted, so the carried gradient must still be the start position's when the
    same engine goes on at the shape's sane step size (3 + 6 transitions)."""
    ref = _compare(monkeypatch, shape, layout, (2, 1), eps=1e160, then=(SHAPES[shape][1], (3, 6)))
    assert ref["divergent"][:3].all() and not ref["accepted"][:3].any() and ref["n_div"] == 3 * C_CHAINS
    assert not ref["divergent"][3:].any() and min(_pairs(ref["accepted"][3:])) >= 10


@pytest.mark.parametrize("shape", ["u0", "obs3"])
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_recorded_and_info_paths(layout, shape, monkeypatch):
    """Three transitions through hmc_step_recorded (launches of one), then 4 + 5 through hmc_step_info: non-null positions and info rows."""
    ref = _compare(monkeypatch, shape, layout, (4, 5), recorded=3)
    assert np.isfinite(ref["pos"]).all() and ref["accepted"].any() and not ref["accepted"].all()
