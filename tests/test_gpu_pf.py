"""The particle filter bank on the device (fugue_amd/csrc/fg_pf.hip) against the oracle and the restatement (tests/pf_restatement.py).

TEACHER-FORCED PARITY.  Every step of a recorded run is judged from the device's own `prev`, its own `propagated` and the log-weights the
host recomputes from the device's previous weights, so that a last-place difference never compounds over time.  Bounds:
  * draws: the oracle's Normal of the stream (seed, i, t, 11) within 1e-11 relative, the standing tolerance of tests/test_gpu_predict.py
    for Normal draws (ocml against glibc inside Box-Muller).  The initial population IS a draw and is compared as such; a transition
    is seen through propagated = prev + draw, an addition both sides round once: |propagated - (prev + draw)| <= 1e-11 |draw| +
    EPS |propagated|.
  * score increment: the log-weight a step adds is not an output; it is recovered as ln w_i + (log_z_inc + ln n) - carried_i for the
    particles with w_i >= 1e-280 and compared with oracle.logpdf within 1e-12 relative (test_gpu_predict.py's bound for a
    log-likelihood) plus what the round trip through exp, the normalisation and the host's log loses: the weight's and log_z_inc's own
    bounds below, and two roundings of the three-term sum at the size of its largest term.  That slack is 1e-12 to 1e-11 absolute at
    these sizes: for scores of ordinary size the SLACK, not the 1e-12 relative, is the operative bound of this comparison (each
    case prints both).  The score itself is the same IEEE operations on both sides; what this check can see is a wrong score, not
    its last places.
  * log_z_inc against oracle.log_sum_exp(lw) - ln n, the weights, ess_frac, mean and var against the restatement in the reference's
    sequential order on the device's arrays: `pf_restatement.tolerances`, which derives every bound from the two summation orders
    ((n - 1) roundings for the sequential sum of non-negative terms, the plan's depth -- a thread's slots + 6 + the waves -- for the
    kernel's), ocml's stated 1 ulp for exp and log, and the roundings of each remaining operation.  No number there is fitted.
  * sum of the weights: within 1e-12 of 1, the bound of tests/test_gpu_smc_step.py.
  * resampled == (device ess_frac < threshold) exactly, and == the restatement's decision: the inputs keep the restatement's ess_frac
    more than 1e-9 from the threshold at every step (asserted first; the seeds were chosen with tests/test_pf_cpu.py, which walks the
    same cases on the CPU).
  * parents == oracle.systematic_indices(device weights, U), except that a slot may differ by one index where the sequential cumulative
    sum at the boundary lies within (n - 1) EPS, relative, of the slot's threshold (`pf_restatement.parent_band`); every such slot is
    reported through tests/knife.used, more than max(1, n / 1000) slots in the band fail the case, any other difference fails.
  * posterior == propagated[parents] bit for bit; identity parents and posterior == propagated when not resampled.
Every output of a step lies between guard words that must come back untouched.

BIT-FOR-BIT INVARIANCES and CORNERS follow.  The U = 0 corner of the search cannot be reached through the filter without a new entry
point (U comes from the stream): it is tested on the restatement's search against k_resample_search through
fg_device_resample_indices, the debug path of the resampler tests."""
import ctypes as C
import math

import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import pf as PF
from oracle import oracle as orc
from tests import knife
from tests import pf_restatement as R
from tests.test_pf_cpu import KALMAN_CASE, REFERENCE_CASE, judge_against_kalman, kalman_observations

pytestmark = pytest.mark.gpu
GUARD = 64
PATTERN = -1234.5


def _guarded(shape, dtype=np.float64):
    n = int(np.prod(shape))
    buf = np.full(n + 2 * GUARD, PATTERN if dtype == np.float64 else -77, dtype=dtype)
    return buf, buf[GUARD:GUARD + n].reshape(shape)


def _ptr(view, ctype):
    return view.ctypes.data_as(C.POINTER(ctype))


def guarded_step(bank, obs, per_filter=0):
    """fg_pf_step with every output between two runs of guard words -> BankStep"""
    B, n = bank.B, bank.n
    o = np.ascontiguousarray(np.atleast_1d(obs), dtype=np.float64)
    bufs = {k: _guarded((B,)) for k in ("ess", "lzi", "mean", "var")}
    bufs["res"] = _guarded((B,), np.int32)
    for k in ("prev", "prop", "w", "post"):
        bufs[k] = _guarded((B, n))
    bufs["par"] = _guarded((B, n), np.int64)
    v = {k: b[1] for k, b in bufs.items()}
    E._check(E.lib().fg_pf_step(bank._handle(), E._dp(o), per_filter, _ptr(v["ess"], C.c_double), _ptr(v["lzi"], C.c_double), _ptr(v["res"], C.c_int32),
                                _ptr(v["mean"], C.c_double), _ptr(v["var"], C.c_double), _ptr(v["prev"], C.c_double), _ptr(v["prop"], C.c_double),
                                _ptr(v["w"], C.c_double), _ptr(v["par"], C.c_int64), _ptr(v["post"], C.c_double)))
    for k, (buf, _) in bufs.items():
        pat = PATTERN if buf.dtype == np.float64 else -77
        assert (buf[:GUARD] == pat).all() and (buf[-GUARD:] == pat).all(), f"guard words around {k} were written"
    return PF.BankStep(v["prev"].copy(), v["prop"].copy(), v["w"].copy(), v["ess"].copy(), v["lzi"].copy(), v["res"].astype(bool), v["par"].copy(),
                       v["post"].copy(), v["mean"].copy(), v["var"].copy())


def judge_step(label, s, b, lw_c, sig_step, sig_obs, threshold, seed, t, obs):
    """one recorded device step of filter b against the oracle and the restatement -> the log-weights it carries on (host's log)"""
    n = s.prev.shape[1]
    prev, prop, w = s.prev[b], s.propagated[b], s.weights[b]
    r = R.step_from(prev, lw_c, sig_step, sig_obs, threshold, seed, t, obs, mode="seq", propagated=prop)
    assert abs(r["ess_frac"] - threshold) > 1e-9, (label, "the inputs put a step on the threshold")
    # the draw
    want = prev + r["draw"]
    err = np.abs(prop - want)
    print(f"{label}: draw, worst |propagated - (prev + draw)| / |draw| {float((err / np.abs(r['draw'])).max()):.3e}")
    assert np.all(err <= 1e-11 * np.abs(r["draw"]) + R.EPS * np.abs(prop)), label
    tol = R.tolerances(r, lw_c, same_math=False)
    # log_z_inc, weights, ess_frac, mean, var
    print(f"{label}: log_z_inc {abs(s.log_z_inc[b] - r['log_z_inc']):.3e} (bound {tol['log_z_inc']:.3e}); weights rel "
          f"{float(np.max(np.abs(w - r['weights']) / np.where(r['weights'] > 0, r['weights'], 1.0))):.3e} (bound {tol['weights_rel']:.3e}); ess_frac rel "
          f"{abs(s.ess_frac[b] - r['ess_frac']) / r['ess_frac']:.3e} (bound {tol['ess_frac_rel']:.3e}); mean {abs(s.mean[b] - r['mean']):.3e} (bound {tol['mean']:.3e}); "
          f"var {abs(s.var[b] - r['var']):.3e} (bound {tol['var']:.3e})")
    if math.isfinite(r["log_z_inc"]):
        assert abs(s.log_z_inc[b] - r["log_z_inc"]) <= tol["log_z_inc"], label
    else:
        assert s.log_z_inc[b] == r["log_z_inc"], label
    assert np.all(np.abs(w - r["weights"]) <= tol["weights_rel"] * r["weights"]), label
    assert abs(s.ess_frac[b] - r["ess_frac"]) <= tol["ess_frac_rel"] * r["ess_frac"], label
    assert abs(s.mean[b] - r["mean"]) <= tol["mean"] and abs(s.var[b] - r["var"]) <= tol["var"], label
    assert abs(math.fsum(w) - 1.0) <= 1e-12, label
    # the score increment, through the weights
    if math.isfinite(s.log_z_inc[b]):
        seen = w >= 1e-280
        lse = s.log_z_inc[b] + math.log(n)
        rec = np.log(w[seen]) + lse - lw_c[seen]
        sc = r["score"][seen]
        big = np.maximum(np.maximum(np.abs(np.log(w[seen])), abs(lse)), np.abs(lw_c[seen]))
        slack = tol["weights_rel"] + tol["log_z_inc"] + R.EPS * np.abs(np.log(w[seen])) + 2.0 * R.EPS * big + 2.0 * R.ULP_LOG * R.EPS * np.abs(lw_c[seen])
        print(f"{label}: score increment, worst excess over 1e-12 relative {float((np.abs(rec - sc) - 1e-12 * np.abs(sc)).max()):.3e} (slack {float(slack.max()):.3e})")
        assert np.all(np.abs(rec - sc) <= 1e-12 * np.abs(sc) + slack), label
    # the decision and the ancestry
    assert bool(s.resampled[b]) == bool(s.ess_frac[b] < threshold) == r["resampled"], label
    if s.resampled[b]:
        want_p = orc.systematic_indices(w, r["U"])
        diff = np.nonzero(s.parents[b] != want_p)[0]
        band = R.parent_band(np.cumsum(w), R.thresholds(n, r["U"]), n)
        assert band.sum() <= max(1, n // 1000), (label, int(band.sum()))
        assert np.all(band[diff]) and np.all(np.abs(s.parents[b][diff] - want_p[diff]) == 1), (label, diff[:8].tolist())
        if diff.size:
            knife.used("particle filter parents against oracle.systematic_indices", case=label, slots=diff.tolist())
        assert np.array_equal(s.posterior[b], prop[s.parents[b]]), label
    else:
        assert np.array_equal(s.parents[b], np.arange(n)) and np.array_equal(s.posterior[b], prop), label
    return R.carried(w, bool(s.resampled[b]))


@pytest.mark.parametrize("n", R.PARITY_SIZES)
def test_teacher_forced_parity_of_every_step(n):
    B = R.PARITY_FILTERS
    cases = [R.parity_case(n, b) for b in range(B)]
    prior_sig, sig_step, sig_obs, threshold, _, observations = cases[0]
    seeds = [c[4] for c in cases]
    with PF.ParticleFilterBank(n, prior_sig, sig_step, sig_obs, threshold, seeds) as bank:
        x = bank.positions()
        for b in range(B):
            want = R.normal_draws(seeds[b], n, 0, prior_sig)
            assert np.all(np.abs(x[b] - want) <= 1e-11 * np.abs(want)), ("initial draw", n, b)
        lw_c = [np.zeros(n) for _ in range(B)]
        log_z = [0.0] * B
        resampled = 0
        for t, obs in enumerate(observations, start=1):
            s = guarded_step(bank, obs)
            for b in range(B):
                assert np.array_equal(s.prev[b], x[b])                                # the state a step leaves is the state the next one finds
                lw_c[b] = judge_step(f"n={n} filter {b} t={t}", s, b, lw_c[b], sig_step, sig_obs, threshold, seeds[b], t, obs)
                log_z[b] += float(s.log_z_inc[b])
                resampled += int(s.resampled[b])
            x = s.posterior
        assert bank.t() == len(observations) and np.array_equal(bank.positions(), x)
        assert np.array_equal(bank.log_evidence(), np.array(log_z))                   # the increments, added in time order
        assert 0 < resampled < B * len(observations)


def test_the_largest_filter_one_workgroup_holds():
    """n = N_CAP declares the whole 160 KiB: three recorded steps judged as above, and the same steps as one run."""
    n = PF.N_CAP
    prior_sig, sig_step, sig_obs, threshold, seed, observations = R.parity_case(n)
    with PF.ParticleFilterBank(n, prior_sig, sig_step, sig_obs, threshold, [seed]) as bank, PF.ParticleFilterBank(n, prior_sig, sig_step, sig_obs, threshold, [seed]) as other:
        lw_c, steps = np.zeros(n), []
        for t, obs in enumerate(observations[:3], start=1):
            steps.append(guarded_step(bank, obs))
            lw_c = judge_step(f"n={n} t={t}", steps[-1], 0, lw_c, sig_step, sig_obs, threshold, seed, t, obs)
        r = other.run(observations[:3])
        assert np.array_equal(r.ess_frac[:, 0], [s.ess_frac[0] for s in steps]) and np.array_equal(r.log_z_inc[:, 0], [s.log_z_inc[0] for s in steps])
        assert np.array_equal(other.positions(), bank.positions()) and np.array_equal(other.log_evidence(), bank.log_evidence())


# ---- bit-for-bit invariances ------------------------------------------------------------------------------------------------------------
def _params(B, seed0=40):
    rng = np.random.default_rng(seed0)
    return dict(prior_sig=rng.uniform(0.5, 2.0, B), sig_step=rng.uniform(0.3, 1.0, B), sig_obs=rng.uniform(0.4, 1.5, B), ess_threshold=rng.uniform(0.3, 0.9, B),
                seeds=np.arange(B, dtype=np.uint64) + 900)


def _run_all(bank, obs):
    r = bank.run(obs)
    return [r.ess_frac, r.log_z_inc, r.resampled, r.mean, r.var, bank.log_evidence()[None, :], bank.positions().T]


def _same(a, b, what):
    for k, (u, v) in enumerate(zip(a, b)):
        assert np.array_equal(u, v, equal_nan=True), (what, k)


OBS12 = np.array([0.3 * t for t in range(12)])


@pytest.mark.parametrize("n", [65, 1025])
def test_filter_b_of_a_bank_is_the_same_filter_alone(n):
    P = _params(8)
    with PF.ParticleFilterBank(n, **P) as bank:
        full = _run_all(bank, OBS12)
    assert full[2].any() and not full[2].all()
    for b in range(8):
        with PF.ParticleFilterBank(n, P["prior_sig"][b], P["sig_step"][b], P["sig_obs"][b], P["ess_threshold"][b], [P["seeds"][b]]) as one:
            _same(_run_all(one, OBS12), [a[:, b:b + 1] for a in full], (n, b))


def test_more_workgroups_than_compute_units():
    P = _params(300)
    with PF.ParticleFilterBank(64, **P) as bank:
        full = _run_all(bank, OBS12[:3])
    for b in range(300):
        with PF.ParticleFilterBank(64, P["prior_sig"][b], P["sig_step"][b], P["sig_obs"][b], P["ess_threshold"][b], [P["seeds"][b]]) as one:
            _same(_run_all(one, OBS12[:3]), [a[:, b:b + 1] for a in full], b)
    with PF.ParticleFilterBank(64, **P) as bank:                                          # every filter singly, as a bank of per-filter steps
        steps = [bank.step(o, record=False) for o in OBS12[:3]]
        _same([np.stack([s.ess_frac for s in steps]), np.stack([s.log_z_inc for s in steps])], full[:2], "steps")


@pytest.mark.parametrize("n", [257, 5000])
def test_run_equals_steps_recorded_or_not_and_any_cut_of_the_run(n):
    """run(obs) == T step calls (recorded and not) == run(obs[:k]) + run(obs[k:]) for k on either side of the plan's steps per launch
    (T = steps per launch + 4 here: the cut of the plan itself lies inside the run)."""
    spl = PF.steps_per_launch(n)
    T = spl + 4 if n == 5000 else 12
    obs = np.sin(0.4 * np.arange(T)) * 2.0
    P = _params(2, 41)
    with PF.ParticleFilterBank(n, **P) as bank:
        full = _run_all(bank, obs)
    assert full[2].any() and not full[2].all()
    for record in ((False, True) if n == 257 else (True,)):
        with PF.ParticleFilterBank(n, **P) as bank:
            steps = [bank.step(o, record=record) for o in obs]
            got = [np.stack([getattr(s, k) for s in steps]) for k in ("ess_frac", "log_z_inc", "resampled", "mean", "var")]
            _same(got + [bank.log_evidence()[None, :], bank.positions().T], full, ("steps", record))
    for k in sorted({1, T - 1, min(spl, T) - 1, min(spl, T - 1), min(spl + 1, T - 1)}):
        with PF.ParticleFilterBank(n, **P) as bank:
            a, b = bank.run(obs[:k]), bank.run(obs[k:])
            got = [np.concatenate([u, v]) for u, v in zip(a, b)]
            _same(got + [bank.log_evidence()[None, :], bank.positions().T], full, ("cut", k))
            assert bank.t() == T


def test_shared_observations_equal_the_same_given_per_filter_and_set_sig_obs_mid_run():
    n, B = 300, 4
    P = _params(B, 42)
    with PF.ParticleFilterBank(n, **P) as bank:
        shared = _run_all(bank, OBS12)
    with PF.ParticleFilterBank(n, **P) as bank:
        _same(_run_all(bank, np.tile(OBS12, (B, 1))), shared, "per filter")
    # per-filter series that differ: filter b of the bank is the filter alone on its own series
    series = np.stack([OBS12 * (1.0 + 0.2 * b) for b in range(B)])
    with PF.ParticleFilterBank(n, **P) as bank:
        per = _run_all(bank, series)
    for b in range(B):
        with PF.ParticleFilterBank(n, P["prior_sig"][b], P["sig_step"][b], P["sig_obs"][b], P["ess_threshold"][b], [P["seeds"][b]]) as one:
            _same(_run_all(one, series[b]), [a[:, b:b + 1] for a in per], ("series", b))
    # set_sig_obs after 5 steps == a bank built with that value, from step 5 on (sig_obs is not read before the first step)
    Q = dict(P, sig_obs=np.full(B, 0.9))
    with PF.ParticleFilterBank(n, **P) as bank, PF.ParticleFilterBank(n, **Q) as other:
        bank.run(OBS12[:5])
        x, lz = bank.positions(), bank.log_evidence()
        bank.set_sig_obs(0.9)
        tail = bank.run(OBS12[5:])
        # the other bank reaches the same state by the same route, then runs the tail under its own (equal) value
        for b in range(B):
            other.set_sig_obs(float(P["sig_obs"][b]), b)
        other.run(OBS12[:5])
        assert np.array_equal(other.positions(), x) and np.array_equal(other.log_evidence(), lz)
        for b in range(B):
            other.set_sig_obs(0.9, b)
        _same(list(other.run(OBS12[5:])), list(tail), "set_sig_obs")
    with PF.ParticleFilterBank(n, **Q) as fresh, PF.ParticleFilterBank(n, **P) as bank:      # from t = 0: set before the first step == built with it
        bank.set_sig_obs(0.9)
        _same(_run_all(bank, OBS12), _run_all(fresh, OBS12), "set before the first step")


# ---- corners -------------------------------------------------------------------------------------------------------------------------
def test_threshold_zero_never_resamples_and_threshold_one_resamples_off_uniform():
    with PF.ParticleFilterBank(257, 1.0, 0.7, 0.6, [0.0, 1.0], [5, 5]) as bank:
        r = bank.run(OBS12)
    assert not r.resampled[:, 0].any()
    assert np.array_equal(r.resampled[:, 1], r.ess_frac[:, 1] < 1.0) and r.resampled[:, 1].all()


def test_the_floor_of_the_carried_log_weights():
    """An outlying observation under threshold 0 drives w_i n below 1e-300 for most particles; the device's carried log-weights are not an
    output, so the floor is read from step 2, whose observation hands the whole mass to the floored particles (pf_restatement.FLOOR_CASE).
    Asserted first, on the device's own step-1 arrays: step 2 restated with the floor differs from step 2 restated without it far beyond
    the bounds (tests/test_pf_cpu.py walks the same on the CPU).  Then the device's step 2 matches the floored restatement within the
    bounds -- and therefore not the unfloored one, which is asserted too."""
    c = R.FLOOR_CASE
    n, seed = c["n"], c["seed"]
    with PF.ParticleFilterBank(n, c["prior_sig"], c["sig_step"], c["sig_obs"], c["threshold"], [seed]) as bank:
        s1 = guarded_step(bank, c["obs"][0])
        judge_step("floor t=1", s1, 0, np.zeros(n), c["sig_step"], c["sig_obs"], c["threshold"], seed, 1, c["obs"][0])
        assert not s1.resampled[0]
        s2 = guarded_step(bank, c["obs"][1])
        floored, with_floor, without, lw_floor = R.floor_step_two(s1.weights[0], s1.posterior[0], propagated=s2.propagated[0])
        tol = R.assert_floor_is_seen(floored, with_floor, without, lw_floor)
        judge_step("floor t=2", s2, 0, lw_floor, c["sig_step"], c["sig_obs"], c["threshold"], seed, 2, c["obs"][1])
        assert np.all(s2.weights[0][floored] > 0.0)
        assert abs(s2.log_z_inc[0] - without["log_z_inc"]) > 1.0 and abs(s2.log_z_inc[0] - with_floor["log_z_inc"]) <= tol["log_z_inc"]


def test_the_all_minus_infinity_population():
    n, seed = 64, 9
    with PF.ParticleFilterBank(n, 1.0, 0.5, 1e-6, 0.5, [seed]) as bank:
        s1 = guarded_step(bank, 1e160)
        r = R.step_from(s1.prev[0], np.zeros(n), 0.5, 1e-6, 0.5, seed, 1, 1e160, propagated=s1.propagated[0])
        assert r["log_z_inc"] == -np.inf and r["ess_frac"] == 1.0 and np.all(r["lw_next"] == 0.0)
        assert s1.log_z_inc[0] == -np.inf and np.all(s1.weights[0] == 1.0 / n) and s1.ess_frac[0] == 1.0 and not s1.resampled[0]
        assert np.array_equal(s1.posterior[0], s1.propagated[0]) and abs(s1.mean[0] - r["mean"]) <= R.tolerances(r, np.zeros(n), False)["mean"]
        bank.set_sig_obs(0.8)
        s2 = guarded_step(bank, 0.2)
        judge_step("after -inf, t=2", s2, 0, np.zeros(n), 0.5, 0.8, 0.5, seed, 2, 0.2)      # the carried log-weight was 0
        assert bank.log_evidence()[0] == -np.inf


def test_parameter_clamps():
    pf = PF.ParticleFilter(1, 0.0, -1.0, 0.0, 7.0, 5)
    assert pf.n == 2 and pf.positions().shape == (2,)
    want = R.normal_draws(5, 2, 0, 1e-6)
    assert np.all(np.abs(pf.positions() - want) <= 1e-11 * np.abs(want))
    out = pf.step(0.0)                                           # sig_step = sig_obs = 1e-6, threshold 1
    f = R.Filter(1, 0.0, -1.0, 0.0, 7.0, 5)
    assert (f.n, f.sig_step, f.sig_obs, f.threshold) == (2, 1e-6, 1e-6, 1.0)
    d = R.normal_draws(5, 2, 1, 1e-6)
    assert np.all(np.abs(out.propagated - (out.prev + d)) <= 1e-11 * np.abs(d) + R.EPS * np.abs(out.propagated))
    assert out.resampled == (out.ess_frac < 1.0)
    pf.close()
    big = PF.ParticleFilter(10 ** 6, 1.0, 1.0, 1.0, -3.0, 5)
    assert big.n == 5000 and not big.step(0.1).resampled and big.t() == 1   # threshold clamped to 0
    big.close()
    with PF.ParticleFilterBank(64, 0.0, 0.0, 0.0, 2.0, [6]) as bank:        # the library's own clamps
        want = R.normal_draws(6, 64, 0, 1e-6)
        assert np.all(np.abs(bank.positions()[0] - want) <= 1e-11 * np.abs(want))
    with pytest.raises(E.EngineError) as ei:
        PF.ParticleFilterBank(PF.N_CAP + 1, 1.0, 1.0, 1.0, 0.5, [1])
    assert ei.value.code == E.FG_E_LIMIT
    with PF.ParticleFilterBank(64, 1.0, 1.0, 1.0, 0.5, [1]) as bank:
        with pytest.raises(E.EngineError) as ei:
            bank.run([0.1, float("inf")])
        assert ei.value.code == E.FG_E_BAD_ARG and bank.t() == 0


def test_the_search_at_u_zero_on_the_restatement_against_k_resample_search():
    """U = 0 (not reachable through the filter: U is the stream's) -- the restatement's search, the rule fg_pf.hip copies from
    k_resample_search, against k_resample_search itself."""
    rng = np.random.default_rng(11)
    for n in (2, 65, 1025):
        w = rng.random(n)
        w[0] = 0.0 if n > 2 else w[0]
        w /= w.sum()
        for U in (0.0, 0.5):
            got = np.minimum(np.searchsorted(np.cumsum(w), R.thresholds(n, U), side="left"), n - 1)
            assert np.array_equal(got, E.device_resample_indices(E.RESAMPLE_SYSTEMATIC, w, U)), (n, U)


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def test_the_references_scenario_on_the_device():
    pf = PF.ParticleFilter(*REFERENCE_CASE)
    any_resampled = False
    for t in range(10):
        out = pf.step(t * 0.3)
        assert out.posterior.shape == (200,) and out.parents.shape == (200,)
        any_resampled |= out.resampled
    assert pf.t() == 10 and math.isfinite(pf.log_evidence()) and any_resampled
    pf.close()


def test_law_on_the_device_against_the_kalman_filter():
    c = KALMAN_CASE
    assert PF.steps_per_launch(c["n"]) >= c["T"]                 # one launch
    with PF.ParticleFilterBank(c["n"], c["prior_sig"], c["sig_step"], c["sig_obs"], c["threshold"], 1000 + np.arange(c["B"], dtype=np.uint64)) as bank:
        r = bank.run(kalman_observations())
        judge_against_kalman(bank.log_evidence(), r.mean[-1])
