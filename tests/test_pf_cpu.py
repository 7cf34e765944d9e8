"""The bootstrap particle filter bank without a GPU: the restatement (tests/pf_restatement.py) against the exact Kalman filter and the
reference's own test, the library's argument codes, the launch plan (fugue_amd/csrc/fg_pf_plan.h) through a stand-alone driver under
-fsanitize=address,undefined, and the two summation orders of the restatement against each other."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import pf as PF
from oracle import oracle as orc
from tests import pf_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g")
PLAN_SIZES = ("2", "63", "64", "65", "256", "257", "1024", "1025", "4999", "5000", "cap", "cap+1")


def test_normal_logpdf_of_the_restatement_is_the_oracles_bit_for_bit():
    rng = np.random.default_rng(5)
    for mu, sigma in ((0.0, 1.0), (0.3, 0.6), (-2.5, 1e-6), (1e160, 1e-6), (7.0, 123.0)):
        x = np.concatenate([rng.normal(mu if abs(mu) < 1e9 else 0.0, 3.0, 60), [0.0, -0.0, 1e300, -1e300, np.inf, -np.inf, np.nan]])
        got = R.normal_logpdf(x, mu, sigma)
        want = np.array([orc.logpdf("Normal", float(v), [mu, sigma]) for v in x])
        assert np.array_equal(got, want, equal_nan=True), (mu, sigma)


def test_streams_of_the_restatement_are_the_oracles():
    d = R.normal_draws(77, 5, 3, 0.7)
    for i in range(5):
        assert d[i] == orc.sample_dist("Normal", [0.0, 0.7], orc.stream(77, i, 3, R.RNG_PF))
    assert R.resample_uniform(77, 3) == orc.sample_dist("Uniform", [0.0, 1.0], orc.stream(77, 0, 3, R.RNG_PF_RESAMPLE))
    assert 0.0 <= R.resample_uniform(77, 3) < 1.0 and R.resample_uniform(77, 3) != R.resample_uniform(77, 4)


# ---- the law -----------------------------------------------------------------------------------------------------------------------
KALMAN_CASE = dict(n=5000, prior_sig=1.0, sig_step=0.5, sig_obs=0.7, threshold=0.5, T=20, B=64)


def kalman_observations():
    """one series of the model itself, from a fixed generator"""
    c = KALMAN_CASE
    rng = np.random.default_rng(20)
    x = rng.normal(0.0, c["prior_sig"])
    obs = []
    for _ in range(c["T"]):
        x += rng.normal(0.0, c["sig_step"])
        obs.append(x + rng.normal(0.0, c["sig_obs"]))
    return np.array(obs)


def judge_against_kalman(log_z, final_mean):
    """Z-hat is unbiased: the mean over the filters of exp(log_z - log_z_Kalman) lies within 4 standard errors of 1; the mean of the
    final filtering means within 4 standard errors of Kalman's.  The standard errors come from the values themselves."""
    c = KALMAN_CASE
    lzk, mk, _ = R.kalman(kalman_observations(), c["prior_sig"], c["sig_step"], c["sig_obs"])
    ratio = np.exp(np.asarray(log_z) - lzk)
    se_r = ratio.std(ddof=1) / math.sqrt(ratio.size)
    fm = np.asarray(final_mean)
    se_m = fm.std(ddof=1) / math.sqrt(fm.size)
    print(f"Kalman log Z {lzk:.6f}, mean {mk:.6f}; Z ratio {ratio.mean():.6f} +- {se_r:.2e}; filtering mean {fm.mean():.6f} +- {se_m:.2e}")
    assert ratio.size == c["B"] and se_r > 0.0 and se_m > 0.0
    assert abs(ratio.mean() - 1.0) <= 4.0 * se_r
    assert abs(fm.mean() - mk) <= 4.0 * se_m


def test_law_of_the_restatement_against_the_kalman_filter():
    c = KALMAN_CASE
    obs = kalman_observations()
    log_z, fm = [], []
    for seed in range(c["B"]):
        f = R.Filter(c["n"], c["prior_sig"], c["sig_step"], c["sig_obs"], c["threshold"], 1000 + seed)
        for y in obs:
            r = f.step(y)
        log_z.append(f.log_evidence())
        fm.append(r["mean"])
    judge_against_kalman(log_z, fm)


# ---- the reference's own test (crates/fugue-wasm/tests/wasm.rs:69-86) ------------------------------------------------------------------
REFERENCE_CASE = (200, 1.6, 0.7, 0.6, 0.5, 11)           # seed 11 resamples under the engine's streams too: no other seed was needed


@pytest.mark.parametrize("mode", ["seq", "plan"])
def test_the_references_scenario_on_the_restatement(mode):
    f = R.Filter(*REFERENCE_CASE, mode=mode)
    any_resampled = False
    for t in range(10):
        r = f.step(t * 0.3)
        assert r["posterior"].shape == (200,)
        any_resampled |= r["resampled"]
    assert f.t() == 10 and math.isfinite(f.log_evidence()) and any_resampled


def test_clamps_of_the_restatement_and_of_the_python_layer():
    assert R.clamp_params(1, 0.0, -3.0, 1e-9, 2.0) == (2, 1e-6, 1e-6, 1e-6, 1.0)
    assert R.clamp_params(10 ** 6, 2.0, 3.0, 4.0, -1.0) == (5000, 2.0, 3.0, 4.0, 0.0)
    assert PF.N_CAP == R.N_CAP >= 5000 and (PF.RNG_PF, PF.RNG_PF_RESAMPLE) == (R.RNG_PF, R.RNG_PF_RESAMPLE) == (11, 12)
    with pytest.raises(ValueError):
        R.Filter(*REFERENCE_CASE).step(float("nan"))


def test_the_floor_case_makes_step_two_depend_on_the_floor():
    """The inputs of tests/test_gpu_pf.py::test_the_floor_of_the_carried_log_weights, walked on the restatement: step 2 with the floored carry
    differs from step 2 with an unfloored carry far beyond the bounds the device is held to, so a kernel without the floor (or with
    another constant) cannot pass there."""
    c = R.FLOOR_CASE
    for mode in ("seq", "plan"):
        f = R.Filter(c["n"], c["prior_sig"], c["sig_step"], c["sig_obs"], c["threshold"], c["seed"], mode=mode, clamp=False)
        r1 = f.step(c["obs"][0])
        assert not r1["resampled"] and np.array_equal(r1["lw_next"][r1["weights"] * c["n"] < 1e-300], np.full(int((r1["weights"] * c["n"] < 1e-300).sum()), np.log(1e-300)))
        R.assert_floor_is_seen(*R.floor_step_two(r1["weights"], r1["posterior"]))
        r2 = f.step(c["obs"][1])                          # the filter itself takes the floored branch
        assert np.array_equal(r2["weights"], R.step_from(r1["posterior"], R.carried(r1["weights"], False), c["sig_step"], c["sig_obs"], c["threshold"], c["seed"], 2,
                                                         c["obs"][1], mode=mode)["weights"])


# ---- the library's argument codes, before any device is looked for ----------------------------------------------------------------------
def test_argument_codes_without_a_device():
    L = E.lib()
    h = C.c_void_p()
    ok = (E.fg_pf_params * 2)(E.fg_pf_params(1.0, 0.5, 0.7, 0.5, 1), E.fg_pf_params(1.0, 0.5, 0.7, 0.5, 2))
    assert L.fg_pf_new(0, 64, 2, ok, None) == E.FG_E_BAD_ARG
    assert L.fg_pf_new(0, 64, 2, None, C.byref(h)) == E.FG_E_BAD_ARG
    assert L.fg_pf_new(0, 64, 0, ok, C.byref(h)) == E.FG_E_BAD_ARG and "n_filters" in E.last_error()
    assert L.fg_pf_new(0, 64, -3, ok, C.byref(h)) == E.FG_E_BAD_ARG
    assert L.fg_pf_new(0, 1, 2, ok, C.byref(h)) == E.FG_E_BAD_ARG
    assert L.fg_pf_new(0, -1, 2, ok, C.byref(h)) == E.FG_E_BAD_ARG
    assert L.fg_pf_new(0, PF.N_CAP + 1, 2, ok, C.byref(h)) == E.FG_E_LIMIT and str(PF.N_CAP) in E.last_error()
    assert L.fg_pf_new(0, 10 ** 9, 2, ok, C.byref(h)) == E.FG_E_LIMIT
    for field in ("prior_sig", "sig_step", "sig_obs", "ess_threshold"):
        for v in (float("nan"), float("inf"), float("-inf")):
            bad = (E.fg_pf_params * 2)(E.fg_pf_params(1.0, 0.5, 0.7, 0.5, 1), E.fg_pf_params(1.0, 0.5, 0.7, 0.5, 2))
            setattr(bad[1], field, v)
            assert L.fg_pf_new(0, 64, 2, bad, C.byref(h)) == E.FG_E_BAD_ARG and "filter 1" in E.last_error(), (field, v)
    assert h.value is None
    one = (C.c_double * 1)(0.5)
    assert L.fg_pf_run(None, one, 1, 0, None, None, None, None, None) == E.FG_E_BAD_ARG
    assert L.fg_pf_step(None, one, 0, *([None] * 10)) == E.FG_E_BAD_ARG
    assert L.fg_pf_set_sig_obs(None, -1, 1.0) == E.FG_E_BAD_ARG
    assert L.fg_pf_log_evidence(None, one) == E.FG_E_BAD_ARG and L.fg_pf_positions(None, one) == E.FG_E_BAD_ARG
    assert L.fg_pf_t(None) == -1
    L.fg_pf_free(None)
    # a valid bank: a device is looked for only now (FG_E_NO_DEVICE without one; with one the remaining codes, still before any launch)
    rc = L.fg_pf_new(0, PF.N_CAP, 2, ok, C.byref(h))
    assert rc in (0, E.FG_E_NO_DEVICE), (rc, E.last_error())
    if rc == 0:
        two = (C.c_double * 2)(0.5, float("nan"))
        assert L.fg_pf_run(h, two, -1, 0, None, None, None, None, None) == E.FG_E_BAD_ARG
        assert L.fg_pf_run(h, two, 2, 0, None, None, None, None, None) == E.FG_E_BAD_ARG and "not finite" in E.last_error()
        assert L.fg_pf_run(h, None, 2, 0, None, None, None, None, None) == E.FG_E_BAD_ARG
        assert L.fg_pf_run(h, two, 1, 2, None, None, None, None, None) == E.FG_E_BAD_ARG
        assert L.fg_pf_step(h, two, 1, *([None] * 10)) == E.FG_E_BAD_ARG
        assert L.fg_pf_set_sig_obs(h, 2, 1.0) == E.FG_E_BAD_ARG and L.fg_pf_set_sig_obs(h, 0, float("nan")) == E.FG_E_BAD_ARG
        assert L.fg_pf_t(h) == 0
        L.fg_pf_free(h)
    with pytest.raises(ValueError):
        PF.ParticleFilterBank(64, [1.0, 2.0], [1.0, 2.0, 3.0], 1.0, 0.5, [1, 2])
    with pytest.raises(E.EngineError) as ei:
        PF.ParticleFilterBank(1, 1.0, 1.0, 1.0, 0.5, [1])
    assert ei.value.code == E.FG_E_BAD_ARG


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
def test_plan_driver_under_address_and_ub_sanitizers(tmp_path):
    assert shutil.which("g++"), "g++ builds the driver"
    exe = os.path.join(str(tmp_path), "pf_plan_driver_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", *SAN, os.path.join(ROOT, "tests", "cpp", "pf_plan_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=24")
    r = subprocess.run([exe, *PLAN_SIZES], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(PLAN_SIZES) + 1 and lines[-1] == "refusals ok"
    threads_seen = set()
    for arg, ln in zip(PLAN_SIZES, lines):
        head, nums, verdict = [s.strip() for s in ln.split("|")]
        n = {"cap": PF.N_CAP, "cap+1": PF.N_CAP + 1}.get(arg) or int(arg)
        assert head == f"plan {n}" and verdict == "ok", ln
        rc, threads, per, n_pad, lds, grid, spl = [int(v) for v in nums.split()]
        if arg == "cap+1":
            assert rc == E.FG_E_LIMIT
            continue
        assert rc == 0 and (threads, per, spl) == R.plan(n) and spl == PF.steps_per_launch(n) and grid == 7
        assert lds <= 163840 and lds >= 3 * 8 * n and threads * per >= n > threads * (per - 1)
        threads_seen.add(threads)
    assert threads_seen == {64, 128, 256, 512, 1024} and PF.N_CAP >= 5000
    assert R.plan(5000)[2] >= 20                              # the Kalman case of tests/test_gpu_pf.py is one launch


# ---- the two summation orders ----------------------------------------------------------------------------------------------------------
def test_plan_sum_and_plan_cumsum_are_sums():
    rng = np.random.default_rng(3)
    for n in (2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4999, 5000, R.N_CAP):
        v = rng.random(n)
        exact = math.fsum(v)
        assert abs(R.plan_sum(v) - exact) <= R.plan_depth(n) * 0.5 * R.EPS * exact * 1.001
        assert abs(R.seq_sum(v) - exact) <= (n - 1) * 0.5 * R.EPS * exact * 1.001
        cum = R.plan_cumsum(v)
        want = np.array([math.fsum(v[:k + 1]) for k in range(n)]) if n <= 1025 else np.cumsum(v)
        assert cum.shape == (n,) and np.all(np.diff(cum) >= 0.0)
        assert np.all(np.abs(cum - want) <= (n - 1 + R.plan_depth(n)) * 0.5 * R.EPS * want * 1.001)


@pytest.mark.parametrize("filt", range(R.PARITY_FILTERS))
@pytest.mark.parametrize("n", R.PARITY_SIZES)
def test_the_two_summation_modes_agree_within_the_derived_bounds(n, filt):
    """Both modes step from the same positions and carried log-weights (those of the sequential filter), on the inputs of the GPU tests:
    every figure within `tolerances(..., same_math=True)`, the same resampling decision, and parents that differ by one index only in
    the band of `parent_band`."""
    from tests import knife
    prior_sig, sig_step, sig_obs, threshold, seed, observations = R.parity_case(n, filt)
    f = R.Filter(n, prior_sig, sig_step, sig_obs, threshold, seed, clamp=False)
    n_resampled = 0
    for t, obs in enumerate(observations, start=1):
        x, lw = f.x.copy(), f.lw.copy()
        a = f.step(obs)
        b = R.step_from(x, lw, f.sig_step, f.sig_obs, f.threshold, f.seed, t, obs, mode="plan")
        tol = R.tolerances(a, lw, same_math=True)
        assert np.array_equal(a["propagated"], b["propagated"]) and np.array_equal(a["lw"], b["lw"])
        assert abs(a["log_z_inc"] - b["log_z_inc"]) <= tol["log_z_inc"]
        assert np.all(np.abs(a["weights"] - b["weights"]) <= tol["weights_rel"] * a["weights"])
        assert abs(a["ess_frac"] - b["ess_frac"]) <= tol["ess_frac_rel"] * a["ess_frac"]
        assert abs(a["mean"] - b["mean"]) <= tol["mean"] and abs(a["var"] - b["var"]) <= tol["var"]
        assert abs(a["ess_frac"] - f.threshold) > 1e-9 and a["resampled"] == b["resampled"]
        n_resampled += a["resampled"]
        if a["resampled"]:
            pb, _ = R.systematic(a["weights"], a["U"], "plan")
            diff = np.nonzero(pb != a["parents"])[0]
            band = R.parent_band(np.cumsum(a["weights"]), R.thresholds(n, a["U"]), n)
            assert band.sum() <= max(1, n // 1000)
            assert np.all(band[diff]) and np.all(np.abs(pb[diff] - a["parents"][diff]) == 1)
            if diff.size:
                knife.used("the two summation modes, parents", n=n, t=t, slots=diff.tolist())
    assert n_resampled < len(observations) and (filt > 0 or n_resampled > 0)      # both branches of a step are on the path
