"""GPU parity: likelihood-tempered SMC (adaptive_smc, src/inference/smc.rs) and its
population-wide primitives (log-sum-exp, next_beta, the three resamplers) through the C ABI
against the CPU oracle.  Resample indices are integer work: exact."""
import math

import numpy as np
from tests import knife
import pytest

from fugue_amd import engine as E
from fugue_amd import workloads as W

pytestmark = pytest.mark.gpu


def test_device_log_sum_exp(oracle):
    rng = np.random.default_rng(0)
    for n in (1, 7, 513, 100_003):
        x = rng.normal(-50, 30, size=n)
        assert E.device_log_sum_exp(x) == pytest.approx(oracle.log_sum_exp(x), rel=1e-13, abs=1e-13)
    # reference known answers (src/core/numerical.rs:152-203, tests/f_dist_numerical.rs:22-85)
    assert E.device_log_sum_exp([700.0, 701.0, 699.0]) == pytest.approx(701.4076059644444, abs=1e-12)
    assert E.device_log_sum_exp([1000.0, 1001.0]) == pytest.approx(1001.3132616875182, abs=1e-12)
    assert E.device_log_sum_exp([-math.inf] * 3) == -math.inf
    assert E.device_log_sum_exp([-math.inf, 0.0]) == 0.0
    assert E.device_log_sum_exp([]) == -math.inf


def test_device_next_beta(oracle):
    rng = np.random.default_rng(1)
    for n, beta, scale in ((1000, 0.0, 5.0), (40_000, 0.3, 2.0), (40_000, 0.0, 0.01)):
        ll = rng.normal(-3, scale, size=n)
        lw = np.full(n, -math.log(n))
        tgt = 0.5 * n
        assert E.device_next_beta(beta, lw, ll, tgt) == pytest.approx(oracle.next_beta(beta, lw, ll, tgt), rel=1e-10)
    assert E.device_next_beta(0.0, lw, ll, tgt) == 1.0          # flat likelihood: jump straight to 1 (smc.rs:604-607)


@pytest.mark.parametrize("method", [E.RESAMPLE_SYSTEMATIC, E.RESAMPLE_STRATIFIED, E.RESAMPLE_MULTINOMIAL])
@pytest.mark.parametrize("n", [5, 1000, 6001])
def test_resample_indices_exact(oracle, method, n):
    rng = np.random.default_rng(n + method)
    w = rng.gamma(0.5, size=n)
    w /= w.sum()
    u = rng.random(n)
    if method == E.RESAMPLE_SYSTEMATIC:
        got, exp = E.device_resample_indices(method, w, u[:1]), oracle.systematic_indices(w, u[0])
    elif method == E.RESAMPLE_STRATIFIED:
        got, exp = E.device_resample_indices(method, w, u), oracle.stratified_indices(w, u)
    else:
        got, exp = E.device_resample_indices(method, w, u), oracle.multinomial_indices(w, u)
    # the parallel prefix sum associates the additions differently from the reference's sequential
    # walk: an index may move by one only where a threshold sits within ~1e-13 of a cumulative weight
    diff = np.nonzero(got != exp)[0]
    cum = np.cumsum(w)
    for j in diff:
        thr = (u[0] / n + j / n) if method == 1 else ((j + u[j]) / n if method == 2 else u[j])
        assert abs(int(got[j]) - int(exp[j])) == 1 and abs(cum[min(got[j], exp[j])] - thr) < 1e-12
        knife.used("resampling indices", method=method, slot=int(j), gpu=int(got[j]), oracle=int(exp[j]), threshold_minus_cum=float(thr - cum[min(got[j], exp[j])]))
    assert len(diff) <= 1


def test_resample_large_population_properties():
    """BASELINE C4 size: 1 048 576 particles.  Systematic resampling keeps every particle
    floor(N w) or ceil(N w) times and the indices are sorted."""
    n = 1 << 20
    rng = np.random.default_rng(4)
    w = rng.gamma(2.0, size=n)
    w /= w.sum()
    idx = E.device_resample_indices(E.RESAMPLE_SYSTEMATIC, w, [0.37])
    assert (np.diff(idx) >= 0).all() and idx.min() >= 0 and idx.max() < n
    counts = np.bincount(idx, minlength=n)
    assert np.abs(counts - n * w).max() < 1.0 + 1e-6


def _smc_pair(oracle, prog, n, seed, **kw):
    cp, om = E.compile_model(prog), oracle.OracleModel(prog)
    eng = E.Engine(cp, n, seed=seed)
    seq = kw.get("sequential", False)
    got = eng.smc_run(rejuvenation_steps=kw.get("R", 0), ess_threshold=kw.get("thr", 0.5), resampling_method=kw.get("method", 1), sequential_adaptation=seq)
    exp = om.smc_run(n, seed, method=kw.get("method", 1), ess_threshold=kw.get("thr", 0.5), rejuvenation_steps=kw.get("R", 0), batched=0 if seq else 1)
    return cp, got, exp


def test_smc_importance_sampling_matches_oracle(oracle):
    """rejuvenation_steps == 0: a single importance-sampling reweight (smc.rs:484-493)."""
    cp, got, exp = _smc_pair(oracle, W.smc_normal(), 4096, seed=42)
    assert got["log_evidence"] == pytest.approx(exp["log_evidence"], rel=1e-12)
    np.testing.assert_allclose(got["values"].view(np.float64), exp["values"].view(np.float64), rtol=1e-11)
    np.testing.assert_allclose(got["weights"], exp["weights"], rtol=1e-9, atol=1e-300)
    assert list(got["betas"]) == [1.0]


@pytest.mark.parametrize("method", [E.RESAMPLE_SYSTEMATIC, E.RESAMPLE_STRATIFIED, E.RESAMPLE_MULTINOMIAL])
def test_smc_tempered_matches_oracle(oracle, method):
    """The full ladder (next_beta bisection, reweight, evidence, resample, gather, tempered
    rejuvenation with the per-sweep adaptation) against the oracle in its batched-adaptation mode."""
    cp, got, exp = _smc_pair(oracle, W.smc_normal(), 3000, seed=42, R=3, method=method)
    np.testing.assert_allclose(got["betas"], exp["betas"], rtol=1e-9)
    assert got["log_evidence"] == pytest.approx(exp["log_evidence"], rel=1e-9)
    g, o = got["values"].view(np.float64)[0], exp["values"].view(np.float64)[0]
    bad = ~np.isclose(g, o, rtol=1e-9, atol=1e-12)
    if bad.any(): knife.used("adaptive_smc: particle values", method=method, particles=np.nonzero(bad)[0].tolist())
    assert bad.sum() <= 3, bad.sum()                   # a knife-edge accept / resample boundary
    np.testing.assert_allclose(got["weights"][~bad], exp["weights"][~bad], rtol=1e-8)
    assert got["n_model_runs"] == exp["n_model_evals"]


@pytest.mark.parametrize("name", ["smc_normal", "refmodel8"])
def test_smc_sequential_adaptation_is_the_references_order(oracle, name):
    """fg_smc_config.sequential_adaptation: particle-major moves with ONE DiminishingAdaptation updated after every move
    (smc.rs:482,544-553,698-713) -- the reference's own semantics, against the oracle's unbatched form: the beta ladder, the
    evidence, every particle and weight.  (The default, batched per sweep, is the documented deviation; this mode closes it.)"""
    from tests.models import ZOO
    prog = W.smc_normal() if name == "smc_normal" else ZOO[name]()
    cp, got, exp = _smc_pair(oracle, prog, 1500, seed=42, R=3, sequential=True)
    np.testing.assert_allclose(got["betas"], exp["betas"], rtol=1e-9)
    assert got["log_evidence"] == pytest.approx(exp["log_evidence"], rel=1e-9)
    bad = np.zeros(1500, dtype=bool)
    for j in range(cp.S):
        bad |= ~np.isclose(got["values"].view(np.float64)[j], exp["values"].view(np.float64)[j], rtol=1e-9, atol=1e-12)
    # an accept on a knife edge changes that particle AND, through the shared adaptation, every later scale by ~1e-4: the comparison is
    # exact or it visibly is not
    assert bad.sum() == 0, bad.sum()
    np.testing.assert_allclose(got["weights"], exp["weights"], rtol=1e-8)
    assert got["n_model_runs"] == exp["n_model_evals"]
    _, got_b, _ = _smc_pair(oracle, prog, 1500, seed=42, R=3)
    assert not np.array_equal(got_b["values"], got["values"])            # ... and it is not the batched form


@pytest.mark.parametrize("n_sites", [6, 40])
def test_smc_multisite_model_matches_oracle(oracle, n_sites):
    """(40 sites: sixteen tiles of 41 rows do not fit a block's LDS -- the rejuvenation kernel takes the tiles per block that do;
    round 3 returned FG_E_LIMIT there)"""
    cp, got, exp = _smc_pair(oracle, W.reference_model(n_sites), 2048, seed=7, R=2)
    np.testing.assert_allclose(got["betas"], exp["betas"], rtol=1e-8)
    assert got["log_evidence"] == pytest.approx(exp["log_evidence"], rel=1e-8)
    g, o = got["values"].view(np.float64), exp["values"].view(np.float64)
    bad = (~np.isclose(g, o, rtol=1e-8, atol=1e-11)).any(axis=0)
    assert bad.sum() <= 4, bad.sum()


def test_smc_million_particles_closed_form():
    """BASELINE C4: mu ~ N(0,1), y ~ N(mu, 0.5) = 1.5 with 1 048 576 particles, Systematic / 0.5 /
    3 rejuvenation moves (examples/smc_inference.rs:36-65): posterior N(1.2, 0.2),
    log Z = -1.9305103088617774."""
    cp = E.compile_model(W.smc_normal())
    n = 1 << 20
    eng = E.Engine(cp, n, seed=42)
    r = eng.smc_run(rejuvenation_steps=3)
    mu = r["values"].view(np.float64)[0]
    mean = float((r["weights"] * mu).sum())
    var = float((r["weights"] * (mu - mean) ** 2).sum())
    assert abs(r["log_evidence"] - (-1.9305103088617774)) < 5e-3
    assert abs(mean - 1.2) < 5e-3 and abs(var - 0.2) < 5e-3
    assert abs(r["weights"].sum() - 1.0) < 1e-9 and len(r["betas"]) >= 2 and r["betas"][-1] == 1.0


def test_standalone_smc_building_blocks(oracle):
    """smc_prior_particles / normalize_particles / effective_sample_size / resample_particles / rejuvenate_particles
    (smc.rs:230-233, 326-349, 698-790) as separate calls over the engine's population."""
    N = 5000
    cp = E.compile_model(W.smc_normal())
    eng = E.Engine(cp, N, seed=42)
    with pytest.raises(E.EngineError):
        eng.smc_ess()                                               # no population yet
    eng.smc_prior_particles()
    lw, w = eng.smc_weights()
    mu = eng.get_values()[0].view(np.float64)
    ll = -0.5 * ((1.5 - mu) / 0.5) ** 2 - np.log(0.5) - 0.5 * np.log(2 * np.pi)
    assert np.allclose(lw, ll, rtol=1e-12)                          # log_weight = log-likelihood only (FG-03)
    ref = np.exp(lw - oracle.log_sum_exp(lw)); ref /= ref.sum()
    assert np.allclose(w, ref, rtol=1e-12) and abs(w.sum() - 1.0) < 1e-12
    assert eng.smc_ess() == pytest.approx(1.0 / np.sum(w * w), rel=1e-12)
    assert eng.smc_ess() == pytest.approx(oracle.ess_particles(w), rel=1e-12)
    assert abs(np.sum(w * mu) - 1.2) < 0.05                         # importance-sampling posterior mean of C4
    # all log-weights -inf -> uniform fallback (smc.rs:735-741)
    eng.smc_set_log_weights(np.full(N, -np.inf)); eng.smc_normalize()
    assert np.array_equal(eng.smc_weights()[1], np.full(N, 1.0 / N))
    eng.smc_set_log_weights(lw); eng.smc_normalize()
    assert np.allclose(eng.smc_weights()[1], ref, rtol=1e-12)
    # resample: the ancestors are those of the tested index primitive for the same uniform; clones; weights exactly 1/N
    before = eng.get_values().copy()
    idx = eng.smc_resample(E.RESAMPLE_SYSTEMATIC, step=3)
    import ctypes
    st = oracle.stream(42, 0, 3, 5)                                 # (seed, chain 0, step, FG_RNG_SMC_RESAMPLE)
    oracle.lib().orc_stream_u01.restype = ctypes.c_double
    U = oracle.lib().orc_stream_u01(ctypes.byref(st))
    assert np.array_equal(idx, E.device_resample_indices(E.RESAMPLE_SYSTEMATIC, w, U))
    assert idx.min() >= 0 and idx.max() < N and (np.diff(idx) >= 0).all()
    assert np.array_equal(eng.get_values(), before[:, idx])
    lw2, w2 = eng.smc_weights()
    assert np.array_equal(w2, np.full(N, 1.0 / N)) and np.array_equal(lw2, np.full(N, np.log(1.0 / N)))
    assert eng.smc_ess() == pytest.approx(N, rel=1e-9)
    # rejuvenation moves particles, leaves the weights exactly uniform (tests/f_smc_smc.rs:45-205) and targets pi_1
    acc = eng.smc_rejuvenate(1.0, 5)
    assert 0.1 < acc < 0.95
    assert np.array_equal(eng.smc_weights()[1], np.full(N, 1.0 / N))
    mu2 = eng.get_values()[0].view(np.float64)
    assert (mu2 != before[0, idx].view(np.float64)).mean() > 0.3
    assert abs(mu2.mean() - 1.2) < 0.05 and abs(mu2.var() - 0.2) < 0.05


@pytest.mark.parametrize("model,n", [("normal_sites400", 128), ("mixture", 3000)])
def test_standalone_rejuvenate_takes_the_runs_sweep(model, n, monkeypatch):
    """smc_prior_particles -> smc_resample -> smc_rejuvenate(beta, 2) launches its sweeps through fg_smc_run's launcher (smc_rejuv_sweep):
    on a program beyond the block histogram (400 sites: the tile in global memory, one wave per block, whatever FG_JIT says) and on a
    stream program with Categorical records (the compiled sweep under FG_JIT=1, k_smc_rejuv<3> under FG_JIT=0).  Which kernel runs does
    not change a result: particles, weights and accept rate are the same under both settings, bit for bit."""
    from tests.models import ZOO
    cp = E.compile_model(W.normal_sites(400) if model == "normal_sites400" else ZOO[model]())
    out = []
    for jit in ("0", "1"):
        monkeypatch.setenv("FG_JIT", jit)
        eng = E.Engine(cp, n, seed=23)
        eng.smc_prior_particles()
        idx = eng.smc_resample(E.RESAMPLE_SYSTEMATIC, step=1)
        before = eng.get_values().copy()
        acc = eng.smc_rejuvenate(0.37, 2)
        lw, w = eng.smc_weights()
        out.append((idx, eng.get_values(), lw, w, np.float64(acc)))
        eng.close()
        assert 0.0 < acc < 1.0 and (out[-1][1] != before).any()                   # the sweeps ran and moved particles
        assert np.array_equal(w, np.full(n, 1.0 / n))                             # ... and left the weights alone (FG-13)
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b, equal_nan=True)


def test_next_beta_zoom_passes_agree_with_the_plain_passes():
    """next_beta brackets the ESS crossing by zoom passes and replays the reference's 64 halvings from the bracket;
    FG_SMC_ZOOM=0 evaluates every halving (three levels per pass).  Both follow the same comparisons `ESS(mid) < target` wherever the
    evaluated ESS is monotone: the ladders agree to a few units in the last place, the evidence to rounding.  (The switch is read once per
    process: tools/ab_smc_zoom.py runs each setting in a child process -- six models, ladders of 2 to ~20 steps, up to 1 048 576 particles.)"""
    import os, re, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "tools", "ab_smc_zoom.py")], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    rows = re.findall(r"^(\S+)\s+steps (\d+)/(\d+)\s+max \|d beta\| (\S+)\s+d logZ (\S+)", out.stdout, flags=re.M)
    assert len(rows) == 6, out.stdout
    for name, s0, s1, db, dz in rows:
        assert s0 == s1, (name, s0, s1)
        assert float(db) <= 1e-14 and float(dz) <= 1e-12, (name, db, dz)


def test_smc_separate_kernels_path_agrees_with_the_fused_launch(monkeypatch):
    """What follows next_beta's last pass is one launch (k_smc_ess2_apply) unless beta' = beta + 1e-9 -- no candidate of any pass -- when the
    separate maximum / sum / finish / apply / scan kernels take the step.  FG_SMC_FORCE_SUM=1 sends every step down that path: the same
    ladder, the evidence and the weights to rounding (the fused launch takes the reweight's sum from the pass that evaluated beta')."""
    cp = E.compile_model(W.normal_sites(8))
    out = []
    for force in ("0", "1"):
        monkeypatch.setenv("FG_SMC_FORCE_SUM", force)
        eng = E.Engine(cp, 20000, seed=9)
        r = eng.smc_run(rejuvenation_steps=2, ess_threshold=0.5)
        out.append(r)
        eng.close()
    a, b = out
    assert len(a["betas"]) >= 3 and np.array_equal(a["betas"], b["betas"])
    assert a["log_evidence"] == pytest.approx(b["log_evidence"], rel=1e-13)
    bad = ~np.isclose(a["values"].view(np.float64), b["values"].view(np.float64), rtol=1e-12, atol=0).all(axis=0)
    assert bad.sum() <= 2, int(bad.sum())                 # (a resampling threshold within rounding of a cumulative weight)
    np.testing.assert_allclose(a["weights"][~bad], b["weights"][~bad], rtol=1e-10)


@pytest.mark.parametrize("method", [0, 1, 2])
def test_adaptive_smc_edge_population_sizes(method):
    """Populations around every grain of the kernels -- one particle, a wave, a scan chunk of 2 048, their neighbours, a prime -- for the
    three resamplers: a finite evidence, weights that sum to one, a strictly increasing ladder that ends at one."""
    cp = E.compile_model(W.normal_sites(8))
    for N in (1, 2, 63, 64, 65, 2047, 2048, 2049, 4097, 100003):
        eng = E.Engine(cp, N, seed=11)
        r = eng.smc_run(rejuvenation_steps=2, ess_threshold=0.5, resampling_method=method)
        eng.close()
        assert np.isfinite(r["log_evidence"]), N
        assert abs(r["weights"].sum() - 1.0) < 1e-9 and (r["weights"] >= 0).all(), N
        assert r["betas"][-1] == 1.0 and (np.diff(r["betas"]) > 0).all(), (N, r["betas"])


# ---- whole ladders against the oracle where the tempering step is hardest ---------------------------------------------------------
def _tie_model():
    """Log-likelihoods with only a few distinct values: two discrete latents, each with an observation whose mean is a constant picked by
    the latent (the pattern of workloads.mixture with the component means given).  No f64 site: rejuvenation moves nothing, the ties
    survive every step, and each step's log-likelihoods are the resampled ones of the step before."""
    from fugue_amd.model import Categorical, Normal, Program, addr, select
    P = Program()
    for i, xi in enumerate((1.3, -0.4)):
        z = P.sample(addr("z", i), Categorical([0.1, 0.2, 0.3, 0.4]))
        P.observe(addr("x", i), Normal(select(z, [-6.0, -2.0, 2.0, 6.0]), 1.0), xi)
    return P


def _resample_host(oracle, w, method, seed, step):
    n = w.size
    if method == E.RESAMPLE_SYSTEMATIC:
        u = np.array([oracle.lib().orc_stream_u01(oracle.stream(seed, 0, step, 5))])
        return oracle.systematic_indices(w, u[0]), (u[0] / n + np.arange(n) / n)
    u = np.array([oracle.lib().orc_stream_u01(oracle.stream(seed, j, step, 5)) for j in range(n)])   # ORC_RNG_SMC_RESAMPLE
    if method == E.RESAMPLE_STRATIFIED:
        return oracle.stratified_indices(w, u), (np.arange(n) + u) / n
    return oracle.multinomial_indices(w, u), u


def _judged_tie_ladder(oracle, N, method, seed):
    """fg_smc_run on the tie model against the oracle's smc_run: every step's beta through the judge on that step's log-likelihoods (the
    ladder replayed on the host with the oracle's primitives, from the device's prior draw), the evidence within the sum of the steps'
    log-normaliser tolerances, the particles exactly unless a resampling threshold lay within 1e-12 of a cumulative weight."""
    from tests import smc_judge as J
    prog = _tie_model()
    cp, om = E.compile_model(prog), oracle.OracleModel(prog)
    eng = E.Engine(cp, N, seed=seed)
    eng.smc_prior_particles(0)                          # fg_smc_run's prior draw (iteration 0, the SMC prior stream)
    ll = eng.smc_weights()[0].copy()                     # log_weight = log_likelihood before any reweight
    got = eng.smc_run(rejuvenation_steps=1, ess_threshold=0.5, resampling_method=method)
    eng.close()
    exp = om.smc_run(N, seed, method=method, ess_threshold=0.5, rejuvenation_steps=1, batched=1)
    assert len(np.unique(ll)) <= 16
    lw0, target = -math.log(N), min(max(0.5 * N, 1.0), float(N))
    # the replay follows the DEVICE's ladder, so that every step is judged on the device's own population (the oracle's sums of tied
    # terms round alike: its betas may sit ~1e-12 off the exact crossing, and a resampling threshold may fall the other way)
    beta, steps, tol, logz, knife_edges, max_db = 0.0, 0, 0.0, 0.0, [], 0.0
    while beta < 1.0:
        steps += 1
        want = oracle.next_beta(beta, np.full(N, lw0), ll, target) if steps < 10000 else 1.0
        assert steps <= len(got["betas"]), (N, method, steps)
        b = got["betas"][steps - 1]
        assert J.accept(J.Curve(ll, beta), target, b, want, case=f"tie ladder N={N} method={method} step={steps}"), (N, method, steps, b, want)
        max_db = max(max_db, abs(b - want) * float(np.ptp(ll)))
        comb = lw0 + (b - beta) * ll
        ln = oracle.log_sum_exp(comb)
        logz += ln
        tol += J.log_norm_tol(ll, beta, b) + J.EPS * (N - 1)      # (+ the oracle's sequential sum)
        lw = comb - ln if math.isfinite(ln) else np.full(N, lw0)
        beta = b
        if beta < 1.0:
            w = np.exp(lw)
            idx, thr = _resample_host(oracle, w, method, seed, steps)
            cum = np.cumsum(w)
            near = np.minimum(np.abs(cum[idx] - thr), np.abs(np.where(idx > 0, cum[np.maximum(idx - 1, 0)], -1.0) - thr))
            if (near < 1e-12 + max_db).any():
                knife_edges.append((steps, int(np.argmin(near)), float(near.min())))
            ll = ll[idx]
    assert len(got["betas"]) == steps == len(exp["betas"]) and got["betas"][-1] == 1.0
    np.testing.assert_allclose(got["betas"], exp["betas"], rtol=1e-9, atol=0)
    assert abs(got["log_evidence"] - logz) <= tol, (got["log_evidence"], logz, tol)
    assert got["log_evidence"] == pytest.approx(exp["log_evidence"], rel=1e-9)
    assert got["n_model_runs"] == exp["n_model_evals"]
    bad = (got["values"] != exp["values"]).any(axis=0)
    if bad.any():
        assert knife_edges and bad.mean() < 0.01, (int(bad.sum()), knife_edges)
        knife.used("tie ladder: resampling indices", N=N, method=method, particles=int(bad.sum()), threshold_minus_cum=knife_edges)
    np.testing.assert_allclose(got["weights"][~bad], exp["weights"][~bad], rtol=1e-9, atol=0)
    return got


@pytest.mark.parametrize("method", [E.RESAMPLE_SYSTEMATIC, E.RESAMPLE_STRATIFIED, E.RESAMPLE_MULTINOMIAL])
@pytest.mark.parametrize("N", [2048, 131073])
def test_tie_heavy_ladder_matches_the_oracle(oracle, N, method):
    """The in-process parity of the tempering step where it is hardest: log-likelihoods with a handful of distinct values, every step."""
    got = _judged_tie_ladder(oracle, N, method, seed=21)
    assert len(got["betas"]) >= 3


@pytest.mark.parametrize("method", [0, 1, 2])
def test_adaptive_smc_edge_population_sizes_match_the_oracle(oracle, method):
    """The edge population sizes of test_adaptive_smc_edge_population_sizes against the oracle's batched smc_run: with rejuvenation
    (normal_sites(8)) the ladder to 1e-9, the evidence to rel 1e-9 and the model-run count exactly; on the tie model every step's beta
    through the judge (the per-step log-likelihoods are known there)."""
    prog = W.normal_sites(8)
    cp, om = E.compile_model(prog), oracle.OracleModel(prog)
    for N in (1, 2, 63, 64, 65, 2047, 2048, 2049, 4097):
        eng = E.Engine(cp, N, seed=11)
        r = eng.smc_run(rejuvenation_steps=2, ess_threshold=0.5, resampling_method=method)
        eng.close()
        exp = om.smc_run(N, 11, method=method, ess_threshold=0.5, rejuvenation_steps=2, batched=1)
        assert len(r["betas"]) == len(exp["betas"]), (N, r["betas"], exp["betas"])
        np.testing.assert_allclose(r["betas"], exp["betas"], rtol=1e-9, atol=0, err_msg=str(N))
        assert r["log_evidence"] == pytest.approx(exp["log_evidence"], rel=1e-9), N
        assert r["n_model_runs"] == exp["n_model_evals"], N
        _judged_tie_ladder(oracle, N, method, seed=11)
