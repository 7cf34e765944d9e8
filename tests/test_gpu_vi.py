"""Mean-field VI on the GPU (fg_vi.hip through the C ABI and fugue_amd.vi) against the plain-Python restatement of vi.rs
(tests/vi_restatement.py): per-sample terms and draws, the two summation orders bit for bit, common-random-numbers exactness, the
optimizer step for step, the posteriors it reaches, the boundaries, estimate_elbo.  Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import model as M
from fugue_amd import vi as V
from fugue_amd import workloads as W
from tests import vi_restatement as R
from tests.test_gpu_parity import _close
from tests.test_vi_cpu import POSTERIOR_BAR

pytestmark = pytest.mark.gpu


def gamma_model() -> M.Program:
    """A positive latent: sigma ~ Gamma(2, 0.5); y#i ~ Normal(0, sigma) observed."""
    P = M.Program()
    s = P.sample(M.addr("sigma"), M.Gamma(2.0, 0.5))
    for i, y in enumerate((0.8, -1.1, 2.3)):
        P.observe(M.addr("y", i), M.Normal(0.0, s), y)
    return P


def observe_only() -> M.Program:
    P = M.Program()
    P.observe(M.addr("y"), M.Normal(0.0, 1.0), 0.5)
    return P


def _logistic():
    return W.logistic_regression(*W.classification_data(14)[:2])


TERM_CASES = {
    # name: (program, guide row without site indices: (family, a, b) per site, extra stray factor or None)
    "conjugate-normal": (W.readme_normal, [(0, 0.3, -0.4)], None),
    "gamma-lognormal": (gamma_model, [(1, 0.2, -0.7)], (0, "zz", 1.0, 0.3)),
    "coin-beta": (W.coin_flip, [(2, math.log(3.0), math.log(2.0))], None),
    "logistic-normal": (_logistic, [(0, -0.5, -0.3), (0, 1.0, -0.5), (0, -0.8, -0.2)], None),
}


def _row(cp, facs, stray):
    row = [(f, j, a, b) for j, (f, a, b) in enumerate(facs)]
    if stray is not None:
        row.append((stray[0], -1, stray[2], stray[3]))    # its address sorts after every site of these models
    return row


@pytest.mark.parametrize("name", list(TERM_CASES))
def test_terms_and_draws_match_the_restatement(oracle, name):
    """Tolerances of tests/test_gpu_parity.py: terms 1e-12 relative (its log-joint accumulators), draws 1e-11 (its prior draws).
    Beta factors only: a sample whose DRAW differs (a rejection loop of the Gamma sampler took another branch under ocml than
    under glibc) is left out, at most 0.1 % of the samples; Normal and LogNormal allow no exclusion."""
    make, facs, stray = TERM_CASES[name]
    prog = make()
    cp, om = E.compile_model(prog), oracle.OracleModel(prog)
    row = _row(cp, facs, stray)
    N, seed, sid, c0 = 2000 if name == "coin-beta" else 200, 23, 5, 1000
    eng = E.Engine(cp, N, seed=seed, chain_offset=c0)
    elbo, terms = eng.vi_elbo_batch([row, row], [sid, sid + 1], want_terms=True)
    got = np.ascontiguousarray(eng.get_values()).view(np.float64)             # the guide traces of evaluation 0
    eng.close()
    print(f"{name}: score-stream records {cp.stream_records[1]} (0 = interpreter only), ELBO {elbo[0]:.6f}")
    if name == "logistic-normal":
        assert cp.stream_records[1] == 0
    exp_t, exp_d = R.sample_terms(oracle, om, row, seed, N, sid, sample0=c0)
    exp_sites = exp_d[:, :cp.S].T
    keep = np.ones(N, dtype=bool)
    if name == "coin-beta":
        keep = (np.abs(got - exp_sites) <= 1e-300 + 1e-11 * np.abs(exp_sites)).all(axis=0)
        print(f"{name}: {int((~keep).sum())} of {N} samples left out (draw differs), cap {N // 1000}")
        assert (~keep).sum() <= N // 1000
    rel_d = np.abs(got - exp_sites)[:, keep] / np.maximum(np.abs(exp_sites[:, keep]), 1e-300)
    rel_t = np.abs(terms[0] - exp_t)[keep] / np.maximum(np.abs(exp_t[keep]), 1.0)
    print(f"{name}: max relative draw difference {rel_d.max():.3e}, max term difference / max(|term|, 1) {rel_t.max():.3e}")
    _close(got[:, keep], exp_sites[:, keep], 1e-11, 1e-300)
    _close(terms[0][keep], exp_t[keep], 1e-12, 1e-12)
    exp_t1, _ = R.sample_terms(oracle, om, row, seed, N, sid + 1, sample0=c0)  # another stream id: other draws, same parity
    if name != "coin-beta":
        _close(terms[1], exp_t1, 1e-12, 1e-12)
    assert not np.array_equal(terms[0], terms[1])


@pytest.mark.parametrize("N", [64, 65, 4096, 65536])
def test_elbo_is_the_documented_sum_of_the_terms(N):
    cp = E.compile_model(W.normal_sites(32))
    ls = V.init_log_sigma(0.0)
    rows = [[(0, j, 0.1 * k, ls + 0.2 * k) for j in range(cp.S)] for k in range(3)]
    eng = E.Engine(cp, N, seed=4)
    elbo, terms = eng.vi_elbo_batch(rows, [0, 7, 7], want_terms=True)
    elbo_only = eng.vi_elbo_batch(rows, [0, 7, 7])
    eng.close()
    for k in range(3):
        exp = R.elbo_of_terms(terms[k])
        print(f"N = {N}, evaluation {k}: ELBO {elbo[k]!r}, numpy restatement of the two orders {exp!r}")
        assert elbo[k] == exp and elbo_only[k] == elbo[k]


def test_global_tile_form_gives_the_same_bits(monkeypatch):
    cp = E.compile_model(W.reference_model(8))
    row = [(0, j, 0.1, -0.5) for j in range(cp.S)]
    out = []
    for gt in ("0", "1"):
        monkeypatch.setenv("FG_GLOBAL_TILE", gt)
        eng = E.Engine(cp, 300, seed=8)
        out.append(eng.vi_elbo_batch([row, row], [1, 2], want_terms=True))
        eng.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])


def test_common_random_numbers_are_exact_on_the_conjugate_model():
    """Location coordinate of the conjugate model: log p is quadratic in x and log q does not change under a shift of m with z fixed,
    so the central difference is the sample mean of d log p / dx at the drawn x up to the rounding of two sums over 2 eps."""
    cp = E.compile_model(W.readme_normal())
    row, eps, N = [(0, 0, 0.3, -0.4)], 0.01, 4096
    eng = E.Engine(cp, N, seed=9)
    elbo, terms = eng.vi_elbo_batch([row, R.shifted(row, 0, 0, eps), R.shifted(row, 0, 0, -eps)], [0, 0, 0], want_terms=True)
    x = np.ascontiguousarray(eng.get_values()).view(np.float64)[0]
    eng.close()
    grad = (elbo[1] - elbo[2]) / (2.0 * eps)
    exact = float(np.mean(-x + (1.2 - x) / 0.25))
    bound = 8.0 * np.abs(terms).max() * 2.0 ** -52 / eps
    print(f"CRN gradient {grad!r}, mean of d log p / dx {exact!r}, |difference| {abs(grad - exact):.3e}, bound {bound:.3e}")
    assert abs(grad - exact) <= bound
    g2 = V.elbo_gradient_fd(9, cp, V.MeanFieldGuide({M.addr("mu"): V.VariationalParam.Normal(0.3, -0.4)}), M.addr("mu"), V.ParamCoord.Location, eps, N)
    e2 = V.elbo_with_guide(9, cp, V.MeanFieldGuide({M.addr("mu"): V.VariationalParam.Normal(0.3, -0.4)}), N)
    assert g2 == grad and e2 == elbo[0]                    # the Python drivers are these evaluations: stream id 0 of seed 9
    assert V.elbo_gradient_fd(9, cp, V.MeanFieldGuide(), M.addr("mu"), V.ParamCoord.Location, eps, N) == 0.0      # vi.rs:696-699


OPT_CASES = {"conjugate-normal": (W.readme_normal, lambda: V.VariationalParam.for_support(V.Support.Real, 0.0)),
             "gamma-lognormal": (gamma_model, lambda: V.VariationalParam.for_support(V.Support.Positive, 1.0))}


@pytest.mark.parametrize("name", list(OPT_CASES))
def test_optimizer_follows_the_restatement(oracle, name):
    """Same seed, N = 256, 50 iterations.  Every guide parameter within 10 n_iter lr 1e-12 max|term| / (2 fd_eps): the per-iteration
    parity error of an ELBO (1e-12 max|term|) through the central difference (/ 2 fd_eps) and the update (x lr), accumulated over the
    iterations without assuming contraction; x 10 for the monitor and the two signs.  The history within the ELBO's own parity error
    plus that bound times the largest gradient the restatement saw."""
    make, init = OPT_CASES[name]
    prog = make()
    cp, om = E.compile_model(prog), oracle.OracleModel(prog)
    p0 = init()
    N, n_iter, lr, fd_eps, seed = 256, 50, 0.1, 0.01, 31
    cfg = V.VIConfig(n_iterations=n_iter, n_samples_per_iter=N, base_learning_rate=lr, fd_eps=fd_eps)
    res = V.optimize_meanfield_vi_with_config(seed, cp, V.MeanFieldGuide({cp.site_names[0]: p0}), cfg)
    row0 = [(p0.family, 0, p0.a, p0.b)]
    exp_row, exp_hist, exp_conv, exp_it, info = R.optimize(oracle, om, row0, seed, N, n_iterations=n_iter, base_learning_rate=lr, fd_eps=fd_eps)
    max_term = max(np.abs(R.sample_terms(oracle, om, r, seed, N, 0)[0]).max() for r in (row0, exp_row))
    bound = 10.0 * n_iter * lr * 1e-12 * max_term / (2.0 * fd_eps)
    got = res.guide.params[cp.site_names[0]]
    dev = max(abs(got.a - exp_row[0][2]), abs(got.b - exp_row[0][3]))
    hist_tol = 1e-12 * max_term + bound * max(1.0, info["max_grad"])
    print(f"{name}: GPU ({got.a!r}, {got.b!r}), restatement ({exp_row[0][2]!r}, {exp_row[0][3]!r}); largest parameter deviation {dev:.3e}, "
          f"bound {bound:.3e}; iterations {res.iterations} / {exp_it}, converged {res.converged} / {exp_conv}")
    assert dev <= bound
    assert res.iterations == exp_it and len(res.elbo_history) == exp_it
    hd = np.abs(res.elbo_history - exp_hist).max()
    print(f"{name}: largest history deviation {hd:.3e}, tolerance {hist_tol:.3e}; plateau statistics {info['plateau'][:3]} ...")
    assert hd <= hist_tol
    margin = 4.0 * hist_tol / max(np.abs(exp_hist).min(), 1e-8)                  # the plateau statistic is no knife edge for this seed
    assert all(abs(st - cfg.convergence_tol) > margin for st in info["plateau"])
    assert res.converged == exp_conv


@pytest.mark.parametrize("name", ["readme", "normal32"])
def test_optimizer_reaches_the_closed_form_posterior(name):
    """N = 65 536 samples per evaluation.  Bar: the restatement's own largest deviation from the closed form at N_small samples
    (tests/test_vi_cpu.py: POSTERIOR_BAR, a CPU run), scaled by sqrt(N_small / N) for the Monte Carlo error, margin 4."""
    bar = POSTERIOR_BAR[name]
    prog = W.readme_normal() if name == "readme" else W.normal_sites(32)
    cp = E.compile_model(prog)
    N = 65536
    guide = V.MeanFieldGuide()
    for a in cp.site_names:
        guide.add_latent(a, V.Support.Real, 0.0)
    cfg = V.VIConfig(n_iterations=bar["n_iterations"], n_samples_per_iter=N, base_learning_rate=bar["base_learning_rate"], convergence_window=0)
    res = V.optimize_meanfield_vi_with_config(bar["seed"], cp, guide, cfg)
    means = np.array([0.96]) if name == "readme" else W.normal_sites_truth(32)[1]
    m = np.array([res.guide.params[a].mu for a in cp.site_names])
    ls = np.array([res.guide.params[a].log_sigma for a in cp.site_names])
    dev = max(np.abs(m - means).max(), np.abs(ls - 0.5 * math.log(0.2)).max())
    tol = 4.0 * bar["deviation"] * math.sqrt(bar["n_small"] / N)
    print(f"{name}: largest |parameter - closed form| {dev:.3e} after {res.iterations} iterations, tolerance {tol:.3e} "
          f"(restatement at N = {bar['n_small']}: {bar['deviation']:.3e}); sigma {np.exp(ls).min():.6f} .. {np.exp(ls).max():.6f}")
    assert res.iterations == bar["n_iterations"] and not res.converged
    assert dev <= tol


def test_support_mismatch_gives_minus_infinity_and_moves_nothing():
    """A Normal factor on the Gamma latent: half the draws are outside the support, every ELBO is -inf, every gradient NaN."""
    cp = E.compile_model(gamma_model())
    guide = V.MeanFieldGuide({M.addr("sigma"): V.VariationalParam.Normal(0.0, 0.0)})
    assert V.elbo_with_guide(3, cp, guide, 256) == -math.inf
    res = V.optimize_meanfield_vi_with_config(3, cp, guide, V.VIConfig(n_iterations=45, n_samples_per_iter=256))
    p = res.guide.params[M.addr("sigma")]
    assert (p.family, p.a, p.b) == (0, 0.0, 0.0) and res.iterations == 45 and not res.converged
    assert np.all(res.elbo_history == -np.inf)


def test_errors():
    cp = E.compile_model(W.normal_sites(4))
    ok = [(0, j, 0.0, 0.0) for j in range(4)]
    eng = E.Engine(cp, 64, seed=1)
    with pytest.raises(E.EngineError) as ei:                                    # a missing factor: ScoreGivenTrace's panic
        eng.vi_elbo_batch([ok[:3]], [0])
    assert ei.value.code == M.ErrorCode.TraceAddressNotFound and "x#3" in E.last_error()
    for bad, code in [((0, 1, float("nan"), 0.0), 100), ((1, 1, 0.0, float("inf")), 101), ((2, 1, float("-inf"), 0.0), 104)]:
        with pytest.raises(E.EngineError) as ei:
            eng.vi_elbo_batch([[ok[0], bad, ok[2], ok[3]]], [0])
        assert ei.value.code == code and "non-finite" in E.last_error()
        with pytest.raises(E.EngineError) as ei:
            eng.vi_optimize([ok[0], bad, ok[2], ok[3]], V.VIConfig(n_iterations=2).raw())
        assert ei.value.code == code
    with pytest.raises(E.EngineError) as ei:
        eng.vi_elbo_batch([[(3, 0, 0.0, 0.0)] + ok[1:]], [0])                    # no such family
    assert ei.value.code == E.FG_E_BAD_ARG
    with pytest.raises(E.EngineError) as ei:
        eng.vi_elbo_batch([[ok[1], ok[0], ok[2], ok[3]]], [0])                   # not in address order
    assert ei.value.code == E.FG_E_BAD_ARG
    import ctypes                                                               # n_iterations (2P + 1) >= 2^32: refused before any iteration
    hist, res, big = np.zeros(4), E.fg_vi_result(), V.VIConfig(n_iterations=2 ** 31 - 1).raw()
    rc = E.lib().fg_vi_optimize(eng.h, eng._vi_factors([ok]), 4, ctypes.byref(big), hist.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), ctypes.byref(res))
    assert rc == E.FG_E_LIMIT and "2^32" in E.last_error()
    assert np.isfinite(eng.vi_elbo_batch([ok], [0])[0])                          # the engine is still usable
    eng.close()
    guide = V.MeanFieldGuide()
    for a in cp.site_names[:3]:
        guide.add_latent(a, V.Support.Real, 0.0)
    with pytest.raises(M.FugueError) as fe:                                      # the Python drivers raise the typed error
        V.elbo_with_guide(1, cp, guide, 64)
    assert fe.value.code == M.ErrorCode.TraceAddressNotFound
    mix = E.compile_model(W.mixture(W.mixture_data(6)[0]))                        # discrete sample sites: UnsupportedDiscreteLatent
    g = V.MeanFieldGuide()
    for a, vt in zip(mix.site_names, mix.site_vtypes):
        if vt == 0:
            g.add_latent(a, V.Support.Real, 0.0)
    with pytest.raises(M.FugueError) as fe:
        V.optimize_meanfield_vi(1, mix, g, 3, 64, 0.1)
    assert fe.value.code == M.ErrorCode.TraceAddressNotFound and "discrete latent" in str(fe.value)


def test_observe_only_program_with_an_empty_guide(oracle):
    cp = E.compile_model(observe_only())
    eng = E.Engine(cp, 100, seed=2)
    elbo, terms = eng.vi_elbo_batch([[]], [0], want_terms=True)
    out, hist, conv, it = eng.vi_optimize([], V.VIConfig(n_iterations=3).raw())
    eng.close()
    lp = oracle.logpdf("Normal", 0.5, [0.0, 1.0])
    assert np.all(terms[0] == terms[0][0]) and terms[0][0] == pytest.approx(lp, rel=1e-12)
    assert elbo[0] == R.elbo_of_terms(terms[0]) and out == [] and it == 3 and np.all(hist == elbo[0])


def test_estimate_elbo_is_the_documented_mean_of_the_prior_runs_likelihood():
    for prog, N in ((W.readme_normal(), 1000), (W.coin_flip(), 4096), (_logistic(), 130)):
        cp = E.compile_model(prog)
        eng = E.Engine(cp, N, seed=6)
        got, got0 = eng.vi_estimate_elbo(2), eng.vi_estimate_elbo(0)
        acc = eng.prior_init(iteration=2)
        eng.close()
        exp = R.elbo_of_terms(acc[1] + acc[2])
        print(f"estimate_elbo {got!r}, restated from prior_init's accumulators {exp!r}")
        assert got == exp and math.isfinite(got)
        assert V.estimate_elbo(6, cp, N) == got0
