"""Mean-field VI without a GPU: the guide bookkeeping of fugue_amd.vi against the reference's known answers (vi.rs:245-279, 412-415,
457-483, 577-600, 747-759), the plain-Python restatement (tests/vi_restatement.py) against the closed-form ELBO, and the ABI's new
symbols.  None of this exists on the parent commit (no fugue_amd.vi, no fg_vi_* symbol)."""
import ctypes
import math
import os

import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import model as M
from fugue_amd import vi as V
from fugue_amd import workloads as W
from tests import vi_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The posterior checks of tests/test_gpu_vi.py take their bar from the restatement at small N (never from the GPU code):
# the optimizer of vi.rs with the plateau test off, from for_support(Real, 0.0), run on the CPU.  (model, N_small, iterations) ->
# largest |parameter - closed form| over m and log_sigma of every factor.  test_posterior_bar_is_the_restatements re-derives the
# conjugate one; the 32-site one (minutes of CPU) is recorded from the same function, see DESIGN.md section 5.
# 200 iterations at learning rate 0.3: the noise-free recursion contracts log_sigma by (1 - 0.6 t^-0.6) per iteration (the ELBO's
# curvature in log_sigma is -10 sigma^2 = -2) and m faster, so what is left of the starting point after 200 iterations is below 1e-5
# and the deviation is Monte Carlo error, which is what scales with 1 / sqrt(N).
POSTERIOR_BAR = {
    "readme": dict(n_small=64, n_iterations=200, base_learning_rate=0.3, seed=11, deviation=0.014556623437597116),
    "normal32": dict(n_small=16, n_iterations=200, base_learning_rate=0.3, seed=11, deviation=0.0628438837157792),
}


def posterior_deviation(orc, name):
    """Runs the restatement's optimizer for POSTERIOR_BAR[name] and returns max |param - closed form|."""
    bar = POSTERIOR_BAR[name]
    prog = W.readme_normal() if name == "readme" else W.normal_sites(32)
    om = orc.OracleModel(prog)
    ls0 = V.init_log_sigma(0.0)
    row = [(0, j, 0.0, ls0) for j in range(om.S)]
    out, _, _, _, _ = R.optimize(orc, om, row, bar["seed"], bar["n_small"], n_iterations=bar["n_iterations"],
                                 base_learning_rate=bar["base_learning_rate"], convergence_window=0)
    if name == "readme":
        means = np.array([0.96])
    else:
        means = W.normal_sites_truth(32)[1]
    m = np.array([q[2] for q in out])
    ls = np.array([q[3] for q in out])
    return float(max(np.abs(m - means).max(), np.abs(ls - 0.5 * math.log(0.2)).max()))


def test_known_answer_values():
    assert V.init_log_sigma(0.0) == math.log(0.1)
    assert V.init_log_sigma(50.0) == math.log(5.0)
    assert V.init_log_sigma(float("nan")) == math.log(0.1)                      # non-finite: scale 1.0 -> max(0.1, 0.1)
    p = V.VariationalParam.for_support(V.Support.Positive, 2.0)
    assert (p.family, p.mu, p.log_sigma) == (1, math.log(2.0), math.log(0.5))
    p = V.VariationalParam.for_support(V.Support.Unit, 0.3)
    assert (p.family, p.log_alpha, p.log_beta) == (2, math.log(0.6), math.log(1.4))
    p = V.VariationalParam.for_support(V.Support.Real, -3.0)
    assert (p.family, p.mu, p.log_sigma) == (0, -3.0, math.log(0.1 * 3.0))
    # vi.rs:251-271: a non-finite or non-positive value falls back to 1.0 (Positive) / is clamped or replaced by 0.5 (Unit)
    for bad in (float("nan"), float("inf"), 0.0, -2.0):
        p = V.VariationalParam.for_support(V.Support.Positive, bad)
        assert (p.mu, p.log_sigma) == (0.0, math.log(0.5))
    p = V.VariationalParam.for_support(V.Support.Unit, float("nan"))
    assert (p.log_alpha, p.log_beta) == (math.log(1.0), math.log(1.0))
    p = V.VariationalParam.for_support(V.Support.Unit, 7.0)
    assert (p.log_alpha, p.log_beta) == (math.log(2.0 * (1.0 - 1e-3)), math.log(2.0 * (1.0 - (1.0 - 1e-3))))
    p = V.VariationalParam.for_support(V.Support.Unit, -1.0)
    assert p.log_alpha == math.log(2.0 * 1e-3)


def test_log_prob_and_sample_of_a_factor():
    n = V.VariationalParam.Normal(1.5, math.log(0.5))
    assert n.log_prob(1.5) == pytest.approx(-math.log(0.5) - 0.5 * math.log(2 * math.pi), rel=1e-15)
    ln = V.VariationalParam.LogNormal(0.0, 0.0)
    assert ln.log_prob(1.0) == pytest.approx(-0.5 * math.log(2 * math.pi), rel=1e-15) and ln.log_prob(-1.0) == -math.inf
    b = V.VariationalParam.Beta(math.log(2.0), math.log(2.0))
    assert b.log_prob(0.5) == pytest.approx(math.log(1.5), rel=1e-14) and b.log_prob(1.5) == -math.inf
    assert 0.0 < b.sample(3) < 1.0 and ln.sample(3) > 0.0 and n.sample(3) == n.sample(3)
    assert math.isnan(V.VariationalParam.Normal(float("nan"), 0.0).sample(1))  # vi.rs:298-300


def test_apply_update_clamps():
    p = V.VariationalParam.Normal(0.0, 0.0)
    p.apply_update(V.ParamCoord.Location, 1e9); assert p.mu == 1.0e6
    p.apply_update(V.ParamCoord.Location, -1e9); assert p.mu == -1.0e6
    p.apply_update(V.ParamCoord.Scale, 100.0); assert p.log_sigma == 20.0
    p.apply_update(V.ParamCoord.Scale, -100.0); assert p.log_sigma == -20.0
    q = V.VariationalParam.LogNormal(0.0, 0.0)
    q.apply_update(V.ParamCoord.Location, 1e9); q.apply_update(V.ParamCoord.Scale, -1e9)
    assert (q.mu, q.log_sigma) == (1.0e6, -20.0)
    b = V.VariationalParam.Beta(0.0, 0.0)
    b.apply_update(V.ParamCoord.Location, 1e9); b.apply_update(V.ParamCoord.Scale, -1e9)
    assert (b.log_alpha, b.log_beta) == (20.0, -20.0)
    for fam, coord, v in [(0, 0, 1e9), (0, 1, 1e9), (1, 0, -1e9), (2, 0, 1e9), (2, 1, -1e9)]:
        p = V.VariationalParam(fam, 0.0, 0.0)
        p.apply_update(coord, v)
        assert R.apply_update((fam, 0, 0.0, 0.0), coord, v)[2:] == (p.a, p.b)   # the restatement clamps alike
    s = V.VariationalParam.Beta(0.25, 0.5).shifted(V.ParamCoord.Scale, 0.01)
    assert (s.a, s.b) == (0.25, 0.51)


def test_config_defaults():
    c = V.VIConfig()
    assert (c.n_iterations, c.n_samples_per_iter, c.base_learning_rate, c.fd_eps, c.convergence_tol, c.convergence_window,
            c.step_decay_exponent) == (1000, 16, 0.1, 0.01, 1e-4, 20, 0.6)
    raw = E.fg_vi_config()
    E.lib().fg_vi_config_default(ctypes.byref(raw))
    assert (raw.n_iterations, raw.convergence_window, raw.base_learning_rate, raw.fd_eps, raw.convergence_tol,
            raw.step_decay_exponent) == (1000, 20, 0.1, 0.01, 1e-4, 0.6)


@pytest.mark.parametrize("vtype,name", [(1, "bool"), (2, "u64"), (3, "usize"), (4, "i64")])
def test_from_trace_refuses_discrete_latents(vtype, name):
    cells = np.array([np.array([1.5]).view(np.int64)[0], 1], dtype=np.int64)
    with pytest.raises(M.FugueError) as ei:
        V.MeanFieldGuide.from_trace(["a", "z"], [0, vtype], cells)
    assert isinstance(ei.value, V.GuideError) and ei.value.addr == "z" and ei.value.value_type == name
    g = V.MeanFieldGuide.from_trace(["a"], [0], cells[:1])
    assert (g.params["a"].family, g.params["a"].mu, g.params["a"].log_sigma) == (0, 1.5, math.log(0.1 * 1.5))


def test_guide_rows_are_address_sorted_with_stray_factors():
    cp = E.compile_model(W.normal_sites(12))
    g = V.MeanFieldGuide()
    for a in reversed(cp.site_names):
        g.add_latent(a, V.Support.Real, 0.0)
    g.add_latent("x#1a", V.Support.Positive, 2.0)          # no site of the model: between "x#10"/"x#11" and "x#2" in address order
    row = g.factor_row(cp)
    assert [q[1] for q in row if q[1] >= 0] == list(range(12)) and sum(q[1] < 0 for q in row) == 1
    names = g.sorted_addresses()
    assert names == sorted(names, key=lambda s: s.encode()) and row[names.index("x#1a")][:2] == (1, -1)


def test_stray_factor_changes_no_term(oracle):
    """vi.rs:659-664: a guide factor for an address the model never visits is drawn but contributes no log q.  Placed LAST in
    address order it leaves every model draw on its stream position, so every term is the same number."""
    om = oracle.OracleModel(W.readme_normal())
    row = [(0, 0, 0.3, -0.4)]
    t0, d0 = R.sample_terms(oracle, om, row, 5, 200, 7)
    t1, d1 = R.sample_terms(oracle, om, row + [(2, -1, 0.1, 0.2)], 5, 200, 7)
    assert np.array_equal(t0, t1) and np.array_equal(d0[:, 0], d1[:, 0]) and np.all((d1[:, 1] > 0) & (d1[:, 1] < 1))
    # placed FIRST it shifts the stream: other draws, but still no log q of its own in any term
    t2, d2 = R.sample_terms(oracle, om, [(0, -1, 5.0, 0.0)] + row, 5, 200, 7)
    x = d2[:, 1]
    lq = np.array([oracle.logpdf("Normal", v, R.dist_params(0, 0.3, -0.4)) for v in x])
    lp = np.array([oracle.logpdf("Normal", v, [0.0, 1.0]) + oracle.logpdf("Normal", 1.2, [v, 0.5]) for v in x])
    assert not np.array_equal(d2[:, 1], d0[:, 0]) and np.allclose(t2, lp - lq, rtol=1e-13, atol=1e-13)


def test_summation_orders_are_sums():
    rng = np.random.default_rng(0)
    for n in (1, 63, 64, 65, 4096, 70000):
        t = rng.standard_normal(n)
        assert R.elbo_of_terms(t) == pytest.approx(t.mean(), rel=1e-12, abs=1e-15)
    t = rng.standard_normal(100); t[17] = -np.inf
    assert R.elbo_of_terms(t) == -np.inf
    t = np.arange(128.0)                                   # the orders themselves, on integers (exact): wave sums, then their sum
    assert list(R.wave_sums(t)) == [t[:64].sum(), t[64:].sum()] and R.block_sum(R.wave_sums(t)) == t.sum()


def closed_form_elbo(m, s, y=1.2, sy=0.5):
    """E_q[log N(mu; 0, 1) + log N(y; mu, sy) - log q(mu)] for q = N(m, s)."""
    e_prior = -0.5 * math.log(2 * math.pi) - 0.5 * (m * m + s * s)
    e_lik = -0.5 * math.log(2 * math.pi) - math.log(sy) - 0.5 * ((y - m) ** 2 + s * s) / (sy * sy)
    entropy = 0.5 * math.log(2 * math.pi * math.e) + math.log(s)
    return e_prior + e_lik + entropy


def test_restated_elbo_matches_closed_form(oracle):
    om = oracle.OracleModel(W.readme_normal())
    N = 65536
    for m, ls in ((0.3, -0.4), (0.96, 0.5 * math.log(0.2))):
        terms, _ = R.sample_terms(oracle, om, [(0, 0, m, ls)], 17, N, 3)
        est, se = R.elbo_of_terms(terms), terms.std(ddof=1) / math.sqrt(N)
        exact = closed_form_elbo(m, math.exp(ls))
        print(f"restated ELBO {est:.6f}, closed form {exact:.6f}, standard error {se:.2e}")
        assert abs(est - exact) <= 4.0 * se
    # at the exact posterior every term is log Z: the estimate has no variance at all
    assert closed_form_elbo(0.96, math.sqrt(0.2)) == pytest.approx(oracle.logpdf("Normal", 1.2, [0.0, math.sqrt(1.25)]), rel=1e-12)


def test_restated_gradient_is_crn_exact(oracle):
    """Conjugate model, location coordinate: the central difference equals the sample mean of d log p / dx at the drawn x."""
    om = oracle.OracleModel(W.readme_normal())
    row, eps, N = [(0, 0, 0.3, -0.4)], 0.01, 512
    g = R.gradient_fd(oracle, om, row, 0, 0, eps, 9, N, 4)
    terms, draws = R.sample_terms(oracle, om, row, 9, N, 4)
    x = draws[:, 0]
    exact = np.mean(-x + (1.2 - x) / 0.25)
    assert abs(g - exact) <= 8.0 * np.abs(terms).max() * 2.0 ** -52 / eps


def test_optimizer_restatement_converges_and_is_reproducible(oracle):
    om = oracle.OracleModel(W.readme_normal())
    row = [(0, 0, 0.0, V.init_log_sigma(0.0))]
    a = R.optimize(oracle, om, row, 3, 32, n_iterations=60)
    b = R.optimize(oracle, om, row, 3, 32, n_iterations=60)
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:4] == b[2:4]
    assert abs(a[0][0][2] - 0.96) < 0.2 and len(a[1]) == a[3]


def test_posterior_bar_is_the_restatements(oracle):
    dev = posterior_deviation(oracle, "readme")
    print("restatement, conjugate model:", POSTERIOR_BAR["readme"], "->", dev)
    assert dev == POSTERIOR_BAR["readme"]["deviation"]


def test_abi_states_the_vi_symbols():
    from tests import abi_check as A
    header = open(os.path.join(ROOT, "include", "fugue_amd.h")).read()
    ffi = open(os.path.join(ROOT, "rust", "fugue-gpu", "src", "ffi.rs")).read()
    parsed = A.parse_header(header)
    for s in ("fg_vi_config_default", "fg_vi_elbo_batch", "fg_vi_optimize", "fg_vi_estimate_elbo"):
        assert s in parsed["fns"] and s in E.ABI_SYMBOLS and hasattr(ctypes.CDLL(E.LIB_PATH), s)
    assert [n for n, _ in parsed["structs"]["fg_vi_factor"]] == ["family", "site", "a", "b"]
    assert [n for n, _ in parsed["structs"]["fg_vi_config"]] == ["n_iterations", "convergence_window", "base_learning_rate", "fd_eps",
                                                                "convergence_tol", "step_decay_exponent"]
    assert ctypes.sizeof(E.fg_vi_factor) == 24 and ctypes.sizeof(E.fg_vi_config) == 40 and ctypes.sizeof(E.fg_vi_result) == 8
    assert A.compare_header_rust(header, ffi) == [] and A.compare_header_ctypes(header, E.lib()) == []
    assert "FG_RNG_VI = 8" in open(os.path.join(ROOT, "fugue_amd", "csrc", "fg_ir.h")).read() and R.FG_RNG_VI == 8


def test_drivers_have_no_cpu_fallback():
    """Without a device the VI drivers fail like every other driver (FG_E_NO_DEVICE); with one they run the kernel."""
    g = V.MeanFieldGuide(); g.add_latent(M.addr("mu"), V.Support.Real, 0.0)
    try:
        v = V.elbo_with_guide(1, W.readme_normal(), g, 64)
    except E.EngineError as ex:
        assert ex.code == E.FG_E_NO_DEVICE
    else:
        assert math.isfinite(v)
