"""GPU tests of the predictive draws on the device (fg_predict.hip: k_predict_eval behind fg_predict_eval, and the drivers above it).

The reference is built from what oracle/oracle.py exports: for (chain c, draw t) the stream oracle.stream(seed, chain_offset + c,
iter0 + t, 9), then oracle.sample_dist on that one stream for each observe statement in program order, and oracle.logpdf for the
pointwise term.  The parameters handed to the oracle are the bits the device used: the test models' observe parameters are a site
value, a constant, or a left-to-right `a + b * x` form (one rounding per operation in numpy, as the interpreter's LOAD / MUL / MAC).
Every compared figure is printed before it is asserted."""
import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import inference as I
from fugue_amd import model as M
from tests import diag_reference as R
from tests import qstream_restatement as Q
from tests.models import ZOO

pytestmark = pytest.mark.gpu

PURPOSE = 9                                                # FG_RNG_PREDICT
ABS_TOL = dict(r_hat=0.0, ess=0.0, mean=1e-12, std=0.0)   # as tests/test_gpu_diag_stream.py
FIGURES = ("r_hat", "ess", "mean", "std")


# ---- running the kernel with guard words around both tables -------------------------------------------------------------------------
def _predict(eng, cells, rows="all", n=None, iter0=0, sel=None, want_y=True, want_ll=True, guard=64):
    """fg_predict_eval over host cells [n][n_rows][C] (None: the engine's current values) -> (cells [n][n_sel][C] int64 or None,
    log-likelihood [n][n_sel][C] or None); each table sits between two runs of guard words that must come back untouched."""
    n = (1 if cells is None else cells.shape[0]) if n is None else n
    n_sel, C = (eng.cp.O if sel is None else len(sel)), eng.C
    d_in = None if cells is None else eng.upload(np.ascontiguousarray(cells))
    pattern = np.full(guard, -1234.5)
    host = np.concatenate([pattern, np.full(n * n_sel * C, 777.0), pattern])
    d_y, d_l = eng.upload(host), eng.upload(host)
    try:
        eng.predict_eval(d_in, n, rows=None if cells is None else (list(range(cells.shape[1])) if rows == "all" else rows), iter0=iter0, sel=sel,
                         out=d_y + guard * 8 if want_y else False, loglik=d_l + guard * 8 if want_ll else False)
        eng.synchronize()
        by, bl = eng.download(d_y, (host.size,)), eng.download(d_l, (host.size,))
    finally:
        for p in (d_in, d_y, d_l):
            if p:
                eng.device_free(p)
    for name, b, want in (("yrep", by, want_y), ("loglik", bl, want_ll)):
        assert np.array_equal(b[:guard], pattern) and np.array_equal(b[-guard:], pattern), f"guard words around {name} were written"
        if not want:
            assert (b[guard:-guard] == 777.0).all(), f"{name} was written although it was left out"
    y = by[guard:-guard].view(np.int64).reshape(n, n_sel, C).copy() if want_y else None
    ll = bl[guard:-guard].reshape(n, n_sel, C).copy() if want_ll else None
    return y, ll


def _bits_equal(label, got, want):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    a = got.view(np.int64) if got.dtype == np.float64 else got
    b = want.view(np.int64) if want.dtype == np.float64 else want
    diff = int((a != b).sum())
    print(f"{label}: {diff} of {a.size} cells differ")
    assert a.shape == b.shape and diff == 0, (label, np.argwhere(a != b)[:5].tolist())


def _close_f64(label, got, want, rel):
    """got == want within `rel` relative; NaN matches NaN, an infinity matches the same infinity.  Prints the worst finite deviation."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    same_special = (np.isnan(got) & np.isnan(want)) | (np.isinf(got) & np.isinf(want) & (np.sign(got) == np.sign(want)))
    with np.errstate(all="ignore"):
        err = np.abs(got - want)
        ok = same_special | (err <= rel * np.abs(want))
        relerr = np.where(np.isfinite(err) & (want != 0.0), err / np.abs(want), 0.0)
    print(f"{label}: worst relative deviation {relerr.max():.3e} over {int(np.isfinite(want).sum())} finite values (bound {rel:.0e}); "
          f"NaN {int(np.isnan(want).sum())}, inf {int(np.isinf(want).sum())}")
    assert got.shape == want.shape and ok.all(), (label, np.argwhere(~ok)[:5].tolist(), got[~ok][:5], want[~ok][:5])


def _f64(cells):
    return np.ascontiguousarray(cells).view(np.float64)


# ---- 1. every distribution against the oracle -------------------------------------------------------------------------------------
# (address, distribution, parameters as a function of the site values -- evaluated once over expressions to build the program and once over
#  numpy values to feed the oracle --, observed value)
EVERY = [
    ("n_pow2", "Normal", lambda v: [v["a"], 2.0], 0.3),                       # sigma = 2^1
    ("n_lin", "Normal", lambda v: [0.5 + v["a"] * 0.25, 0.7], -0.4),          # sigma != 2^k, a + b x location
    ("unif", "Uniform", lambda v: [v["u"], 3.0], 2.5),
    ("lognormal", "LogNormal", lambda v: [v["a"], v["s"]], 1.3),
    ("expo", "Exponential", lambda v: [v["s"]], 0.8),
    ("bern", "Bernoulli", lambda v: [v["b"]], 1),
    ("beta", "Beta", lambda v: [v["s"], 1.5], 0.35),
    ("gamma", "Gamma", lambda v: [v["s"], 2.0], 1.1),
    ("binom", "Binomial", lambda v: [12, v["b"]], 5),
    ("pois", "Poisson", lambda v: [v["s"]], 2),
    ("studt", "StudentT", lambda v: [4.0, v["a"], v["s"]], 0.6),
    ("cauchy", "Cauchy", lambda v: [v["a"], v["s"]], -0.2),
    ("laplace", "Laplace", lambda v: [v["a"], v["s"]], 0.4),
    ("weibull", "Weibull", lambda v: [1.5, v["s"]], 0.9),
    ("chisq", "ChiSquared", lambda v: [v["s"]], 2.2),
    ("invgamma", "InverseGamma", lambda v: [3.0, v["s"]], 0.7),
    ("du", "DiscreteUniform", lambda v: [-3, 8], 4),
    ("cat_const", "Categorical", lambda v: [0.1, 0.2, 0.3, 0.4], 2),          # a constant table (in the pool)
    ("cat_sites", "Categorical", lambda v: [v["b"], 1.0 - v["b"]], 1),        # a table computed from sites (in slots)
    ("n_bad_sigma", "Normal", lambda v: [0.0, v["a"]], 0.1),                  # invalid for the chains whose a <= 0
    ("expo_bad", "Exponential", lambda v: [v["u"]], 0.5),                     # invalid for the chains whose u <= 0
    ("pois_big", "Poisson", lambda v: [40.0], 37),                            # the transformed-rejection branch
    ("binom_big", "Binomial", lambda v: [40, 0.3], 11),                       # ... of the Binomial
    ("n_const_invalid", "Normal", lambda v: [0.0, v["neg2"] * 0.5], 0.2),     # a constant the compiler folds to sigma = -1: FG_F_INVALID
]
DISCRETE = {"Bernoulli", "Binomial", "Poisson", "Categorical", "DiscreteUniform"}


def _every_program():
    P = M.Program()
    v = dict(a=P.sample(M.addr("a"), M.Normal(0.0, 1.0)), s=P.sample(M.addr("s"), M.Gamma(2.0, 1.5)), b=P.sample(M.addr("b"), M.Beta(2.0, 3.0)),
             u=P.sample(M.addr("u"), M.Uniform(-2.0, 2.0)), neg2=M.as_expr(-2.0))     # (neg2 * 0.5 is no constant to the model's own checks)
    P.factor(v["a"] * 0.1)                                 # a factor statement between the sites and the observes: skipped
    for name, dist, par, obs in EVERY:
        P.observe(M.addr(name), getattr(M, dist)(par(v)) if dist == "Categorical" else getattr(M, dist)(*par(v)), obs)
    return P


def _oracle_tables(oracle, stmts, site_vals, seed, chain0, iter0):
    """stmts: (dist, params(v), observed); site_vals: name -> [n][C] values.  -> (y [n][O][C] python numbers as float64 / int64 cells, ll [n][O][C])."""
    any_site = next(iter(site_vals.values()))
    n, C = any_site.shape
    y = np.zeros((n, len(stmts), C), dtype=np.int64)
    ll = np.zeros((n, len(stmts), C))
    for t in range(n):
        for c in range(C):
            s = oracle.stream(seed, chain0 + c, iter0 + t, PURPOSE)
            v = {k: a[t, c] for k, a in site_vals.items()}
            for k, (dist, par, obs) in enumerate(stmts):
                p = [float(x) for x in par(v)]
                draw = oracle.sample_dist(dist, p, s)
                y[t, k, c] = int(draw) if dist in DISCRETE else np.array([draw]).view(np.int64)[0]
                ll[t, k, c] = oracle.logpdf(dist, obs, p)
    return y, ll


def test_every_distribution_matches_the_oracle(oracle):
    """17 distribution kinds (24 observe statements) at C = 130, chain_offset = 1000, n = 3, iter0 = 5.  Discrete cells exact; f64 cells
    within 1e-11 relative, the standing tolerance of test_prior_init_matches_oracle (ocml against glibc inside the samplers); the
    pointwise log-likelihood within 1e-12 relative of oracle.logpdf."""
    cp = E.compile_model(_every_program())
    assert cp.O == len(EVERY) and len({d for _, d, _, _ in EVERY}) == 17 and cp.observe_names == [e[0] for e in EVERY]
    C, n = 130, 3
    eng = E.Engine(cp, C, seed=77, chain_offset=1000)
    cells = np.zeros((n, cp.S, C), dtype=np.int64)
    for t in range(n):                                     # in-support site values: three prior draws
        eng.prior_init(iteration=40 + t)
        cells[t] = eng.get_values()
    assert all(vt == 0 for vt in cp.site_vtypes)
    vals = {nm: _f64(cells[:, j, :]) for j, nm in enumerate(cp.site_names)}
    vals["neg2"] = np.full((n, C), -2.0)
    assert (vals["a"] <= 0).any() and (vals["a"] > 0).any() and (vals["u"] <= 0).any() and (vals["u"] > 0).any()
    y, ll = _predict(eng, cells, iter0=5)
    eng.close()
    wy, wl = _oracle_tables(oracle, [(d, p, o) for _, d, p, o in EVERY], vals, 77, 1000, 5)
    for k, (name, dist, _, _) in enumerate(EVERY):
        if dist in DISCRETE:
            assert cp.observe_vtypes[k] != 0
            print(f"{name} ({dist}): {int((y[:, k] != wy[:, k]).sum())} of {y[:, k].size} integer cells differ; values {np.unique(wy[:, k])[:8].tolist()}")
            assert np.array_equal(y[:, k], wy[:, k]), name
        else:
            assert cp.observe_vtypes[k] == 0
            _close_f64(f"{name} ({dist}) draws", _f64(y[:, k]), _f64(wy[:, k]), 1e-11)
        _close_f64(f"{name} ({dist}) log-likelihood", ll[:, k], wl[:, k], 1e-12)
    bad = EVERY.index(next(e for e in EVERY if e[0] == "n_bad_sigma"))
    assert np.isnan(_f64(y[:, bad])[vals["a"] <= 0]).all() and np.isfinite(_f64(y[:, bad])[vals["a"] > 0]).all() and np.isneginf(ll[:, bad][vals["a"] <= 0]).all()
    inv = len(EVERY) - 1
    assert np.isnan(_f64(y[:, inv])).all() and np.isneginf(ll[:, inv]).all()      # what FG_MODE_PRIOR gives a sample statement with the flag; the score is -inf


# ---- 2. the pointwise terms are the scoring run's terms -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["readme", "coin", "ridge", "linreg", "mixture", "hier_scale", "alldists"])
def test_pointwise_terms_add_up_to_the_scoring_runs_log_likelihood_bit_for_bit(name):
    cp = E.compile_model(ZOO[name]())
    C = 70
    eng = E.Engine(cp, C, seed=21)
    eng.prior_init(iteration=2)
    want = eng.log_joint()[1]
    _, ll = _predict(eng, None, want_y=False)
    eng.close()
    tot = np.zeros(C)                                      # +0.0, then the O terms in program order, as A.lik receives them
    for k in range(cp.O):
        tot = tot + ll[0, k]
    same = (tot.view(np.int64) == want.view(np.int64)) | (np.isnan(tot) & np.isnan(want))
    print(f"{name}: O = {cp.O}, {int((~same).sum())} of {C} chains differ; -inf {int(np.isneginf(want).sum())}, NaN {int(np.isnan(want).sum())}, "
          f"range [{np.nanmin(want[np.isfinite(want)]) if np.isfinite(want).any() else float('nan'):.6g}, {np.nanmax(want[np.isfinite(want)]) if np.isfinite(want).any() else float('nan'):.6g}]")
    assert same.all(), (name, np.argwhere(~same)[:5].tolist(), tot[~same][:5], want[~same][:5])


# ---- 3. shapes ------------------------------------------------------------------------------------------------------------------
XS = [(-1.5, 0.3), (-0.5, 1.1), (0.25, -0.7), (1.0, 0.45), (2.0, -1.2)]
YS = [0.4, -0.1, 0.9, 1.7, 2.2]
NMAX, CMAX, SEED = 7, 130, 11


def _regression():
    """3 coefficients, 5 observations: y#i ~ Normal(beta#0 + beta#1 x1 + beta#2 x2, 0.5)."""
    P = M.Program()
    b = [P.sample(M.addr("beta", j), M.Normal(0.0, 2.0)) for j in range(3)]
    for i, (x1, x2) in enumerate(XS):
        P.observe(M.addr("y", i), M.Normal(b[0] + b[1] * x1 + b[2] * x2, 0.5), YS[i])
    return P


REG_STMTS = [("Normal", (lambda x1, x2: (lambda v: [(v["beta#0"] + v["beta#1"] * x1) + v["beta#2"] * x2, 0.5]))(x1, x2), YS[i]) for i, (x1, x2) in enumerate(XS)]


class _Reg:
    def __init__(self, oracle):
        self.cp = E.compile_model(_regression())
        assert self.cp.site_names == ["beta#0", "beta#1", "beta#2"] and self.cp.O == 5
        rng = np.random.default_rng(5)
        self.draws = rng.normal(0.0, 1.5, (NMAX, 3, CMAX))                       # [n][3][C] f64
        self.cells = self.draws.view(np.int64)
        vals = {nm: self.draws[:, j, :] for j, nm in enumerate(self.cp.site_names)}
        self.y, self.ll = _oracle_tables(oracle, REG_STMTS, vals, SEED, 0, 0)    # computed once, shared, never changed
        self.y.setflags(write=False), self.ll.setflags(write=False)
        self.engines = {}

    def engine(self, C, chain_offset=0):
        if (C, chain_offset) not in self.engines:
            self.engines[(C, chain_offset)] = E.Engine(self.cp, C, seed=SEED, chain_offset=chain_offset)
        return self.engines[(C, chain_offset)]

    def close(self):
        for e in self.engines.values():
            e.close()


@pytest.fixture(scope="module")
def reg(oracle):
    r = _Reg(oracle)
    yield r
    r.close()


@pytest.mark.parametrize("n", [1, 2, 7])
@pytest.mark.parametrize("C", [1, 63, 64, 65, 130])
def test_shapes_lds_and_global_forms_rows_and_guards(reg, monkeypatch, C, n):
    eng = reg.engine(C)
    cells = np.ascontiguousarray(reg.cells[:n, :, :C])
    y, ll = _predict(eng, cells)
    _close_f64(f"C={C} n={n} draws against the oracle", _f64(y), _f64(reg.y[:n, :, :C]), 1e-11)
    _close_f64(f"C={C} n={n} log-likelihood against the oracle", ll, reg.ll[:n, :, :C], 1e-12)
    monkeypatch.setenv("FG_PREDICT_GLOBAL_TILE", "1")
    gy, gl = _predict(eng, cells)
    monkeypatch.delenv("FG_PREDICT_GLOBAL_TILE")
    _bits_equal(f"C={C} n={n} global form, draws", gy, y)
    _bits_equal(f"C={C} n={n} global form, log-likelihood", gl, ll)
    perm = [2, 0, 1]                                       # row j of the draw holds site perm[j]
    py, pl = _predict(eng, np.ascontiguousarray(cells[:, perm, :]), rows=perm)
    _bits_equal(f"C={C} n={n} permuted rows, draws", py, y)
    _bits_equal(f"C={C} n={n} permuted rows, log-likelihood", pl, ll)
    # sites left out of the rows come from the engine's current values: hold sites 0 and 2 at draw 0's values, vary site 1
    held = np.ascontiguousarray(reg.cells[0, :, :C])
    eng.set_values(held)
    oy, ol = _predict(eng, np.ascontiguousarray(cells[:, 1:2, :]), rows=[1])
    mixed = cells.copy()
    mixed[:, 0, :], mixed[:, 2, :] = held[0], held[2]
    my, ml = _predict(eng, mixed)
    _bits_equal(f"C={C} n={n} sites 0 and 2 from the current values, draws", oy, my)
    _bits_equal(f"C={C} n={n} sites 0 and 2 from the current values, log-likelihood", ol, ml)
    if n == 1:                                             # draw 0 with its own values held: the oracle's table again, and the d_draws == NULL form
        _bits_equal(f"C={C} draw 0 through left-out sites", oy, y)
        cy, cl = _predict(eng, None)
        _bits_equal(f"C={C} current values, draws", cy, y)
        _bits_equal(f"C={C} current values, log-likelihood", cl, ll)


def test_left_out_sites_agree_with_the_oracle(reg, oracle):
    C, n = 130, 2
    eng = reg.engine(C)
    held = np.ascontiguousarray(reg.cells[3, :, :C])
    eng.set_values(held)
    y, ll = _predict(eng, np.ascontiguousarray(reg.cells[:n, 1:2, :C]), rows=[1], iter0=9)
    vals = {"beta#0": np.broadcast_to(reg.draws[3, 0, :C], (n, C)), "beta#1": reg.draws[:n, 1, :C], "beta#2": np.broadcast_to(reg.draws[3, 2, :C], (n, C))}
    wy, wl = _oracle_tables(oracle, REG_STMTS, vals, SEED, 0, 9)
    _close_f64("left-out sites, draws against the oracle", _f64(y), _f64(wy), 1e-11)
    _close_f64("left-out sites, log-likelihood against the oracle", ll, wl, 1e-12)


# ---- 4. invariances, all bit-exact ------------------------------------------------------------------------------------------------
def test_invariances(reg):
    C = 130
    eng = reg.engine(C)
    full_y, full_l = _predict(eng, reg.cells, iter0=3)
    a_y, a_l = _predict(eng, reg.cells[:3], iter0=3)
    b_y, b_l = _predict(eng, reg.cells[3:], iter0=6)
    _bits_equal("n = 7 against 3 + 4 with iter0 advanced, draws", np.concatenate([a_y, b_y]), full_y)
    _bits_equal("n = 7 against 3 + 4 with iter0 advanced, log-likelihood", np.concatenate([a_l, b_l]), full_l)
    lo_y, lo_l = _predict(reg.engine(64), np.ascontiguousarray(reg.cells[:, :, :64]), iter0=3)
    hi_y, hi_l = _predict(reg.engine(66, chain_offset=64), np.ascontiguousarray(reg.cells[:, :, 64:]), iter0=3)
    _bits_equal("130 chains against 64 + 66 with chain offsets, draws", np.concatenate([lo_y, hi_y], axis=2), full_y)
    _bits_equal("130 chains against 64 + 66 with chain offsets, log-likelihood", np.concatenate([lo_l, hi_l], axis=2), full_l)
    s_y, s_l = _predict(eng, reg.cells, iter0=3, sel=[3, 1])
    _bits_equal("a selection of 2 of 5, draws", s_y, full_y[:, [3, 1], :])
    _bits_equal("a selection of 2 of 5, log-likelihood", s_l, full_l[:, [3, 1], :])
    y_only, none = _predict(eng, reg.cells, iter0=3, want_ll=False)
    none2, l_only = _predict(eng, reg.cells, iter0=3, want_y=False)
    assert none is None and none2 is None
    _bits_equal("draws alone", y_only, full_y)
    _bits_equal("log-likelihood alone", l_only, full_l)
    again_y, again_l = _predict(eng, reg.cells, iter0=3)
    _bits_equal("a second call, draws", again_y, full_y)
    _bits_equal("a second call, log-likelihood", again_l, full_l)
    other_y, _ = _predict(eng, reg.cells, iter0=4)
    assert (other_y != full_y).mean() > 0.99               # another iteration word is another stream


# ---- 5. neutrality ----------------------------------------------------------------------------------------------------------------
def _hier():
    P = M.Program()
    mu = P.sample(M.addr("mu"), M.Normal(0.0, 2.0))
    k = P.sample(M.addr("k"), M.Categorical([0.3, 0.7]))
    for i, yv in enumerate([2.1, 1.8, 2.3]):
        P.observe(M.addr("y", i), M.Normal(mu + k * 0.5, 1.0), yv)
    return P


@pytest.mark.parametrize("sampler", ["hmc", "mh"])
def test_a_call_between_steps_changes_nothing_of_a_session(sampler, monkeypatch):
    monkeypatch.setenv("FG_JIT", "0")
    cp = E.compile_model(_hier())
    C, seen = 70, []
    for call in (False, True):
        eng = E.Engine(cp, C, seed=13)
        rec = list(range(cp.S))
        rows = cp.d if sampler == "hmc" else cp.S
        buf = eng.device_alloc(10 * rows * C * 8)
        step = (lambda n, p: eng.hmc_step(n, p)) if sampler == "hmc" else (lambda n, p: eng.mh_step(n, rec, p))
        if sampler == "hmc":
            eng.hmc_init(E.hmc_config(), 3)
        else:
            eng.mh_init(3, None)
        eng.hmc_step(3) if sampler == "hmc" else eng.mh_step(3)
        step(5, buf)
        if call:
            y, ll = _predict(eng, eng.download(buf, (5, rows, C), dtype=np.int64), rows=None if sampler == "hmc" else rec, iter0=0)
            assert np.isfinite(_f64(y)).all() and np.isfinite(ll).all()
            _predict(eng, None)
        step(5, buf + 5 * rows * C * 8)
        out = dict(draws=eng.download(buf, (10, rows, C), dtype=np.int64), values=eng.get_values(), state=np.frombuffer(eng.state_export(), dtype=np.uint8))
        if sampler == "hmc":
            out.update(lj=eng.hmc_log_joint(), eps=eng.hmc_step_sizes(), accept=np.float64(eng.hmc_stats().accept_rate))
        else:
            out.update(lw=eng.mh_log_weight(), scales=eng.mh_scales(), accept=np.float64(eng.mh_stats().accept_rate))
        eng.device_free(buf)
        eng.close()
        seen.append(out)
    for k in seen[0]:
        _bits_equal(f"{sampler} {k} with and without the call", np.asarray(seen[1][k]), np.asarray(seen[0][k]))


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(E.EngineError) as ei:
        fn()
    print(ei.value)
    return ei.value.code


def test_error_codes_and_value_errors(reg):
    eng = reg.engine(65)
    cells = np.ascontiguousarray(reg.cells[:2, :, :65])
    d_in = eng.upload(cells)
    d_out = eng.upload(np.full(2 * 5 * 65, 777.0))
    try:
        bad = lambda **kw: _code(lambda: eng.predict_eval(d_in, kw.pop("n", 2), out=kw.pop("out", d_out), loglik=kw.pop("loglik", False), **kw))
        assert bad(rows=[0, 1, 3]) == E.FG_E_BAD_ARG       # a row outside [0, S)
        assert bad(rows=[0, -1, 2]) == E.FG_E_BAD_ARG
        assert bad(rows=[0, 1, 1]) == E.FG_E_BAD_ARG       # a site given twice
        assert bad(rows=[0, 1, 2], sel=[5]) == E.FG_E_BAD_ARG      # a selection outside [0, O)
        assert bad(rows=[0, 1, 2], sel=[-1]) == E.FG_E_BAD_ARG
        assert bad(rows=[0, 1, 2], sel=[1, 1]) == E.FG_E_BAD_ARG   # ... given twice
        assert bad(rows=[0, 1, 2], out=False) == E.FG_E_BAD_ARG    # both outputs NULL
        assert bad(n=-1, rows=[0, 1, 2]) == E.FG_E_BAD_ARG
        assert _code(lambda: eng.predict_eval(None, 2, out=d_out, loglik=False)) == E.FG_E_BAD_ARG     # without draws n must be 1
        assert E.lib().fg_predict_eval(eng.h, d_in, 2, None, 2, 0, None, 0, d_out, None) == E.FG_E_BAD_ARG       # the HMC layout: n_rows must be d
        eng.predict_eval(d_in, 0, rows=[0, 1, 2], out=d_out, loglik=False)            # n == 0: FG_OK, nothing launched
        eng.synchronize()
        assert (eng.download(d_out, (2 * 5 * 65,)) == 777.0).all()
        assert bad(n=0, rows=[0, 1, 7]) == E.FG_E_BAD_ARG  # the arguments are still checked
    finally:
        eng.device_free(d_in), eng.device_free(d_out)
    bare = E.compile_model(lambda: M.sample(M.addr("x"), M.Normal(0.0, 1.0)))
    assert bare.O == 0 and bare.observe_names == []
    e0 = E.Engine(bare, 64, seed=1)
    e0.prior_init()
    assert _code(lambda: e0.predict_eval(None, 1)) == E.FG_E_STATE
    e0.close()
    with pytest.raises(ValueError, match="no observe"):
        I.hmc_chain(1, bare, 4, 4, n_chains=64, predictive=True)
    with pytest.raises(ValueError, match="nope"):
        I.hmc_chain(1, reg.cp, 4, 4, n_chains=64, predictive=["y#0", "nope"])
    with pytest.raises(ValueError, match="twice"):
        I.adaptive_mcmc_chain(1, reg.cp, 4, 4, n_chains=64, predictive=["y#0", "y#0"])
    coin = E.compile_model(ZOO["coin"]())
    with pytest.raises(ValueError, match="flip#0"):        # a discrete observe site in a summary: named
        I.hmc_chain_summary(1, coin, 8, 4, n_chains=64, predictive=True)
    with pytest.raises(ValueError, match="flip#3"):
        I.adaptive_mcmc_chain_summary(1, coin, 8, 4, n_chains=64, predictive=["flip#3"])
    with pytest.raises(ValueError, match="discrete=True"):
        I.adaptive_mcmc_chain_summary(1, _hier(), 8, 4, n_chains=64, predictive=True)


# ---- 7. the law, with a derived bound ---------------------------------------------------------------------------------------------
OBS = [2.1, 1.8, 2.3, 1.9, 2.0]


def _readme_style():
    return lambda: M.sample(M.addr("mu"), M.Normal(0.0, 2.0)).bind(
        lambda mu: M.sequence_vec([M.observe(M.addr("y", i), M.Normal(mu, 1.0), y) for i, y in enumerate(OBS)]).map(lambda _: mu))


def test_posterior_predictive_law(monkeypatch):
    """mu ~ Normal(0, 2), y_i ~ Normal(mu, 1); 256 chains x 200 draws.  Given the draws, y_rep - mu is iid N(0, 1) over N = 51 200 cells
    per site: the mean has standard error 1 / sqrt(N), the variance sqrt(2 / N).  Five standard errors: a false failure below 1e-6."""
    monkeypatch.setenv("FG_JIT", "0")
    b = I.hmc_chain(42, _readme_style(), 200, 50, n_chains=256, predictive=True)
    mu = b.get_f64("mu")
    N = mu.size
    assert N == 51200 and b.predictive.shape == (200, 5, 256) and b.predictive_names == [f"y#{i}" for i in range(5)] and b.log_likelihood is None
    for i in range(5):
        z = b.get_predictive(f"y#{i}") - mu
        m, v = float(z.mean()), float(z.var())
        print(f"y#{i}: mean(y_rep - mu) = {m:+.5f} (bound {5 / np.sqrt(N):.5f}), var = {v:.5f} (|var - 1| bound {5 * np.sqrt(2 / N):.5f})")
        assert abs(m) < 5.0 / np.sqrt(N)
        assert abs(v - 1.0) < 5.0 * np.sqrt(2.0 / N)


def test_prior_predictive_law_on_the_coin():
    """p ~ Beta(2, 2), flip_i ~ Bernoulli(p): given p, a replicate has mean p and variance p (1 - p) <= 1/4, so
    |mean(y_rep) - mean(p)| has standard error at most sqrt(1/4 / N) over the N replicates."""
    def coin():
        return M.sample(M.addr("p"), M.Beta(2.0, 2.0)).bind(
            lambda p: M.sequence_vec([M.observe(M.addr("flip", i), M.Bernoulli(p), bool(f)) for i, f in enumerate([1, 0, 1, 1, 0])]).map(lambda _: p))
    pp = I.prior_predictive(9, coin, 8192, iteration=4)
    p = pp.get_f64("p")
    assert pp.predictive.shape == (5, 8192) and pp.predictive_vtypes == [M.BOOL] * 5 and set(np.unique(pp.predictive)) == {0, 1}
    N = pp.predictive.size
    gap = abs(float(pp.predictive.mean()) - float(p.mean()))
    print(f"prior predictive coin: mean(y_rep) = {pp.predictive.mean():.5f}, mean(p) = {p.mean():.5f}, gap {gap:.5f} (bound {5 * np.sqrt(0.25 / N):.5f})")
    assert gap < 5.0 * np.sqrt(0.25 / N)
    # the sites are prior_init's and the replicates are the kernel's at those values
    eng = E.Engine(E.compile_model(coin), 8192, seed=9)
    eng.prior_init(4)
    assert np.array_equal(eng.get_values(), pp.cells)
    y, _ = _predict(eng, None, iter0=4, want_ll=False)
    eng.close()
    assert np.array_equal(y[0], pp.predictive)
    assert np.array_equal(pp.get_predictive("flip#2"), pp.predictive[2])


# ---- 8. the drivers ---------------------------------------------------------------------------------------------------------------
def _reeval(cp, seed, cells, sel=None, iter0=0):
    eng = E.Engine(cp, cells.shape[2], seed=seed)
    try:
        return _predict(eng, np.ascontiguousarray(cells), iter0=iter0, sel=sel)
    finally:
        eng.close()


def _same_batch(label, a, b, skip=()):
    for f in a.__dataclass_fields__:
        if f in skip:
            continue
        x, y = getattr(a, f), getattr(b, f)
        if isinstance(x, np.ndarray):
            _bits_equal(f"{label}.{f}", x, y)
        else:
            assert (x == y) or (isinstance(x, float) and np.isnan(x) and np.isnan(y)), (label, f, x, y)


PRED_FIELDS = ("predictive", "predictive_names", "predictive_vtypes", "log_likelihood")


def test_stored_runs_carry_the_tables(monkeypatch):
    monkeypatch.setenv("FG_JIT", "0")
    cp = E.compile_model(_readme_style())
    names = [f"y#{i}" for i in range(5)]
    plain = I.hmc_chain(3, cp, 10, 10, n_chains=70)
    assert plain.predictive is None and plain.log_likelihood is None and plain.predictive_names == []
    hm = I.hmc_chain(3, cp, 10, 10, n_chains=70, predictive=True, pointwise=True)
    _same_batch("hmc_chain defaults", plain, hm, skip=PRED_FIELDS)
    y, ll = _reeval(cp, 3, hm.cells)
    assert hm.predictive_names == names and hm.predictive_vtypes == [0] * 5
    _bits_equal("hmc_chain.predictive", hm.predictive, y)
    _bits_equal("hmc_chain.log_likelihood", hm.log_likelihood, ll)
    assert np.array_equal(hm.get_predictive("y#2"), _f64(hm.predictive[:, 2, :]))
    with pytest.raises(M.FugueError):
        hm.get_predictive("y#9")
    only_ll = I.hmc_chain(3, cp, 10, 10, n_chains=70, pointwise=True)
    assert only_ll.predictive is None and only_ll.predictive_names == names
    _bits_equal("hmc_chain(pointwise=True).log_likelihood", only_ll.log_likelihood, ll)
    mplain = I.adaptive_mcmc_chain(3, cp, 10, 10, n_chains=70)
    mh = I.adaptive_mcmc_chain(3, cp, 10, 10, n_chains=70, predictive=["y#4", "y#1"])
    _same_batch("adaptive_mcmc_chain defaults", mplain, mh, skip=PRED_FIELDS)
    my, _ = _reeval(cp, 3, mh.cells, sel=[4, 1])
    assert mh.predictive_names == ["y#4", "y#1"] and mh.log_likelihood is None and mplain.predictive is None
    _bits_equal("adaptive_mcmc_chain.predictive", mh.predictive, my)
    ov = I.adaptive_mcmc_chain_with_overrides(3, cp, 10, 10, [("mu", I.SiteProposal.Gaussian())], n_chains=70, predictive=True)
    oy, _ = _reeval(cp, 3, ov.cells)
    _bits_equal("adaptive_mcmc_chain_with_overrides.predictive", ov.predictive, oy)
    splain = I.adaptive_smc(3, 70, cp)
    smc = I.adaptive_smc(3, 70, cp, predictive=True, pointwise=True)
    _same_batch("adaptive_smc defaults", splain, smc, skip=PRED_FIELDS)
    sy, sl = _reeval(cp, 3, smc.cells[None])
    assert smc.predictive.shape == (5, 70) and splain.predictive is None
    _bits_equal("adaptive_smc.predictive: one replicate per particle", smc.predictive, sy[0])
    _bits_equal("adaptive_smc.log_likelihood", smc.log_likelihood, sl[0])
    # discrete sites under hmc_chain keep their prior draw and reach the parameters from the engine's values
    hx = I.hmc_chain(4, _hier(), 5, 5, n_chains=65, predictive=True)
    hy, _ = _reeval(E.compile_model(_hier()), 4, hx.cells)
    _bits_equal("hmc_chain.predictive with a discrete site", hx.predictive, hy)


def test_hmc_chain_summary_with_predictive_and_quantiles(monkeypatch):
    """chunk = 16 over 64 draws: the figures of the replicated data against the stored-draw summary of ChainBatch.predictive through
    diag_rhat_ess / diag_quantiles -- the quantiles exact, the others within the tolerances of tests/test_gpu_diag_stream.py; the site
    figures bitwise those of predictive=False."""
    monkeypatch.setenv("FG_JIT", "0")
    a = dict(seed=7, model_fn=_readme_style(), n_samples=64, n_warmup=20, n_chains=128)
    chains = I.hmc_chain(predictive=True, **a)
    plain = I.hmc_chain_summary(chunk=16, quantiles=True, **a)
    summ = I.hmc_chain_summary(chunk=16, quantiles=True, predictive=True, **a)
    ps = summ.predictive
    assert plain.predictive is None and ps.sites == chains.predictive_names and (ps.n_samples, ps.n_chains) == (64, 128)
    eng = E.Engine(E.compile_model(_readme_style()), 128, seed=1)
    ptr = eng.upload(_f64(chains.predictive))
    stored = eng.diag_rhat_ess(ptr, 64, 5)
    want_q = eng.diag_quantiles(ptr, 64, 5, I.QUANTILE_PROBS)
    eng.device_free(ptr)
    eng.close()
    for i, nm in enumerate(ps.sites):
        for k in FIGURES:
            got, want = float(getattr(ps, k)[i]), float(stored[k][i])
            print(f"{nm} {k}: streamed {got!r} stored {want!r}")
    for i, nm in enumerate(ps.sites):
        for k in FIGURES:
            got, want = float(getattr(ps, k)[i]), float(stored[k][i])
            assert np.isfinite(got) and abs(got - want) <= max(R.FIGURE_TOL[k] * abs(want), ABS_TOL[k]), (nm, k, got, want)
        print(f"{nm} quantiles: summary {ps.quantiles[i].tolist()} stored {want_q[i].tolist()}")
    assert np.array_equal(Q.bits(ps.quantiles), Q.bits(want_q))
    assert np.array_equal(Q.bits(ps.quantiles), Q.bits(Q.reference_all(_f64(chains.predictive), I.QUANTILE_PROBS)))
    print(f"passes: sites {summ.passes}, predictive {ps.passes}")
    for k in ("mean", "std", "r_hat", "ess", "quantiles"):
        assert np.array_equal(Q.bits(getattr(summ, k)), Q.bits(getattr(plain, k))), k
    assert (summ.accept_rate, summ.mean_step_size, summ.n_divergent, summ.passes) == (plain.accept_rate, plain.mean_step_size, plain.n_divergent, plain.passes)
    # MH, a selection
    b = dict(seed=7, model_fn=_readme_style(), n_samples=40, n_warmup=20, n_chains=128)
    mh = I.adaptive_mcmc_chain(predictive=["y#3"], **b)
    ms = I.adaptive_mcmc_chain_summary(chunk=16, predictive=["y#3"], **b)
    eng = E.Engine(E.compile_model(_readme_style()), 128, seed=1)
    ptr = eng.upload(_f64(mh.predictive))
    stored = eng.diag_rhat_ess(ptr, 40, 1)
    eng.device_free(ptr)
    eng.close()
    assert ms.predictive.sites == ["y#3"]
    for k in ("mean", "std", "r_hat"):
        got, want = float(getattr(ms.predictive, k)[0]), float(stored[k][0])
        print(f"mh y#3 {k}: streamed {got!r} stored {want!r}")
        assert abs(got - want) <= max(R.FIGURE_TOL[k] * abs(want), ABS_TOL[k]), (k, got, want)


# ---- 9. the reference's workflow, with the device path ------------------------------------------------------------------------------
def test_workflow_complete_bayesian_analysis_with_the_device_predictive():
    """inference_integration.rs:717-740: after the MCMC run, one replicate per posterior draw from Normal(mu, 1) -- here sampled by the
    kernel at every draw instead of on the host from downloaded draws -- is finite and centred on the observations."""
    import fugue_amd as F
    model = lambda: F.sample(F.addr("mu"), F.Normal(0.0, 2.0)).bind(
        lambda mu: F.sequence_vec([F.observe(F.addr("y", i), F.Normal(mu, 1.0), y) for i, y in enumerate(OBS)]).map(lambda _: mu))
    chains = F.adaptive_mcmc_chain(42, model, 200, 50, n_chains=3, predictive=[F.addr("y", 0)])
    s = F.summarize_f64_parameter(chains, F.addr("mu"))
    obs_mean = float(np.mean(OBS))
    assert abs(s.mean - obs_mean) < 0.5
    pred = chains.get_predictive(F.addr("y", 0)).T.ravel()[:100]                 # the first 100 posterior draws of chain 0, as the reference takes them
    print(f"posterior predictive: mean {pred.mean():.4f} (observations {obs_mean:.4f}), std {pred.std():.4f}")
    assert pred.shape == (100,) and np.isfinite(pred).all() and abs(pred.mean() - obs_mean) < 1.0
    prior = F.prior_predictive(42, model, 64)
    assert prior.predictive.shape == (5, 64) and np.isfinite(prior.get_predictive(F.addr("y", 4))).all()
