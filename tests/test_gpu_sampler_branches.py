"""GPU tests of fg_sample_dist (fugue_amd/csrc/fg_math.h) on every branch of its rejection samplers and on every device path that calls it:
the prior draw (k_prior_init and the run-time compiled k_prior_jit), the predictive draws (k_predict_eval) and MH's prior-resample
proposals.  The cases, the law helpers and their thresholds are those of tests/sampler_cases.py; tests/test_sampler_law_cpu.py runs the same
checks over the oracle's draws from the same streams.

Two judges.  The oracle (same algorithms, glibc in place of ocml) pins every draw and, through the site that follows a sampler, the number
of Philox blocks each lane consumed.  The analytic law (scipy) judges what the oracle cannot: a wrong constant would sit in both.

Integer cells must equal the oracle's except where a one-ulp difference between ocml and glibc flips an accept test: at most 0.1 % of a
case's chains (the cap tests/test_gpu_vi.py grants this sampler), each printed with both values.  f64 cells: 1e-11 relative, the standing
bound of test_prior_init_matches_oracle.  The law checks exclude nothing.  Every figure is printed before it is asserted.

Figures seen on an MI355X (16421 draws per case; no integer cell of any case, of the mixed model or of the predictive tables differed from
the oracle's, so nothing was excluded):
  pois_30            chi-square   44.8 on   37 df, p = 0.1759, mean z 0.62      gamma_0.3_2      KS D 0.00515, mean z 1.10
  pois_30_pred       chi-square   40.4 on   37 df, p = 0.3212, mean z 0.09      gamma_1_1        KS D 0.00393, mean z 0.67
  pois_100.5         chi-square   49.6 on   65 df, p = 0.9209, mean z 0.07      gamma_0.05_1     KS D 0.00589, mean z 1.29
  pois_5000          chi-square  372.4 on  380 df, p = 0.5994, mean z 0.16      beta_0.5_0.5     KS D 0.00950, mean z 1.06
  binom_40_0.3       chi-square   22.9 on   19 df, p = 0.2406, mean z 0.17      beta_0.2_3       KS D 0.00541, mean z 1.66
  binom_40_0.7       chi-square   22.9 on   19 df, p = 0.2406, mean z 0.17      chisq_1          KS D 0.00476, mean z 1.34
  binom_1000_0.5     chi-square   90.8 on  100 df, p = 0.7336, mean z 0.34      studt_1.5        KS D 0.00438 (no finite standard error)
  binom_30_0.9       chi-square   11.4 on   10 df, p = 0.3295, mean z 1.25      invgamma_0.7_2   KS D 0.00558 (no finite standard error)
  binom_1e5_5e-5     chi-square   15.1 on   14 df, p = 0.3744, mean z 1.40      (KS critical value 0.01521)
  binom_25_0.4       chi-square   19.0 on   16 df, p = 0.2683, mean z 0.09
  binom_20_0.5       chi-square   22.2 on   14 df, p = 0.0745, mean z 0.69
  binom_20_0.5_succ  chi-square   15.9 on   14 df, p = 0.3212, mean z 1.25
  binom_1e6_0.37     chi-square 1807.3 on 1758 df, p = 0.2017, mean z 0.17
  at 2^20 draws, p-values: pois_30 0.1085, pois_100.5 0.0519, pois_5000 0.4805, binom_40_0.3 and binom_40_0.7 0.4457, binom_1000_0.5 0.1159,
  binom_25_0.4 0.1795, binom_20_0.5 0.6094, binom_1e6_0.37 0.0496 (the oracle's figures to the digit: the draws are the same)
  mixed model, PIT KS D: a_u 0.00485, b_pois 0.00585, c_bin 0.00800, d_gam 0.00845, e_z 0.00662
With fg_math.h and the oracle mutated alike (never committed; parity then holds and only the law judges): dropping the flip fails
binom_40_0.7, binom_30_0.9 and the mixed model's c_bin (PIT D 0.381); the boost with exponent k fails all seven boosted cases (gamma_0.3_2:
KS D 0.519) and the mixed model's d_gam; PTRS vr * 1.05 fails pois_5000 at 2^20 draws (chi-square 719.2 on 558 df); BTRS alpha * 1.05 fails
binom_1e6_0.37 at 2^20 draws (3721.1 on 3315 df).  The last two pass every check at 16421 draws."""
import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import model as M
from tests import oracle_margins
from tests import parity_cases as PC
from tests import sampler_cases as SC
from tests.test_gpu_mh import _compare as _mh_compare
from tests.test_gpu_predict import _close_f64, _f64, _oracle_tables, _predict

pytestmark = pytest.mark.gpu

C_LAW = SC.N + 37                    # 256 full waves and a ragged one of 37 lanes
N_PARITY = 4096                      # chains compared with the oracle draw for draw
REL = 1e-11


def _ids(cases):
    return [c.name for c in cases]


def _prior_cells(cp, C, seed, iteration=0):
    eng = E.Engine(cp, C, seed=seed)
    acc = eng.prior_init(iteration)
    cells = eng.get_values().copy()
    eng.close()
    return cells, acc


def _int_parity(label, got, want, ok=None):
    """Integer cells against the oracle's over the chains in `ok` (None: all).  Returns the mask of chains that differ; at most 0.1 % may."""
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    ok = np.ones(len(want), dtype=bool) if ok is None else ok
    bad = ok & (got != want)
    for c in np.nonzero(bad)[0]:
        print(f"{label}: chain {c} device {got[c]} oracle {want[c]} (an accept test flipped)")
    cap = len(want) // 1000
    print(f"{label}: {int(bad.sum())} of {int(ok.sum())} integer cells differ from the oracle (cap {cap})")
    assert bad.sum() <= cap, (label, np.nonzero(bad)[0][:10].tolist())
    return bad


# ---- a. the prior draw of every table case: oracle and law -------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.CASES, ids=_ids(SC.CASES))
def test_prior_draw_of_a_branch_case_matches_the_oracle_and_its_law(oracle, case):
    cp = E.compile_model(SC.one_site_model(case))
    cells, _ = _prior_cells(cp, C_LAW, case.seed)
    want, blocks = SC.oracle_draws(oracle, case, N_PARITY)
    print(f"{case.name}: code path {SC.branch_reached(case)}; oracle blocks per draw min {blocks.min()}, mean {blocks.mean():.2f}, max {blocks.max()}")
    if SC.is_discrete(case):
        x = cells[0]
        _int_parity(case.name, x[:N_PARITY], want)
    else:
        x = _f64(cells[0])
        _close_f64(f"{case.name} draws against the oracle", x[:N_PARITY], want, REL)
    SC.check_case(case, x)                                  # every device draw, the ragged wave included; nothing excluded


@pytest.mark.parametrize("case", SC.LARGE, ids=_ids(SC.LARGE))
def test_large_sample_law_of_the_transformed_rejection_branches(case):
    """2^20 draws.  At N = 16384 the law cannot see a squeeze constant of PTRS / BTRS that is 5 % off: the exact acceptance test behind the
    squeeze repairs most of it (tests/test_sampler_law_cpu.py has the figures); at 2^20 draws Poisson(5000), Binomial(1000, 0.5) and
    Binomial(10^6, 0.37) do."""
    cp = E.compile_model(SC.one_site_model(case))
    cells, _ = _prior_cells(cp, SC.N_LARGE, case.seed)
    assert np.array_equal(cells[0, :256], _prior_cells(cp, 256, case.seed)[0][0])      # the same streams as the small run
    SC.check_case(case, cells[0])


# ---- b. mixed waves --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_oracle(oracle):
    """The oracle's run of the mixed model on chains 0 .. N_PARITY-1: cells [5][n], accumulators [3][n].  Computed once, never changed."""
    om = oracle.OracleModel(SC.mixed_program())
    assert om.site_names == SC.MIXED_SITES
    runs = [om.run_prior(SC.SEED_MIXED, c, 0) for c in range(N_PARITY)]
    cells, acc = np.stack([r[0] for r in runs], axis=1), np.stack([r[1] for r in runs], axis=1)
    cells.setflags(write=False), acc.setflags(write=False)
    return cells, acc


def _mixed_parity(label, cells, acc, mixed_oracle):
    """All five sites and the three accumulators against the oracle; a site is compared in the chains whose earlier sites agree."""
    wc, wa = mixed_oracle
    n = wc.shape[1]
    _close_f64(f"{label} a_u", _f64(cells[0, :n]), _f64(wc[0]), REL)
    bad = _int_parity(f"{label} b_pois", cells[1, :n], wc[1])
    bad |= _int_parity(f"{label} c_bin", cells[2, :n], wc[2], ~bad)
    ok = ~bad
    print(f"{label}: {int(ok.sum())} of {n} chains agree on the two integer sites")
    _close_f64(f"{label} d_gam where the earlier sites agree", _f64(cells[3, :n])[ok], _f64(wc[3])[ok], REL)
    # e_z behind three samplers with lane-dependent block counts: equal only if every lane's samplers consumed what the oracle's did
    _close_f64(f"{label} e_z where the earlier sites agree", _f64(cells[4, :n])[ok], _f64(wc[4])[ok], REL)
    for k, name in enumerate(("log_prior", "log_likelihood", "log_factors")):
        got, want = acc[k, :n][ok], wa[k][ok]
        err = np.abs(got - want)
        print(f"{label} {name}: worst |difference| {np.nanmax(err) if err.size else 0.0:.3e} (bound 1e-10 + 1e-10 |x|)")
        assert (err <= 1e-10 + 1e-10 * np.abs(want)).all(), (label, name)


def test_mixed_waves_match_the_oracle_and_the_law_given_the_parent(mixed_oracle):
    cp = E.compile_model(SC.mixed_program())
    assert cp.site_names == SC.MIXED_SITES
    cells, acc = _prior_cells(cp, C_LAW, SC.SEED_MIXED)
    _mixed_parity("mixed model", cells, acc, mixed_oracle)
    SC.check_mixed(cells)


# ---- c. the compiled prior draw ---------------------------------------------------------------------------------------------------
def _with_follower(case):
    """The case's site followed by a Normal(0, 1): an f64 coordinate (the compiled unit needs one) that also shows where the sampler left
    the stream."""
    P = M.Program()
    P.sample(M.addr("x"), SC.dist_of(case))
    P.sample(M.addr("y_after"), M.Normal(0.0, 1.0))
    return P


JIT_PROGRAMS = {"mixed": SC.mixed_program, "gamma_0.3_2": lambda: _with_follower(SC.BY_NAME["gamma_0.3_2"]),
                "pois_100.5": lambda: _with_follower(SC.BY_NAME["pois_100.5"]), "binom_40_0.7": lambda: _with_follower(SC.BY_NAME["binom_40_0.7"])}


@pytest.mark.parametrize("name", list(JIT_PROGRAMS))
def test_compiled_prior_draw_is_identical_to_the_interpreter(name, monkeypatch, capfd):
    """k_prior_jit against k_prior_init, as test_jit_prior_draw_is_identical_to_the_interpreter does it: the same cells and accumulators bit
    for bit, here on the rejection samplers with both branches in every wave.  The unit is built by a session's step-size search first;
    FG_JIT_VERBOSE names every reason for which the draw would have fallen back to the interpreter: none may be printed."""
    cp = E.compile_model(JIT_PROGRAMS[name]())
    assert cp.d >= 1
    out = []
    for jit in ("0", "1"):
        monkeypatch.setenv("FG_JIT", jit)
        monkeypatch.setenv("FG_JIT_VERBOSE", "1")
        eng = E.Engine(cp, 700, seed=SC.SEED_MIXED, chain_offset=3)
        if jit == "1":
            eng.hmc_init(E.hmc_config(n_leapfrog=2), 0)
        capfd.readouterr()
        acc = eng.prior_init(5)
        err = capfd.readouterr().err
        out.append((acc, eng.get_values().copy()))
        if jit == "1":                                     # the unit exists: a transition of this engine runs on it
            eng.hmc_step(1)
            kernel = eng.hmc_last_kernel()
            print(f"{name}: FG_JIT_VERBOSE during the compiled draw: {err!r}; a transition runs on {kernel}")
            assert "jit" in kernel, kernel
            assert "no compiled prior draw" not in err and "has no k_prior_jit" not in err and "unavailable" not in err, err
        eng.close()
    diff = int((out[0][1] != out[1][1]).sum())
    print(f"{name}: {diff} of {out[0][1].size} cells differ between k_prior_init and k_prior_jit")
    assert np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][0], out[1][0], equal_nan=True)


# ---- d. the predictive path -------------------------------------------------------------------------------------------------------
def _observed(case_or_family):
    fam = case_or_family if isinstance(case_or_family, str) else case_or_family.family
    return 1 if fam in SC.INT_FAMILIES else 0.5


PRED = [(c.name, c.family, (lambda ps: (lambda v: list(ps)))(c.params), _observed(c)) for c in SC.CASES] + [
    ("fed_pois", "Poisson", lambda v: [20.0 + v["u"] * 20.0], 1),
    ("fed_bin", "Binomial", lambda v: [30, 0.1 + v["u"] * 0.8], 1),
    ("fed_gam", "Gamma", lambda v: [0.25 + v["u"] * 1.5, 2.0], 0.5),
    ("fed_z", "Normal", lambda v: [0.0, 1.0], 0.5),
]


def test_predictive_draws_on_every_branch_match_the_oracle(oracle):
    """Observe statements carrying the table cases (constant parameters) and the mixed model's site-fed forms, through predict_eval at
    C = 130, n = 3: every replicate against oracle.sample_dist on the purpose-9 stream, statement after statement on one stream per
    (draw, chain) -- a sampler that consumed another number of blocks than the oracle's moves every later statement."""
    P = M.Program()
    v = dict(u=P.sample(M.addr("u"), M.Uniform(0.0, 1.0)))
    for name, fam, par, obs in PRED:
        P.observe(M.addr(name), getattr(M, fam)(*par(v)), obs)
    cp = E.compile_model(P)
    assert cp.observe_names == [p[0] for p in PRED] and cp.site_names == ["u"]
    C, n = 130, 3
    eng = E.Engine(cp, C, seed=77, chain_offset=1000)
    cells = np.zeros((n, cp.S, C), dtype=np.int64)
    for t in range(n):
        eng.prior_init(iteration=40 + t)
        cells[t] = eng.get_values()
    y, _ = _predict(eng, cells, iter0=5, want_ll=False)
    eng.close()
    vals = {"u": _f64(cells[:, 0, :])}
    shares = SC.mixed_branch_shares(vals["u"])
    print(f"site-fed forms: lanes on PTRS {shares['ptrs']:.3f}, BTRS {shares['btrs']:.3f}, flip {shares['flip']:.3f}, boost {shares['boost']:.3f}")
    assert all(0.2 < shares[k] < 0.8 for k in ("ptrs", "btrs", "flip", "boost"))
    wy, _ = _oracle_tables(oracle, [(f, p, o) for _, f, p, o in PRED], vals, 77, 1000, 5)
    for k, (name, fam, _, _) in enumerate(PRED):
        if fam in SC.INT_FAMILIES:
            diff = int((y[:, k] != wy[:, k]).sum())
            print(f"{name} ({fam}): {diff} of {y[:, k].size} integer cells differ (cap {y[:, k].size // 1000})")
            assert diff <= y[:, k].size // 1000, name
        else:
            _close_f64(f"{name} ({fam}) replicates", _f64(y[:, k]), _f64(wy[:, k]), REL)


# ---- e. MH prior-resample ---------------------------------------------------------------------------------------------------------
MH_KERNELS = [   # (id, FG_JIT, FG_HMC_INTERP_MW, what the kernel's name starts with)
    ("interpreter", "0", "0", ("k_mh_steps",)),
    ("compiled", "1", "1", ("k_mh_jit_steps", "k_mh_mw_jit_steps")),
]


@pytest.mark.parametrize("variant", MH_KERNELS, ids=[v[0] for v in MH_KERNELS])
def test_mh_prior_resample_of_a_boosted_gamma_matches_the_oracle(oracle, variant, monkeypatch):
    """g ~ Gamma(0.3, 2) under PROP_PRIOR_RESAMPLE: every proposal is a boosted Marsaglia-Tsang draw from the step's stream, and the accept
    uniform comes from the block after the ones it consumed.  50 + 150 steps at C = 256 against the oracle's MH with the tolerances of
    tests/test_gpu_mh.py (f64 1e-9; a chain may part ways only behind an accept decision of the oracle's within 1e-6 of its uniform, and
    tests/test_knife_margins_cpu.py shows that this run has none), on the interpreter's one-wave kernel and on the kernel whose statements
    are compiled at run time.  The observations' mean is an expression of g (tests/parity_cases.boosted_gamma_model), so the program has no
    score stream: the compiled MH kernels take prior-resample proposals for such programs only."""
    _, jit, interp_mw, starts = variant
    monkeypatch.setenv("FG_JIT", jit)
    monkeypatch.setenv("FG_HMC_INTERP_MW", interp_mw)
    case = PC.MH_CASES["boosted-gamma"]
    P = case.make()
    cp, om = E.compile_model(P), oracle.OracleModel(P)
    assert cp.stream_records[1] == 0
    ov = case.overrides_for(om.site_names)
    assert ov == [(E.PROP_PRIOR_RESAMPLE, 0.0, 0.0)]
    C, nw, ns, seed = case.C, case.nw, case.ns, case.seed
    eng = E.Engine(cp, C, seed=seed)
    d_draws = eng.device_alloc(ns * cp.S * C * 8)
    st = eng.mh_run(ns, nw, ov, [0], d_draws)
    draws = eng.download(d_draws, (ns, cp.S, C), dtype=np.int64)
    eng.device_free(d_draws)
    kernel = eng.mh_last_kernel()
    eng.close()
    odraws, _, _, ost = om.mh_run(seed, C, nw, ns, ov, [0], n_threads=8)
    moved = (draws[1:] != draws[:-1]).mean()
    print(f"{variant[0]}: kernel {kernel}; accept rate device {st.accept_rate:.4f} oracle {ost.accept_rate:.4f}; {moved:.3f} of the recorded steps moved")
    assert kernel.startswith(starts), kernel
    dist, _ = oracle_margins.mh_margins(om, seed, C, nw, ns, ov, case.chain0)
    _mh_compare(cp, draws, odraws, dist, case.chain0, where=f"MH prior resample of a boosted Gamma ({variant[0]})")
    x = _f64(draws[:, 0, :])
    assert (x > 0).all() and moved > 0.05
    assert abs(st.accept_rate - ost.accept_rate) < 2e-3           # as test_mh_chain_matches_oracle


# ---- f. edge parameters ----------------------------------------------------------------------------------------------------------
def _edge_dist(family, params):
    return M.Dist(family, [p if isinstance(p, M.Expr) else M.as_expr(float(p)) for p in params])      # no constructor validation


def _edge_program(fed):
    """Every edge of SC.EDGES as a sample site followed by a Normal(0, 1) site.  fed: the last parameter is parent * 0 + value, an
    expression of a drawn site, so nothing of it is folded or hoisted by the compiler."""
    P = M.Program()
    for i, (name, family, params, _, _) in enumerate(SC.EDGES):
        params = list(params)
        if fed:
            parent = P.sample(M.addr(f"e{i}_a_parent"), M.Normal(0.0, 1.0))
            params[-1] = parent * 0.0 + float(params[-1])
        P.sample(M.addr(f"e{i}_b_{name}"), _edge_dist(family, params))
        P.sample(M.addr(f"e{i}_c_after"), M.Normal(0.0, 1.0))
    return P


@pytest.mark.parametrize("jit", ["0", "1"])
@pytest.mark.parametrize("fed", [False, True], ids=["constant", "site-fed"])
def test_edge_parameters_through_the_prior_draw(oracle, fed, jit, monkeypatch):
    """Binomial(0, .), Binomial(., 0), Binomial(., 1), Poisson(inf) draw nothing; Poisson(1e-300) one block; Binomial(10, NaN) is 0 without a
    draw and Poisson(1e19) saturates: the cells SC.EDGES names, equal to the oracle's, and every following Normal(0, 1) equal to the
    oracle's too (the stream position).  C = 67: two waves, the second ragged.  prior_init draws every site, so the site-fed form
    feeds the parameter as `parent * 0 + value`; the form with the parent set by set_values goes through predict_eval below."""
    monkeypatch.setenv("FG_JIT", jit)
    P = _edge_program(fed)
    cp, om = E.compile_model(P), oracle.OracleModel(P)
    assert cp.site_names == om.site_names
    C, seed = 67, 5
    cells, acc = _prior_cells(cp, C, seed)
    want = np.stack([om.run_prior(seed, c, 0)[0] for c in range(C)], axis=1)
    wacc = np.stack([om.run_prior(seed, c, 0)[1] for c in range(C)], axis=1)
    for j, nm in enumerate(cp.site_names):
        if cp.site_vtypes[j] == 0:
            _close_f64(f"{nm}", _f64(cells[j]), _f64(want[j]), REL)
        else:
            i = int(nm[1:nm.index("_")])
            print(f"{nm}: device {np.unique(cells[j]).tolist()} oracle {np.unique(want[j]).tolist()} table {SC.EDGES[i][3]}")
            assert np.array_equal(cells[j], want[j]) and (cells[j] == SC.EDGES[i][3]).all(), nm
    with np.errstate(invalid="ignore"):                    # (-inf) - (-inf)
        same = (np.isnan(acc) & np.isnan(wacc)) | (acc == wacc) | (np.abs(acc - wacc) <= 1e-10 + 1e-10 * np.abs(wacc))
    print(f"accumulators: {int((~same).sum())} of {same.size} differ from the oracle; log_prior values {np.unique(acc[0])[:4].tolist()}")
    assert same.all()


def test_edge_parameters_fed_by_set_values_through_the_predictive_path(oracle):
    """The parent sites hold the edge values themselves, the NaN and the infinity included, put there by set_values; each edge is an
    observe statement fed by its parent (an M.Dist without constructor validation) and followed by a Normal(0, 1) statement.  The
    replicates of predict_eval at the current values against oracle.sample_dist on the purpose-9 stream."""
    P = M.Program()
    parents, stmts = [], []
    for i, (name, family, params, _, _) in enumerate(SC.EDGES):
        parents.append(P.sample(M.addr(f"p{i}"), M.Normal(0.0, 1.0)))
    for i, (name, family, params, _, _) in enumerate(SC.EDGES):
        head = [float(p) for p in params[:-1]]
        P.observe(M.addr(f"o{i}_a_{name}"), _edge_dist(family, head + [parents[i]]), 1)
        P.observe(M.addr(f"o{i}_b_after"), M.Normal(0.0, 1.0), 0.5)
        stmts.append((family, (lambda head, i: (lambda v: head + [v[f"p{i}"]]))(head, i), 1))
        stmts.append(("Normal", lambda v: [0.0, 1.0], 0.5))
    cp = E.compile_model(P)
    assert cp.site_names == [f"p{i}" for i in range(len(SC.EDGES))] and cp.O == 2 * len(SC.EDGES)
    C = 67
    cells = np.zeros((cp.S, C), dtype=np.int64)
    for i, e in enumerate(SC.EDGES):
        cells[i, :] = np.array([float(e[2][-1])]).view(np.int64)[0]
    eng = E.Engine(cp, C, seed=5, chain_offset=7)
    eng.set_values(cells)
    y, _ = _predict(eng, None, iter0=2, want_ll=False)
    eng.close()
    vals = {f"p{i}": np.full((1, C), float(e[2][-1])) for i, e in enumerate(SC.EDGES)}
    wy, _ = _oracle_tables(oracle, stmts, vals, 5, 7, 2)
    for i, e in enumerate(SC.EDGES):
        got, want = y[0, 2 * i], wy[0, 2 * i]
        print(f"{e[0]}: device {np.unique(got).tolist()} oracle {np.unique(want).tolist()} table {e[3]}")
        assert np.array_equal(got, want) and (got == e[3]).all(), e[0]
        _close_f64(f"Normal(0, 1) after {e[0]}", _f64(y[0, 2 * i + 1]), _f64(wy[0, 2 * i + 1]), REL)
