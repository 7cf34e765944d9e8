"""GPU tests of the model's return value on the device (fg_result.hip: k_result_eval behind fg_result_eval).

Reference, computed once per module: for every result expression e a TWIN program -- the same statements plus `factor(e)` -- is
scored draw by draw (set_values, fg_log_joint); its log_factors accumulator 0.0 + e is what the interpreter gives e.  The kernel's
output must equal it bit for bit (+0.0 and -0.0 counted equal: the accumulator starts at +0.0; any NaN equal to any NaN: IEEE leaves
the payload an addition hands on open).  Every other shape is then compared with slices of that one reference: a chain's result
depends on that chain's cells only.  Synthetic draws (tests/result_cases.py) hold -0.0, +-inf, NaN and an out-of-range category.
Every compared figure is printed before it is asserted."""
import numpy as np
import pytest

from fugue_amd import diagnostics as D
from fugue_amd import engine as E
from fugue_amd import inference as I
from fugue_amd import model as M
from fugue_amd import session as Sn
from fugue_amd import workloads as W
from tests import diag_reference as R
from tests import qstream_restatement as Q
from tests import result_cases as K

pytestmark = pytest.mark.gpu

N, CMAX = 7, 130
FIGURES = ("r_hat", "ess", "mean", "std")
ABS_TOL = dict(r_hat=0.0, ess=0.0, mean=1e-12, std=0.0)          # as tests/test_gpu_diag_stream.py


def _program(names=None, twin_of=None):
    """The base program with the named results (None: all, in table order), or the twin of one expression (factor(e), no result)."""
    P, v = K.base_program()
    exact, trans = K.expressions(v)
    table = {**exact, **trans}
    if twin_of is not None:
        P.factor(table[twin_of])
        P.result = None
    else:
        P.result = {k: table[k] for k in (names or list(table))}
    return P


ALL = list({**K.expressions(K.base_program()[1])[0], **K.expressions(K.base_program()[1])[1]})
EXACT = list(K.expressions(K.base_program()[1])[0])


def _same_bits(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return (got.view(np.int64) == want.view(np.int64)) | ((got == 0.0) & (want == 0.0)) | (np.isnan(got) & np.isnan(want))


def _assert_bits(label, got, want):
    ok = _same_bits(got, want)
    print(f"{label}: {ok.size - int(ok.sum())} of {ok.size} values differ; NaN {int(np.isnan(want).sum())}, inf {int(np.isinf(want).sum())}, zero {int((want == 0).sum())}")
    assert got.shape == want.shape and ok.all(), (label, np.argwhere(~ok)[:5].tolist(), got[~ok][:5], want[~ok][:5])


class _Ctx:
    def __init__(self):
        self.cells = K.draws(N, CMAX)                     # [N][13][CMAX]
        self.cp_all = E.compile_model(_program())
        self.engines = {}

    def engine(self, cp, C):
        key = (id(cp), C)
        if key not in self.engines:
            self.engines[key] = E.Engine(cp, C, seed=3)
        return self.engines[key]

    def close(self):
        for e in self.engines.values():
            e.close()


@pytest.fixture(scope="module")
def ctx():
    c = _Ctx()
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref(ctx):
    """[N][len(ALL)][CMAX]: the twins' log_factors accumulators, draw by draw."""
    out = np.zeros((N, len(ALL), CMAX))
    for r, name in enumerate(ALL):
        eng = E.Engine(E.compile_model(_program(twin_of=name)), CMAX, seed=3)
        for t in range(N):
            eng.set_values(ctx.cells[t])
            out[t, r] = eng.log_joint()[2]
        eng.close()
    return out


def _eval(eng, cells, rows="all", n=None, guard=64):
    """fg_result_eval over host cells [n][n_rows][C] -> [n][R][C]; the output buffer sits between two runs of guard words."""
    n = cells.shape[0] if n is None else n
    Rr, C = eng.cp.R, eng.C
    d_in = eng.upload(np.ascontiguousarray(cells))
    pattern = np.full(guard, -1234.5)
    host = np.concatenate([pattern, np.full(n * Rr * C, 777.0), pattern])
    d_out = eng.upload(host)
    try:
        eng.result_eval(d_in, n, rows=(list(range(cells.shape[1])) if rows == "all" else rows), out=d_out + guard * 8)
        eng.synchronize()
        back = eng.download(d_out, (host.size,))
    finally:
        eng.device_free(d_in)
        eng.device_free(d_out)
    assert np.array_equal(back[:guard], pattern) and np.array_equal(back[-guard:], pattern), "guard words around d_out were written"
    return back[guard:-guard].reshape(n, Rr, C)


# ---- 1. device identity and the oracle ---------------------------------------------------------------------------------------------
def test_every_opcode_gives_the_interpreters_bits(ctx, ref):
    eng = ctx.engine(ctx.cp_all, CMAX)
    assert ctx.cp_all.result_names == ["result." + k for k in ALL]
    got = _eval(eng, ctx.cells)
    for r, name in enumerate(ALL):
        _assert_bits(f"identity {name}", got[:, r], ref[:, r])
    assert np.isnan(ref[:, ALL.index("select")]).sum() >= 2          # the out-of-range categories did give NaN
    assert np.isinf(ref).any() and (ref[:, ALL.index("no_site")] == 7.0).all()


def test_oracle_parity(ctx, oracle):
    """The same twins through the oracle's factor accumulator: bit-equal for the exact expressions, 1e-12 relative (ocml against
    glibc, tests/test_gpu_parity.py::_close) where a transcendental is involved.  No case is excluded."""
    got = _eval(ctx.engine(ctx.cp_all, CMAX), ctx.cells)
    for r, name in enumerate(ALL):
        om = oracle.OracleModel(_program(twin_of=name))
        want = np.array([[om.run_score(ctx.cells[t, :, c])[0][2] for c in range(CMAX)] for t in range(N)])
        if name in EXACT:
            _assert_bits(f"oracle {name}", got[:, r], want)
        else:
            g, w = got[:, r], want
            both_inf = np.isinf(g) & np.isinf(w) & (np.sign(g) == np.sign(w))
            both_nan = np.isnan(g) & np.isnan(w)
            with np.errstate(all="ignore"):
                rel = np.abs(g - w) / np.abs(w)
                ok = both_inf | both_nan | (np.abs(g - w) <= 1e-12 * np.abs(w))
            fin = np.isfinite(rel)
            print(f"oracle {name}: worst relative difference {rel[fin].max() if fin.any() else 0.0:.3e}; {int((~ok).sum())} outside 1e-12")
            assert ok.all(), (name, g[~ok][:5], w[~ok][:5])


# ---- 2. shapes -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small_programs():
    return {1: E.compile_model(_program(["lin9"])), 3: E.compile_model(_program(["select", "exp", "clamp"]))}


@pytest.mark.parametrize("C", [1, 63, 64, 65, 130])
def test_chain_counts_draw_counts_and_result_counts(ctx, ref, small_programs, C):
    for Rr, cp in small_programs.items():
        idx = [ALL.index(k.split(".", 1)[1]) for k in cp.result_names]
        eng = ctx.engine(cp, C)
        for n in (1, 2, 7):
            got = _eval(eng, ctx.cells[:n, :, :C])
            _assert_bits(f"C={C} n={n} R={Rr}", got, ref[:n][:, idx][:, :, :C])


def test_row_layouts(ctx, ref):
    """A subset and a permutation of the sites as rows (MH layout), h_rows == NULL (the f64 sites in coordinate order) and no draws
    at all: a site that is not among the rows comes from the engine's current values."""
    eng = ctx.engine(ctx.cp_all, CMAX)
    cp = ctx.cp_all
    cur = ctx.cells[3]                                    # the engine's values: draw 3
    eng.set_values(cur)
    # the reference for "site j not recorded": the full layout on draws whose row j is the current value in every draw
    def expected(recorded):
        mod = ctx.cells.copy()
        for j in range(cp.S):
            if j not in recorded:
                mod[:, j] = cur[j][None]
        return _eval(eng, mod)
    rows = [12, 0, 5, 10, 3, 8, 1]                        # u, b#0, b#5, k, b#3, b#8, b#1: the others (b#2, b#4, b#6, b#7, f, s) are not recorded
    got = _eval(eng, np.ascontiguousarray(ctx.cells[:, rows]), rows=rows)
    _assert_bits("rows: subset and permutation", got, expected(rows))
    f64 = list(cp.f64_sites)
    assert f64 == [0, 1, 2, 3, 4, 5, 6, 7, 8, 11, 12]
    got = _eval(eng, np.ascontiguousarray(ctx.cells[:, f64]), rows=None)
    _assert_bits("rows: NULL (HMC draw layout)", got, expected(f64))
    _assert_bits("no draws: the current values", eng.result_values(), ref[3])
    # bad rows are refused before anything is launched
    d_in = eng.upload(ctx.cells)
    d_out = eng.device_alloc(N * cp.R * CMAX * 8)
    try:
        for bad in ([0, 1, 13], [0, -1], [2, 5, 2]):
            with pytest.raises(E.EngineError) as err:
                eng.result_eval(d_in, N, rows=bad, out=d_out)
            assert err.value.code == E.FG_E_BAD_ARG, bad
        arr = (E.C.c_int32 * 3)(0, 1, 2)
        assert E.lib().fg_result_eval(eng.h, d_in, N, None, 3, d_out) == E.FG_E_BAD_ARG      # h_rows == NULL needs n_rows == d
        assert E.lib().fg_result_eval(eng.h, None, 2, None, 0, d_out) == E.FG_E_BAD_ARG      # no draws: n must be 1
        assert E.lib().fg_result_eval(eng.h, d_in, 0, arr, 3, None) == 0                      # n == 0: FG_OK, nothing launched
    finally:
        eng.device_free(d_in)
        eng.device_free(d_out)
    plain = E.Engine(E.compile_model(_program(twin_of="lin9")), 64, seed=1)                # a program without results
    assert E.lib().fg_result_eval(plain.h, None, 1, None, 0, None) == E.FG_E_STATE
    plain.close()


def test_chunks_and_the_global_tile_form(ctx, ref, monkeypatch):
    eng = ctx.engine(ctx.cp_all, CMAX)
    whole = _eval(eng, ctx.cells)
    _assert_bits("whole buffer", whole, ref)
    for step in (1, 3, N):
        parts = [_eval(eng, ctx.cells[t:t + step]) for t in range(0, N, step)]
        _assert_bits(f"chunks of {step}", np.concatenate(parts), whole)
    monkeypatch.setenv("FG_RESULT_GLOBAL_TILE", "1")      # read per call
    _assert_bits("global tile form", _eval(eng, ctx.cells), whole)
    eng1 = ctx.engine(ctx.cp_all, 1)
    _assert_bits("global tile form, C = 1", _eval(eng1, ctx.cells[:, :, :1]), whole[:, :, :1])
    monkeypatch.delenv("FG_RESULT_GLOBAL_TILE")
    _assert_bits("LDS form again", _eval(eng, ctx.cells), whole)


# ---- 3. nothing else moves -----------------------------------------------------------------------------------------------------
def _with_results(make):
    P = make()
    sites = [M.Expr("site", a=h) for h in range(P.n_samples)]
    lin = M.as_expr(0.25)
    for j, s in enumerate(sites[:9]):
        lin = lin + s * (0.5 + 0.125 * j)
    P.result = (sites[0] * 2.0 + 1.0, M.exp(sites[-1]), lin)
    return P


def _without_results(make):
    P = make()
    P.result = None
    return P


@pytest.mark.parametrize("name", ["refmodel4", "indep_mixed"])
def test_a_program_with_results_runs_the_same_kernels_to_the_same_bits(name, monkeypatch):
    monkeypatch.setenv("FG_JIT", "0")                     # the library's own kernels (a unit compiled at run time takes longer than this test may)
    from tests.models import indep_mixed
    make = (lambda: W.reference_model(4)) if name == "refmodel4" else indep_mixed
    seen = []
    for build in (_without_results, _with_results):
        cp = E.compile_model(build(make))
        C = 130
        out = {}
        eng = E.Engine(cp, C, seed=5)
        buf = eng.device_alloc(12 * cp.d * C * 8)
        eng.hmc_run(E.hmc_config(), 12, 12, buf)
        out["hmc"] = eng.download(buf, (12, cp.d, C), dtype=np.int64)
        out["hmc_kernel"], out["hmc_state"] = eng.hmc_last_kernel(), len(eng.state_export())
        eng.device_free(buf); eng.close()
        eng = E.Engine(cp, C, seed=5)
        buf = eng.device_alloc(12 * cp.S * C * 8)
        eng.mh_run(12, 12, None, list(range(cp.S)), buf)
        out["mh"] = eng.download(buf, (12, cp.S, C), dtype=np.int64)
        out["mh_kernel"], out["mh_state"] = eng.mh_last_kernel(), len(eng.state_export())
        eng.device_free(buf); eng.close()
        eng = E.Engine(cp, C, seed=5)
        r = eng.smc_run(rejuvenation_steps=1)
        out["smc"], out["smc_w"], out["smc_lw"], out["smc_ev"], out["smc_betas"] = r["values"], r["weights"], r["log_w"], np.float64(r["log_evidence"]), r["betas"]
        eng.close()
        seen.append((cp.R, out))
    (r0, a), (r1, b) = seen
    assert (r0, r1) == (0, 3)
    print(name, a["hmc_kernel"], "|", a["mh_kernel"], "| state bytes", a["hmc_state"], a["mh_state"], "| log evidence", a["smc_ev"])
    for k in a:
        if isinstance(a[k], (str, int)):
            assert a[k] == b[k], (k, a[k], b[k])
        else:
            assert np.array_equal(np.asarray(a[k]).view(np.int64) if np.asarray(a[k]).dtype == np.float64 else np.asarray(a[k]),
                                  np.asarray(b[k]).view(np.int64) if np.asarray(b[k]).dtype == np.float64 else np.asarray(b[k])), k


# ---- 4. the drivers ------------------------------------------------------------------------------------------------------------
def _driver_model():
    """Normal sites only (the hand-written HMC kernels, nothing compiled at run time); A = {sigma, contrast, pred}."""
    P = M.Program()
    ls = P.sample(M.addr("log_sigma"), M.Normal(0.0, 0.5))
    a = P.sample(M.addr("mu_a"), M.Normal(0.0, 1.0))
    b = P.sample(M.addr("mu_b"), M.Normal(0.5, 1.0))
    P.observe(M.addr("ya"), M.Normal(a, 0.5), 0.7)
    P.observe(M.addr("yb"), M.Normal(b, 0.5), -0.2)
    P.result = {"sigma": M.exp(ls), "contrast": a - b, "pred": a * 0.5 + b * 2.0 + 1.0}
    return P


def _reeval(cp, cells):
    """fg_result_eval over returned cells [n][S][C] (all sites as rows) on a fresh engine."""
    eng = E.Engine(cp, cells.shape[2], seed=99)
    try:
        return _eval(eng, cells)
    finally:
        eng.close()


def test_stored_runs_carry_the_results(monkeypatch):
    monkeypatch.setenv("FG_JIT", "0")                     # the hand-written and interpreter kernels: nothing is compiled at run time here
    cp = E.compile_model(_driver_model())
    names = ["result.sigma", "result.contrast", "result.pred"]
    hm = I.hmc_chain(3, cp, 10, 10, n_chains=70)
    assert hm.result_names == names and hm.results.shape == (10, 3, 70)
    _assert_bits("hmc_chain.results", hm.results, _reeval(cp, hm.cells))
    assert np.array_equal(hm.get_result("result.sigma"), hm.results[:, 0]) and np.isfinite(hm.results).all()
    print("hmc_chain: mean sigma", hm.get_result("result.sigma").mean(), "mean exp(log_sigma) on the host", np.exp(hm.get_f64("log_sigma")).mean())
    assert np.allclose(hm.get_result("result.sigma"), np.exp(hm.get_f64("log_sigma")), rtol=1e-12) and np.array_equal(hm.get_result("result.contrast"), hm.get_f64("mu_a") - hm.get_f64("mu_b"))
    mh = I.adaptive_mcmc_chain(3, cp, 10, 10, n_chains=70)
    assert mh.result_names == names
    _assert_bits("adaptive_mcmc_chain.results", mh.results, _reeval(cp, mh.cells))
    smc = I.adaptive_smc(3, 70, cp)
    assert smc.result_names == names and smc.results.shape == (3, 70)
    _assert_bits("adaptive_smc.results", smc.results, _reeval(cp, smc.cells[None])[0])
    # a model with discrete sites under hmc_chain: they keep their prior draw and reach the results from the engine's values
    mixed = E.compile_model(_program(["int_sites", "bool_site", "select"]))
    hx = I.hmc_chain(4, mixed, 5, 5, n_chains=65)
    _assert_bits("hmc_chain.results with discrete sites", hx.results, _reeval(mixed, hx.cells))
    with pytest.raises(M.FugueError):
        hm.get_result("result.nope")
    none = I.hmc_chain(3, _without_results(_driver_model), 4, 4, n_chains=64)
    assert none.results is None and none.result_names == []
    s = Sn.HmcSession(_driver_model(), n_chains=64, seed=2, n_warmup=5)
    s.step(6)
    v = s.eng.get_values()
    assert s.result_names() == names
    _assert_bits("HmcSession.result", s.result(), _reeval(s.cp, v[None])[0])
    s.close()
    m = Sn.MhSession(_driver_model(), n_chains=64, seed=2)
    m.step(6)
    _assert_bits("MhSession.result", m.result(), _reeval(m.cp, m.eng.get_values()[None])[0])
    m.close()


def test_hmc_chain_summary_with_results_and_quantiles(monkeypatch):
    """C = 128, n = 96, chunk = 20: the figures of the results against the stored-draws diagnostics of hmc_chain(...).results from the
    same seed (the comparison tests/test_gpu_diag_stream.py makes between the streamed and the stored form), their quantiles the
    exact order statistics, the site figures bitwise those of results=False."""
    monkeypatch.setenv("FG_JIT", "0")
    a = dict(seed=7, model_fn=_driver_model(), n_samples=96, n_warmup=20, n_chains=128)
    chains = I.hmc_chain(**a)
    plain = I.hmc_chain_summary(chunk=20, max_lag=96, quantiles=True, **a)              # 96 lags >= n - 1: Geyer's sequence cannot ask for more
    summ = I.hmc_chain_summary(chunk=20, max_lag=96, quantiles=True, results=True, **a)
    rs = summ.results
    assert plain.results is None and rs.sites == chains.result_names and (rs.n_samples, rs.n_chains) == (96, 128)
    stored = D.ChainDiagnostics(D.HostMoments(np.ascontiguousarray(chains.results))).summary()
    for i, nm in enumerate(rs.sites):
        for k in FIGURES:
            print(f"{nm} {k}: streamed {getattr(rs, k)[i]!r} stored {float(stored[k][i])!r}")
    for i, nm in enumerate(rs.sites):
        for k in FIGURES:
            got, want = float(getattr(rs, k)[i]), float(stored[k][i])
            assert np.isfinite(got) and abs(got - want) <= max(R.FIGURE_TOL[k] * abs(want), ABS_TOL[k]), (nm, k, got, want)
    want_q = Q.reference_all(np.ascontiguousarray(chains.results), I.QUANTILE_PROBS)
    for i, nm in enumerate(rs.sites):
        print(f"{nm} quantiles: summary {rs.quantiles[i].tolist()} sort of the stored results {want_q[i].tolist()}")
    assert np.array_equal(Q.bits(rs.quantiles), Q.bits(want_q))
    print(f"passes: sites {summ.passes}, results {rs.passes}")
    for k in ("mean", "std", "r_hat", "ess", "quantiles"):
        assert np.array_equal(Q.bits(getattr(summ, k)), Q.bits(getattr(plain, k))), k
    assert (summ.accept_rate, summ.mean_step_size, summ.n_divergent, summ.passes) == (plain.accept_rate, plain.mean_step_size, plain.n_divergent, plain.passes)
    # MH: every site the results read is a recorded f64 site
    b = dict(seed=7, model_fn=_driver_model(), n_samples=40, n_warmup=20, n_chains=128)
    mh = I.adaptive_mcmc_chain(**b)
    ms = I.adaptive_mcmc_chain_summary(chunk=16, results=True, **b)
    stored = D.ChainDiagnostics(D.HostMoments(np.ascontiguousarray(mh.results))).summary()
    for i, nm in enumerate(ms.results.sites):
        for k in ("mean", "std", "r_hat"):
            got, want = float(getattr(ms.results, k)[i]), float(stored[k][i])
            print(f"mh {nm} {k}: streamed {got!r} stored {want!r}")
            assert abs(got - want) <= max(R.FIGURE_TOL[k] * abs(want), ABS_TOL[k]), (nm, k, got, want)
    with pytest.raises(ValueError):
        I.hmc_chain_summary(3, _without_results(_driver_model), 8, 4, n_chains=64, results=True)
