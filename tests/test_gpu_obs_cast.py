"""Observed counts convert on the device as the reference does (crates/fugue-wasm/src/dsl.rs:71-84, 843-856, 985-1006), on every path that
evaluates an observe statement.  The programs and their expectation are tests/obs_cast_programs.py's: the plain-integer restatement
(tests/obs_cast_restatement.py, checked against tests/golden/observed_casts.json on the CPU) picks the integer, the oracle's integer
densities (pinned by tests/test_oracle_kats.py) score it -- nothing of the expectation passes through a conversion under test.

An accumulator is a sum, so the programs whose accumulators are compared hold at most one statement per chain that can leave its support
(RUNTIME: one case per chain) or none at all (SMALL, BIG, STREAM_SMALL: literals whose expectation is finite); each of these tests asserts
how many of its chains have a finite expected likelihood, so that a -inf cannot come to hide the rest unnoticed.

Which assertion covers which copy of the conversion:
  interpreter (fg_interp.h, both call sites)   `log_joint()` accumulators of RUNTIME (Categorical: the first site, every other family the second)
  predictive kernel (fg_predict.hip, both)     `predict_eval`'s loglik table, every statement of RUNTIME and ALL
  run-time compiled unit (fg_jit.cpp)          `log_joint_compiled()` accumulators (k_log_joint_jit, no fall-back) of RUNTIME, SMALL and BIG
  host, hoisted ln k! / ln C(n, k)             the pois_s / binom_s statements (FG_F_XHOIST) of ALL per statement, of SMALL / BIG per accumulator
  host, constant of a stream record            `log_joint_stream(want_records=True)` of STREAM per record, of STREAM_SMALL per accumulator
  Binomial n (fg_logpdf / fg_hoist)            the binom_n statement of RUNTIME (n from the site `w`, its own cases) on all of the above

Comparison: exact where the expectation is not finite, 1e-12 max(1, |expected|) otherwise (the project's log-joint tolerance: ocml and
glibc differ by a few ulp in log / lgamma / exp), no chain, case or statement left out."""
import math

import numpy as np
import pytest

from fugue_amd import engine as E
from tests import obs_cast_programs as OC

pytestmark = pytest.mark.gpu

C = OC.C


class _Case:
    """one program, its value tables [table][chain] and the expectation of each: computed once, never written to"""

    def __init__(self, oracle, statements, sites, tables):
        self.statements, self.sites, self.tables = statements, sites, tables
        self.cp = E.compile_model(OC.build(statements, sites))
        assert self.cp.O == len(statements) and self.cp.observe_names == [st.address for st in statements]
        self.cells = [OC.cells_of(self.cp.site_names, t) for t in tables]
        self.exp = [OC.expected_table(oracle, statements, t) for t in tables]                  # [O][C] each
        self.prior = [np.array([OC.prior_of(sites, s) for s in t]) for t in tables]
        self.lik = [np.array([OC.in_order_sum(e[:, k]) for k in range(len(t))]) for e, t in zip(self.exp, tables)]
        for a in self.exp + self.prior + self.lik:
            a.setflags(write=False)

    def finite_share(self):
        return float(np.mean([np.isfinite(l).mean() for l in self.lik]))


@pytest.fixture(scope="module")
def cases(oracle):
    small, big, _rest = OC.split_statements(oracle)
    const = [OC.const_site_values(C)]
    return {"runtime": _Case(oracle, OC.runtime_statements(), OC.RUNTIME_SITES, OC.runtime_tables(C)),
            "small": _Case(oracle, small, OC.CONST_SITES, const), "big": _Case(oracle, big, OC.CONST_SITES, const),
            "all": _Case(oracle, OC.all_statements(), OC.CONST_SITES, const),
            "stream": _Case(oracle, OC.streamable(OC.all_statements()), OC.CONST_SITES, const),
            "stream_small": _Case(oracle, OC.streamable(small), OC.CONST_SITES, const)}


def _check_statements(case, t, table, what):
    assert table.shape == case.exp[t].shape
    for i, st in enumerate(case.statements):
        for k in range(C):
            OC.check(table[i, k], case.exp[t][i, k], (what, st.address, "table", t, "chain", k, case.tables[t][k]))


def _check_accumulators(case, t, acc, what):
    for k in range(C):
        OC.check(acc[0, k], case.prior[t][k], (what, "prior", "table", t, "chain", k, case.tables[t][k]))
        OC.check(acc[1, k], case.lik[t][k], (what, "likelihood", "table", t, "chain", k, case.tables[t][k]))
        assert acc[2, k] == 0.0


def _loglik_table(eng):
    _, d_ll = eng.predict_eval(None, 1, out=False)
    try:
        return eng.download(d_ll, (1, eng.cp.O, eng.C))[0]
    finally:
        eng.device_free(d_ll)


def test_the_layout_lets_numbers_decide(cases):
    """Every case is on some chain; most chains' expected likelihood is finite, and where it is not exactly one statement is -inf; every
    conversion outcome decides a finite likelihood on some chain of RUNTIME and in some statement of SMALL or BIG."""
    rt = cases["runtime"]
    assert len(rt.tables) * C >= OC.N_CASES and rt.finite_share() > 0.5
    for e in rt.exp:
        assert (np.isinf(e).sum(axis=0) <= 1).all()
    row = {st.address: i for i, st in enumerate(rt.statements)}
    case_of = lambda name, value: row[name] * len(OC.VALUES) + [OC.R.to_bits(v) for v in OC.VALUES].index(OC.R.to_bits(value))
    lik = lambda n: rt.lik[n // C][n % C]
    term = lambda name, value: rt.exp[case_of(name, value) // C][row[name], case_of(name, value) % C]
    # fraction -> 0, negative -> 0 (a count) or kept (i64), saturation, the large exact integers, NaN -> 0, each a finite number on its chain
    assert term("pois_c", 2.5) == term("pois_c", -2.0) == term("pois_c", -1e300) == term("pois_c", math.nan) == term("pois_c", -0.5) == -3.0
    assert abs(term("pois_c", 1e300) / -3.834124404243824e20 - 1.0) < 1e-12 and term("pois_c", 1e300) == term("pois_c", OC.P63) != term("pois_c", OC.TOP)
    assert term("du", 2.5) == -math.inf and term("du_neg", -2.0) == term("du_neg", 2.5) == -math.log(5.0) and term("du_neg", -1e300) == -math.inf
    assert math.isfinite(term("du_52", OC.P52)) and term("du_52", 2.0 ** 53) == -math.inf
    assert math.isfinite(term("du_top", OC.TOP)) and term("du_top", OC.P63) == -math.inf and math.isfinite(term("du_max", OC.P63))
    for name, value in [("pois_x", 2.5), ("pois_c", -2.0), ("binom", -0.5), ("cat", -2.5), ("pois_c", 1e300), ("pois_x", OC.P63), ("pois_c", OC.TOP),
                        ("pois_c", OC.P52), ("du_neg", -2.0), ("bern", math.nan), ("cat", math.inf)]:
        assert math.isfinite(lik(case_of(name, value))), (name, value)
    bn = [rt.exp[(OC.N_V * len(OC.VALUES) + r) // C][row["binom_n"], (OC.N_V * len(OC.VALUES) + r) % C] for r in range(len(OC.BINOMIAL_N))]
    assert [math.isfinite(v) for v in bn] == [r["valid"] and int(r["n"]) >= 2 for r in OC.FIX["binomial_n"]]
    for name in ("small", "big", "stream_small"):
        assert cases[name].finite_share() == 1.0 and len(cases[name].statements) >= 8, name
    tags = lambda name: {st.address for st in cases[name].statements}
    idx = {OC.R.to_bits(v): i for i, v in enumerate(OC.FINITE)}
    assert {f"pois_s#{idx[OC.R.to_bits(v)]}" for v in (2.5, -2.0, -1e300, 0.5)} | {f"binom_s#{idx[OC.R.to_bits(2.5)]}", f"cat_s#{idx[OC.R.to_bits(-2.5)]}"} <= tags("small")
    assert {f"pois_s#{idx[OC.R.to_bits(v)]}" for v in (OC.P52, OC.TOP, OC.P63, 1e300)} <= tags("big") and all(a.startswith("pois") for a in tags("big"))


@pytest.mark.parametrize("which", ["runtime", "small", "big", "all", "stream", "stream_small"])
def test_interpreter_and_predictive_kernel_score_as_the_reference(cases, which, monkeypatch):
    """predict_eval's loglik table per statement on every program; the accumulators of log_joint() (the interpreter kernel) and of
    log_joint_stream() where no -inf or huge term hides a neighbour; the score-stream records per statement."""
    monkeypatch.setenv("FG_JIT", "0")
    case = cases[which]
    sums = which in ("runtime", "small", "big", "stream_small")
    eng = E.Engine(case.cp, C, seed=5)
    n_rec = case.cp.stream_records[1]
    assert (n_rec > 0) == (which in ("big", "stream", "stream_small")), case.cp.stream_records      # (BIG is Poisson statements only: all records)
    for t in range(len(case.tables)):
        eng.set_values(case.cells[t])
        _check_statements(case, t, _loglik_table(eng), (which, "predict_eval loglik"))
        if sums:
            _check_accumulators(case, t, eng.log_joint(), (which, "log_joint"))
        if n_rec > 0:
            acc, rec = eng.log_joint_stream(want_records=True)
            assert n_rec == len(case.sites) + len(case.statements)
            _check_statements(case, t, rec[len(case.sites):], (which, "score-stream record"))
            if sums:
                _check_accumulators(case, t, acc, (which, "log_joint_stream"))
        assert np.array_equal(eng.get_values(), case.cells[t])
    eng.close()


def test_global_tile_instantiations_on_the_runtime_program(cases, monkeypatch):
    monkeypatch.setenv("FG_JIT", "0")
    monkeypatch.setenv("FG_GLOBAL_TILE", "1")
    case = cases["runtime"]
    eng = E.Engine(case.cp, C, seed=5)
    for t in range(len(case.tables)):
        eng.set_values(case.cells[t])
        _check_statements(case, t, _loglik_table(eng), "global tile: predict_eval loglik")
        _check_accumulators(case, t, eng.log_joint(), "global tile: log_joint")
    eng.close()


@pytest.mark.parametrize("which", ["runtime", "small", "big"])
def test_compiled_unit_scores_as_the_reference(cases, which, monkeypatch):
    """The three accumulators of k_log_joint_jit, the ScoreGivenTrace of the unit compiled at run time (`log_joint_compiled` launches that
    kernel or fails: there is no fall-back to the interpreter), against the expectation and, bit for bit, against the interpreter kernel.
    Under FG_JIT=0 there is no unit and the call says so."""
    case = cases[which]
    monkeypatch.setenv("FG_JIT", "0")
    eng = E.Engine(case.cp, C, seed=5)
    with pytest.raises(E.EngineError):
        eng.log_joint_compiled()
    eng.close()
    monkeypatch.setenv("FG_JIT", "1")
    eng = E.Engine(case.cp, C, seed=5)
    for t in range(len(case.tables)):
        eng.set_values(case.cells[t])
        acc = eng.log_joint_compiled()
        _check_accumulators(case, t, acc, (which, "log_joint_compiled"))
        assert np.array_equal(acc, eng.log_joint(), equal_nan=True)
    eng.hmc_init(E.hmc_config(n_leapfrog=1, init_step_size=0.01), 0)       # the session re-scores its state with the same kernel after set_values
    eng.set_values(case.cells[0])
    lj = eng.hmc_log_joint()
    for k in range(C):
        OC.check(lj[k], (case.prior[0][k] + case.lik[0][k]) + 0.0, (which, "session log-joint", k))
    eng.close()
