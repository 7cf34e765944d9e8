"""Observed counts convert as the reference does (crates/fugue-wasm/src/dsl.rs:71-84, 843-856, 985-1006), on the CPU:

  * tests/golden/observed_casts.json (rows derived by hand from those lines) against the plain-integer restatement;
  * the oracle's `run_score` on the programs of tests/obs_cast_programs.py against restatement + the oracle's integer densities (pinned
    by tests/test_oracle_kats.py) -- the oracle's own conversion (orc_model.c) is what is under test here;
  * the saturated count: Poisson(3) at k = 2^63 - 1 against k ln 3 - 3 - lgamma(k + 1) at 200 bits, so that the expectation at i64::MAX
    rests on something other than the oracle;
  * the host side of the library without a device: the hoisted ln k! / ln C(n, k) cannot be read back, but `fg_program_observe_value`
    returns the value as observed, and a DSL text program compiles to the program of its Python mirror.

Before the conversion was written from dsl.rs the oracle (and, by the same misreading, the device) truncated any finite value toward zero
and clamped nothing: Poisson(3) observed at 2.5 scored -1.4959226032237258 (k = 2) where the reference scores -3.0 (k = 0), at -2.0 and at
1e300 -inf where the reference scores -3.0 and -3.834124404243824e20, Binomial(8, .25) at 2.5 -1.1664766467752623 for -2.301456579614247."""
import math

import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import model as M
from tests import obs_cast_programs as OC
from tests import obs_cast_restatement as R


# ---- the fixture and the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vtype", ["u64", "usize", "i64", "bool"])
def test_restatement_reproduces_every_fixture_row(vtype):
    rows = [r for r in OC.FIX["observed"] if r["vtype"] == vtype]
    assert len(rows) == 21
    for r in rows:
        got = R.observed_int(vtype, R.from_bits(r["value"]))
        assert isinstance(got, int) and got == int(r["expect"]), (r, got)


def test_restatement_reproduces_the_binomial_n_table():
    assert len(OC.FIX["binomial_n"]) >= 6
    for r in OC.FIX["binomial_n"]:
        ok, n = R.binomial_n(R.from_bits(r["value"]))
        assert ok == r["valid"] and (n is None if r["n"] is None else n == int(r["n"])), (r, ok, n)


def test_fixture_holds_the_values_and_expectations_the_conversion_is_defined_by():
    """The rows a truncating cast gets wrong are there, with the reference's answer."""
    row = {(r["vtype"], r["readable"]): r["expect"] for r in OC.FIX["observed"]}
    for vt in ("u64", "usize", "i64"):
        assert row[(vt, "2.5")] == "0" and row[(vt, "2^63")] == row[(vt, "1e300")] == "9223372036854775807"
        assert row[(vt, "NaN")] == row[(vt, "+inf")] == row[(vt, "-inf")] == "0"
    assert row[("u64", "-2.0")] == row[("usize", "-2.0")] == "0" and row[("i64", "-2.0")] == "-2"
    assert row[("u64", "-1e300")] == "0" and row[("i64", "-1e300")] == "-9223372036854775808"
    assert [row[("bool", k)] for k in ("0.0", "-0.0", "NaN", "5e-324")] == ["0", "0", "1", "1"]
    bn = {r["readable"]: (r["valid"], r["n"]) for r in OC.FIX["binomial_n"]}
    assert bn["8.5"] == bn["-1.0"] == bn["NaN"] == bn["+inf"] == (False, None) and bn["-0.0"] == (True, "0") and bn["1e300"] == (True, "18446744073709551615")


# ---- the oracle ------------------------------------------------------------------------------------------------------------------
def _oracle_scores(oracle, program, site_values):
    om = oracle.OracleModel(program)
    cells = OC.cells_of(om.site_names, site_values)
    return np.array([om.run_score(cells[:, k])[0] for k in range(cells.shape[1])]).T          # [3][C]


@pytest.mark.parametrize("which", ["runtime", "small", "big", "stream_small"])
def test_oracle_scores_the_programs_as_the_reference_does(oracle, which):
    """The three accumulators of every chain: prior from the formulas, likelihood = the statements' expected terms added in program order.
    The programs are laid out so that numbers decide (tests/obs_cast_programs.py): most chains of RUNTIME and every chain of the literal
    programs have a finite expected likelihood."""
    small, big, rest = OC.split_statements(oracle)
    assert len(small) + len(big) + len(rest) == len(OC.all_statements()) and len(small) >= 100 and len(big) == 10
    stmts, sites, tables = {"runtime": (OC.runtime_statements(), OC.RUNTIME_SITES, OC.runtime_tables()), "small": (small, OC.CONST_SITES, [OC.const_site_values(16)]),
                            "big": (big, OC.CONST_SITES, [OC.const_site_values(16)]), "stream_small": (OC.streamable(small), OC.CONST_SITES, [OC.const_site_values(16)])}[which]
    prog = OC.build(stmts, sites)
    n_finite = n = 0
    for values in tables:
        exp = OC.expected_table(oracle, stmts, values)
        acc = _oracle_scores(oracle, prog, values)
        for k, s in enumerate(values):
            lik = OC.in_order_sum(exp[:, k])
            n_finite, n = n_finite + math.isfinite(lik), n + 1
            OC.check(acc[0, k], OC.prior_of(sites, s), (which, "prior", k, s))
            OC.check(acc[1, k], lik, (which, "likelihood", k, s))
            assert acc[2, k] == 0.0
    print(which, "chains with a finite expected likelihood:", n_finite, "of", n)
    assert n_finite > n / 2 if which == "runtime" else n_finite == n


FAMILIES = [("Poisson", [3.0]), ("Binomial", [8.0, 0.25]), ("Categorical", [0.2, 0.5, 0.3]), ("DiscreteUniform", [1, 9]), ("Bernoulli", [0.3])]


@pytest.mark.parametrize("family,params", FAMILIES, ids=[f for f, _ in FAMILIES])
def test_oracle_converts_every_fixture_value_one_statement_at_a_time(oracle, family, params):
    """One observe statement per program, so that no -inf of a neighbour hides a term: the value as a literal and as an f64 site."""
    dist = {"Poisson": lambda: M.Poisson(3.0), "Binomial": lambda: M.Binomial(8, 0.25), "Categorical": lambda: M.Categorical([0.2, 0.5, 0.3]),
            "DiscreteUniform": lambda: M.DiscreteUniform(1, 9), "Bernoulli": lambda: M.Bernoulli(0.3)}[family]
    P = M.Program()
    v = P.sample(M.addr("v"), M.Normal(0.0, 1.0))
    P.observe(M.addr("o"), dist(), v)
    om = oracle.OracleModel(P)
    for x in OC.VALUES:
        exp = R.expected_logpdf(oracle, family, x, params)
        print(family, repr(x), "expected", exp)
        OC.check(om.run_score(np.array([R.to_bits(x)], dtype=np.int64))[0][1], exp, (family, "site", x))
        Q = M.Program()
        Q.observe(M.addr("o"), dist(), x)
        OC.check(oracle.OracleModel(Q).run_score(np.zeros(0, dtype=np.int64))[0][1], exp, (family, "literal", x))


def test_the_rows_the_truncating_cast_got_wrong(oracle):
    """The four rows measured on the oracle before its conversion was rewritten, with the reference's integers and log-densities."""
    for family, params, x, k, lp in [("Poisson", [3.0], 2.5, 0, -3.0), ("Poisson", [3.0], -2.0, 0, -3.0), ("Poisson", [3.0], 1e300, R.I64_MAX, -3.834124404243824e20),
                                     ("Binomial", [8.0, 0.25], 2.5, 0, -2.301456579614247)]:
        assert R.observed_int("u64", x) == k
        P = M.Program()
        P.observe(M.addr("o"), M.Dist(family, [M.as_expr(p) for p in params]), x)
        got = oracle.OracleModel(P).run_score(np.zeros(0, dtype=np.int64))[0][1]
        print(family, x, "->", got)
        OC.check(got, lp, (family, x))


def test_oracle_binomial_n_follows_build_dist(oracle):
    for r in OC.FIX["binomial_n"]:
        n = R.from_bits(r["value"])
        got = oracle.logpdf("Binomial", 2, [n, 0.25])
        if not r["valid"]:
            assert got == -math.inf, (r, got)
        elif int(r["n"]) < 2:
            assert got == -math.inf, (r, got)                                  # k > n
        else:
            assert math.isfinite(got), (r, got)
            OC.check(got, oracle.logpdf("Binomial", 2, [float(int(r["n"])), 0.25]), r)


def test_poisson_at_the_saturated_count_against_200_bits(oracle):
    mp = pytest.importorskip("mpmath")
    mp.mp.prec = 200
    for k in (R.I64_MAX, R.I64_MAX - 1023):                                     # 2^63 - 1 and 2^63 - 1024
        want = mp.mpf(k) * mp.log(3) - 3 - mp.loggamma(mp.mpf(k) + 1)
        got = oracle.logpdf("Poisson", k, [3.0])
        rel = abs((mp.mpf(got) - want) / want)
        print("k =", k, "oracle", got, "200 bits", mp.nstr(want, 20), "relative", mp.nstr(rel, 3))
        assert rel <= mp.mpf("1e-13")


# ---- the library's host side -------------------------------------------------------------------------------------------------------
def test_observe_value_is_the_value_as_observed():
    """`fg_program_observe_value` of a discrete statement: the converted integer (fugue_amd/checks.py compares replicated counts with it);
    an f64 statement keeps its number."""
    for vtype, family in (("u64", "Poisson"), ("usize", "Categorical"), ("i64", "DiscreteUniform"), ("bool", "Bernoulli")):
        dist = {"Poisson": lambda: M.Poisson(3.0), "Categorical": lambda: M.Categorical([0.2, 0.5, 0.3]), "DiscreteUniform": lambda: M.DiscreteUniform(1, 9),
                "Bernoulli": lambda: M.Bernoulli(0.3)}[family]
        P = M.Program()
        data = P.bind_data("y", OC.FINITE)
        for i, x in enumerate(OC.VALUES):
            P.observe(M.addr("lit", i), dist(), x)
        for i in range(len(OC.FINITE)):
            P.observe(M.addr("dat", i), dist(), data[i])
        P.observe(M.addr("f"), M.Normal(0.0, 1.0), 2.5)
        cp = E.compile_model(P)
        want = [float(R.observed_int(vtype, x)) for x in OC.VALUES] + [float(R.observed_int(vtype, x)) for x in OC.FINITE] + [2.5]
        print(family, cp.observe_values)
        assert cp.observe_values == want and cp.observe_vtypes[:-1] == [R.VTYPES[vtype]] * (len(want) - 1)


def test_dsl_text_with_a_fractional_count_compiles_to_its_mirror():
    from tests.dsl_models import PAIRS
    src, data, mirror = PAIRS["obs_cast"]
    assert 'observe(addr!("k"), Poisson(3.0), 2.5)' in src
    cp, ref = E.CompiledProgram.from_dsl(src, data), E.compile_model(mirror())
    assert (cp.S, cp.d, cp.O, cp.n_instructions, cp.n_slots) == (ref.S, ref.d, ref.O, ref.n_instructions, ref.n_slots)
    assert cp.observe_names == ref.observe_names and cp.observe_vtypes == ref.observe_vtypes
    assert cp.observe_values == ref.observe_values and cp.observe_values[ref.observe_names.index("k")] == 0.0
    assert cp.warnings == []
