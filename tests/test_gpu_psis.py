"""GPU tests of Pareto-smoothed LOO on a stored table (fg_psis.hip, `Engine.psis_loo`) against tests/psis_restatement.py:
the returned sorted tail bit-equal to the M smallest cells, every count and status exact, every double within
`psis_restatement.tolerances` of that input; ties and signed zeros; the multiset property; a statement alone against the same statement
in a table of three and a call against its repetition, bit for bit; non-finite cells; a session is left as it was; the drivers end to
end.  Every compared figure is printed before it is asserted."""
import math

import numpy as np
import pytest

from fugue_amd import comparison as CMP
from fugue_amd import engine as E
from fugue_amd import inference as I
from fugue_amd import workloads as W
from tests import psis_restatement as R
from tests.models import ZOO

pytestmark = pytest.mark.gpu


class _Engines:
    """One engine per chain count for the whole module (the model does not matter to the call)."""

    def __init__(self):
        self.cp, self.by_c = E.compile_model(W.normal_sites(1)), {}

    def get(self, C: int):
        if C not in self.by_c:
            self.by_c[C] = E.Engine(self.cp, C, seed=1)
        return self.by_c[C]

    def close(self):
        for e in self.by_c.values():
            e.close()


@pytest.fixture(scope="module")
def engines():
    pool = _Engines()
    yield pool
    pool.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run(engines, table):
    table = np.ascontiguousarray(table, dtype=np.float64)
    n, n_sel, C = table.shape
    eng = engines.get(C)
    ptr = eng.upload(table)
    try:
        return eng.psis_loo(ptr, n, n_sel, tail=True)
    finally:
        eng.device_free(ptr)


def same_class(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b or (math.isfinite(a) and math.isfinite(b))


def check(res, table, label):
    """the device's rows and tails against the restatement of every statement; -> the restatement's cases"""
    cases, misses = [], []
    for k in range(table.shape[1]):
        x = R.pooled(table, k)
        want, want_ld = R.psis_statement(x), R.psis_statement(x, ld=True)
        tol = R.tolerances(want, want_ld)
        cases.append(want)
        got_c = {name: int(res[name][k]) for name in R.COUNT_NAMES}
        print(f"{label} statement {k}: counts {got_c}")
        assert got_c == {name: int(want[name]) for name in R.COUNT_NAMES}, (label, k)
        equal_tail = np.array_equal(_bits(res["tail"][k]), _bits(want["tail"]))
        print(f"{label} statement {k}: the sorted tail of {want['M']} bit-equal {equal_tail}")
        assert equal_tail, (label, k)
        for name in R.WORD_NAMES:
            g, w = float(res[name][k]), float(want[name])
            err = abs(g - w) if math.isfinite(g) and math.isfinite(w) else 0.0
            print(f"{label} statement {k} {name}: {g!r} / {w!r}: err {err:.3e} tol {tol[name]:.3e}")
            assert same_class(g, w), (label, k, name, g, w)
            if not err <= tol[name]:
                misses.append((label, k, name, g, w, err, tol[name]))
    assert not misses, misses                                # every figure is printed first; the misses are listed together
    return cases


@pytest.mark.parametrize("n_sel", (1, 3))
@pytest.mark.parametrize("n,C", R.GPU_SHAPES)
def test_shapes_against_the_restatement(engines, n, C, n_sel):
    """(1, 20): no fit; (1, 21), (5, 5): M = 5; (3, 75): S = 225; (7, 193): C no multiple of 64, M = 111 no power of two; (2, 4 097):
    crosses a block of 256 and a level of the block tree; (16, 1 024): M = 384, G = 49; (1, 65 536): M = 768.

    The fit runs in double-double on the device (Arithmetic): a plain double evaluation with the device's own exp / log1p
    was measured up to 8.5 x outside the 4 x |float64 - longdouble| rule on theta_hat, khat, sigma, the tail's sum and the elpd (a
    last-place difference of exp, multiplied by exp(lw_j) - exp(lw_cut) near the cutoff and carried on by the profile)."""
    table = R.table(n, C, n_sel, seed=100 * n + C)
    cases = check(run(engines, table), table, f"({n}, {C}) x {n_sel}")
    assert all(c["status"] == (R.TOO_FEW if n * C <= 20 else R.FITTED) for c in cases)


def test_ties(engines):
    rng = np.random.default_rng(11)
    n, C = 2, 250
    S, M = n * C, R.tail_len(n * C)
    base = np.sort(rng.normal(-1.0, 1.0, size=S))
    all_equal = np.full(S, -1.25)
    low_equal = base.copy(); low_equal[:M + 3] = base[0]
    two = base.copy(); two[M] = two[M - 1]                          # the M-th and (M + 1)-th smallest: one copy inside the tail, one outside
    zeros = np.abs(base) + 0.5; zeros[:M - 2] = -zeros[:M - 2]; zeros[M - 2:M + 1] = (-0.0, 0.0, 0.0)       # -0.0, +0.0 | +0.0 on the cutoff
    cols = [rng.permutation(v) for v in (all_equal, low_equal, two, zeros)]
    table = np.ascontiguousarray(np.stack([c.reshape(n, C) for c in cols], axis=1))
    res = run(engines, table)
    cases = check(res, table, "ties")
    assert [c["status"] for c in cases] == [R.DEGENERATE, R.DEGENERATE, R.FITTED, R.FITTED]
    assert cases[2]["n_below"] == M - 1 and cases[2]["n_equal"] == 2
    t3 = res["tail"][3]
    assert np.signbit(t3[M - 2]) and t3[M - 2] == 0.0 and not np.signbit(t3[M - 1]) and t3[M - 1] == 0.0 and cases[3]["n_equal"] == 2


def test_the_figures_depend_on_the_multiset_only(engines):
    """the chains reversed, and draws and chains of a square table transposed: the same tail bits; every figure within its tolerance of
    the restatement of its own layout (the body's sum runs in the table's order, so the layouts are not held bit-equal)"""
    table = R.table(40, 40, 2, seed=9)
    res = run(engines, table)
    check(res, table, "square")
    for label, other in (("chains reversed", table[:, :, ::-1]), ("transposed", table.transpose(2, 1, 0))):
        other = np.ascontiguousarray(other)
        r2 = run(engines, other)
        check(r2, other, label)
        assert np.array_equal(_bits(r2["tail"]), _bits(res["tail"])) and np.array_equal(r2["counts"], res["counts"]), label
        for name in ("x_min", "x_cut", "exp_cutoff", "t_star", "theta_hat", "khat", "sigma", "tail_sum", "tail_num"):      # functions of the sorted tail alone
            assert np.array_equal(_bits(r2[name]), _bits(res[name])), (label, name)


def test_a_statement_alone_equals_itself_among_three_and_a_call_equals_its_repetition(engines):
    table = R.table(7, 193, 3, seed=21)
    whole, again = run(engines, table), run(engines, table)
    for key in ("words", "counts", "tail"):
        assert np.array_equal(np.ascontiguousarray(whole[key]).view(np.uint64), np.ascontiguousarray(again[key]).view(np.uint64)), key
    for k in range(3):
        one = run(engines, table[:, k:k + 1, :])
        for key in ("words", "counts", "tail"):
            a, b = np.ascontiguousarray(one[key][0]).view(np.uint64), np.ascontiguousarray(whole[key][k]).view(np.uint64)
            print(f"statement {k} alone, {key}: equal {np.array_equal(a, b)}")
            assert np.array_equal(a, b), (k, key)


def test_non_finite_cells_and_their_neighbours(engines):
    table = R.table(5, 130, 6, seed=33)
    table[2, 1, 17] = np.nan
    table[0, 3, 5] = -np.inf
    table[4, 5, 129] = np.inf
    res = run(engines, table)
    cases = check(res, table, "non-finite")
    assert [c["status"] for c in cases] == [R.FITTED, R.NONFINITE, R.FITTED, R.NONFINITE, R.FITTED, R.FITTED]
    assert all(math.isnan(float(res[name][1])) for name in R.WORD_NAMES if name != "khat_threshold") and res["n_nan"][1] == 1
    assert res["elpd_loo_psis"][3] == -np.inf and res["khat"][3] == np.inf and res["n_neg_inf"][3] == 1
    assert res["n_pos_inf"][5] == 1 and res["lppd"][5] == np.inf and math.isfinite(res["elpd_loo_psis"][5]) and math.isfinite(res["khat"][5])
    clean = run(engines, np.ascontiguousarray(table[:, [0, 2, 4], :]))
    for key in ("words", "counts", "tail"):
        a, b = np.ascontiguousarray(res[key][[0, 2, 4]]).view(np.uint64), np.ascontiguousarray(clean[key]).view(np.uint64)
        assert np.array_equal(a, b), key


def test_a_call_between_steps_changes_nothing_of_a_session(monkeypatch):
    monkeypatch.setenv("FG_JIT", "0")
    cp = E.compile_model(ZOO["hier"]())
    C, seen = 70, []
    for call in (False, True):
        eng = E.Engine(cp, C, seed=13)
        buf = eng.device_alloc(10 * cp.d * C * 8)
        eng.hmc_init(E.hmc_config(), 3)
        eng.hmc_step(3)
        eng.hmc_step(5, buf)
        if call:
            _, ll = eng.predict_eval(buf, 5, out=False)
            res = eng.psis_loo(ll, 5, cp.O)
            assert np.isfinite(res["elpd_loo_psis"]).all() and not res["n_nan"].any() and (res["tail_len"] == R.tail_len(5 * C)).all()
            eng.device_free(ll)
        eng.hmc_step(5, buf + 5 * cp.d * C * 8)
        seen.append(dict(draws=eng.download(buf, (10, cp.d, C), dtype=np.int64), values=eng.get_values(), lj=eng.hmc_log_joint(), eps=eng.hmc_step_sizes(),
                         state=np.frombuffer(eng.state_export(), dtype=np.uint8), accept=np.float64(eng.hmc_stats().accept_rate)))
        eng.device_free(buf)
        eng.close()
    for k in seen[0]:
        a, b = (np.atleast_1d(np.ascontiguousarray(seen[j][k])) for j in (1, 0))
        print(f"{k}: equal {a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))}")
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), k


def test_end_to_end_on_the_readme_model():
    """64 chains x 200 draws: `psis_loo` of the stored run equals `model_comparison(..., psis=True).psis` bit for bit and the restatement
    within tolerance; without `psis` the comparison is what the same call returns again, field by field, and carries none."""
    batch = I.hmc_chain(5, E.compile_model(W.readme_normal()), 200, 100, n_chains=64, pointwise=True)
    ps = CMP.psis_loo(batch)
    both = CMP.model_comparison(batch, psis=True)
    plain, plain2 = CMP.model_comparison(batch), CMP.model_comparison(batch)
    table = np.ascontiguousarray(batch.log_likelihood, dtype=np.float64)
    want = R.psis_statement(R.pooled(table, 0))
    tol = R.tolerances(want, R.psis_statement(R.pooled(table, 0), ld=True))
    print("elpd_loo_psis", ps.elpd_loo_psis, float(want["elpd_loo_psis"]), "khat", ps.khat, float(want["khat"]), "raw elpd_loo", plain.elpd_loo)
    assert ps.names == both.psis.names == list(batch.predictive_names) and ps.n_draws == 64 * 200 and ps.tail_len[0] == R.tail_len(12800)
    for name in CMP.PSIS_POINTWISE:
        assert np.array_equal(_bits(getattr(ps, name)), _bits(getattr(both.psis, name))), name
        assert abs(float(getattr(ps, name)[0]) - float(want[name])) <= tol[name], name
    for name in ("tail_len", "status", "n_capped", "n_neg_inf", "n_pos_inf", "n_nan"):
        assert np.array_equal(getattr(ps, name), getattr(both.psis, name)) and int(getattr(ps, name)[0]) == int(want[name]), name
    assert ps.status_words() == ["fitted"] and ps.n_bad_k() == int(not float(want["khat"]) <= float(want["khat_threshold"]))
    assert plain.psis is None and plain2.psis is None
    for name in CMP.POINTWISE + ("n_neg_inf", "n_pos_inf", "n_nan"):
        a, b, c = (np.ascontiguousarray(getattr(p, name)) for p in (plain, plain2, both))
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.array_equal(a.view(np.uint64), c.view(np.uint64)), name
    assert plain.names == plain2.names and plain.n_draws == plain2.n_draws
    d, se = CMP.compare_models(both, both, which="elpd_loo_psis")
    assert d == 0.0
