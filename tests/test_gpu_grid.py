"""Log-joint surfaces on the device (fugue_amd/csrc/fg_grid.hip) against `Engine.log_joint` (bit for bit), the oracle, the restatement
of the reductions (tests/grid_restatement.py, within its derived bounds) and the law.  Shapes: the smallest that can go wrong -- one
cell, a wave less one, whole waves, a wave and one, a tail wave behind two -- on an engine of five chains, one base and three bases
that do not start at chain 0."""
import ctypes as C
import math

import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import grid as G
from fugue_amd import model as M
from tests import grid_restatement as R
from tests.models import ZOO

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1), (63, 1), (64, 2), (65, 3), (130, 2))
BASES = ((0, 1), (2, 3))                                 # (chain0, n_bases) of an engine of C = 5
C_ENGINE = 5
MODELS = ("readme", "refmodel8", "mixture", "alldists", "hier_scale", "logistic")
REF_CHAINS = 130 * 2 * 3                                 # the largest (shape, bases): the engine Engine.log_joint scores the same cells on


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


def _axes(values, ja, jb, n_a, n_b, c):
    """axes around base c's own values (in support where the site has one; a cell out of it is -inf on both sides)"""
    va = float(values[ja:ja + 1, c].view(np.float64)[0])
    a = np.linspace(0.6 * va, 1.4 * va, n_a) if n_a > 1 else np.array([0.9 * va])
    if jb is None:
        return a, None
    vb = float(values[jb:jb + 1, c].view(np.float64)[0])
    return a, (np.linspace(0.7 * vb - 0.1, 1.3 * vb + 0.1, n_b) if n_b > 1 else np.array([1.1 * vb]))


def _cells_of(values, chain0, n_bases, ja, a, jb, b):
    """[S][n_bases * n_b * n_a]: the trace of every cell, host-built as a caller of the parent API builds it"""
    n_a, n_b = a.size, 1 if b is None else b.size
    out = np.repeat(values[:, chain0:chain0 + n_bases], n_a * n_b, axis=1)
    out[ja] = np.tile(np.tile(_bits(a), n_b), n_bases)
    if jb is not None:
        out[jb] = np.tile(np.repeat(_bits(b), n_a), n_bases)          # after a: the same site twice -> b wins (grid.rs:52-57)
    return out


def _log_joint_of(ref, cells):
    """Engine.log_joint on `ref` (REF_CHAINS chains) holding `cells` in its first columns -> acc [3][n]"""
    n = cells.shape[1]
    full = np.repeat(cells[:, :1], REF_CHAINS, axis=1)
    full[:, :n] = cells
    ref.set_values(full)
    return ref.log_joint()[:, :n]


def _check_reductions(lj, s, la, lb, base, extra=""):
    """summary / marginals of one base against the restatement applied to the device's own surface: the non-finite figures, the mode
    and the counts exactly; the finite marginals and log_norm within `tolerances()`; columns against the oracle's log_sum_exp"""
    from oracle import oracle as orc
    n_b, n_a = lj.shape
    want = R.summary(lj, "plan")
    tol = R.tolerances(n_a, n_b, want)
    assert int(s["argmax"][base]) == want["argmax"] == R.fold_argmax(lj)[0], extra
    assert (s["max"][base] == want["max"]) and s["counts"][base].tolist() == want["counts"].tolist(), extra
    assert R.close(lb[base], want["log_marg_b"], tol["marg_b"]), extra
    assert R.close(la[base], want["log_marg_a"], tol["marg_a"]), extra
    assert R.close(la[base], [orc.log_sum_exp(lj[:, i]) for i in range(n_a)], tol["marg_a"]), extra
    assert R.close(s["log_norm"][base], want["log_norm"], tol["log_norm"]), extra
    seq = R.summary(lj, "seq")
    assert R.close(lb[base], seq["log_marg_b"], tol["marg_b_seq"]), extra


# ---- bit identity with Engine.log_joint, the oracle at test_log_joint_matches_oracle's tolerances, read-only ---------------------------
@pytest.mark.parametrize("name", MODELS)
def test_cells_are_log_joints_bit_for_bit(oracle, name):
    prog = ZOO[name]()
    cp, om = E.compile_model(prog), oracle.OracleModel(prog)
    ja = cp.f64_sites[0]
    jb = cp.f64_sites[1] if cp.d > 1 else None            # readme has one f64 site: the one-axis grids
    eng, ref = E.Engine(cp, C_ENGINE, seed=21), E.Engine(cp, REF_CHAINS, seed=1)
    try:
        eng.prior_init()
        values = eng.get_values().copy()
        for n_a, n_b in SHAPES:
            if jb is None:
                n_b = 1
            for chain0, n_bases in BASES:
                a, b = _axes(values, ja, jb, n_a, n_b, chain0)
                g = eng.grid(ja, a, jb, b)
                lj, acc = g.eval(chain0, n_bases, want_acc=True)
                assert lj.shape == (n_bases, n_b, n_a) and g.count == n_bases
                want = _log_joint_of(ref, _cells_of(values, chain0, n_bases, ja, a, jb, b)).reshape(3, n_bases, n_b, n_a)
                assert np.array_equal(acc, want, equal_nan=True), (name, n_a, n_b, chain0)
                assert np.array_equal(lj, (want[0] + want[1]) + want[2], equal_nan=True), (name, n_a, n_b, chain0)
                assert np.array_equal(eng.get_values(), values)                         # the engine is read only
                s, (la, lb) = g.summary(), g.marginals()
                for k in range(n_bases):
                    _check_reductions(lj[k], s, la, lb, k, (name, n_a, n_b, chain0, k))
                if (n_a, n_b) in ((65, 3), (65, 1)):                                    # against the oracle, every cell of every base
                    for k in range(n_bases):
                        olj, oacc = R.surface(om, values[:, chain0 + k], ja, a, jb, b, want_acc=True)
                        for got, exp in ((acc[:, k], oacc), (lj[k], olj)):
                            both = (np.isinf(got) & np.isinf(exp) & (np.sign(got) == np.sign(exp))) | (np.isnan(got) & np.isnan(exp))
                            with np.errstate(invalid="ignore"):
                                assert np.all(both | (np.abs(got - exp) <= 1e-12 + 1e-12 * np.abs(exp))), (name, chain0, k)
                g.close()
    finally:
        eng.close()
        ref.close()


def _reference_engine(C_=C_ENGINE, seed=5):
    cp = E.compile_model(R.reference_program())
    eng = E.Engine(cp, C_, seed=seed)
    eng.prior_init()
    return cp, eng


def test_the_same_site_twice_b_wins_and_one_axis():
    cp, eng = _reference_engine()
    ref = E.Engine(cp, REF_CHAINS, seed=1)
    try:
        values = eng.get_values().copy()
        a, b = np.linspace(-1.0, 2.0, 65), np.array([0.25, 0.5, 4.0])
        g = eng.grid("a", a, "a", b)                          # grid.rs:52-57 with addr_a == addr_b
        lj = g.eval(2, 3)
        cells = _cells_of(values, 2, 3, 0, a, 0, b)
        assert np.array_equal(cells[0].reshape(3, 3, 65)[:, :, 0], np.tile(_bits(b), (3, 1)))
        acc = _log_joint_of(ref, cells)
        assert np.array_equal(lj, ((acc[0] + acc[1]) + acc[2]).reshape(3, 3, 65))
        assert np.all(lj == lj[:, :, :1]) and not np.all(lj[:, 0] == lj[:, 1])      # a's axis is overwritten: constant along i
        g.close()
        g = eng.grid("b", a)                                  # one axis: only the one site is overwritten
        lj = g.eval(0, C_ENGINE)
        assert lj.shape == (5, 1, 65) and (g.n_b, g.b_values) == (1, None)
        acc = _log_joint_of(ref, _cells_of(values, 0, 5, 1, a, None, None))
        assert np.array_equal(lj, ((acc[0] + acc[1]) + acc[2]).reshape(5, 1, 65))
        assert not np.array_equal(lj[0], lj[1])               # the other site stays at each base's own value
        s, (la, lb) = g.summary(), g.marginals()
        for k in range(5):
            _check_reductions(lj[k], s, la, lb, k)
        assert np.array_equal(eng.get_values(), values)
        g.close()
    finally:
        eng.close()
        ref.close()


@pytest.mark.parametrize("n_a", [257, 1025])
def test_reductions_at_every_workgroup_size_of_the_row_plan(n_a):
    """128 and 256 threads a row (the shapes above all take 64), several cells a thread; cells hundreds of units apart"""
    cp, eng = _reference_engine(C_=2)
    try:
        a = np.linspace(-40.0, 40.0, n_a)
        g = eng.grid("a", a, "b", np.array([-3.0, 1.0, 55.0]))
        lj = g.eval(0, 2)
        assert R.plan(n_a)["row_threads"] == {257: 128, 1025: 256}[n_a]
        s, (la, lb) = g.summary(), g.marginals()
        for k in range(2):
            _check_reductions(lj[k], s, la, lb, k)
        assert np.array_equal(lj[0], lj[1])
        g.close()
    finally:
        eng.close()


# ---- non-finite and out-of-support cells ---------------------------------------------------------------------------------------------
def _scale_program():
    P = M.Program()
    a = P.sample(M.addr("a"), M.Normal(0.0, 1.0))
    s = P.sample(M.addr("s"), M.Gamma(2.0, 1.5))
    P.sample(M.addr("x"), M.Normal(a, s))
    P.observe(M.addr("y"), M.Normal(a, 0.5), 0.3)
    return P


def test_non_finite_and_out_of_support_axis_values_score_minus_infinity():
    cp = E.compile_model(_scale_program())
    eng = E.Engine(cp, C_ENGINE, seed=3)
    try:
        eng.prior_init()
        a = np.array([-0.5, np.inf, 0.25, np.nan, -np.inf, 1.0] + [0.1 * k for k in range(59)])       # 65
        b = np.array([0.7, -1.0, 0.0])                                                                # a negative and a zero scale
        g = eng.grid("a", a, "s", b)
        lj = g.eval(2, 3)
        bad = ~np.isfinite(a)[None, :] | (b <= 0.0)[:, None]
        for k in range(3):
            assert np.all(np.isneginf(lj[k][bad])) and np.all(np.isfinite(lj[k][~bad]))
        s, (la, lb) = g.summary(), g.marginals()
        assert s["counts"].tolist() == [[0, int(bad.sum()), 0]] * 3
        for k in range(3):
            _check_reductions(lj[k], s, la, lb, k)
            assert np.all(np.isneginf(lb[k][1:])) and np.all(np.isneginf(la[k][~np.isfinite(a)])) and math.isfinite(s["log_norm"][k])
        lm, n_mixed, n_skipped = g.mixture()
        assert (n_mixed, n_skipped) == (3, 0) and np.all(np.isneginf(lm[bad])) and np.all(np.isfinite(lm[~bad]))
        g.close()
        g = eng.grid("s", np.array([-2.0, 0.0, -np.inf, np.nan]))                                    # no cell exceeds -inf
        lj = g.eval(0, 2)
        s, (la, lb) = g.summary(), g.marginals()
        assert np.all(np.isneginf(lj)) and s["argmax"].tolist() == [-1, -1] and np.all(np.isneginf(s["max"])) and np.all(np.isneginf(s["log_norm"]))
        assert s["counts"].tolist() == [[0, 4, 0]] * 2 and np.all(np.isneginf(la)) and np.all(np.isneginf(lb))
        lm, n_mixed, n_skipped = g.mixture()
        assert (n_mixed, n_skipped) == (0, 2) and np.all(np.isnan(lm))
        g.close()
    finally:
        eng.close()


def test_a_plus_infinity_cell_and_the_summary_rules():
    """Beta(0.5, 0.5) at 0 is +inf (distribution.rs:897-956): the cell is +inf, the mode is its first occurrence, its row's and its
    column's marginals and the normaliser are NaN (inf - inf in numerical.rs:31), and the base is skipped by the mixture"""
    P = M.Program()
    p = P.sample(M.addr("p"), M.Beta(0.5, 0.5))
    q = P.sample(M.addr("q"), M.Normal(0.0, 1.0))
    P.observe(M.addr("y"), M.Normal(q, 1.0), 0.4)
    cp = E.compile_model(P)
    eng = E.Engine(cp, C_ENGINE, seed=4)
    try:
        eng.prior_init()
        a = np.concatenate([[0.3, 0.0, 0.6, 1.0, 1.5], np.linspace(0.05, 0.95, 60)])                  # 65: 0 and 1 are +inf, 1.5 is out of support
        b = np.array([-1.0, 0.5, 2.0])
        g = eng.grid("p", a, "q", b)
        lj = g.eval(0, 1)
        assert np.all(np.isposinf(lj[0][:, [1, 3]])) and np.all(np.isneginf(lj[0][:, 4]))
        s, (la, lb) = g.summary(), g.marginals()
        assert s["counts"][0].tolist() == [0, 3, 6] and int(s["argmax"][0]) == 1 and np.isposinf(s["max"][0])
        assert np.all(np.isnan(lb[0])) and np.isnan(la[0][1]) and np.isnan(la[0][3]) and np.isneginf(la[0][4]) and np.isfinite(la[0][0])
        assert s["log_norm"][0] == -np.inf                    # every row marginal is NaN and the max fold never takes NaN
        _check_reductions(lj[0], s, la, lb, 0)
        lm, n_mixed, n_skipped = g.mixture()
        assert (n_mixed, n_skipped) == (0, 1)
        g.close()
        g2 = eng.grid("p", a[4:], "q", b)                     # without the two end points: finite but for the out-of-support column
        lj2 = g2.eval(0, 2)
        s2 = g2.summary()
        assert np.all(np.isfinite(s2["log_norm"])) and s2["counts"].tolist() == [[0, 3, 0]] * 2 and np.all(lj2[:, :, 0] == -np.inf)
        g2.close()
    finally:
        eng.close()


# ---- bit for bit: alone, in a bank, under any chunking, with or without the table, in one call or two ----------------------------------
def test_a_base_is_the_same_alone_in_a_bank_and_under_any_chunking():
    prog = ZOO["hier_scale"]()
    cp = E.compile_model(prog)
    eng = E.Engine(cp, C_ENGINE, seed=9)
    try:
        eng.prior_init()
        values = eng.get_values().copy()
        ja, jb = cp.site_names.index("mu"), cp.site_names.index("tau")
        a, b = np.linspace(-2.0, 2.0, 65), np.array([0.5, 1.0, 2.5])

        def run(calls, base_chunk, keep):
            g = eng.grid(ja, a, jb, b, base_chunk=base_chunk)
            ljs = [g.eval(c0, n, keep=keep) for c0, n in calls]
            out = (np.concatenate(ljs) if keep else None, g.summary(), g.marginals(), g.mixture())
            g.close()
            return out

        def same(x, y, surfaces=True):
            assert (not surfaces) or np.array_equal(x[0], y[0])
            assert all(np.array_equal(x[1][k], y[1][k]) for k in x[1])
            assert np.array_equal(x[2][0], y[2][0]) and np.array_equal(x[2][1], y[2][1])

        whole = run([(0, 5)], 0, True)
        assert np.all(np.isfinite(whole[1]["log_norm"])) and not np.array_equal(whole[0][0], whole[0][1])
        for base_chunk in (1, 2):
            other = run([(0, 5)], base_chunk, True)
            same(whole, other)
            assert np.array_equal(whole[3][0], other[3][0]) and whole[3][1:] == other[3][1:] == (5, 0)     # the mixture under every chunking
        no_table = run([(0, 5)], 2, False)                    # d_out NULL
        same(whole, no_table, surfaces=False)
        assert np.array_equal(whole[3][0], no_table[3][0])
        two = run([(0, 2), (2, 3)], 0, True)                  # two calls, the same arrival order
        same(whole, two)
        assert np.array_equal(whole[3][0], two[3][0])
        for c in range(C_ENGINE):                             # alone
            alone = run([(c, 1)], 0, True)
            assert np.array_equal(alone[0][0], whole[0][c])
            assert all(np.array_equal(alone[1][k][0], whole[1][k][c]) for k in alone[1])
            assert np.array_equal(alone[2][0][0], whole[2][0][c]) and np.array_equal(alone[2][1][0], whole[2][1][c])
        # the mixture is the restatement's over the device's own surfaces, within the bound of its terms
        mix, n_mixed, _, _ = R.mixture(whole[0], whole[1]["log_norm"])
        tol = R.tolerances(65, 3, R.summary(whole[0][0]))
        with np.errstate(divide="ignore"):
            want = np.log(mix / n_mixed)
        assert np.all(np.abs(whole[3][0] - want) <= 1.01 * (tol["mix_rel"] + (5 + 2) * R.EPS) + R.EPS * np.abs(want))
        assert np.array_equal(eng.get_values(), values)
    finally:
        eng.close()


# ---- the law on the device ---------------------------------------------------------------------------------------------------------------
REFERENCE_SOURCE = """
    let a <- sample(addr!("a"), Normal(0.0, 2.0));
    let b <- sample(addr!("b"), Normal(0.0, 2.0));
    observe(addr!("y"), Normal(a + b, 0.5), 2.0);
    pure(a)
"""


def test_the_references_scenario():
    """crates/fugue-wasm/tests/wasm.rs:103-131 through log_joint_grid, DSL source and all"""
    axis = R.REFERENCE_AXIS
    grids = [G.log_joint_grid(REFERENCE_SOURCE, "a", "b", axis, axis, seed) for seed in (1, 2, 3)]
    assert grids[0].shape == (21 * 21,)
    best, _ = R.fold_argmax(grids[0])
    a, b = axis[best % 21], axis[best // 21]
    assert abs(a - 1.0) < 0.5 and abs(b - 1.0) < 0.5, (a, b)
    assert np.array_equal(grids[0], grids[1]) and np.array_equal(grids[0], grids[2])
    s = G.log_joint_surface(R.reference_program(), "a", axis, "b", axis, seed=1)
    assert np.array_equal(s.log_joint[0].reshape(-1), grids[0]) and s.peak == (a, b) and int(s.argmax[0]) == best


def test_quadrature_of_the_evidence_and_the_marginal_mean_on_the_device():
    s = G.log_joint_surface(R.reference_program(), "a", R.QUAD_AXIS, "b", R.QUAD_AXIS, seed=1)
    log_ev = s.log_evidence(0.25 * 0.25)
    print(f"log evidence {log_ev:.8f} against {R.QUAD_LOG_EVIDENCE:.8f} (error {abs(log_ev - R.QUAD_LOG_EVIDENCE):.1e}); mean of a error {abs(s.mean()[0] - R.QUAD_MEAN_A):.1e}")
    assert abs(log_ev - R.QUAD_LOG_EVIDENCE) <= 1e-5
    assert abs(s.mean()[0] - R.QUAD_MEAN_A) <= 1e-6 and abs(s.mean()[1] - R.QUAD_MEAN_A) <= 1e-6
    assert abs(float(np.sum(np.exp(s.log_marginal_b[0] - s.log_norm[0]))) - 1.0) <= 65 * R.EPS
    assert (s.n_mixed, s.n_skipped) == (1, 0)
    with np.errstate(divide="ignore"):
        assert np.all(np.abs(s.log_mixture - (s.log_joint[0] - s.log_norm[0])) <= 1e-12 * (1.0 + np.abs(s.log_mixture)))    # one base: its own normalised surface


def test_mixture_law_on_the_device():
    """the same seed and caps as tests/test_grid_cpu.py::test_mixture_law_of_the_restatement; 4096 bases in one call, no table kept"""
    _, se, _ = R.mixture_law_restated()
    s = G.log_joint_surface(R.mixture_program(), "a", R.MIX_AXIS, seed=R.MIX_SEED, n_bases=R.MIX_BASES, keep=False)
    assert s.log_joint is None and (s.n_mixed, s.n_skipped) == (R.MIX_BASES, 0) and s.log_mixture.shape == (1, 129)
    mix = np.exp(s.log_mixture).reshape(-1)
    assert abs(mix.sum() - 1.0) < 1e-9
    R.judge_mixture_law(mix, se)


def test_bases_of_a_sampler_that_has_just_run():
    """engine=: the bases are the chains' current states after hmc_run; the surfaces change with them and nothing else does"""
    cp = E.compile_model(ZOO["refmodel8"]())
    eng = E.Engine(cp, 64, seed=2)
    try:
        eng.prior_init()
        eng.hmc_run(E.hmc_config(n_leapfrog=4), 8, 8)
        values = eng.get_values().copy()
        axis = np.linspace(-1.5, 1.5, 21)
        s = G.log_joint_surface(None, "mu", axis, "x#0", axis, engine=eng, n_bases=64, keep=False)
        assert s.n_mixed == 64 and s.log_norm.shape == (64,) and np.all(np.isfinite(s.log_mixture)) and len(set(s.log_norm.tolist())) > 1
        assert abs(float(np.sum(np.exp(s.log_mixture))) - 1.0) < 1e-9 and np.array_equal(eng.get_values(), values)
    finally:
        eng.close()


# ---- error codes -----------------------------------------------------------------------------------------------------------------------------
def test_error_codes(monkeypatch):
    L = E.lib()
    P = M.Program()
    a = P.sample(M.addr("a"), M.Normal(0.0, 1.0))
    P.sample(M.addr("k"), M.Bernoulli(0.3))
    P.observe(M.addr("y"), M.Normal(a, 1.0), 0.5)
    cp = E.compile_model(P)
    eng = E.Engine(cp, C_ENGINE, seed=1)
    h = C.c_void_p()
    two = (C.c_double * 2)(0.5, 1.0)
    try:
        eng.prior_init()
        ja, jk = cp.site_names.index("a"), cp.site_names.index("k")
        assert L.fg_grid_new(eng.h, ja, jk, two, 2, two, 2, 0, C.byref(h)) == E.FG_E_BAD_ARG                 # a site that is not f64
        assert E.last_error() == "sites `a`/`k` must be f64 sample sites of the model" and h.value is None
        assert L.fg_grid_new(eng.h, jk, -1, two, 2, None, 0, 0, C.byref(h)) == E.FG_E_BAD_ARG
        assert L.fg_grid_new(eng.h, ja, 7, two, 2, two, 2, 0, C.byref(h)) == E.FG_E_BAD_ARG and L.fg_grid_new(eng.h, -2, -1, two, 2, None, 0, 0, C.byref(h)) == E.FG_E_BAD_ARG
        assert L.fg_grid_new(eng.h, ja, -1, two, 0, None, 0, 0, C.byref(h)) == E.FG_E_BAD_ARG and "n_a" in E.last_error()     # n_a = 0
        assert L.fg_grid_new(eng.h, ja, ja, two, 2, two, 0, 0, C.byref(h)) == E.FG_E_BAD_ARG                 # n_b = 0 on two axes
        assert L.fg_grid_new(eng.h, ja, -1, two, 2, None, 0, -1, C.byref(h)) == E.FG_E_BAD_ARG and L.fg_grid_new(eng.h, ja, -1, None, 2, None, 0, 0, C.byref(h)) == E.FG_E_BAD_ARG
        assert L.fg_grid_new(eng.h, ja, -1, two, 1 << 31, None, 0, 0, C.byref(h)) == E.FG_E_LIMIT and h.value is None
        with pytest.raises(ValueError):
            eng.grid("a", [0.0, 1.0], "k", [0.0, 1.0])
        g = eng.grid("a", [0.0, 1.0])
        for call in (g.summary, g.marginals, g.mixture):                                                   # a read-out before any base has arrived
            with pytest.raises(E.EngineError) as ei:
                call()
            assert ei.value.code == E.FG_E_STATE
        assert g.count == 0
        for chain0, n in ((3, 3), (5, 1), (0, 6), (0, 0), (-1, 2), (0, -1)):                               # chain0 + n_bases > C, and none
            with pytest.raises(E.EngineError) as ei:
                g.eval(chain0, n)
            assert ei.value.code == E.FG_E_BAD_ARG and g.count == 0
        assert g.eval(4, 1).shape == (1, 1, 2) and g.count == 1
        g.close()
        with pytest.raises(ValueError):
            g.summary()
    finally:
        eng.close()
    monkeypatch.setenv("FG_GLOBAL_TILE", "1")                 # any program through the global-tile instantiations (fg_engine_new)
    gt = E.Engine(cp, C_ENGINE, seed=1)
    try:
        gt.prior_init()
        with pytest.raises(E.EngineError) as ei:
            gt.grid("a", [0.0, 1.0])
        assert ei.value.code == E.FG_E_LIMIT
    finally:
        gt.close()
