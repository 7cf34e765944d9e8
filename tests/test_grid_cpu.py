"""The log-joint surfaces without a GPU: the launch plan (fugue_amd/csrc/fg_grid_plan.h) through a stand-alone driver under
-fsanitize=address,undefined, the restatement (tests/grid_restatement.py) on the reference's own scenario, against exact quadrature
targets and on the mixture law, log_sum_exp's rules, the derived bounds, and the Python layer's refusals before any engine exists."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import grid as G
from fugue_amd import model as M
from oracle import oracle as orc
from tests import grid_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g")
PLAN_SHAPES = [(n_a, n_b) for n_a in (1, 63, 64, 65, 4097) for n_b in (1, 2, 1025)]


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    orc.build()


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
def test_plan_driver_under_address_and_ub_sanitizers(tmp_path):
    """every shape with the plan's own chunk and a caller's, bases below, at and one past a chunk boundary, and every refusal (cells
    at 2^31 and beyond, sizes below 1, a negative chunk, bases outside the engine's chains): inside the driver"""
    assert shutil.which("g++"), "g++ builds the driver"
    exe = os.path.join(str(tmp_path), "grid_plan_driver_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", *SAN, os.path.join(ROOT, "tests", "cpp", "grid_plan_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=24")
    r = subprocess.run([exe, *[str(v) for s in PLAN_SHAPES for v in s]], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    assert len(lines) == len(PLAN_SHAPES) + 1 and lines[-1] == "refusals ok"
    threads_seen = set()
    for (n_a, n_b), ln in zip(PLAN_SHAPES, lines):
        head, nums, verdict = [s.strip() for s in ln.split("|")]
        assert head == f"plan {n_a} {n_b}" and verdict == "ok", ln
        rc, cells, waves, bc, threads, per, colb, mixb = [int(v) for v in nums.split()]
        p = R.plan(n_a, n_b)
        assert rc == 0 and (cells, waves, bc, threads, per, colb, mixb) == (p["cells"], p["waves"], p["base_chunk"], p["row_threads"], p["row_per_thread"], p["col_blocks"], p["mix_blocks"]), ln
        assert bc == 1 or bc * cells * 8 <= R.CHUNK_BYTES
        threads_seen.add(threads)
    assert threads_seen == {64, 256} and R.plan(300)["row_threads"] == 128 and R.plan(4097, 1025)["base_chunk"] == 7


def test_plan_row_sum_is_a_sum_within_its_depth():
    rng = np.random.default_rng(3)
    for n in (1, 2, 63, 64, 65, 130, 255, 256, 257, 1023, 1025, 4097):
        v = rng.random((3, n))
        exact = np.array([math.fsum(r) for r in v])
        assert np.all(np.abs(R.plan_row_sum(v) - exact) <= R.plan_depth(n) * 0.5 * R.EPS * exact * 1.001)
        assert np.all(np.abs(R.seq_sum(v) - exact) <= max(n - 1, 1) * 0.5 * R.EPS * exact * 1.001)
        assert R.plan_row_sum(v[0]) == R.plan_row_sum(v)[0]
    assert R.plan_depth(4097) == 17 + 6 + 4 and R.plan_depth(64) == 1 + 6 + 1


# ---- numerical.rs:15-38, rule for rule ---------------------------------------------------------------------------------------------------
LSE_ROWS = {
    "only -inf": [-np.inf] * 5,
    "-inf beside NaN": [-np.inf, np.nan, -np.inf],
    "+inf": [0.5, np.inf, -1.0],
    "two +inf": [np.inf, np.inf],
    "NaN": [0.5, np.nan, -1.0],
    "NaN alone": [np.nan],
    "finite": [-1.0, -2.0, -3.0],
    "far apart": [-1000.0, 0.0, -800.0],
    "one": [3.25],
    "-inf among finite": [-np.inf, 2.0, -np.inf, 1.0],
}


@pytest.mark.parametrize("name", list(LSE_ROWS))
def test_log_sum_exp_rules_against_the_oracle(name):
    row = np.array(LSE_ROWS[name])
    want = orc.log_sum_exp(row)
    for order in ("seq", "plan"):
        got = R.log_sum_exp(row, order)
        tol = R.lse_tolerance(R.plan_depth(row.size), row.size - 1, row.size, want)
        assert R.close(got, want, tol), (name, order, got, want)
    if name in ("only -inf", "-inf beside NaN"):
        assert want == -np.inf                                # -inf before any sum, even beside NaN
    if name in ("+inf", "two +inf", "NaN"):
        assert math.isnan(want)                               # inf - inf, and NaN itself, pass through exp, the sum and ln
    if name == "NaN alone":
        assert want == -np.inf                                # the max fold never takes NaN: the row counts as all -inf
    wide = np.tile(row, 70)                                   # more than one wave of the plan's order
    assert R.close(R.log_sum_exp(wide, "plan"), orc.log_sum_exp(wide), R.lse_tolerance(R.plan_depth(wide.size), wide.size - 1, wide.size, orc.log_sum_exp(wide)))


def test_fold_argmax_is_the_references_fold():
    assert R.fold_argmax([1.0, 3.0, 3.0, np.nan, 2.0]) == (1, 3.0)        # the first maximum; NaN never wins
    assert R.fold_argmax([-np.inf, np.nan, -np.inf]) == (-1, -np.inf)     # no cell exceeds -inf
    assert R.fold_argmax([np.nan, -5.0, np.inf, np.inf]) == (2, np.inf)
    s = R.summary(np.array([[0.0, np.nan, -np.inf], [np.inf, 1.0, -np.inf]]))
    assert s["argmax"] == 3 and s["counts"].tolist() == [1, 2, 1] and np.isnan(s["log_marg_b"]).all()
    assert s["log_norm"] == -np.inf                           # every row marginal is NaN and the max fold never takes NaN: numerical.rs:21-28
    s = R.summary(np.array([[0.0, np.nan, -np.inf], [-1.0, 1.0, -np.inf]]))
    assert math.isnan(s["log_norm"]) and s["argmax"] == 4     # one finite row marginal: the NaN of the other passes through the sum


# ---- the reference's own scenario (crates/fugue-wasm/tests/wasm.rs:103-131) ---------------------------------------------------------------
def _reference_surface(seed, axis):
    om = orc.OracleModel(R.reference_program())
    assert om.site_names == ["a", "b"]
    return R.surface(om, R.prior_bases(om, seed, 1)[:, 0], 0, axis, 1, axis)


def test_the_references_scenario_on_the_restatement():
    axis = R.REFERENCE_AXIS
    ljs = [_reference_surface(seed, axis) for seed in (1, 2, 3)]
    assert ljs[0].shape == (21, 21)
    best, _ = R.fold_argmax(ljs[0])
    a, b = axis[best % 21], axis[best // 21]
    assert abs(a - 1.0) < 0.5 and abs(b - 1.0) < 0.5, (a, b)
    assert np.array_equal(ljs[0], ljs[1]) and np.array_equal(ljs[0], ljs[2])     # both latent sites are pinned: the base does not matter


def test_quadrature_of_the_evidence_and_of_the_marginal_mean():
    s = R.summary(_reference_surface(1, R.QUAD_AXIS))
    h = R.QUAD_AXIS[1] - R.QUAD_AXIS[0]
    log_ev = s["log_norm"] + 2.0 * math.log(h)
    w = np.exp(s["log_marg_a"] - s["log_norm"])
    mean_a = float(np.sum(w * R.QUAD_AXIS) / np.sum(w))
    print(f"log evidence {log_ev:.8f} against {R.QUAD_LOG_EVIDENCE:.8f} (error {abs(log_ev - R.QUAD_LOG_EVIDENCE):.1e}); mean of a error {abs(mean_a - R.QUAD_MEAN_A):.1e}")
    assert h == 0.25 and abs(log_ev - R.QUAD_LOG_EVIDENCE) <= 1e-5
    assert abs(mean_a - R.QUAD_MEAN_A) <= 1e-6
    assert abs(float(np.sum(np.exp(s["log_marg_b"] - s["log_norm"]))) - 1.0) <= 65 * R.EPS      # the row masses sum to 1 up to rounding


def test_the_two_orders_agree_within_the_derived_bounds():
    """`tolerances` is consistent with the restatement itself: rows in the plan's order against rows in index order, columns against
    the oracle's log_sum_exp, on a surface with cells far apart and -inf cells"""
    lj = _reference_surface(1, np.linspace(-30.0, 30.0, 130))[:3]
    lj[1, 5] = -np.inf
    lj[2, :] = -np.inf
    a, b = R.summary(lj, "plan"), R.summary(lj, "seq")
    tol = R.tolerances(130, 3, a)
    assert R.close(a["log_marg_b"], b["log_marg_b"], tol["marg_b_seq"]) and b["log_marg_b"][2] == -np.inf
    assert R.close(a["log_norm"], b["log_norm"], tol["log_norm"])
    assert R.close(a["log_marg_a"], [orc.log_sum_exp(lj[:, i]) for i in range(130)], tol["marg_a"])
    assert np.all(tol["marg_b_seq"] < 1e-12) and tol["log_norm"] < 1e-12 and tol["mix_rel"] < 1e-12


# ---- the mixture law -----------------------------------------------------------------------------------------------------------------------
def test_the_vectorised_mixture_surfaces_are_the_oracles_bit_for_bit():
    om = orc.OracleModel(R.mixture_program())
    assert om.site_names == ["a", "z"]
    bases = R.prior_bases(om, R.MIX_SEED, 6)
    bases[1, 4] = np.array([np.inf]).view(np.int64)[0]
    bases[1, 5] = np.array([np.nan]).view(np.int64)[0]
    fast = R.mixture_surfaces(bases[1].view(np.float64))
    for c in range(6):
        assert np.array_equal(fast[c], R.surface(om, bases[:, c], 0, R.MIX_AXIS), equal_nan=True), c


def test_mixture_law_of_the_restatement():
    """the mean over 4096 prior bases of the normalised conditional surfaces of `a` is the N(0, 1) cell mass"""
    mix, se, n_mixed = R.mixture_law_restated()
    assert n_mixed == R.MIX_BASES and abs(mix.sum() - 1.0) < 1e-9
    R.judge_mixture_law(mix, se)


# ---- the Python layer before any engine exists ---------------------------------------------------------------------------------------------
def _mixed_program():
    P = M.Program()
    a = P.sample(M.addr("a"), M.Normal(0.0, 1.0))
    P.sample(M.addr("k"), M.Bernoulli(0.3))
    P.observe(M.addr("y"), M.Normal(a, 1.0), 0.5)
    return P


def test_value_errors_for_unknown_and_non_f64_sites():
    axis = [0.0, 1.0]
    for sa, sb in (("a", "nope"), ("nope", "a"), ("a", "k"), ("k", "a"), ("y", "a")):
        with pytest.raises(ValueError) as ei:
            G.log_joint_grid(_mixed_program(), sa, sb, axis, axis, 1)
        assert str(ei.value) == f"sites `{sa}`/`{sb}` must be f64 sample sites of the model"      # grid.rs:43-45
        with pytest.raises(ValueError):
            G.log_joint_surface(_mixed_program(), sa, axis, sb, axis)
    src = 'let a <- sample(addr!("a"), Normal(0.0, 2.0));\nobserve(addr!("y"), Normal(a, 0.5), 2.0);\npure(a)'
    with pytest.raises(ValueError) as ei:
        G.log_joint_grid(src, "a", "b", axis, axis, 1)
    assert str(ei.value) == "sites `a`/`b` must be f64 sample sites of the model"
    with pytest.raises(ValueError):
        G.log_joint_surface(_mixed_program(), "k", axis)


def test_argument_codes_without_an_engine():
    L = E.lib()
    import ctypes as C
    h = C.c_void_p()
    one = (C.c_double * 1)(0.5)
    assert L.fg_grid_new(None, 0, 1, one, 1, one, 1, 0, C.byref(h)) == E.FG_E_BAD_ARG and h.value is None
    assert L.fg_grid_new(None, 0, 1, one, 1, one, 1, 0, None) == E.FG_E_BAD_ARG
    assert L.fg_grid_eval(None, 0, 1, None, None) == E.FG_E_BAD_ARG
    assert L.fg_grid_summary(None, None, None, None, None) == E.FG_E_BAD_ARG
    assert L.fg_grid_marginals(None, None, None) == E.FG_E_BAD_ARG and L.fg_grid_mixture(None, None, None, None) == E.FG_E_BAD_ARG
    assert L.fg_grid_count(None) == -1
    L.fg_grid_free(None)
    assert {"fg_grid_new", "fg_grid_eval", "fg_grid_summary", "fg_grid_marginals", "fg_grid_mixture", "fg_grid_count", "fg_grid_free"} <= set(E.ABI_SYMBOLS)


def test_grid_surface_read_outs_on_the_host():
    """GridSurface's own arithmetic (peak, log_evidence, mean, std) on the restatement's figures"""
    lj = _reference_surface(1, R.QUAD_AXIS)
    s = R.summary(lj)
    gs = G.GridSurface(R.QUAD_AXIS, R.QUAD_AXIS, lj[None], np.array([s["log_norm"]]), np.array([s["max"]]), np.array([s["argmax"]]), s["counts"][None],
                       s["log_marg_a"][None], s["log_marg_b"][None], np.zeros_like(lj), 1, 0)
    assert gs.peak == (R.QUAD_AXIS[s["argmax"] % 65], R.QUAD_AXIS[s["argmax"] // 65]) and gs.peak == (1.0, 1.0)
    assert abs(gs.log_evidence(0.25 * 0.25) - R.QUAD_LOG_EVIDENCE) <= 1e-5
    ma, mb = gs.mean()
    sa, sb = gs.std()
    var = 4.0 - 16.0 / 8.25                                   # Var[a | y]: 4 - 4 * 4 / 8.25
    assert abs(ma - R.QUAD_MEAN_A) <= 1e-6 and abs(mb - R.QUAD_MEAN_A) <= 1e-6 and abs(sb - sa) <= 1e-12
    # the axis ends 4.9 posterior standard deviations above the mean: the cut tail (mass 5e-7 at 24 variances) takes 1e-5 off the deviation
    assert abs(sa - math.sqrt(var)) <= 1e-4
    none = gs._replace(argmax=np.array([-1]))
    assert none.peak is None
