"""The exact Gibbs moves without a GPU: the plan (fugue_amd/csrc/fg_gibbs_plan.h) through a stand-alone driver under
-fsanitize=address,undefined, the supports the program states, the restatement (tests/gibbs_restatement.py) over the oracle -- its
knife-edge margin at the seeds the device test uses, its non-finite rules, the invariance law on two models -- the three statements
of the new ABI entries, and the argument codes that need no engine."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import gibbs as GB
from fugue_amd import model as M
from oracle import oracle as orc
from tests import abi_check
from tests import gibbs_restatement as R
from tests.models import all_dists_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g")
PLAN_KS = (1, 2, 64, 4096)
NEW = ["fg_program_site_support", "fg_gibbs_new", "fg_gibbs_n_sites", "fg_gibbs_n_cells", "fg_gibbs_layout", "fg_gibbs_sweep", "fg_gibbs_count", "fg_gibbs_seek",
       "fg_gibbs_stats", "fg_gibbs_probs", "fg_gibbs_free"]


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    orc.build()


# ---- the plan ------------------------------------------------------------------------------------------------------------------------
def test_plan_driver_under_address_and_ub_sanitizers(tmp_path):
    """sites of 1, 2, 64 and 4096 values at 1, 64, 65 and 130 chains, the automatic list, and every refusal with its message"""
    assert shutil.which("g++"), "g++ builds the driver"
    exe = os.path.join(str(tmp_path), "gibbs_plan_driver_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", *SAN, os.path.join(ROOT, "tests", "cpp", "gibbs_plan_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=24")
    r = subprocess.run([exe, *[str(k) for k in PLAN_KS]], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    lines = r.stdout.splitlines()
    plans = [ln for ln in lines if ln.startswith("plan ")]
    cell0, n_cells = R.layout([(j, -3, K) for j, K in enumerate(PLAN_KS)])
    assert cell0 == [0, 1, 3, 67] and n_cells == 4163
    for Cn, ln in zip((1, 64, 65, 130), plans):
        head, nums, cells, verdict = [s.strip() for s in ln.split("|")]
        assert head == f"plan {Cn}" and verdict == "ok", ln
        rc, n_sites, nc, k_max, grid, work, cell_bytes = [int(v) for v in nums.split()]
        assert (rc, n_sites, nc, k_max, grid, work, cell_bytes) == (0, 4, n_cells, 4096, -(-Cn // 64), 4096 * Cn * 8, n_cells * Cn * 8), ln
        assert [int(v) for v in cells.split()] == cell0
    assert len(plans) == 4 and lines[-1] == "sweeps ok"
    ref = {}
    for ln in lines:
        if ln.startswith("refusal "):
            head, rc, msg = [s.strip() for s in ln.split("|")]
            ref[head.split()[1]] = (int(rc), msg)
    want = {"k_cap": (E.FG_E_LIMIT, "site `big` has 4097 values, beyond 4096"), "f64": (E.FG_E_BAD_ARG, "site `x` is not a discrete site"),
            "no_support": (E.FG_E_BAD_ARG, "site `po` has no finite support known from constants"), "empty_support": (E.FG_E_BAD_ARG, "site `empty` has no finite support"),
            "twice": (E.FG_E_BAD_ARG, "site `s#0` is listed twice"), "negative_n": (E.FG_E_BAD_ARG, "n_sites < 0"), "null_list": (E.FG_E_BAD_ARG, "null site list"),
            "outside": (E.FG_E_BAD_ARG, "site #8 is outside [0, 8)"), "below": (E.FG_E_BAD_ARG, "site #-1 is outside"), "no_chains": (E.FG_E_BAD_ARG, "no chains"),
            "null_out": (E.FG_E_BAD_ARG, "null plan"), "empty_list": (E.FG_E_BAD_ARG, "the model has no discrete site with a finite constant support")}
    assert set(ref) == set(want)
    for name, (rc, word) in want.items():
        assert ref[name][0] == rc and word in ref[name][1] and ref[name][1].startswith("fg_gibbs_new: "), (name, ref[name])


# ---- the supports ----------------------------------------------------------------------------------------------------------------------
def test_site_support_of_every_discrete_distribution():
    cp = E.compile_model(all_dists_model())
    got = {a: GB.site_support(cp, j) for j, a in enumerate(cp.site_names)}
    assert got["be"] == (0, 1) and got["cat"] == (0, 1) and got["cat#2"] == (0, 2) and got["bi"] == (0, 10) and got["du"] == (-2, 5)
    assert got["po"] is None and got["a"] is None and got["s"] is None
    assert {a for a, v in got.items() if v is not None} == set(R.PICK_ADDRS)
    assert {a: got[a] for a in R.PICK_ADDRS} == R.PICK_SUPPORT
    lo, hi = C.c_int64(7), C.c_int64(7)
    L = E.lib()
    for bad in (-1, cp.S):
        assert L.fg_program_site_support(cp.h, bad, C.byref(lo), C.byref(hi)) == E.FG_E_BAD_ARG
    assert L.fg_program_site_support(cp.h, 0, None, C.byref(hi)) == E.FG_E_BAD_ARG and L.fg_program_site_support(cp.h, 0, C.byref(lo), None) == E.FG_E_BAD_ARG
    assert L.fg_program_site_support(cp.h, cp.site_names.index("po"), C.byref(lo), C.byref(hi)) == 0 and (lo.value, hi.value) == (7, 7)
    # bounds that read a site, a Binomial whose n does
    P = M.Program()
    k = P.sample(M.addr("k"), M.Binomial(4, 0.5))
    P.sample(M.addr("m"), M.Binomial(k, 0.5))
    P.sample(M.addr("u"), M.DiscreteUniform(0, k))
    P.sample(M.addr("v"), M.DiscreteUniform(3, 3))
    cp2 = E.compile_model(P)
    got2 = {a: GB.site_support(cp2, j) for j, a in enumerate(cp2.site_names)}
    assert got2 == {"k": (0, 4), "m": None, "u": None, "v": (3, 3)}


# ---- the restatement over the oracle ---------------------------------------------------------------------------------------------------------
def test_no_pick_of_the_device_tests_seeds_is_near_a_knife_edge():
    """the margin the device test relies on, with a factor 1000 to spare, on the oracle's scores: the seed is fixed here"""
    prog = all_dists_model()
    om = orc.OracleModel(prog)
    sites = R.pick_sites(om.site_names)
    assert [K for _, _, K in sites] == [2, 2, 3, 11, 8]
    score, u = R.oracle_scorer(om), R.oracle_uniform(R.PICK_SEED)
    worst = np.inf
    for Cn in R.PICK_SHAPES:
        cells = np.stack([om.run_prior(R.PICK_SEED, c)[0] for c in range(Cn)], axis=1)
        for t in range(R.PICK_SWEEPS):
            out = R.sweep(cells, sites, score, u, t)
            assert not out["stuck"].any() and np.isfinite(out["scores"]).all()
            worst = min(worst, float(out["margin"].min()))
            cells = out["cells"]
    print(f"smallest margin {worst:.3g} bounds")
    assert worst > 1000.0


def test_a_chain_sweeps_the_same_alone_and_under_any_offset():
    om = orc.OracleModel(all_dists_model())
    sites = R.pick_sites(om.site_names)
    score, u = R.oracle_scorer(om), R.oracle_uniform(R.PICK_SEED)
    cells = np.stack([om.run_prior(R.PICK_SEED, c)[0] for c in range(5)], axis=1)
    whole = R.sweep(cells, sites, score, u, 3)
    part = R.sweep(cells[:, 3:], sites, score, u, 3, chain0=3)
    assert np.array_equal(whole["cells"][:, 3:], part["cells"]) and np.array_equal(whole["cond"][:, 3:], part["cond"])
    other = R.sweep(cells, sites, score, u, 4)
    assert not np.array_equal(whole["picks"], other["picks"])           # the sweep index is in the stream


def test_non_finite_scores_by_the_rule():
    sites = [(0, 0, 4)]
    cells = np.zeros((1, 3), dtype=np.int64)
    table = {0: [-np.inf, np.nan, np.inf], 1: [0.0, -np.inf, 1.0], 2: [np.nan, -np.inf, np.nan], 3: [-1.0, np.nan, 2.0]}
    score = lambda c: np.array([table[int(c[0, j])][j] for j in range(3)])
    out = R.sweep(cells, sites, score, lambda ch, t, i: np.array([0.999999, 0.5, 0.5]), 0)
    assert out["stuck"].tolist() == [[False, True, True]] and out["picks"][0, 1:].tolist() == [-1, -1] and out["cells"][0, 1:].tolist() == [0, 0]
    assert np.isnan(out["cond"][:, 1:]).all() and out["counts"][0].tolist() == [1, 2, 4, 3]
    p = out["cond"][:, 0]
    assert p[0] == 0.0 and p[2] == 0.0 and abs(p.sum() - 1.0) < 4 * R.EPS and out["picks"][0, 0] == 3     # x >= every running sum but the last: the pick is the last positive weight
    out = R.sweep(cells, [(0, 0, 3)], lambda c: np.array([[0.0, 0.0, -np.inf][int(c[0, 0])]] * 3), lambda ch, t, i: np.array([1.0, 0.0, 0.49999]), 0)
    assert out["picks"][0].tolist() == [1, 0, 0]                   # u T = T: no running sum exceeds it, and the last cell has no weight
    assert R.pool_sum(np.arange(1.0, 8.0)) == 28.0 and R.pool_sum(np.ones((3, 130))).tolist() == [130.0] * 3


@pytest.mark.parametrize("which", ["ab", "select"])
def test_invariance_law_of_the_restatement(which):
    """16 384 chains start from the exact joint; after one sweep every joint cell is within 5 binomial standard errors of its mass"""
    prog = R.law_program_ab() if which == "ab" else R.law_program_select()
    om = orc.OracleModel(prog)
    assert om.site_names == (["a", "b"] if which == "ab" else ["i", "j"])
    start = R.law_start(which)
    R.judge_law(which, start)                                      # the start itself obeys the law
    out = R.sweep(start, R.LAW_SITES, R.oracle_scorer(om), R.oracle_uniform(R.LAW_SEED), 0)
    assert out["counts"][:, R.MOVED].min() > R.LAW_CHAINS // 10       # the chains do move
    R.judge_law(which, out["cells"])
    exact = R.law_exact(which)
    # the conditionals are the exact ones: p(a | b) of the first site from the start
    pa = exact / exact.sum(axis=0, keepdims=True)
    assert np.allclose(out["cond"][0:2], pa[:, start[1]], rtol=1e-12, atol=0)


# ---- the three statements of the ABI -----------------------------------------------------------------------------------------------------
def test_abi_check_passes_with_the_new_entries():
    header = open(os.path.join(ROOT, "include", "fugue_amd.h")).read()
    rust = open(os.path.join(ROOT, "rust", "fugue-gpu", "src", "ffi.rs")).read()
    H, Rs = abi_check.parse_header(header), abi_check.parse_rust(rust)
    for f in NEW:
        assert f in H["fns"] and f in Rs["fns"] and f in E.ABI_SYMBOLS, f
    assert abi_check.compare_header_rust(header, rust) == []
    assert abi_check.compare_header_ctypes(header, E.lib()) == []
    for line in ("#define FG_GIBBS_K_CAP 4096", "#define FG_GIBBS_COUNTS 4"):
        assert line in header, line
    assert GB.K_CAP == R.K_CAP == 4096 and len(GB.COUNT_NAMES) == R.COUNTS == 4
    assert "FG_RNG_GIBBS = 13" in open(os.path.join(ROOT, "fugue_amd", "csrc", "fg_ir.h")).read() and R.RNG_GIBBS == 13


def test_argument_codes_without_an_engine():
    L = E.lib()
    h = C.c_void_p(5)
    one = (C.c_int32 * 1)(0)
    assert L.fg_gibbs_new(None, one, 1, C.byref(h)) == E.FG_E_BAD_ARG and h.value is None and "null engine" in E.last_error()
    assert L.fg_gibbs_new(None, one, 1, None) == E.FG_E_BAD_ARG and "null out" in E.last_error()
    assert L.fg_gibbs_n_sites(None) == E.FG_E_BAD_ARG and L.fg_gibbs_n_cells(None) == -1 and L.fg_gibbs_count(None) == -1
    assert L.fg_gibbs_layout(None, None, None, None, None) == E.FG_E_BAD_ARG
    assert L.fg_gibbs_sweep(None, 1, None, 0, None, None, None) == E.FG_E_BAD_ARG and "null handle" in E.last_error()
    assert L.fg_gibbs_seek(None, 0) == E.FG_E_BAD_ARG and L.fg_gibbs_stats(None, None) == E.FG_E_BAD_ARG and L.fg_gibbs_probs(None, None, None) == E.FG_E_BAD_ARG
    L.fg_gibbs_free(None)
    import fugue_amd as F
    assert F.hmc_gibbs_chain is GB.hmc_gibbs_chain and F.gibbs_chain is GB.gibbs_chain and F.GibbsSweep is GB.GibbsSweep
    assert "predictive=" in GB.hmc_gibbs_chain.__doc__ and "not offered" in GB.hmc_gibbs_chain.__doc__
    cp = E.compile_model(all_dists_model())
    with pytest.raises(ValueError):
        GB._site_list(cp, ["nope"])
    with pytest.raises(ValueError):
        GB._site_list(cp, [])
    assert GB._site_list(cp, None) is None and GB._site_list(cp, ["du", 3]) == [cp.site_names.index("du"), 3]
