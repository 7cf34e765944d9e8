"""ABC on the host side (no GPU): the sequential restatement (tests/abc_restatement.py) against the reference's doc-test values, the
launch planners of fg_abc_plan.h over a grid of shapes as a stand-alone program under AddressSanitizer / UBSan
(tests/cpp/abc_plan_driver.cpp), the three statements of the ABI with the new entries, the promise that the zoo's programs compile to
what they compiled to, and the Python layer's refusal of a simulator it does not know."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import fugue_amd as F
from fugue_amd import abc as A
from fugue_amd import engine as E
from fugue_amd import model as M
from tests import abc_restatement as R
from tests import abi_check
from tests.models import ZOO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_doc_test_values():
    assert abs(R.euclidean([1.0, 2.0, 3.0], [1.1, 2.1, 2.9]) - 0.173) < 0.01            # abc.rs:124-128
    assert abs(R.manhattan([1.0, 2.0, 3.0], [1.5, 1.5, 3.5]) - 1.5) < 0.001             # abc.rs:160-164
    assert R.euclidean([1.0], [1.0, 2.0]) == math.inf and R.manhattan([1.0, 2.0], [1.0]) == math.inf


def test_restatement_summary_stats_and_its_edges():
    assert R.compute_stats([]) == [0.0, 0.0, 0.0]
    assert R.compute_stats([3.0, 1.0, 2.0]) == [2.0, math.sqrt(2.0 / 3.0), 2.0]
    assert R.compute_stats([4.0, 1.0, 3.0, 2.0])[2] == 2.5                               # the even-K average
    assert R.compute_stats([1.0, float("nan")]) is None
    assert math.isnan(R.summary_stats([1.0, 2.0], [1.0, float("nan")], [1.0, 1.0, 1.0]))
    o, s = [1.0, 2.0, 4.0], [2.0, 2.0, 2.0]
    full = R.summary_stats(o, s, [1.0, 1.0, 1.0])
    assert R.summary_stats(o, s, [1.0, 1.0, 1.0, 9.0, 9.0]) == full                      # more than three weights are ignored
    assert R.summary_stats(o, s, []) == 0.0 and R.summary_stats(o, s, [1.0]) == abs(7.0 / 3.0 - 2.0)
    with pytest.raises(ValueError):
        R.summary_stats([float("nan")], s, [1.0])


def test_restatement_bandwidths_index_mixture_and_stop_rule():
    coords = [[0.0, 5.0], [2.0, 5.0], [4.0, 5.0]]
    bw = R.kernel_bandwidths(coords, [0.25, 0.5, 0.25])
    assert bw[0] == math.sqrt(2.0 * 2.0) and bw[1] == 1e-3                               # a degenerate component: the 1e-3 branch
    assert R.kernel_bandwidths(coords, [0.0, 0.0, 0.0]) == [1e-3, 1e-3]
    w = [0.1, 0.0, 0.6, 0.3]
    assert [R.sample_index(u, w) for u in (0.0, 0.1, 0.1000001, 0.69, 0.71, 0.9999999)] == [0, 0, 2, 2, 3, 3]
    assert R.sample_index(1.0, [0.5, 0.25]) == 1                                         # u total beyond every cumulative sum: the last index
    # one center, weight 1: the mixture is the Gaussian itself
    got = R.kernel_mixture_log_density([0.3], [[0.1]], [1.0], [0.5])
    assert abs(got - (-0.5 * 0.16 - math.log(0.5) - 0.5 * math.log(2 * math.pi))) < 1e-15
    assert R.kernel_mixture_log_density([0.3], [[0.1], [0.2]], [0.0, 0.0], [0.5]) == -math.inf
    assert R.stage_weights([0.0, 0.0], [-math.inf, -math.inf]) == [0.5, 0.5]             # a normaliser that is not finite: 1 / n
    assert R.stop_rule([0, 1, 0, 1, 1, 1], 2, 100) == ([1, 3], 4)                        # right after the n-th accept
    assert R.stop_rule([0, 1, 0, 1, 1, 1], 5, 3) == ([1], 3)                             # the budget ends it
    assert R.stop_rule([0, 0, 0], 1, 3) == ([], 3)


def test_python_sample_index_and_uniforms_are_the_restatement_and_the_oracle():
    from oracle import oracle as orc
    w = [0.2, 0.0, 0.5, 0.3]
    for u in np.linspace(0.0, 0.999, 41):
        assert A.sample_index(float(u), w) == R.sample_index(float(u), w)
    u = A._uniforms(0x123456789ABCDEF, 5, 3)
    for i in range(5):
        assert u[i] == orc.sample_dist("Uniform", [0.0, 1.0], orc.stream(0x123456789ABCDEF, i, 3, A.RNG_ABC))


# ---- the launch planners --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cu", [256, 1])
def test_plans_over_the_grid_of_shapes_under_asan_ubsan(tmp_path, n_cu):
    """m in {0, 1, 63, 64, 65, 130, 4 096} x n in {1, 10, 64, 65, 257, 1 000, 65 536} x d in {0, 1, 5, 8, 9, 33} x forced splits in
    {none, 1, 7, 300}: every (tile, center) pair owned once in split order, empty ranges legal, every partial cell written once -- checked
    by the driver with the kernel's own item and index helpers; the shape of the plans is checked here."""
    assert shutil.which("g++"), "g++ builds the driver"
    exe = os.path.join(str(tmp_path), "abc_plan_driver_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        os.path.join(ROOT, "tests", "cpp", "abc_plan_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=24")
    r = subprocess.run([exe, str(n_cu)], capture_output=True, text=True, env=env, timeout=600)
    lines = r.stdout.splitlines()
    bad = [ln for ln in lines if not ln.endswith("ok")]
    assert r.returncode == 0 and not bad, (r.returncode, bad[:5], r.stderr[-2000:])
    pts = [ln for ln in lines if ln.startswith("mix")]
    assert len(pts) == 7 * 7 * 6 * 4 and lines[-1] == "refusals ok" and lines[-2] == "rounds ok"
    assert len([ln for ln in lines if ln.startswith("compact")]) == 9
    seen_reg, seen_empty = set(), False
    for ln in pts:
        head, plan, _ = ln.split("|")
        m, n, d, cu, force = (int(v) for v in head.split()[1:])
        tiles, splits, cps, items, grid, fgrid, d_reg, partial, table = (int(v) for v in plan.split())
        assert tiles == -(-m // 64) and table == n * (d + 1) and d_reg == (d if 1 <= d <= 8 else 0)
        seen_reg.add(d_reg)
        if m == 0:
            assert grid == 0 and items == 0 and partial == 0
            continue
        assert items == tiles * splits and grid == -(-items // 4) and 0 < grid < 2 ** 31 and partial == splits * m and fgrid == -(-m // 256)
        assert cps * splits >= n
        if force:
            assert splits == force
            seen_empty = seen_empty or (splits - 1) * cps >= n
        else:
            want = n_cu * 16                               # the waves the grid aims at
            assert splits <= n and (splits - 1) * cps < n and items <= want + tiles
            if tiles >= want or n == 1:
                assert splits == 1
    assert seen_reg == {0, 1, 5, 8} and seen_empty


# ---- the three statements of the ABI --------------------------------------------------------------------------------------------
NEW = ("fg_abc_distance", "fg_abc_mixture", "fg_abc_new", "fg_abc_free", "fg_abc_round_prior", "fg_abc_stage_begin", "fg_abc_round_stage", "fg_abc_stage_end",
       "fg_abc_last_round", "fg_abc_get_population", "fg_abc_set_population")


def test_abi_check_passes_with_the_new_entries():
    header = open(os.path.join(ROOT, "include", "fugue_amd.h")).read()
    rust = open(os.path.join(ROOT, "rust", "fugue-gpu", "src", "ffi.rs")).read()
    H, Rs = abi_check.parse_header(header), abi_check.parse_rust(rust)
    for f in NEW:
        assert f in H["fns"] and f in Rs["fns"] and f in E.ABI_SYMBOLS and hasattr(E.lib(), f), f
    assert H["fns"]["fg_abc_distance"][0] == "i32" and len(H["fns"]["fg_abc_distance"][1]) == 10
    assert H["fns"]["fg_abc_round_stage"][1][1] == "u32"   # the stage = the iteration word
    assert abi_check.compare_header_rust(header, rust) == []
    assert abi_check.compare_header_ctypes(header, E.lib()) == []
    assert set(H["fns"]) == set(E.ABI_SYMBOLS)
    assert 'define FG_ABI_VERSION 1' in header and E.lib().fg_abi_version() == 1
    ir = open(os.path.join(ROOT, "fugue_amd", "csrc", "fg_ir.h")).read()
    assert "FG_RNG_ABC = 10" in ir and A.RNG_ABC == 10


# ---- programs are what they were ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ZOO))
def test_programs_of_the_zoo_compile_to_the_same_counts(name):
    L = E.lib()

    def shape(cp):
        return (cp.S, cp.d, cp.O, cp.R, L.fg_program_n_instructions(cp.h), L.fg_program_n_slots(cp.h), cp.site_names, cp.site_vtypes, cp.f64_sites,
                [L.fg_program_dep_count(cp.h, k) for k in range(cp.d)], tuple(L.fg_program_stream_records(cp.h, w) for w in range(5)))

    cp = E.compile_model(ZOO[name]())
    before = shape(cp)
    if cp.O:
        A._simulator(cp, "observe"), A._simulator(cp, cp.observe_names[:1])   # what the ABC layer reads of a program
    assert shape(cp) == before == shape(E.compile_model(ZOO[name]()))


def test_run_time_compiler_source_is_what_it_was():
    L = E.lib()
    L.fg_debug_jit_compile.argtypes = [C.c_void_p, C.c_char_p, C.c_longlong, C.c_char_p, C.c_longlong, C.POINTER(C.c_longlong)]
    texts = []
    for _ in range(2):
        cp = E.compile_model(ZOO["coin"]())
        A._simulator(cp, "observe")
        src = C.create_string_buffer(8 << 20); log = C.create_string_buffer(1 << 20); n = C.c_longlong()
        assert L.fg_debug_jit_compile(cp.h, src, len(src), log, len(log), C.byref(n)) == 0, log.value.decode()[:2000]
        texts.append(src.value)
    assert len(texts[0]) > 1000 and texts[0] == texts[1]
    assert b"k_abc" not in texts[0] and b"fg_abc_plan" not in texts[0]   # the unit holds no ABC code (the C header's declarations are text it always carried)


# ---- the Python layer -----------------------------------------------------------------------------------------------------------
def _normal_mean():
    return M.sample(M.addr("mu"), M.Normal(0.0, 2.0)).bind(lambda mu: M.observe(M.addr("y"), M.Normal(mu, 1.0), 2.0).map(lambda _: mu))


@pytest.mark.parametrize("bad", [None, 3, "obs", [], ["nope"], ["y", "result"], [1, 2], lambda t: 0.0])
def test_a_wrong_simulator_raises_value_error_naming_the_two_forms(bad):
    cp = E.compile_model(_normal_mean())
    with pytest.raises(ValueError, match="observe addresses.*result names"):
        A._simulator(cp, bad)
    with pytest.raises(ValueError, match="observe addresses.*result names"):
        F.abc_rejection(1, cp, bad, [2.0], F.EuclideanDistance(), 0.5, 5)


def test_simulator_forms_and_default_observed_data():
    cp = E.compile_model(_normal_mean())
    assert A._simulator(cp, "observe") == (A.SIM_OBSERVE, [0]) and A._simulator(cp, ["y"]) == (A.SIM_OBSERVE, [0])
    assert A._simulator(cp, ["result"]) == (A.SIM_RESULT, [0])
    assert A._observed(cp, A.SIM_OBSERVE, [0], None).tolist() == [2.0]                   # the model's own observed value
    assert A._observed(cp, A.SIM_RESULT, [0], 2.0).tolist() == [2.0]
    with pytest.raises(ValueError):
        A._observed(cp, A.SIM_RESULT, [0], None)
    coin = E.compile_model(ZOO["coin"]())
    k, idx = A._simulator(coin, ["flip#3", "flip#1"])
    assert (k, idx) == (A.SIM_OBSERVE, [1, 3])                                           # program order
    assert A._observed(coin, k, idx, None).tolist() == [0.0, 1.0]


def test_error_type_carries_the_references_fields_and_text():
    e = F.ABCError("EmptyInitialPopulation", 0.5, 300)
    assert (e.kind, e.tolerance, e.attempts) == ("EmptyInitialPopulation", 0.5, 300)
    assert str(e) == "ABC-SMC initial population is empty: no draw fell within tolerance 0.5 in 300 attempts"
    s = F.ABCError("StageExhausted", 0.25, 1000, accepted=3, requested=20)
    assert (s.accepted, s.requested, s.attempts) == (3, 20, 1000)
    assert str(s) == "ABC-SMC stage at tolerance 0.25 exhausted its budget of 1000 attempts with only 3/20 particles accepted"
    assert F.ABC_SMC_DEFAULT_ATTEMPT_FACTOR == 100
    cfg = F.ABCSMCConfig(initial_tolerance=1.0, tolerance_schedule=[0.5], particles_per_round=20)          # abc.rs:688-692
    assert (cfg.initial_tolerance, cfg.tolerance_schedule, cfg.particles_per_round) == (1.0, [0.5], 20)
