"""Predictive draws on the host side (no GPU): the observe-statement read-outs of the C ABI (fg_program_observe_name / _vtype / _dist)
over the zoo, the promise that reading them changes nothing of a program, the launch planner of k_predict_eval over a grid of
shapes as a stand-alone program under AddressSanitizer / UBSan (tests/cpp/predict_plan_driver.cpp), and the three statements of the
ABI (header, ctypes, ffi.rs) with the new entries."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

from fugue_amd import engine as E
from fugue_amd import model as M
from tests import abi_check
from tests.models import ZOO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VTYPE_OF = {"Bernoulli": M.BOOL, "Binomial": M.U64, "Poisson": M.U64, "Categorical": M.USIZE, "DiscreteUniform": M.I64}


@pytest.mark.parametrize("name", list(ZOO))
def test_observe_read_outs_are_the_models_own_list_in_program_order(name):
    prog = ZOO[name]()
    cp = E.compile_model(prog)
    own = [st for st in prog.stmts if st.kind == M.OBSERVE]
    assert cp.O == len(own) == len(cp.observe_names)
    assert cp.observe_names == [st.addr for st in own]
    assert cp.observe_dists == [st.dist.kind for st in own]
    assert cp.observe_vtypes == [VTYPE_OF.get(st.dist.name, M.F64) for st in own]
    L = E.lib()
    for k in (-1, cp.O):                                  # like fg_program_site_name outside [0, S)
        assert L.fg_program_observe_name(cp.h, k, None, 0) == 500 and L.fg_program_observe_vtype(cp.h, k) == 500 and L.fg_program_observe_dist(cp.h, k) == 500
    if cp.O:
        full = cp.observe_names[0].encode("utf-8")
        small = C.create_string_buffer(2)                  # truncated, NUL-terminated, the full size returned
        assert L.fg_program_observe_name(cp.h, 0, small, 2) == len(full) + 1 and small.value == full[:1]


def test_read_outs_need_a_finalized_program():
    L = E.lib()
    h = L.fg_program_new()
    try:
        assert L.fg_program_observe_name(h, 0, None, 0) == E.FG_E_NOT_FINALIZED
        assert L.fg_program_observe_vtype(h, 0) == E.FG_E_NOT_FINALIZED and L.fg_program_observe_dist(h, 0) == E.FG_E_NOT_FINALIZED
    finally:
        L.fg_program_free(h)


@pytest.mark.parametrize("name", list(ZOO))
def test_programs_are_unchanged_by_the_read_outs(name):
    """Counts, site tables and record streams before and after every observe statement has been read out, and against a second
    compilation that was never asked: the accessors read the statement list and write nothing."""
    L = E.lib()

    def shape(cp):
        return (cp.S, cp.d, L.fg_program_n_observe(cp.h), L.fg_program_n_instructions(cp.h), L.fg_program_n_slots(cp.h), cp.site_names, cp.site_vtypes,
                cp.f64_sites, [L.fg_program_dep_count(cp.h, k) for k in range(cp.d)], tuple(L.fg_program_stream_records(cp.h, w) for w in range(5)))

    cp = E.compile_model(ZOO[name]())
    before = shape(cp)
    buf = C.create_string_buffer(4096)
    for _ in range(2):
        for k in range(cp.O):
            L.fg_program_observe_name(cp.h, k, buf, 4096), L.fg_program_observe_vtype(cp.h, k), L.fg_program_observe_dist(cp.h, k)
    assert shape(cp) == before == shape(E.compile_model(ZOO[name]()))


def test_run_time_compiler_source_does_not_see_the_read_outs():
    L = E.lib()
    L.fg_debug_jit_compile.argtypes = [C.c_void_p, C.c_char_p, C.c_longlong, C.c_char_p, C.c_longlong, C.POINTER(C.c_longlong)]
    cp = E.compile_model(ZOO["coin"]())
    texts = []
    for _ in range(2):
        src = C.create_string_buffer(8 << 20); log = C.create_string_buffer(1 << 20); n = C.c_longlong()
        assert L.fg_debug_jit_compile(cp.h, src, len(src), log, len(log), C.byref(n)) == 0, log.value.decode()[:2000]
        texts.append(src.value)
        assert cp.observe_names == [E.compile_model(ZOO["coin"]()).observe_names[k] for k in range(cp.O)]
    assert len(texts[0]) > 1000 and texts[0] == texts[1]


# ---- the launch planner ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_cu", [256, 1])
def test_plan_over_the_grid_of_shapes_under_asan_ubsan(tmp_path, n_cu):
    """C in {1, 63, 64, 65, 130, 65 536} x n in {0, 1, 2, 7, 1 000} x n_slots in {2, 40, 320, 321, 2 000}, LDS and forced-global: every
    (tile, draw) pair owned exactly once, LDS within budget, the global form when and only when the plan has to take it -- checked by
    the driver with the kernel's own item and index helpers; the shape of the plans is checked here."""
    assert shutil.which("g++"), "g++ builds the driver"
    exe = os.path.join(str(tmp_path), "predict_plan_driver_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        os.path.join(ROOT, "tests", "cpp", "predict_plan_driver.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=24")
    r = subprocess.run([exe, str(n_cu)], capture_output=True, text=True, env=env, timeout=600)
    lines = r.stdout.splitlines()
    bad = [ln for ln in lines if not ln.endswith("ok")]
    assert r.returncode == 0 and not bad, (r.returncode, bad[:5], r.stderr[-2000:])
    pts = [ln for ln in lines if ln.startswith("point")]
    assert len(pts) == 6 * 5 * 5 * 2 and lines[-1] == "refusals ok"
    seen_forms, seen_c, seen_n, seen_s = set(), set(), set(), set()
    for ln in pts:
        head, plan, _ = ln.split("|")
        _, Cc, n, n_slots, cu, force = head.split()
        W, dpw, tiles, chunks, items, grid, lds, glob, scratch = (int(v) for v in plan.split())
        Cc, n, n_slots, force = int(Cc), int(n), int(n_slots), int(force)
        seen_c.add(Cc), seen_n.add(n), seen_s.add(n_slots)
        assert W * 64 <= 1024 and lds <= 160 * 1024 and 0 <= grid < 2 ** 31 and items == tiles * chunks and tiles == -(-Cc // 64)
        assert glob == (1 if (force or n_slots * 512 > 160 * 1024) else 0)
        if not glob:
            assert W == (4 if 4 * n_slots * 512 <= 65536 else 2 if 2 * n_slots * 512 <= 65536 else 1) and lds == W * n_slots * 512
        if n == 0:
            assert grid == 0 and items == 0
            continue
        want = n_cu * (4 if glob else 16)                  # the waves the grid aims at
        assert chunks == -(-n // dpw) and items <= want + tiles and grid == -(-items // W)
        if tiles >= want or n == 1:
            assert chunks == 1 and dpw == n                # many tiles: every wave streams all draws of its tile
        seen_forms.add((glob, W))
    assert seen_forms >= {(0, 4), (0, 2), (0, 1), (1, 4)}
    assert seen_c == {1, 63, 64, 65, 130, 65536} and seen_n == {0, 1, 2, 7, 1000} and seen_s == {2, 40, 320, 321, 2000}


# ---- the three statements of the ABI --------------------------------------------------------------------------------------------
NEW = ("fg_program_observe_name", "fg_program_observe_vtype", "fg_program_observe_dist", "fg_predict_eval")


def test_abi_check_passes_with_the_new_entries():
    header = open(os.path.join(ROOT, "include", "fugue_amd.h")).read()
    rust = open(os.path.join(ROOT, "rust", "fugue-gpu", "src", "ffi.rs")).read()
    H, R = abi_check.parse_header(header), abi_check.parse_rust(rust)
    for f in NEW:
        assert f in H["fns"] and f in R["fns"] and f in E.ABI_SYMBOLS, f
    assert H["fns"]["fg_predict_eval"][0] == "i32" and len(H["fns"]["fg_predict_eval"][1]) == 10
    assert H["fns"]["fg_predict_eval"][1][5] == "u32"     # iter0
    assert abi_check.compare_header_rust(header, rust) == []
    assert abi_check.compare_header_ctypes(header, E.lib()) == []
    assert set(H["fns"]) == set(E.ABI_SYMBOLS)
