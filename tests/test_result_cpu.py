"""The model's return value on the host side (no GPU): the result builder of the C ABI (fg_program_result and its read-outs), the
promise that a program with results compiles to the same statements as the program without them, the flattening of
`Program.result` into named scalars, the DSL's closing `pure(..)`, the launch planner of k_result_eval over a grid of shapes
(tests/cpp/result_plan_driver.cpp) and the builder under AddressSanitizer / UBSan as a stand-alone program
(tests/cpp/result_driver.cpp)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import model as M
from tests.models import ZOO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fugue_amd", "csrc")


def _toks(expr):
    t = []
    E._postfix(M.as_expr(expr), t)
    return E._tok_array(t), len(t)


def _two_sites():
    """-> (library, unfinalized program handle, site expressions): sites "b" (handle 0), "a" (1), "k" (2, Categorical)."""
    L = E.lib()
    h = L.fg_program_new()
    par, plen = _toks(0.0), (C.c_int32 * 2)(1, 1)
    arr = (E.fg_tok * 2)(E.fg_tok(0, 0, 0, 0, 0.0), E.fg_tok(0, 0, 0, 0, 1.0))
    assert L.fg_program_sample(h, b"b", 12, arr, plen, 2) == 0
    assert L.fg_program_sample(h, b"a", 12, arr, plen, 2) == 1
    cat = (E.fg_tok * 2)(E.fg_tok(0, 0, 0, 0, 0.5), E.fg_tok(0, 0, 0, 0, 0.5))
    assert L.fg_program_sample(h, b"k", 3, cat, plen, 2) == 2
    del par
    return L, h, [M.Expr("site", a=i) for i in range(3)]


def _name(L, h, r):
    buf = C.create_string_buffer(64)
    need = L.fg_program_result_name(h, r, buf, 64)
    return need, buf.value.decode()


def test_names_and_count_round_trip():
    L, h, (b, a, k) = _two_sites()
    try:
        assert L.fg_program_n_results(h) == 0
        for r, (name, ex) in enumerate([("scale", M.exp(a)), ("contrast", a - b), ("résumé.k", M.select(k, [a, b])), ("const", M.as_expr(2.5))]):
            t, n = _toks(ex)
            assert L.fg_program_result(h, name.encode("utf-8"), t, n) == r
        assert L.fg_program_finalize(h) == 0
        assert L.fg_program_n_results(h) == 4
        assert [_name(L, h, r)[1] for r in range(4)] == ["scale", "contrast", "résumé.k", "const"]
        assert _name(L, h, 0)[0] == len("scale") + 1
        small = C.create_string_buffer(3)                      # like fg_program_site_name: truncated, NUL-terminated, full size returned
        assert L.fg_program_result_name(h, 1, small, 3) == len("contrast") + 1 and small.value == b"co"
        assert L.fg_program_result_name(h, 4, None, 0) == 500 and L.fg_program_result_name(h, -1, None, 0) == 500
    finally:
        L.fg_program_free(h)


def test_builder_error_codes():
    L, h, (b, a, k) = _two_sites()
    try:
        good, n = _toks(a + b)
        assert L.fg_program_result(h, b"sum", good, n) == 0
        assert L.fg_program_result(h, b"sum", good, n) == E.FG_E_BAD_ARG and "duplicate" in E.last_error()
        assert L.fg_program_result(h, b"", good, n) == E.FG_E_BAD_ARG
        assert L.fg_program_result(h, b"trunc", good, n - 1) == E.FG_E_BAD_ARG           # `a b` without its `+`: two values left on the stack
        assert L.fg_program_result(h, b"empty", good, 0) == E.FG_E_BAD_ARG
        under = (E.fg_tok * 2)(E.fg_tok(E.TOK["site"], 0, 0, 0, 0.0), E.fg_tok(E.TOK["add"], 0, 0, 0, 0.0))
        assert L.fg_program_result(h, b"under", under, 2) == E.FG_E_BAD_ARG              # stack underflow
        unknown = (E.fg_tok * 1)(E.fg_tok(E.TOK["site"], 3, 0, 0, 0.0))
        assert L.fg_program_result(h, b"handle", unknown, 1) == E.FG_E_BAD_ARG and "unknown site handle" in E.last_error()
        sel = (E.fg_tok * 3)(E.fg_tok(E.TOK["site"], 2, 0, 0, 0.0), E.fg_tok(E.TOK["const"], 0, 0, 0, 1.0), E.fg_tok(E.TOK["select"], 4, 0, 0, 0.0))
        assert L.fg_program_result(h, b"select", sel, 3) == E.FG_E_BAD_ARG               # four options announced, one given
        junk = (E.fg_tok * 1)(E.fg_tok(77, 0, 0, 0, 0.0))
        assert L.fg_program_result(h, b"junk", junk, 1) == E.FG_E_BAD_ARG
        assert L.fg_program_n_results(h) == 1                                              # a refused result leaves nothing behind
        assert L.fg_program_result_sites(h, None, 0) == E.FG_E_NOT_FINALIZED
        assert L.fg_program_finalize(h) == 0
        assert L.fg_program_result(h, b"late", good, n) == E.FG_E_STATE
        assert L.fg_program_n_results(h) == 1
    finally:
        L.fg_program_free(h)


def test_result_sites_are_the_sorted_sites_some_result_reads():
    P = M.Program()
    z = P.sample(M.addr("z"), M.Normal(0, 1))            # sorted order: a, k, m, z
    m = P.sample(M.addr("m"), M.Normal(0, 1))
    a = P.sample(M.addr("a"), M.Normal(0, 1))
    k = P.sample(M.addr("k"), M.Categorical([0.5, 0.5]))
    P.observe(M.addr("y"), M.Normal(m, 1.0), 0.3)
    P.result = {"pick": M.select(k, [z, 1.0]), "twice_z": z * 2.0, "none": 3.0}
    cp = E.compile_model(P)
    assert cp.site_names == ["a", "k", "m", "z"]
    assert cp.result_names == ["result.pick", "result.twice_z", "result.none"] and cp.R == 3
    assert cp.result_sites == [1, 3]                      # k and z; neither a nor m
    short = (C.c_int32 * 1)(-9)
    assert E.lib().fg_program_result_sites(cp.h, short, 1) == 2 and short[0] == 1      # the count, whatever the capacity
    P2 = M.Program()
    P2.sample(M.addr("x"), M.Normal(0, 1))
    P2.result = 4.0
    cp2 = E.compile_model(P2)
    assert cp2.R == 1 and cp2.result_sites == []          # a result reading no site


def _three_results(prog):
    """Three results over whatever sites the program has: an affine map of the first, a transcendental of the last, and a linear
    predictor over up to nine of them (long enough to be fused into FG_OP_DOT, whose terms go to a constant pool)."""
    sites = [M.Expr("site", a=h) for h in range(prog.n_samples)]
    lin = M.as_expr(0.25)
    for j, s in enumerate(sites[:9]):
        lin = lin + s * (0.5 + 0.125 * j)
    return (sites[0] * 2.0 + 1.0, M.exp(sites[-1]), lin)


@pytest.mark.parametrize("name", list(ZOO))
def test_results_change_nothing_of_the_statement_program(name):
    """Same instructions, slots and record streams with and without three results: the sampler kernels see the same program."""
    L = E.lib()
    bare = ZOO[name]()
    bare.result = None                                     # (some of the zoo's models return an expression: here the program without any result)
    plain = E.compile_model(bare)
    prog = ZOO[name]()
    prog.result = _three_results(prog)
    withr = E.compile_model(prog)
    assert plain.R == 0 and withr.R == 3 and withr.result_skipped == []
    for cp in (plain, withr):
        cp.shape = (cp.S, cp.d, cp.O, cp.n_instructions, cp.n_slots, cp.site_names, cp.site_vtypes, cp.f64_sites, cp.dep_counts,
                    tuple(L.fg_program_stream_records(cp.h, w) for w in range(5)))
    print(name, plain.shape[:5], plain.shape[-1])
    assert plain.shape == withr.shape


def test_run_time_compiler_source_is_the_same_with_results():
    """fg_jit.cpp's generated translation unit (its text is the cache key's input) does not see the results."""
    L = E.lib()
    L.fg_debug_jit_compile.argtypes = [C.c_void_p, C.c_char_p, C.c_longlong, C.c_char_p, C.c_longlong, C.POINTER(C.c_longlong)]
    texts = []
    for with_results in (False, True):
        prog = ZOO["coin"]()
        prog.result = _three_results(prog) if with_results else None
        cp = E.compile_model(prog)
        src = C.create_string_buffer(8 << 20); log = C.create_string_buffer(1 << 20); n = C.c_longlong()
        assert L.fg_debug_jit_compile(cp.h, src, len(src), log, len(log), C.byref(n)) == 0, log.value.decode()[:2000]
        texts.append(src.value)
    assert len(texts[0]) > 1000 and texts[0] == texts[1]


# ---- flattening Program.result ---------------------------------------------------------------------------------------------------
def test_flattening_names_scalars_tuples_and_dicts():
    x, y = M.Expr("site", a=0), M.Expr("site", a=1)
    assert M.flatten_result(x)[0] == ["result"]
    assert M.flatten_result(1.5)[0] == ["result"] and M.flatten_result(np.float64(2.0))[1][0].value == 2.0 and M.flatten_result(3)[1][0].value == 3.0
    names, exprs, skipped = M.flatten_result((x, [y, (x + y, 2.0)], {"mu": x, "pair": (x, y), "nested": {"deep": y}}))
    assert names == ["result[0]", "result[1][0]", "result[1][1][0]", "result[1][1][1]", "result[2].mu", "result[2].pair[0]", "result[2].pair[1]", "result[2].nested.deep"]
    assert skipped == [] and exprs[0] is x and exprs[3].value == 2.0
    names, _, skipped = M.flatten_result({"sd": x.exp(), "label": "text", "ok": x < y, "none": None, "v": [y, None], 7: x})
    assert names == [] and skipped == ["result"]          # a dict with a non-string key is no container of named results: one skipped leaf
    names, _, skipped = M.flatten_result({"sd": x.exp(), "label": "text", "ok": x < y, "none": None, "v": [y, None]})
    assert names == ["result.sd", "result.v[0]"] and skipped == ["result.label", "result.ok", "result.none", "result.v[1]"]
    assert M.flatten_result(None) == ([], [], ["result"]) and M.flatten_result(()) == ([], [], [])


def test_compile_model_registers_the_flattened_result():
    def model():
        return M.sample(M.addr("log_sigma"), M.Normal(0.0, 1.0)).bind(
            lambda ls: M.sample(M.addr("mu_a"), M.Normal(0.0, 2.0)).bind(
                lambda ma: M.sample(M.addr("mu_b"), M.Normal(0.0, 2.0)).bind(
                    lambda mb: M.observe(M.addr("y"), M.Normal(ma, M.exp(ls)), 0.4).bind(
                        lambda _: M.pure({"sigma": M.exp(ls), "contrast": ma - mb, "what": "a label", "raw": (ls, 1.0)})))))
    cp = E.compile_model(model)
    assert cp.result_names == ["result.sigma", "result.contrast", "result.raw[0]", "result.raw[1]"] and cp.R == 4
    assert cp.result_skipped == ["result.what"]
    assert [cp.site_names[j] for j in cp.result_sites] == ["log_sigma", "mu_a", "mu_b"]


def test_models_whose_return_value_means_nothing_keep_compiling():
    none = E.compile_model(lambda: M.sample(M.addr("x"), M.Normal(0, 1)).bind(lambda x: M.observe(M.addr("y"), M.Normal(x, 1.0), 0.1)))   # ends in pure(None)
    assert none.R == 0 and none.result_names == [] and none.result_skipped == ["result"] and none.result_sites == []
    cond = E.compile_model(lambda: M.sample(M.addr("x"), M.Normal(0, 1)).bind(lambda x: M.pure(x > 0.0)))
    assert cond.R == 0 and cond.result_skipped == ["result"]
    imperative = E.compile_model(ZOO["alldists"]())       # an imperative Program that never sets .result
    assert imperative.R == 0
    # models that have always returned expressions compile as before -- and now keep them
    seq = E.compile_model(lambda: M.plate(range(3), lambda i: M.sample(M.addr("z", i), M.Normal(0.0, 1.0))))
    assert seq.result_names == ["result[0]", "result[1]", "result[2]"] and seq.S == 3 and seq.n_instructions == 3
    pair = E.compile_model(lambda: M.zip_models(M.sample(M.addr("u"), M.Normal(0, 1)), M.sample(M.addr("k"), M.Poisson(2.0))))
    assert pair.result_names == ["result[0]", "result[1]"] and pair.result_sites == [0, 1]


def test_dsl_registers_its_closing_pure_when_numeric():
    from tests import dsl_models as Dm
    coin = E.CompiledProgram.from_dsl(Dm.COIN, Dm.COIN_DATA)
    assert coin.result_names == ["result"] and coin.result_sites == [coin.site_names.index("p")]
    mirror = E.compile_model(Dm.coin_mirror())
    assert (coin.S, coin.d, coin.O, coin.n_instructions, coin.n_slots, coin.stream_records) == (mirror.S, mirror.d, mirror.O, mirror.n_instructions, mirror.n_slots, mirror.stream_records)
    const = E.CompiledProgram.from_dsl(Dm.INDEXED)
    assert const.result_names == ["result"] and const.result_sites == []
    expr = E.CompiledProgram.from_dsl('let a <- sample(addr!("a"), Normal(0.0, 1.0)); let b <- sample(addr!("b"), Normal(0.0, 1.0)); pure(exp(a) - b * 2.0)')
    assert expr.R == 1 and expr.result_sites == [0, 1]
    arr = E.CompiledProgram.from_dsl('let a <- sample(addr!("a"), Normal(0.0, 1.0)); pure(data)', "[1, 2, 3]")
    assert arr.R == 0                                     # an array is no number: ignored as before


# ---- the launch planner ---------------------------------------------------------------------------------------------------------
def _gxx(out_dir, src, name, extra=(), more=()):
    assert shutil.which("g++"), "g++ builds the driver"
    exe = os.path.join(str(out_dir), name)
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", src), *more, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.mark.parametrize("n_cu", [256, 1])
def test_plan_over_the_grid_of_shapes(tmp_path, n_cu):
    """Every (tile, draw) pair owned once, LDS <= 160 KB, <= 1 024 threads, grids within HIP's limits, 64-bit index products: checked
    by the driver with the kernel's own item and index helpers; the shape of the plans is checked here."""
    exe = _gxx(tmp_path, "result_plan_driver.cpp", "result_plan_driver")
    r = subprocess.run([exe, str(n_cu)], capture_output=True, text=True)
    lines = r.stdout.splitlines()
    bad = [ln for ln in lines if not ln.endswith("ok")]
    assert r.returncode == 0 and not bad, (r.returncode, bad[:5], r.stderr[-1000:])
    pts = [ln for ln in lines if ln.startswith("point")]
    assert len(pts) == 6 * 5 * 10 * 2 and lines[-1] == "refusals ok"
    seen_forms = set()
    for ln in pts:
        head, plan, _ = ln.split("|")
        _, Cc, n, n_slots, cu, force = head.split()
        W, dpw, tiles, chunks, items, grid, lds, glob, scratch = (int(v) for v in plan.split())
        Cc, n, n_slots, force = int(Cc), int(n), int(n_slots), int(force)
        assert W * 64 <= 1024 and lds <= 160 * 1024 and 1 <= grid < 2 ** 31 and items == tiles * chunks
        assert glob == (1 if (force or n_slots * 512 > 160 * 1024) else 0)
        if not glob:
            assert W == (4 if 4 * n_slots * 512 <= 65536 else 2 if 2 * n_slots * 512 <= 65536 else 1) and lds == W * n_slots * 512
        want = n_cu * (4 if glob else 16)                  # the waves the grid aims at
        assert chunks == -(-n // dpw) and (chunks == 1 or items >= min(want, tiles * n) // 2)
        if tiles >= want or n == 1:
            assert chunks == 1 and dpw == n                # many tiles: every wave streams all draws of its tile
        if Cc <= 64 and n == 10 ** 6 and n_cu == 256:
            assert chunks > want * 9 // 10                 # one tile: the parallelism comes from splitting the draws
        assert items <= want + tiles
        seen_forms.add((glob, W))
    assert seen_forms >= {(0, 4), (0, 2), (0, 1), (1, 4)}


def test_result_builder_stand_alone_under_asan_ubsan(tmp_path):
    """tests/cpp/result_driver.cpp with its own main, built from the host sources with the sanitizers and run as a child process:
    well-formed and corrupted token streams through fg_program_result, the compiled list walked as the kernel reads it."""
    exe = _gxx(tmp_path, "result_driver.cpp", "result_driver_san",
               ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-DFG_BUILD", "-Wno-unknown-pragmas"),
               (os.path.join(CSRC, "fg_program.cpp"),))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:exitcode=23", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1:exitcode=24")
    accepted = refused = 0
    for seed in (1, 2, 3):
        r = subprocess.run([exe, str(seed)], capture_output=True, text=True, errors="replace", env=env, timeout=600)
        assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        last = r.stdout.strip().splitlines()[-1].split()
        assert last[0] == "results" and int(last[6]) == 200
        accepted += int(last[2]); refused += int(last[4])
    print("accepted", accepted, "refused", refused)
    assert accepted > 200 and refused > 200                # both the accepting and the refusing paths ran


# ---- the oracle comparison of tests/test_gpu_result.py is well conditioned -----------------------------------------------------------
def test_transcendental_cases_keep_a_one_ulp_difference_below_the_tolerance():
    """tests/test_gpu_result.py compares the transcendental results with the oracle at 1e-12 relative (ocml against glibc).  That is
    a statement about the expressions only if a one-ulp difference in each transcendental stays far below 1e-12 in the result:
    evaluate every case on the shared draws with each transcendental's value moved one ulp up and one ulp down."""
    from tests import result_cases as K
    P, v = K.base_program()
    _, transcendental = K.expressions(v)
    cells = K.draws(7, 130)
    order = sorted(range(P.n_samples), key=lambda h: P.sample_addresses()[h].encode())      # handle of each sorted site
    vals = {h: (cells[:, j].view(np.float64) if j not in (9, 10) else cells[:, j].astype(np.float64)) for j, h in enumerate(order)}
    assert (vals[v["s"].a] >= 0.5).all() and (vals[v["s"].a] <= 1.5).all()                 # sin / cos arguments inside [0.5, 1.5]
    for name, ex in transcendental.items():
        mid = K.evaluate(ex, vals)
        up = K.evaluate(ex, vals, lambda op, r: np.nextafter(r, np.inf))
        dn = K.evaluate(ex, vals, lambda op, r: np.nextafter(r, -np.inf))
        fin = np.isfinite(mid) & (mid != 0.0)
        with np.errstate(all="ignore"):
            worst = max(np.abs((up - mid) / mid)[fin].max(), np.abs((dn - mid) / mid)[fin].max())
        print(f"{name}: worst relative move under one ulp per transcendental = {worst:.3e} over {fin.sum()} finite values")
        assert fin.sum() > 800 and worst < 1e-15 * 4
        assert (np.isnan(up) == np.isnan(mid)).all() and (np.isinf(up) == np.isinf(mid))[~(np.abs(mid) > 1e308)].all()
