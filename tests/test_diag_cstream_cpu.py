"""The streamed frequency tables on the host: tests/cpp/cstream_driver.cpp (fg_diag_cstream_plan.h, the planner the device code
calls, with a host loop in place of the kernel) == tests/cstream_restatement.py exactly, whatever the chunking; every refused
argument; the call-order errors and the integrity error; the launch split of a chunk of 2^33 elements from arithmetic alone; the
same driver under AddressSanitizer / UBSan (a stand-alone binary); the driver keyword.  Every compared figure is printed before it
is asserted."""
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import cstream_restatement as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build(out_dir, name, extra=()):
    assert shutil.which("g++"), "g++ builds the driver"
    exe = os.path.join(str(out_dir), name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "cstream_driver.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("cstream"), "cstream_driver")


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("cstream_san"), "cstream_driver_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def run_driver(exe, work_dir, cells, watch, chunks, form="default", short=0, expect_rc=0, n_total=None, n_rec=None):
    """cells [n][n_rec][C] int64 -> the tables (a list of dicts, with "form"), or (rc, message) of a reported error."""
    n, nr, C = cells.shape
    path = os.path.join(str(work_dir), "cells.i64")
    np.ascontiguousarray(cells, dtype=np.int64).tofile(path)
    csv = lambda v: ",".join(str(int(x)) for x in v)
    cmd = [exe, "run", str(n if n_total is None else n_total), str(nr if n_rec is None else n_rec), str(C), form, csv(watch["rows"]), csv(watch["vtypes"]),
           csv(watch["lo"]), csv(watch["bins"]), path + "@" + csv(chunks)] + ([str(short)] if short else [])
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode == 2:
        _, rc, msg = r.stdout.strip().split(" ", 2)
        assert expect_rc and int(rc) == expect_rc, r.stdout
        return int(rc), msg
    assert r.returncode == 0 and not expect_rc, (r.returncode, r.stdout, r.stderr)
    out = []
    for k, ln in enumerate(r.stdout.splitlines()):
        w = ln.split()
        assert w[0] == "row" and int(w[1]) == k and w[2] == "form" and w[4] == "below" and w[6] == "above" and w[8] == "min" and w[10] == "max" and w[12] == "counts"
        out.append(dict(form=w[3], below=int(w[5]), above=int(w[7]), min=int(w[9]), max=int(w[11]), counts=np.array([int(x) for x in w[13].split(",")], dtype=np.uint64)))
    assert len(out) == len(watch["rows"])
    return out


def test_driver_equals_the_restatement_under_every_chunking(driver, tmp_path):
    """cells [97][5][70]: an unwatched f64 row, a bool row, a usize row with K = 4, an i64 row with lo = -3, bins = 9 and values on
    both sides, a u64 row holding 2^63 + 5 with bins = 8; fed as [97], as [5, 31, 1, 60] and as 97 chunks of one."""
    cells, watch = T.mixed_input()
    want = T.tabulate(cells, **watch)
    T.show("restatement", want)
    assert want[2]["below"] > 0 and want[2]["above"] > 0 and want[3]["above"] > 0 and want[3]["max"] == 2 ** 63 + 5 and want[3]["below"] == 0
    for t in want:
        assert int(t["counts"].sum()) + t["below"] + t["above"] == 97 * 70
    first = None
    for chunks in T.CHUNKINGS:
        got = run_driver(driver, tmp_path, cells, watch, chunks)
        T.show(f"driver {len(chunks)} chunks", got)
        assert [g["form"] for g in got] == ["narrow", "narrow", "wide", "narrow"]
        assert T.same_tables(got, want)
        first = first or got
        assert T.same_tables(got, first)
    wide = run_driver(driver, tmp_path, cells, watch, [5, 31, 1, 60], form="wide")
    narrow = run_driver(driver, tmp_path, cells, watch, [5, 31, 1, 60], form="narrow")
    print("forms forced wide:", [g["form"] for g in wide], "narrow:", [g["form"] for g in narrow])
    assert [g["form"] for g in wide] == ["wide"] * 4 and [g["form"] for g in narrow] == ["narrow", "narrow", "wide", "narrow"]
    assert T.same_tables(wide, want) and T.same_tables(narrow, want)


def test_signed_and_unsigned_bounds_at_the_ends_of_the_types(driver, tmp_path):
    """An i64 row around INT64_MIN and INT64_MAX and a u64 row around 2^63: the comparison is the row's own."""
    cells = np.zeros((3, 2, 4), dtype=np.int64)
    cells[:, 0, :] = np.array([np.iinfo(np.int64).min, -1, 0, np.iinfo(np.int64).max])[None]
    cells[:, 1, :] = np.array([0, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64).view(np.int64)[None]
    for lo_i, lo_u in ((np.iinfo(np.int64).min, 0), (np.iinfo(np.int64).max - 3, 2 ** 63 - 2), (-2, 1)):
        watch = dict(rows=[0, 1], vtypes=[T.FG_I64, T.FG_U64], lo=[lo_i, lo_u], bins=[4, 4])
        want = T.tabulate(cells, **watch)
        got = run_driver(driver, tmp_path, cells, watch, [2, 1])
        T.show(f"lo {lo_i} / {lo_u} restatement", want)
        T.show(f"lo {lo_i} / {lo_u} driver", got)
        assert T.same_tables(got, want)


def test_every_refused_argument(driver, tmp_path):
    cells, watch = T.mixed_input(n=4, C=3)
    ok = run_driver(driver, tmp_path, cells, watch, [4])
    assert len(ok) == 4
    cases = {
        "n_total < 1": dict(n_total=0),
        "n_rec < 1": dict(n_rec=0),
        "a row past n_rec": dict(watch=dict(watch, rows=[1, 2, 3, 5])),
        "a negative row": dict(watch=dict(watch, rows=[-1, 2, 3, 4])),
        "a row given twice": dict(watch=dict(watch, rows=[1, 2, 2, 4])),
        "an f64 row": dict(watch=dict(watch, rows=[0, 2, 3, 4], vtypes=[T.FG_F64, T.FG_USIZE, T.FG_I64, T.FG_U64])),
        "an unknown tag": dict(watch=dict(watch, vtypes=[T.FG_BOOL, 5, T.FG_I64, T.FG_U64])),
        "a negative tag": dict(watch=dict(watch, vtypes=[T.FG_BOOL, -1, T.FG_I64, T.FG_U64])),
        "bins = 0": dict(watch=dict(watch, bins=[2, 0, 9, 8])),
        "bins = 4097": dict(watch=dict(watch, bins=[2, 4, 4097, 8])),
        "lo + bins past INT64_MAX": dict(watch=dict(watch, lo=[0, 0, 2 ** 63 - 8, 0])),
        "a negative lo on a u64 row": dict(watch=dict(watch, lo=[0, 0, -3, -1])),
    }
    for label, kw in cases.items():
        args = dict(watch=watch, chunks=[4])
        args.update(kw)
        rc, msg = run_driver(driver, tmp_path, cells, expect_rc=T.FG_E_BAD_ARG, **args)
        print(f"{label}: rc {rc}: {msg}")
        assert rc == T.FG_E_BAD_ARG
    # the last value the type holds is a legal last bin
    got = run_driver(driver, tmp_path, cells, dict(watch, lo=[0, 0, 2 ** 63 - 9, 0]), [4])
    print("lo = INT64_MAX - 8, bins = 9:", got[2]["below"], got[2]["above"])
    assert got[2]["below"] == 12 and got[2]["above"] == 0
    # n_watch outside [1, 65535]: none, and 65536 rows
    r = subprocess.run([driver, "split", "0", "64", "8"], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 2 and r.stdout.startswith(f"error {T.FG_E_BAD_ARG} ")
    r = subprocess.run([driver, "split", "65536", "64", "8"], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 2 and r.stdout.startswith(f"error {T.FG_E_BAD_ARG} ")


def test_call_order_and_the_integrity_check(driver, tmp_path):
    cells, watch = T.mixed_input()
    rc, msg = run_driver(driver, tmp_path, cells, watch, [90, 8], expect_rc=T.FG_E_STATE)
    print("past n_total:", rc, msg)
    assert rc == T.FG_E_STATE and "pass n_total" in msg
    rc, msg = run_driver(driver, tmp_path, cells, watch, [90], expect_rc=T.FG_E_STATE)
    print("before the end:", rc, msg)
    assert rc == T.FG_E_STATE and "90 of 97" in msg
    rc, msg = run_driver(driver, tmp_path, cells, watch, [0, 97], expect_rc=T.FG_E_BAD_ARG)
    print("an empty chunk:", rc, msg)
    assert rc == T.FG_E_BAD_ARG
    # the plan took 97 draws, the counters saw 96: the read-out reports it instead of a table
    rc, msg = run_driver(driver, tmp_path, cells, watch, [5, 31, 1, 60], short=1, expect_rc=T.FG_E_STATE)
    print("a short last chunk:", rc, msg)
    assert rc == T.FG_E_STATE and f"counted {96 * 70} cells where {97 * 70} arrived" in msg


@pytest.mark.parametrize("n_watch", [1, 64, 4096, 65535])
def test_launch_split_of_a_chunk_of_2_to_the_33_elements(driver, n_watch):
    """C = 2^20 chains, 2^13 draws: every launch leaves a block fewer than 2^32 elements, and the launches tile the chunk.  Pure
    arithmetic: nothing of that size is allocated."""
    C, n_chunk = 2 ** 20, 2 ** 13
    r = subprocess.run([driver, "split", str(n_watch), str(C), str(n_chunk)], capture_output=True, text=True)
    print(f"n_watch {n_watch}:", r.stdout.strip())
    assert r.returncode == 0, (r.stdout, r.stderr)
    w = r.stdout.split()
    blocks, launches, draws, most = int(w[1]), int(w[3]), int(w[5]), int(w[7])
    assert draws == n_chunk and blocks >= 1 and most < 2 ** 32
    assert launches >= -(-(n_chunk * C) // (blocks * 256 * (2 ** 24 - 1)))
    if n_watch == 65535:
        assert blocks == 1 and launches >= 3                     # one block per row: 2^33 elements cannot go in fewer


def test_one_draw_wider_than_a_launch_raises_the_block_count(driver):
    """C = 2^40 chains with one block per row would hand that block 2^40 elements of a single draw: the plan adds blocks instead."""
    r = subprocess.run([driver, "split", "65535", str(2 ** 40), "2"], capture_output=True, text=True)
    print(r.stdout.strip())
    w = r.stdout.split()
    assert r.returncode == 0 and int(w[1]) >= 2 ** 40 // (256 * (2 ** 24 - 1)) and int(w[3]) == 2 and int(w[7]) < 2 ** 32


def test_driver_under_address_and_ub_sanitizers(driver_san, tmp_path):
    """The stand-alone driver built with -fsanitize=address,undefined on the mixed input: a finding ends the run with a non-zero
    status."""
    cells, watch = T.mixed_input()
    want = T.tabulate(cells, **watch)
    for chunks in T.CHUNKINGS[:2]:
        for form in ("default", "wide"):
            got = run_driver(driver_san, tmp_path, cells, watch, chunks, form=form)
            T.show(f"sanitizers {form} {len(chunks)} chunks", got)
            assert T.same_tables(got, want)
    rc, _ = run_driver(driver_san, tmp_path, cells, watch, [5, 31, 1, 60], short=1, expect_rc=T.FG_E_STATE)
    assert rc == T.FG_E_STATE


def test_the_driver_takes_the_keyword_and_the_boundary_holds():
    """adaptive_mcmc_chain_summary accepts discrete= / discrete_bins= (default off), ChainSummary carries `discrete`, and the three
    statements of the C ABI (header, ctypes, ffi.rs) still agree -- tests/test_boundary_cpu.py's own checks, run from here."""
    from fugue_amd import engine as E
    from fugue_amd import inference as I
    from tests import test_boundary_cpu as B
    sig = inspect.signature(I.adaptive_mcmc_chain_summary)
    print("adaptive_mcmc_chain_summary:", [p for p in sig.parameters if p.startswith("discrete")])
    assert sig.parameters["discrete"].default is False and sig.parameters["discrete_bins"].default is None
    assert "discrete" in I.ChainSummary.__dataclass_fields__ and hasattr(I.DiscreteSummary, "probs")
    for name in ("fg_diag_cstream_new", "fg_diag_cstream_update", "fg_diag_cstream_count", "fg_diag_cstream_result", "fg_diag_cstream_free", "fg_diag_cells_f64"):
        assert name in E.ABI_SYMBOLS, name
    assert hasattr(E.Engine, "diag_cstream") and hasattr(E.Engine, "cells_f64")
    for name in ("update", "count", "result", "close"):
        assert hasattr(E.DiagCountStream, name), name
    B.test_library_exports_every_declared_symbol()
    B.test_rust_binding_declares_every_entry_point()
    B.test_rust_binding_and_ctypes_state_the_headers_abi()


def test_default_bins_come_from_the_program():
    from fugue_amd import engine as E
    from fugue_amd import inference as I
    from fugue_amd import model as M
    P = M.Program()
    P.sample(M.addr("b"), M.Bernoulli(0.3))
    P.sample(M.addr("c"), M.Categorical([0.2, 0.3, 0.5]))
    P.sample(M.addr("d"), M.DiscreteUniform(-2, 7))
    P.sample(M.addr("e"), M.DiscreteUniform(0, 100000))
    P.sample(M.addr("n"), M.Binomial(12, 0.5))
    P.sample(M.addr("p"), M.Poisson(2.0))
    x = P.sample(M.addr("x"), M.Normal(0.0, 1.0))
    cp = E.compile_model(P)
    got = {cp.site_names[j]: I._default_bins(cp, j) for j in range(cp.S) if cp.site_vtypes[j] != 0}
    print(got)
    assert got == {"b": (0, 2), "c": (0, 3), "d": (-2, 10), "e": (0, 4096), "n": (0, 13), "p": (0, 64)}
