"""The streamed quantile selection on the host: tests/cpp/qstream_driver.cpp (fg_diag_qstream_plan.h, the planner the device code
calls, with host loops in place of the kernels) == tests/qstream_restatement.py == a sort by key, bit for bit and with equal pass
counts, on every slot of every input; the integrity error; independence of chunking and chain order; the same driver under
AddressSanitizer / UBSan (a stand-alone binary).  Every compared figure is printed before it is asserted."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import qstream_restatement as Q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FG_E_BAD_ARG, FG_E_STATE = -3, -5


def _build(out_dir, name, extra=()):
    assert shutil.which("g++"), "g++ builds the driver"
    exe = os.path.join(str(out_dir), name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", *extra, os.path.join(ROOT, "tests", "cpp", "qstream_driver.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("qstream"), "qstream_driver")


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("qstream_san"), "qstream_driver_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def run_driver(exe, work_dir, passes, probs, digit_bits, capacity, expect_rc=0):
    """passes: [(x [n][d][C], chunk lengths)], one per pass (the last again when more follow) ->
    (values [d][np] as uint64 bits, slot passes [d][np], passes), or (rc, message) of a reported error."""
    n, d, C = passes[0][0].shape
    specs = []
    for k, (x, chunks) in enumerate(passes):
        assert x.shape == (n, d, C) and sum(chunks) == n
        path = os.path.join(str(work_dir), f"pass{k}.f64")
        np.ascontiguousarray(x, dtype=np.float64).tofile(path)
        specs.append(path + "@" + ",".join(str(c) for c in chunks))
    r = subprocess.run([exe, str(n), str(d), str(C), str(digit_bits), str(capacity), ",".join(repr(float(p)) for p in probs)] + specs,
                       capture_output=True, text=True)
    if r.returncode == 2:
        _, rc, msg = r.stdout.strip().split(" ", 2)
        assert expect_rc and int(rc) == expect_rc, r.stdout
        return int(rc), msg
    assert r.returncode == 0 and not expect_rc, (r.returncode, r.stdout, r.stderr)
    vals, sp = np.zeros((d, len(probs)), dtype=np.uint64), np.zeros((d, len(probs)), dtype=np.int32)
    lines = r.stdout.splitlines()
    assert len(lines) == d * len(probs) + 1
    for ln in lines[:-1]:
        _, i, q, hexbits, p = ln.split()
        vals[int(i), int(q)], sp[int(i), int(q)] = int(hexbits, 16), int(p)
    return vals, sp, int(lines[-1].split()[1])


def check_all(label, exe, work_dir, x, probs, digit_bits, capacity, chunks=None):
    """driver == restatement == key sort on every slot of x, with the restatement's pass counts; returns the slot passes."""
    want, want_sp, want_passes = Q.select_all(x, probs, digit_bits, capacity)
    ref = Q.reference_all(x, probs)
    got, got_sp, got_passes = run_driver(exe, work_dir, [(x, chunks or [x.shape[0]])], probs, digit_bits, capacity)
    for i in range(x.shape[1]):
        for q, p in enumerate(probs):
            print(f"{label} bits {digit_bits} cap {capacity} [{i}] p={p}: driver {int(got[i, q]):016x} ({got_sp[i, q]} passes) "
                  f"restatement {int(Q.bits(want)[i, q]):016x} ({want_sp[i, q]}) sort {int(Q.bits(ref)[i, q]):016x}")
    print(f"{label}: passes driver {got_passes} restatement {want_passes}")
    assert np.array_equal(Q.bits(want), Q.bits(ref))
    assert np.array_equal(got, Q.bits(ref))
    assert np.array_equal(got_sp, want_sp) and got_passes == want_passes
    return want_sp


NORMAL_SETTINGS = [(12, 0), (12, 8), (12, 7000), (5, 0)]


@pytest.mark.parametrize("digit_bits,capacity", NORMAL_SETTINGS)
def test_normal_draws(driver, tmp_path, digit_bits, capacity):
    """97 x 3 x 70 N(0, 1) draws, the five default probabilities, fed as [5, 31, 1, 60]."""
    check_all("normal", driver, tmp_path, Q.normal_input(), Q.DEFAULT_PROBS, digit_bits, capacity, [5, 31, 1, 60])


@pytest.mark.parametrize("capacity", [0, 8, 500])
def test_values_that_differ_in_the_last_four_bits(driver, tmp_path, capacity):
    """1 + k 2^-52: no 12-bit digit before the last four bits separates the values, and min != max throughout."""
    check_all("last bits", driver, tmp_path, Q.last_bits_column()[:, None, :], Q.DEFAULT_PROBS, 12, capacity)


@pytest.mark.parametrize("capacity", [0, 8, 7000])
def test_constant_column(driver, tmp_path, capacity):
    check_all("constant", driver, tmp_path, Q.constant_column()[:, None, :], Q.DEFAULT_PROBS, 12, capacity)


@pytest.mark.parametrize("digit_bits,capacity", [(12, 0), (12, 8), (12, 7000), (5, 0), (1, 40)])
def test_special_values(driver, tmp_path, digit_bits, capacity):
    """-inf, -1.5, -0.0, +0.0, +-5e-324, 1, 1 + 2^-52, +inf, NaN with the eight probabilities that include 0 and 1."""
    check_all("specials", driver, tmp_path, Q.specials_column()[:, None, :], Q.PROBS8, digit_bits, capacity, [40, 57])


@pytest.mark.parametrize("value", [0.0, -0.0, np.nan, -3.25, np.inf])
@pytest.mark.parametrize("capacity", [0, 1])
def test_a_single_element(driver, tmp_path, value, capacity):
    check_all("len 1", driver, tmp_path, np.full((1, 1, 1), value), Q.PROBS8, 12, capacity)


def test_all_three_adversarial_columns_in_one_stream(driver, tmp_path):
    """d = 3 with different pass counts per coordinate: a finished coordinate stays finished while the others go on."""
    for C in (70, 65):
        for capacity in (0, 8):
            check_all(f"adversarial C={C}", driver, tmp_path, Q.adversarial_input(C), Q.PROBS8, 12, capacity)


def test_a_replay_that_differs_by_one_element_is_reported(driver, tmp_path):
    """The second pass differs from the first by one element of a live bucket (the median's): FG_E_STATE, no quantile.  The
    restatement raises on the same input."""
    x = Q.normal_input()
    y = x.copy()
    med = Q.reference(x[:, 0, :], (0.5,))[0]
    t, c = np.argwhere(x[:, 0, :] == med)[0]
    y[t, 0, c] = 1e300                               # leaves the median's 12-bit bucket
    for capacity in (0, 8, 1000):
        with pytest.raises(Q.ReplayDiverged):
            Q.select(x[:, 0, :], Q.DEFAULT_PROBS, 12, capacity, replays=[y[:, 0, :]])
        rc, msg = run_driver(driver, tmp_path, [(x, [97]), (y, [97])], Q.DEFAULT_PROBS, 12, capacity, expect_rc=FG_E_STATE)
        print(f"cap {capacity}: rc {rc}: {msg}")
        assert rc == FG_E_STATE and "did not reproduce the previous one" in msg


def test_later_passes_in_another_chunking_or_chain_order_change_nothing(driver, tmp_path):
    x = Q.normal_input()
    perm = np.random.default_rng(3).permutation(x.shape[2])
    for digit_bits, capacity in NORMAL_SETTINGS:
        base = run_driver(driver, tmp_path, [(x, [97])], Q.DEFAULT_PROBS, digit_bits, capacity)
        for label, passes in (("chunking", [(x, [97]), (x, [5, 31, 1, 60]), (x, [1] * 97)]),
                              ("chains permuted", [(x, [97]), (x[:, :, perm], [50, 47])])):
            got = run_driver(driver, tmp_path, passes, Q.DEFAULT_PROBS, digit_bits, capacity)
            print(f"bits {digit_bits} cap {capacity} {label}: equal values {np.array_equal(got[0], base[0])}, passes {got[2]} / {base[2]}")
            assert np.array_equal(got[0], base[0]) and np.array_equal(got[1], base[1]) and got[2] == base[2]


def test_protocol_errors_of_the_planner(driver, tmp_path):
    x = Q.normal_input()
    bad = [dict(probs=(1.5,)), dict(probs=(float("nan"),)), dict(probs=(-0.1,)), dict(digit_bits=0), dict(digit_bits=13), dict(capacity=-1),
           dict(probs=tuple([0.5] * 9))]
    for kw in bad:
        args = dict(probs=Q.DEFAULT_PROBS, digit_bits=12, capacity=8)
        args.update(kw)
        rc, msg = run_driver(driver, tmp_path, [(x, [97])], expect_rc=FG_E_BAD_ARG, **args)
        print(kw, rc, msg)
        assert rc == FG_E_BAD_ARG
    # a chunk past n_total; end_pass before n_total draws (the driver ends the pass after the listed chunks)
    r = subprocess.run([driver, "97", "3", "70", "12", "8", "0.5", os.path.join(str(tmp_path), "pass0.f64") + "@90,8"], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 2 and r.stdout.startswith(f"error {FG_E_STATE} ") and "pass n_total" in r.stdout
    r = subprocess.run([driver, "97", "3", "70", "12", "8", "0.5", os.path.join(str(tmp_path), "pass0.f64") + "@90"], capture_output=True, text=True)
    print(r.stdout.strip())
    assert r.returncode == 2 and r.stdout.startswith(f"error {FG_E_STATE} ") and "90 of 97" in r.stdout


def test_driver_under_address_and_ub_sanitizers(driver_san, tmp_path):
    """The stand-alone driver built with -fsanitize=address,undefined: the normal and the specials input, every setting; a finding
    ends the run with a non-zero status."""
    for digit_bits, capacity in NORMAL_SETTINGS:
        check_all("normal (sanitizers)", driver_san, tmp_path, Q.normal_input(), Q.DEFAULT_PROBS, digit_bits, capacity, [5, 31, 1, 60])
    for digit_bits, capacity in [(12, 0), (12, 8), (5, 0)]:
        check_all("specials (sanitizers)", driver_san, tmp_path, Q.specials_column()[:, None, :], Q.PROBS8, digit_bits, capacity)
