"""Rank-normalised diagnostics without a GPU: the rule of fugue_amd/csrc/fg_diag_rank_plan.h through the stand-alone
tests/cpp/rank_driver.cpp (built a second time with AddressSanitizer / UBSan and run directly) against tests/rank_restatement.py and
scipy's average ranks; the normal score against mpmath; the argument codes; the ABI; the Python layer.  Every compared figure is
printed before it is asserted."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import abi_check
from tests import rank_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FG_E_BAD_ARG, FG_E_LIMIT = -3, -7
NEW = ["fg_diag_rank_words", "fg_diag_rank_transform", "fg_diag_rank_rhat_ess"]
SIZES = (1, 2, 21, 777, 9000)                      # 9 000: three radix tiles, nine run tiles


def _build(out_dir, name, extra=()):
    assert shutil.which("g++"), "g++ builds the driver"
    exe = os.path.join(str(out_dir), name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", *extra, os.path.join(ROOT, "tests", "cpp", "rank_driver.cpp"), "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("rank"), "rank_driver")


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("rank_san"), "rank_driver_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _run(exe, args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    print(r.stdout[-2000:], r.stderr[-3000:])
    return r


def _coord(exe, tmp, x, probs=(0.05, 0.95)):
    src, dst = os.path.join(str(tmp), "x.f64"), os.path.join(str(tmp), "out.f64")
    np.ascontiguousarray(x, dtype=np.float64).tofile(src)
    r = _run(exe, ["coord", src, repr(probs[0]), repr(probs[1]), dst])
    assert r.returncode == 0 and r.stdout.strip().endswith("| ok"), r.stdout
    o, S = np.fromfile(dst, dtype=np.float64), x.size
    return dict(r2=o[:S].astype(np.int64), z=o[S:2 * S], z_folded=o[2 * S:3 * S], i_lo=o[3 * S:4 * S], i_hi=o[4 * S:5 * S], median=o[5 * S], x_lo=o[5 * S + 1],
                x_hi=o[5 * S + 2], counts=o[5 * S + 3:].astype(np.int64))


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _compare(got, x, label, probs=(0.05, 0.95)):
    want = R.transform(x, probs)
    assert np.array_equal(got["r2"], want["r2"]) and np.array_equal(got["r2"], R.scipy_r2(x)), label
    assert got["r2"].min() >= 2 and got["r2"].max() <= 2 * x.size
    for name, cen in (("z", want["central"]), ("z_folded", want["central_folded"])):
        assert np.array_equal(got[name][cen].view(np.uint64), want[name][cen].view(np.uint64)), (label, name)
        rel = np.abs(got[name][~cen] - want[name][~cen]) / np.abs(want[name][~cen])
        print(f"{label} {name}: {int(cen.sum())} central cells bit-equal, {int((~cen).sum())} tail cells, largest relative difference {rel.max() if rel.size else 0.0:.3e}")
        assert (rel <= R.Z_TOL).all(), (label, name)
    assert np.array_equal(got["i_lo"], want["i_lo"]) and np.array_equal(got["i_hi"], want["i_hi"]), label
    assert _same(got["median"], want["median"]) and _same(got["x_lo"], want["x_lo"]) and _same(got["x_hi"], want["x_hi"]), label
    print(f"{label}: counts {got['counts'].tolist()} / {[want['counts'][k] for k in R.COUNT_NAMES]}")
    assert got["counts"].tolist() == [want["counts"][k] for k in R.COUNT_NAMES], label
    return want


@pytest.mark.parametrize("S", SIZES)
def test_driver_and_restatement_agree_on_every_input(driver, tmp_path, S):
    for name, x in R.inputs(S, seed=3 * S + 1).items():
        want = _compare(_coord(driver, tmp_path, x), x, f"S = {S} {name}")
        if name == "constant":
            assert want["counts"]["n_runs"] == 1 and want["counts"]["n_passes"] == 0 and (want["r2"] == S + 1).all() and (want["z"] == 0.0).all()
        if name in ("low_byte", "top_byte") and S > 2:
            assert R.passes_run(R.keys(x)) == 1, name
        if name == "tie_runs" and S == 9000:
            assert want["counts"]["longest_run"] > R.TILE
        if name == "infs":
            assert np.isfinite(want["z"]).all() and want["counts"]["n_nan"] == 0
        if name == "nans":
            assert want["counts"]["n_nan"] > 0 and (want["r2"][np.isnan(x)] == want["r2"].max()).all()


def test_driver_under_address_and_ub_sanitizers(driver_san, tmp_path):
    """the stand-alone program itself runs under the sanitizers: no Python process does"""
    for S in (1, 2, 4099):
        for name, x in R.inputs(S, seed=S).items():
            _compare(_coord(driver_san, tmp_path, x, (0.1, 0.7)), x, f"sanitized S = {S} {name}", (0.1, 0.7))
    assert _run(driver_san, ["refusals"]).returncode == 0
    x = np.r_[np.full(40, np.inf), np.arange(30.0)]                  # more than half the cells +inf: the median is +inf, the folded cells there NaN
    got = _compare(_coord(driver_san, tmp_path, x), x, "median +inf")
    assert got["median"] == np.inf and got["counts"]["n_nan_folded"] == 40 and got["counts"]["n_nan"] == 0
    for p in ((0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (0.5, 0.5)):
        _compare(_coord(driver_san, tmp_path, np.arange(10.0)[::-1], p), np.arange(10.0)[::-1], f"probs {p}", p)


def test_plan_and_refusals(driver):
    assert _run(driver, ["refusals"]).returncode == 0
    shapes = [(1, 1, 1, 0, 1), (7, 3, 2, 1, 1), (61, 200, 3, 0, 3), (97, 131, 3, 2, 1), (300, 1031, 1, 0, 1), (1000, 65536, 4, 0, 4), (200, 8192, 64, 3, 61), (32767, 65536, 1, 0, 1)]
    r = _run(driver, ["plan"] + [v for s in shapes for v in (*s, 0.05, 0.95)])
    lines = [l for l in r.stdout.splitlines() if l.startswith("plan ")]
    assert r.returncode == 0 and len(lines) == len(shapes) and all(l.endswith("| ok") for l in lines)
    for (n, C, d, j0, nj), line in zip(shapes, lines):
        got = [int(v) for v in line.split("|")[1].split()]
        S = n * C
        assert got[:6] == [0, S, R.kp(S, 0.05), R.kp(S, 0.95), -(-S // R.TILE), -(-S // R.RUN_TILE)], line
        assert got[7] == max(1, min(d, 65535 // 4, (1 << 30) // (32 * S))), line


def _mp_truth(r2, S):
    import mpmath as mp
    p = mp.mpf(4 * int(r2) - 3) / mp.mpf(8 * S + 2)
    return mp.sqrt(2) * mp.erfinv(2 * p - 1)


def test_normal_score_against_mpmath_and_its_antisymmetry(driver, tmp_path):
    """z = ndtri((r - 3/8) / (S + 1/4)) against mpmath's inverse normal CDF at 50 digits, over every doubled rank up to the centre of
    S = 1, 2, 21, 4 096 (the upper half is the exact negative, asserted here for the restatement and inside the driver for the rule) and
    the 2 000 ranks of `rank_restatement.big_ranks` over S = 2^31 - 1.

    Measured: the restatement's largest relative deviation is 5.90e-16 (S = 4 096; 5.66e-16 at S = 2^31 - 1).  The tolerance of every
    tail comparison, here and on the device, is four times that: rank_restatement.Z_TOL = 2.36e-15."""
    import mpmath as mp
    mp.mp.dps = 50
    worst = {"restatement": 0.0, "driver": 0.0}
    for S in (1, 2, 21, 4096, 2 ** 31 - 1):
        r2 = np.arange(2, S + 2) if S < 2 ** 30 else R.big_ranks(S)
        src, dst = os.path.join(str(tmp_path), "r2.i64"), os.path.join(str(tmp_path), "z.f64")
        r2.astype(np.int64).tofile(src)
        r = _run(driver, ["z", S, src, dst])                         # the driver checks z(r2) == -z(2 S + 2 - r2) bit for bit
        assert r.returncode == 0 and r.stdout.strip().endswith("| ok")
        zs = {"restatement": R.z_of(r2, S), "driver": np.fromfile(dst, dtype=np.float64)}
        mirror = R.z_of(2 * S + 2 - r2, S)
        assert np.array_equal((-zs["restatement"]).view(np.uint64)[r2 != S + 1], mirror.view(np.uint64)[r2 != S + 1]) and (mirror[r2 == S + 1] == 0.0).all()
        cen = R.central(r2, S)
        assert np.array_equal(zs["restatement"][cen].view(np.uint64), zs["driver"][cen].view(np.uint64))
        truth = [_mp_truth(a, S) for a in r2]
        for who, z in zs.items():
            dev = max(float(abs(mp.mpf(float(b)) - t) / abs(t)) if t != 0 else abs(float(b)) for b, t in zip(z, truth))
            print(f"S = {S}: {r2.size} ranks, {who}: largest relative deviation from mpmath {dev:.4e}")
            worst[who] = max(worst[who], dev)
    print("largest:", worst, "measured", R.Z_MEASURED_DEV, "tolerance", R.Z_TOL)
    assert worst["restatement"] <= R.Z_MEASURED_DEV                  # the recorded measurement still stands ...
    assert worst["driver"] <= R.Z_TOL                                # ... and the rule in C++ is within four times it


def test_argument_codes_need_no_device():
    """every argument is checked before the engine and the device are looked at; FG_E_LIMIT needs the engine's chain count and is
    checked where it is decided, in fg_rank_plan through the driver (test_plan_and_refusals)"""
    from fugue_amd import engine as E
    import ctypes as C
    L = E.lib()
    assert L.fg_diag_rank_words() == len(R.WORD_NAMES) == len(E.RANK_WORD_NAMES) and E.RANK_COUNTS == len(R.COUNT_NAMES) and E.RANK_ROWS == 4
    assert tuple(E.RANK_WORD_NAMES) == R.WORD_NAMES and tuple(E.RANK_COUNT_NAMES) == R.COUNT_NAMES
    words, med, counts = np.zeros(10), np.zeros(1), np.zeros(8, dtype=np.int64)
    cp = counts.ctypes.data_as(C.POINTER(C.c_int64))
    fig = lambda draws=8, n=4, d=1, lo=0.05, hi=0.95, mob=0, w=E._dp(words), c=cp: L.fg_diag_rank_rhat_ess(None, draws, n, d, lo, hi, mob, w, c)
    tr = lambda draws=8, n=4, d=2, j0=0, nj=1, lo=0.05, hi=0.95, out=8, m=E._dp(med), c=cp: L.fg_diag_rank_transform(None, draws, n, d, j0, nj, lo, hi, out, None, m, c)
    cases = [(fig(), "null engine"), (fig(draws=None), "null"), (fig(w=None), "null"), (fig(c=None), "null"), (fig(n=0), "n must"), (fig(d=0), "d outside"), (fig(d=65536), "d outside"),
             (fig(lo=-0.5), "probabilities"), (fig(hi=1.5), "probabilities"), (fig(lo=0.7, hi=0.2), "probabilities"), (fig(lo=float("nan")), "probabilities"), (fig(mob=-1), "max_out_bytes"),
             (tr(), "null engine"), (tr(out=None), "null"), (tr(m=None), "null"), (tr(c=None), "null"), (tr(n=-3), "n must"), (tr(d=0), "d outside"), (tr(j0=2), "block"), (tr(j0=-1), "block"),
             (tr(nj=0), "block"), (tr(j0=1, nj=2), "block"), (tr(hi=2.0), "probabilities")]
    for rc, _ in cases:
        assert rc == FG_E_BAD_ARG
    for call, word in ((lambda: fig(n=0), "n must"), (lambda: tr(j0=2), "block"), (lambda: fig(), "null engine"), (lambda: fig(lo=0.7, hi=0.2), "probabilities"), (lambda: fig(mob=-1), "max_out_bytes")):
        assert call() == FG_E_BAD_ARG and word in E.last_error(), (word, E.last_error())


def test_abi_check_passes_with_the_new_entries():
    from fugue_amd import engine as E
    header = open(os.path.join(ROOT, "include", "fugue_amd.h")).read()
    rust = open(os.path.join(ROOT, "rust", "fugue-gpu", "src", "ffi.rs")).read()
    H, Rs = abi_check.parse_header(header), abi_check.parse_rust(rust)
    for f in NEW:
        assert f in H["fns"] and f in Rs["fns"] and f in E.ABI_SYMBOLS, f
    assert abi_check.compare_header_rust(header, rust) == []
    assert abi_check.compare_header_ctypes(header, E.lib()) == []
    assert "#define FG_RANK_ROWS 4" in header and "#define FG_RANK_WORDS 10" in header and "#define FG_RANK_COUNTS 8" in header


def test_the_figures_see_what_the_plain_ones_miss():
    """the restatement on the issue's construction: half the chains with three times the scale leave the plain split R-hat near 1 and
    raise the folded one; a column with one +inf and one -inf has NaN plain figures and finite rank figures"""
    from oracle import oracle as orc
    rng = np.random.default_rng(77)
    n, C = 200, 16
    x = rng.normal(size=(n, 1, C))
    x[:, 0, :C // 2] *= 3.0
    t = R.coordinate(x, 0)
    plain = orc.split_rhat(np.ascontiguousarray(x[:, 0, :].T))
    print("plain split R-hat", plain, "rank figures", t["figures"])
    assert plain < 1.01 and t["figures"]["rhat_folded"] > 1.05 and t["figures"]["rhat_rank"] == t["figures"]["rhat_folded"] and t["figures"]["ess_tail"] < t["figures"]["ess_bulk"]
    y = rng.normal(size=(n, 1, C))
    y[3, 0, 2], y[9, 0, 5] = np.inf, -np.inf
    t = R.coordinate(y, 0)
    print("with +-inf:", orc.split_rhat(np.ascontiguousarray(y[:, 0, :].T)), t["figures"])
    assert math.isnan(orc.split_rhat(np.ascontiguousarray(y[:, 0, :].T))) and all(math.isfinite(v) for v in t["figures"].values())


def test_python_layer_without_a_device():
    import fugue_amd as F
    from fugue_amd import diagnostics as D
    z = np.zeros(2)
    rd = D.RankDiagnostics(names=["a", "b"], n_draws=100, rhat_rank=np.array([1.0, 1.2]), rhat_bulk=z, rhat_folded=z, ess_bulk=z, ess_tail=z, ess_lower=z, ess_upper=z, median=z,
                           x_lo=z, x_hi=z, counts={k: np.zeros(2, dtype=np.int64) for k in R.COUNT_NAMES})
    assert rd.d == 2 and rd.of("b")["rhat_rank"] == 1.2 and set(rd.of("a")) == set(R.WORD_NAMES)
    assert F.RankDiagnostics is D.RankDiagnostics and F.rank_diagnostics is D.rank_diagnostics and F.ess_bulk is D.ess_bulk and F.ess_tail is D.ess_tail and F.rank_r_hat_f64 is D.rank_r_hat_f64
    with pytest.raises(ValueError, match=r"\[n\]\[d\]\[C\]"):
        D.rank_diagnostics(np.zeros((3, 4)))
    with pytest.raises(KeyError):
        rd.of("c")
