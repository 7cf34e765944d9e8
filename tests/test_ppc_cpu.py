"""The posterior predictive check stream without a GPU: tests/cpp/ppc_stream_driver.cpp (fg_ppc_stream_plan.h's statistics, update,
merge and finish functions, pieces, launch cuts and tree schedule, with host loops for the kernels) against the Python restatement,
bit for bit in every state word, T_obs, the pooled counters and the pooled mean / ssd, over several chunkings and under
AddressSanitizer / UBSan (a stand-alone binary); the restatement against numpy on integer-valued cells (exactly) and on f64 rows
(within DESIGN 3.5's conditioning of the pivoted sums); the ABI of the new entry points and every FG_E_BAD_ARG / FG_E_STATE case of
the plan; fg_program_observe_value.  Every compared figure is printed before it is asserted."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import abi_check
from tests import ppc_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FG_E_BAD_ARG, FG_E_STATE = -3, -5
EPS = 2.0 ** -52
CS, KS, NS = (1, 2, 3, 64, 65), (1, 2, 3, 8), (1, 2, 9, 40)
NEW = ["fg_ppc_stream_new", "fg_ppc_stream_update", "fg_ppc_stream_count", "fg_ppc_stream_n_slots", "fg_ppc_stream_observed", "fg_ppc_stream_pooled",
       "fg_ppc_stream_chains", "fg_ppc_stream_free", "fg_program_observe_value"]


def _build(out_dir, name, extra=()):
    assert shutil.which("g++"), "g++ builds the driver"
    exe = os.path.join(str(out_dir), name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-ffp-contract=off", *extra, os.path.join(ROOT, "tests", "cpp", "ppc_stream_driver.cpp"), "-o", exe],
                   check=True)
    return exe


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("ppcstream"), "ppc_stream_driver")


@pytest.fixture(scope="module")
def driver_san(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("ppcstream_san"), "ppc_stream_driver_san", ("-fsanitize=address,undefined", "-fno-sanitize-recover=all"))


def _write_spec(path, vtypes, offsets, members, masks, observed):
    with open(path, "w") as f:
        for lst in (vtypes, offsets, members, masks):
            f.write(" ".join(str(int(v)) for v in lst) + "\n")
        f.write(" ".join(f"{R.bits(v):016x}" for v in observed) + "\n")


def _csr(checks):
    offsets, members, masks, observed = [0], [], [], []
    for rows, mask, obs in checks:
        members += list(rows)
        observed += list(obs)
        offsets.append(len(members))
        masks.append(mask)
    return offsets, members, masks, observed


def run_driver(exe, work_dir, x, vtypes, checks, chunks, grid=(), expect_rc=0, raw=None, n_total=None):
    """x uint64 [n][n_rows][C] -> dict(t_obs bits, state words [6][n_slots][C], counts, moment bits, shape), or (rc, message).  `raw`: the
    four lists and the observed values as given (for lists the plan must refuse)."""
    n, n_rows, C = x.shape
    table, spec = os.path.join(str(work_dir), "table.u64"), os.path.join(str(work_dir), "spec.txt")
    np.ascontiguousarray(x, dtype=np.uint64).tofile(table)
    offsets, members, masks, observed = raw if raw is not None else _csr(checks)
    _write_spec(spec, vtypes, offsets, members, masks, observed)
    r = subprocess.run([exe, str(n if n_total is None else n_total), str(n_rows), str(C), spec, table, ",".join(str(c) for c in chunks)] + [str(g) for g in grid],
                       capture_output=True, text=True)
    if r.returncode == 2:
        _, rc, msg = r.stdout.strip().split(" ", 2)
        assert expect_rc and int(rc) == expect_rc, r.stdout
        return int(rc), msg
    assert r.returncode == 0 and not expect_rc, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    t_obs, state, counts, moments, shape = {}, {}, {}, {}, None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "tobs":
            t_obs[int(w[1])] = int(w[2], 16)
        elif w[0] == "state":
            state[(int(w[2]), int(w[1]))] = [int(v, 16) for v in w[3:]]
        elif w[0] == "pooled":
            counts[int(w[1])] = [int(v) for v in w[2:7]]
            moments[int(w[1])] = [int(v, 16) for v in w[7:9]]
        elif w[0] == "launches":
            shape = tuple(int(w[i]) for i in (1, 3, 5, 7, 9))
    n_slots = len(t_obs)
    return dict(t_obs=[t_obs[k] for k in range(n_slots)], state=[[state[(w, k)] for k in range(n_slots)] for w in range(R.WORDS)],
                counts=[counts[k] for k in range(n_slots)], moments=[moments[k] for k in range(n_slots)], shape=shape)


def chunkings(n):
    out = [(n,), (1,) * n]
    if n > 8:
        out.append((1, 7, n - 8))
    return out


def check_driver(exe, tmp_path, x, vtypes, checks, label, grid=(), labels=None):
    want = R.stream(x, vtypes, checks)
    slots = R.slots_of(checks)
    w_tobs = [R.bits(v) for v in want["t_obs"]]
    w_mom = [[R.bits(v) for v in m] for m in want["moments"]]
    shape = None
    for chunks in chunkings(x.shape[0]):
        got = run_driver(exe, tmp_path, x, vtypes, checks, chunks, grid)
        shape = got["shape"]
        same_state = got["state"] == want["state"]
        for k, (q, st) in enumerate(slots):
            ok = got["t_obs"][k] == w_tobs[k] and got["counts"][k] == want["counts"][k] and got["moments"][k] == w_mom[k]
            if not ok or len(chunks) == 1:
                print(f"{label} chunks {chunks if len(chunks) < 4 else '(1,)*n'} {labels[q] if labels else q}.{R.STAT_NAMES[st]}: T_obs {want['t_obs'][k]!r} equal "
                      f"{got['t_obs'][k] == w_tobs[k]}, counts {got['counts'][k]} / {want['counts'][k]}, mean ssd {want['moments'][k]} equal {got['moments'][k] == w_mom[k]}")
            assert ok
        print(f"{label} chunks {chunks if len(chunks) < 4 else '(1,)*n'}: all {R.WORDS} x {len(slots)} x {x.shape[2]} state words equal {same_state}")
        assert same_state
    return shape, want


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("C", CS)
def test_driver_equals_the_restatement_bit_for_bit(driver, tmp_path, C, K):
    """Every row kind and check of ppc_restatement.standard_checks at n in {1, 2, 9, 40}, chunkings (n,), (1,) * n, (1, 7, n - 8)."""
    kinds, checks, labels = R.standard_checks(K, seed=C)
    for n in NS:
        x, vtypes = R.table(kinds, n, C, seed=C + n)
        _, want = check_driver(driver, tmp_path, x, vtypes, checks, f"C {C} K {K} n {n}", labels=labels)
        slots = R.slots_of(checks)
        N = n * C
        for k, (q, st) in enumerate(slots):
            lt, eq, gt, nan, fin = want["counts"][k]
            assert lt + eq + gt + nan == N
            if labels[q] == "constant" and (st != R.VAR or K > 1):
                assert eq == N, (labels[q], st)
            if labels[q] == "obs_nan" or (len(checks[q][0]) == 1 and st == R.VAR):
                assert nan == N, (labels[q], st)
            if labels[q] == "obs_nan" and st != R.VAR:
                assert fin == N                                   # the moments of the replicated statistic do not depend on the data


def test_the_conversion_rounds_at_and_above_2_to_the_53(driver, tmp_path):
    """u64 cells 2^53 + 1 (a tie, to even: 2^53), 2^53 + 3 (a tie: 2^53 + 4), 2^64 - 1 (2^64); i64 cells -2^63 and -(2^53 + 1); a bool."""
    cells = [2 ** 53 + 1, 2 ** 53 + 3, 2 ** 64 - 1, 2 ** 63, (1 << 64) - (2 ** 53 + 1), 1]
    vts = [R.U64, R.U64, R.U64, R.I64, R.I64, R.BOOL]
    want = [2.0 ** 53, 2.0 ** 53 + 4, 2.0 ** 64, -2.0 ** 63, -2.0 ** 53, 1.0]
    got = [R.cell(u, vt) for u, vt in zip(cells, vts)]
    print(got, want)
    assert got == want
    x = np.array(cells, dtype=np.uint64).reshape(1, 6, 1)
    checks = [([r], 1 << R.MEAN, [want[r]]) for r in range(6)]
    check_driver(driver, tmp_path, x, vts, checks, "conversion")
    assert [c[1] for c in R.stream(x, vts, checks)["counts"]] == [1] * 6          # every converted cell equals the double written by hand


def test_launch_cuts_and_slices_change_nothing(driver, tmp_path):
    """Grid limits of 1 block along the chains and 2 along y: more launches, the same bits (the restatement knows no launch).  C = 600
    spans three blocks of a tree level, so the tree has two levels; n = 40 is three pieces of at most 16 draws."""
    kinds, checks, labels = R.standard_checks(2, seed=5)
    x, vtypes = R.table(kinds, 40, 600, seed=5)
    checks = checks[:3] + checks[5:6]
    n_slots = len(R.slots_of(checks))
    base, _ = check_driver(driver, tmp_path, x, vtypes, checks, "default grid")
    cut, _ = check_driver(driver, tmp_path, x, vtypes, checks, "cut grid", grid=(1, 2))
    print("launches, levels, slices, statistics launches, update launches (the last chunking, (1, 7, 32)):", base, cut)
    assert n_slots == 17
    assert base == (1, 2, 1, 4, 4)                                # pieces 1, 7, 16, 16
    pairs = lambda n: math.ceil(n * len(checks) / 2)
    assert cut == (3, 2, 9, 3 * (pairs(1) + pairs(7) + 2 * pairs(16)), 3 * 9 * 4)


def test_a_tree_of_three_levels(driver, tmp_path):
    """C = 65 537 chains: 65 537 -> 257 -> 2 -> 1, the last block of every level partial.  One check of one N(0, 1) member, its mean,
    one draw, the default grid."""
    x, vtypes = R.table(["normal"], 1, 65537, seed=3)
    shape, want = check_driver(driver, tmp_path, x, vtypes, [([0], 1 << R.MEAN, [0.25])], "C 65537")
    print("launches, levels, slices, statistics launches, update launches:", shape, "counts", want["counts"])
    assert shape == (1, 3, 1, 1, 1) and sum(want["counts"][0][:4]) == 65537 and want["counts"][0][4] == 65537


def test_driver_under_address_and_ub_sanitizers(driver_san, tmp_path):
    for C, K in ((1, 1), (3, 3), (65, 8)):
        kinds, checks, labels = R.standard_checks(K, seed=C)
        x, vtypes = R.table(kinds, 23, C, seed=C)
        check_driver(driver_san, tmp_path, x, vtypes, checks, f"sanitizers C {C} K {K}", labels=labels)
    kinds, checks, labels = R.standard_checks(2, seed=1)
    x, vtypes = R.table(kinds, 9, 600, seed=1)
    check_driver(driver_san, tmp_path, x, vtypes, checks[:4], "sanitizers C 600, cut", grid=(1, 2))


def test_protocol_errors_of_the_plan(driver, tmp_path):
    """Every FG_E_BAD_ARG case of fg_ppc_stream_new and the FG_E_STATE cases of update and read-out, none of which needs a device."""
    x, vtypes = R.table(["normal", "bernoulli", "normal"], 10, 3)
    good = ([0, 2, 3], [0, 1, 2], [R.ALL, 1], [0.5, 1.0, 0.25])
    bad = {
        "an empty check": ([0, 2, 2], [0, 1], [R.ALL, 1], [0.5, 1.0]),
        "an empty mask": ([0, 2, 3], [0, 1, 2], [R.ALL, 0], [0.5, 1.0, 0.25]),
        "a mask bit >= 5": ([0, 2, 3], [0, 1, 2], [R.ALL, 32], [0.5, 1.0, 0.25]),
        "a negative mask": ([0, 2, 3], [0, 1, 2], [R.ALL, -1], [0.5, 1.0, 0.25]),
        "a member past the rows": ([0, 2, 3], [0, 3, 2], [R.ALL, 1], [0.5, 1.0, 0.25]),
        "a negative member": ([0, 2, 3], [0, -1, 2], [R.ALL, 1], [0.5, 1.0, 0.25]),
        "non-monotone offsets": ([0, 2, 1], [0, 1, 2], [R.ALL, 1], [0.5, 1.0, 0.25]),
        "offsets that do not start at 0": ([1, 2, 3], [0, 1, 2], [R.ALL, 1], [0.5, 1.0, 0.25]),
    }
    for what, raw in bad.items():
        rc, msg = run_driver(driver, tmp_path, x, vtypes, None, (10,), expect_rc=FG_E_BAD_ARG, raw=raw)
        print(what, "->", rc, msg)
        assert msg.startswith("fg_ppc_stream_new: ")
    rc, msg = run_driver(driver, tmp_path, x, [R.F64, 7, R.F64], None, (10,), expect_rc=FG_E_BAD_ARG, raw=good)
    print("an unknown value type ->", rc, msg)
    assert "value type 7" in msg
    rc, msg = run_driver(driver, tmp_path, x, vtypes, None, (1,), expect_rc=FG_E_BAD_ARG, raw=good, n_total=0)
    print("n_total < 1 ->", rc, msg)
    assert "n_total < 1" in msg
    rc, msg = run_driver(driver, tmp_path, x, vtypes, None, (9, 2), expect_rc=FG_E_STATE, raw=good)
    print(rc, msg)
    assert "pass n_total" in msg
    rc, msg = run_driver(driver, tmp_path, x, vtypes, None, (4, 0, 5), expect_rc=FG_E_STATE, raw=good)
    print(rc, msg)
    assert "9 of 10" in msg
    rc, msg = run_driver(driver, tmp_path, x, vtypes, None, (4, -1, 6), expect_rc=FG_E_BAD_ARG, raw=good)
    print(rc, msg)
    a = run_driver(driver, tmp_path, x, vtypes, None, (4, 0, 6), raw=good)        # an empty chunk is a no-op
    b = run_driver(driver, tmp_path, x, vtypes, None, (10,), raw=good)
    assert a["state"] == b["state"] and a["counts"] == b["counts"] and a["moments"] == b["moments"]


# ---- the restatement against independent arithmetic ---------------------------------------------------------------------------------
@pytest.mark.parametrize("C", CS)
def test_integer_valued_cells_match_numpy_reductions_exactly(C):
    """Bernoulli and small negative i64 cells: every in-order sum is exact, so numpy's sum / mean / min / max of the converted cells are
    the statistics, and the counters are plain comparisons against the statistic of the observed vector."""
    n, K = 23, 5
    x, vtypes = R.table(["bernoulli"] * K + ["neg_i64"] * K, n, C, seed=C)
    mask = (1 << R.MEAN) | (1 << R.MIN) | (1 << R.MAX) | (1 << R.SUM)
    obs = ([1.0, 0.0, 1.0, 1.0, 0.0], [-2.0, 1.0, -5.0, 0.0, -2.0])
    checks = [(list(range(K)), mask, obs[0]), (list(range(K, 2 * K)), mask, obs[1])]
    got = R.stream(x, vtypes, checks)
    vals = x.view(np.int64).astype(np.float64)                     # [n][2 K][C], exact
    k = 0
    for q in range(2):
        cells, y = vals[:, q * K:(q + 1) * K, :], np.array(obs[q])
        for name, f in (("mean", np.mean), ("min", np.min), ("max", np.max), ("sum", np.sum)):
            T, t_obs = f(cells, axis=1), float(f(y))
            want = [int((T < t_obs).sum()), int((T == t_obs).sum()), int((T > t_obs).sum()), 0, n * C]
            print(f"C {C} check {q} {name}: T_obs {got['t_obs'][k]!r} / {t_obs!r}, counts {got['counts'][k]} / {want}")
            assert got["t_obs"][k] == t_obs and got["counts"][k] == want
            per_chain = [(T < t_obs).sum(axis=0).tolist(), (T == t_obs).sum(axis=0).tolist(), (T > t_obs).sum(axis=0).tolist()]
            assert got["chains"][k][:3] == per_chain
            k += 1


def _moments_against_numpy(kind, C, extra):
    """t_rep_mean / t_rep_sd of a marginal check (K = 1: T is the cell) and of the mean of 3 rows of `kind`, n = 23, against numpy's
    two-pass mean and variance of the same T values.  The bounds are DESIGN 3.5's for the pivoted sums: they lose about
    (1 + mu^2 / var) 2^-53 relative per operation, mu measured from the pivot, so over the N terms of a sequential sum the variance is
    relative within (N + 8) 2^-52 (1 + mu^2 / var) and the mean absolute within (N + 8) 2^-52 max|T - pivot| -- the bounds the
    log-likelihood stream's moments are held to.  `extra(T, N, C, var)` -> (absolute term on the mean, relative term on the variance)
    added to them: (0, 0) for the rows the stream is specified on."""
    n = 23
    x, vtypes = R.table([kind] * 3, n, C, seed=C)
    checks = [([0], 1 << R.MEAN, [0.0]), ([0, 1, 2], 1 << R.MEAN, [0.0, 0.0, 0.0])]
    got = R.stream(x, vtypes, checks)
    N = n * C
    bound = (N + 8) * EPS
    for k in range(2):
        T = np.array(got["T"], dtype=np.float64)[:, k, :]
        mean, ssd = got["moments"][k]
        assert got["counts"][k][4] == N
        pivot = float(T[0, 0])
        w_mean, w_var = float(np.mean(T)), float(np.var(T, ddof=1)) if N > 1 else 0.0
        more_mean, more_var = extra(T, N, C, w_var)
        mean_bound = bound * float(np.max(np.abs(T - pivot))) + more_mean
        print(f"{kind} C {C} slot {k}: mean {mean!r} numpy {w_mean!r} err {abs(mean - w_mean):.3e} bound {mean_bound:.3e}")
        assert abs(mean - w_mean) <= mean_bound
        if N > 1:
            sd = math.sqrt(ssd / (N - 1))
            if w_var == 0.0:
                print(f"  sd {sd!r}, exact 0")
                assert sd == 0.0
            else:
                mu = w_mean - pivot
                rel_bound = bound * (1.0 + mu * mu / w_var) + more_var
                rel = abs(ssd / (N - 1) - w_var) / w_var
                print(f"  sd {sd!r} numpy {math.sqrt(w_var)!r}: rel err of the variance {rel:.3e} bound {rel_bound:.3e}")
                assert rel <= rel_bound
        else:
            assert ssd == 0.0 and math.copysign(1.0, ssd) == 1.0    # n_fin = 1: ssd = +0.0


@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("kind", ("normal", "constant"))
def test_f64_moments_are_within_the_conditioning_of_the_pivoted_sums(kind, C):
    """N(0, 1) and constant rows, held to DESIGN 3.5's bound alone: (N + 8) 2^-52 max|T - pivot| on the mean,
    (N + 8) 2^-52 (1 + mu^2 / var) relative on the variance.  Nothing is added."""
    _moments_against_numpy(kind, C, lambda T, N, C_, var: (0.0, 0.0))


def _far_terms(T, N, C, var):
    """What a statistic far from zero adds, from the arithmetic and not from a measured error:
      - the number format: a mean is a double of magnitude up to M = max|T|, rounded once at the leaf (pivot + mu) and once per level
        of the L = ceil(log2 C) levels of the tree, and numpy's pairwise mean rounds about log2 N times more: together
        E_fmt = (L + log2 N + 4) 2^-52 M on the mean, whatever the algorithm;
      - the pair merges read delta = mean_b - mean_a from means that carry E = 3.5's term + E_fmt, and add delta^2 w, w = n_a n_b / n:
        the error 4 |delta| E w summed over the tree is, by Cauchy-Schwarz with sum w <= L N / 4 and sum delta^2 w <= ssd, at most
        2 E sqrt(L N ssd), i.e. 2 E sqrt(L N / ssd) relative to the variance."""
    levels = math.ceil(math.log2(C)) if C > 1 else 0
    pivot = float(T[0, 0])
    e_fmt = (levels + math.log2(N) + 4) * EPS * float(np.max(np.abs(T)))
    e = (N + 8) * EPS * float(np.max(np.abs(T - pivot))) + e_fmt
    return e_fmt, (2.0 * e * math.sqrt(levels * N / (var * (N - 1))) if var > 0.0 and N > 1 else 0.0)


@pytest.mark.parametrize("C", CS)
def test_a_statistic_far_from_zero_loses_what_the_number_format_and_the_pair_merge_cost(C):
    """A SEPARATE case, beyond the rows the stream is specified on: 1e6 + N(0, 1), a chain that starts inside its own distribution
    but far from zero.  Half an ulp of such a mean is already above DESIGN 3.5's bound, so the bound here is 3.5's plus the two terms
    `_far_terms` derives; the ordinary rows above are never held to it."""
    _moments_against_numpy("far", C, _far_terms)


def test_read_out_of_empty_and_single_draw_columns():
    """n_fin = 0 gives NaN mean and ssd; n_fin = 1 gives ssd = +0.0."""
    x = np.array([np.nan, 2.5], dtype=np.float64).view(np.uint64).reshape(1, 2, 1)
    got = R.stream(x, [R.F64, R.F64], [([0], 1, [0.0]), ([1], 1, [2.5])])
    print(got["counts"], got["moments"])
    assert got["counts"] == [[0, 0, 0, 1, 0], [0, 1, 0, 0, 1]]
    assert got["moments"][0][0] != got["moments"][0][0] and got["moments"][0][1] != got["moments"][0][1]
    assert got["moments"][1] == [2.5, 0.0] and R.bits(got["moments"][1][1]) == 0


# ---- ABI --------------------------------------------------------------------------------------------------------------------
def test_abi_check_passes_with_the_new_entries():
    from fugue_amd import engine as E
    header = open(os.path.join(ROOT, "include", "fugue_amd.h")).read()
    rust = open(os.path.join(ROOT, "rust", "fugue-gpu", "src", "ffi.rs")).read()
    H, Rs = abi_check.parse_header(header), abi_check.parse_rust(rust)
    for f in NEW:
        assert f in H["fns"] and f in Rs["fns"] and f in E.ABI_SYMBOLS, f
    assert abi_check.compare_header_rust(header, rust) == []
    assert abi_check.compare_header_ctypes(header, E.lib()) == []
    assert set(H["fns"]) == set(E.ABI_SYMBOLS)
    for name, value in (("FG_PPC_MEAN", 0), ("FG_PPC_VAR", 1), ("FG_PPC_MIN", 2), ("FG_PPC_MAX", 3), ("FG_PPC_SUM", 4), ("FG_PPC_N_STATS", 5)):
        assert f"{name} = {value}" in header
    assert E.PPC_STATS == R.STAT_NAMES
    plan = open(os.path.join(ROOT, "fugue_amd", "csrc", "fg_ppc_stream_plan.h")).read()
    assert f"#define FG_PPC_SCRATCH_DRAWS {E.PPC_SCRATCH_DRAWS} " in plan


# ---- fg_program_observe_value -------------------------------------------------------------------------------------------------
def test_observe_value_of_literals_data_elements_and_site_valued_observes():
    import ctypes as C
    from fugue_amd import engine as E
    from fugue_amd import model as M
    from fugue_amd import workloads as W
    from tests.models import all_dists_model
    coin = E.compile_model(W.coin_flip())
    print("coin_flip:", coin.observe_values)
    assert coin.observe_values == [1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0, 0.0, 1.0, 1.0] and coin.observe_vtypes == [M.BOOL] * 10
    P = M.Program()
    y = P.bind_data("y", [0.75, -3.5, 2.0 ** 60])
    mu = P.sample(M.addr("mu"), M.Normal(0.0, 1.0))
    for i in range(3):
        P.observe(M.addr("y", i), M.Normal(mu, 1.0), y[i])
    P.observe(M.addr("z"), M.Normal(mu, 1.0), y[1] * 2.0 + 1.0)    # a constant expression reads no site either
    P.observe(M.addr("w"), M.Normal(0.0, 1.0), mu * 0.0)           # reads a site, whatever it evaluates to
    data = E.compile_model(P)
    print("data elements:", data.observe_values)
    assert data.observe_values == [0.75, -3.5, 2.0 ** 60, -6.0, None]
    zoo = E.compile_model(all_dists_model())
    k = zoo.observe_names.index(M.addr("o", 4))
    print("o#4:", zoo.observe_values[k], "o#1:", zoo.observe_values[zoo.observe_names.index(M.addr("o", 1))])
    assert zoo.observe_values[k] is None and zoo.observe_values[zoo.observe_names.index(M.addr("o", 1))] == 0.25
    L, v = E.lib(), C.c_double(-7.0)
    assert L.fg_program_observe_value(zoo.h, k, C.byref(v)) == 0 and v.value == -7.0     # left alone
    for bad in (-1, zoo.O, zoo.O + 5):
        rc = L.fg_program_observe_value(zoo.h, bad, C.byref(v))
        print("k =", bad, "->", rc, E.last_error())
        assert rc == FG_E_BAD_ARG
    assert L.fg_program_observe_value(zoo.h, 0, None) == FG_E_BAD_ARG


# ---- the Python layer that needs no device --------------------------------------------------------------------------------------
def test_check_specs_and_p_values():
    from fugue_amd import checks as K
    with pytest.raises(ValueError):
        K.CheckSpec("c", [])
    with pytest.raises(ValueError):
        K.CheckSpec("c", ["a"], ("median",))
    with pytest.raises(ValueError):
        K.CheckSpec("c", ["a"], ("mean", "mean"))
    m = K.marginal_checks(["y#0", "y#1"])
    assert [(c.name, c.addresses, c.statistics) for c in m] == [("y#0", ["y#0"], ["mean"]), ("y#1", ["y#1"], ["mean"])]
    specs, tuples = K.resolve_checks(None, ["a", "b"], [1.0, None], {"b": 2.0}, "t")
    assert specs[0].name == "all" and tuples == [([0, 1], list(K.STATISTICS), [1.0, 2.0])]
    with pytest.raises(ValueError, match="'b'"):
        K.resolve_checks(None, ["a", "b"], [1.0, None], None, "t")
    with pytest.raises(ValueError):
        K.resolve_checks([K.CheckSpec("c", ["nope"])], ["a"], [1.0], None, "t")
    z = np.zeros(2)
    pc = K.PredictiveCheck(["c", "c"], ["mean", "sum"], 10, 2, z, np.array([2, 0]), np.array([3, 0]), np.array([5, 0]), np.array([0, 10]), np.array([10, 1]),
                           z, np.array([9.0, 0.0]))
    print(pc.p_ge, pc.p_gt, pc.p_mid, pc.t_rep_sd)
    assert pc.p_ge[0] == 0.8 and pc.p_gt[0] == 0.5 and pc.p_mid[0] == 0.65 and pc.t_rep_sd[0] == 1.0
    assert all(np.isnan(v[1]) for v in (pc.p_ge, pc.p_gt, pc.p_mid, pc.t_rep_sd))
    assert pc.slot("c", "sum") == 1


def test_the_intervals_of_the_coin_law_are_not_trivial():
    """The three 5-sigma intervals the GPU test holds the counts of 4 096 prior predictive draws to: inside (0, C), pairwise
    disjoint, and the probabilities are those of the Beta-Binomial(10, 2, 2) pmf."""
    C = 4096
    law = R.coin_law(C)
    print(law)
    assert abs(sum(m for m, _ in law) - C) < 1e-9
    assert [round(m * 286 / C) for m, _ in law] == [196, 32, 58]
    iv = sorted((m - h, m + h) for m, h in law)
    assert iv[0][0] > 0 and iv[-1][1] < C
    assert all(iv[i][1] < iv[i + 1][0] for i in range(2))
