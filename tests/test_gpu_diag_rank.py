"""GPU tests of the rank-normalised diagnostics (fg_diag_rank.hip, `Engine.diag_rank_transform`, `Engine.diag_rank`)
against tests/rank_restatement.py: the doubled ranks as integers, the indicators, the median, the order statistics and every count
exact; the normal scores bit-equal in the central branch and within `rank_restatement.Z_TOL` (four times the measured deviation of the
restatement from mpmath, tests/test_diag_rank_cpu.py) in the tails; the figures against the oracle's combination on the downloaded rows
(R-hat rel 1e-10, ESS rel 1e-8: tests/test_gpu_diag.py's tolerances for the same combination) and against the full restatement (rel
1e-6, the wiring only); the invariances bit for bit; non-finite cells; a session is left as it was; the drivers end to end.  Every
compared figure is printed before it is asserted."""
import math

import numpy as np
import pytest

from fugue_amd import diagnostics as D
from fugue_amd import engine as E
from fugue_amd import inference as I
from fugue_amd import workloads as W
from tests import rank_restatement as R
from tests.models import ZOO

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1, 1), (7, 3, 2), (61, 200, 3), (97, 131, 3), (300, 1031, 1))
RHAT_WORDS, ESS_WORDS = ("rhat_rank", "rhat_bulk", "rhat_folded"), ("ess_bulk", "ess_tail", "ess_lower", "ess_upper")


class _Engines:
    """One engine per chain count for the whole module (the model does not matter to the calls)."""

    def __init__(self):
        self.cp, self.by_c = E.compile_model(W.normal_sites(1)), {}

    def get(self, C: int):
        if C not in self.by_c:
            self.by_c[C] = E.Engine(self.cp, C, seed=1)
        return self.by_c[C]

    def close(self):
        for e in self.by_c.values():
            e.close()


@pytest.fixture(scope="module")
def engines():
    pool = _Engines()
    yield pool
    pool.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def run(engines, table, probs=(0.05, 0.95), j0=0, n_j=None, max_out_bytes=0, figures=True):
    """-> (the transform's result with rank2, the figures' result)"""
    table = np.ascontiguousarray(table, dtype=np.float64)
    n, d, C = table.shape
    eng = engines.get(C)
    ptr = eng.upload(table)
    try:
        tr = eng.diag_rank_transform(ptr, n, d, j0=j0, n_j=n_j, probs=probs, rank2=True)
        return tr, (eng.diag_rank(ptr, n, d, probs=probs, max_out_bytes=max_out_bytes) if figures else None)
    finally:
        eng.device_free(ptr)


def _same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _close(g, w, rel):
    return _same(g, w) or (math.isfinite(g) and math.isfinite(w) and abs(g - w) <= rel * abs(w))


def check_transform(tr, fig, table, label, probs=(0.05, 0.95), j0=0):
    """the device's rows, ranks, medians, order statistics and counts against the restatement of every coordinate; -> the restatements"""
    n, _, C = table.shape
    wants = []
    for k in range(tr["median"].size):
        j = j0 + k
        want = R.transform(table[:, j, :].reshape(-1), probs)
        wants.append(want)
        r2 = tr["rank2"][:, k, :].reshape(-1).astype(np.int64)
        rows = tr["out"][:, 4 * k:4 * k + 4, :]
        equal_r2 = np.array_equal(r2, want["r2"])
        print(f"{label} coordinate {j}: r2 equal {equal_r2}; counts {tr['counts'][k].tolist()} / {[want['counts'][c] for c in R.COUNT_NAMES]}; median {tr['median'][k]!r} / {want['median']!r}")
        assert equal_r2, (label, j)
        assert tr["counts"][k].tolist() == [want["counts"][c] for c in R.COUNT_NAMES], (label, j)
        assert _same(float(tr["median"][k]), want["median"]), (label, j)
        for i, (name, cen) in enumerate((("z", want["central"]), ("z_folded", want["central_folded"]))):
            g, w = rows[:, i, :].reshape(-1), want[name]
            central_equal = np.array_equal(_bits(g[cen]), _bits(w[cen]))
            rel = np.abs(g[~cen] - w[~cen]) / np.abs(w[~cen])
            print(f"{label} coordinate {j} {name}: {int(cen.sum())} central cells bit-equal {central_equal}; {int((~cen).sum())} tail cells, largest relative difference "
                  f"{rel.max() if rel.size else 0.0:.3e} (tolerance {R.Z_TOL:.3e})")
            assert central_equal and (rel <= R.Z_TOL).all(), (label, j, name)
        assert np.array_equal(_bits(rows[:, 2, :].reshape(-1)), _bits(want["i_lo"])) and np.array_equal(_bits(rows[:, 3, :].reshape(-1)), _bits(want["i_hi"])), (label, j)
        if fig is not None:
            assert fig["counts"][j].tolist() == tr["counts"][k].tolist(), (label, j)
            nan = want["counts"]["n_nan"] > 0
            for name in ("median", "x_lo", "x_hi"):
                print(f"{label} coordinate {j} {name}: {float(fig[name][j])!r} / {want[name]!r}")
                assert math.isnan(float(fig[name][j])) if nan else _same(float(fig[name][j]), want[name]), (label, j, name)
    return wants


def check_figures(tr, fig, table, label, wants):
    """the figures against the oracle's combination on the DOWNLOADED rows (tight) and against the full restatement (the wiring)"""
    misses = []
    for j, want in enumerate(wants):
        on_rows = R.figures_from_rows(tr["out"][:, 4 * j:4 * j + 4, :], want["counts"], want["median"], want["x_lo"], want["x_hi"])
        full = R.coordinate(table, j)["figures"]
        for name in RHAT_WORDS + ESS_WORDS:
            g = float(fig[name][j])
            tol = 1e-10 if name in RHAT_WORDS else 1e-8
            print(f"{label} coordinate {j} {name}: {g!r}; the oracle on the device's rows {on_rows[name]!r} (rel {tol:g}); the restatement {full[name]!r} (rel 1e-6)")
            if not _close(g, on_rows[name], tol):
                misses.append((label, j, name, g, on_rows[name], tol))
            if not _close(g, full[name], 1e-6):
                misses.append((label, j, name, g, full[name], 1e-6))
    assert not misses, misses


def shape_table(n, C, d):
    cols = R.inputs(n * C, seed=1000 * n + C)
    return np.ascontiguousarray(np.stack([cols[k].reshape(n, C) for k in ("normal", "cauchy", "thirds")[:d]], axis=1))


@pytest.mark.parametrize("n,C,d", SHAPES)
def test_shapes_against_the_restatement(engines, n, C, d):
    """(1, 1, 1): one cell; (7, 3, 2); (61, 200, 3): odd n, the split drops the middle draw; (97, 131, 3): odd C, four radix tiles;
    (300, 1 031, 1): S = 309 300, 76 radix tiles and 303 run tiles"""
    table = shape_table(n, C, d)
    tr, fig = run(engines, table)
    wants = check_transform(tr, fig, table, f"({n}, {C}, {d})")
    check_figures(tr, fig, table, f"({n}, {C}, {d})", wants)


def test_every_input_kind(engines):
    """n = 97, C = 131 (S = 12 707): normal, Cauchy, heavy ties, a constant column, columns that differ in their lowest byte / in their
    sign-and-exponent byte only (one radix pass in the first sort), a tie run longer than a radix tile and one across a block boundary,
    signed zeros and denormals, infinities, NaN cells"""
    n, C = 97, 131
    cols = R.inputs(n * C, seed=5)
    names = list(cols)
    table = np.ascontiguousarray(np.stack([cols[k].reshape(n, C) for k in names], axis=1))
    tr, fig = run(engines, table)
    wants = check_transform(tr, fig, table, "inputs")
    check_figures(tr, fig, table, "inputs", wants)
    by = dict(zip(names, wants))
    assert by["constant"]["counts"]["n_passes"] == 0 and by["constant"]["counts"]["n_runs"] == 1 and by["constant"]["counts"]["longest_run"] == n * C
    for k in ("low_byte", "top_byte"):
        first = R.passes_run(R.keys(cols[k]))
        print(k, "passes of the first sort", first, "both sorts", int(tr["n_passes"][names.index(k)]))
        assert first == 1 and tr["n_passes"][names.index(k)] == by[k]["counts"]["n_passes"]
    assert by["tie_runs"]["counts"]["longest_run"] > R.TILE
    assert by["nans"]["counts"]["n_nan"] > 0 and all(math.isnan(float(fig[w][names.index("nans")])) for w in R.WORD_NAMES)
    assert all(math.isfinite(float(fig[w][names.index("infs")])) for w in RHAT_WORDS + ESS_WORDS) and by["infs"]["counts"]["n_pos_inf"] > 0 and by["infs"]["counts"]["n_neg_inf"] > 0


def test_invariances_bit_for_bit(engines):
    n, C, d = 61, 200, 3
    table = shape_table(n, C, d)
    tr, fig = run(engines, table)
    tr_again, fig_again = run(engines, table)
    one, _ = run(engines, table, j0=1, n_j=1, figures=False)
    _, fig_blocks = run(engines, table, max_out_bytes=1)
    for key in ("out", "median"):
        assert np.array_equal(_bits(tr[key]), _bits(tr_again[key])), key
    assert np.array_equal(tr["rank2"], tr_again["rank2"]) and np.array_equal(tr["counts"], tr_again["counts"])
    assert np.array_equal(_bits(fig["words"]), _bits(fig_again["words"])) and np.array_equal(fig["counts"], fig_again["counts"])
    print("coordinate 1 alone:", np.array_equal(_bits(one["out"]), _bits(tr["out"][:, 4:8, :])), "one coordinate per block:", np.array_equal(_bits(fig["words"]), _bits(fig_blocks["words"])))
    assert np.array_equal(_bits(one["out"]), _bits(tr["out"][:, 4:8, :])) and np.array_equal(one["rank2"][:, 0, :], tr["rank2"][:, 1, :])
    assert _bits(one["median"])[0] == _bits(tr["median"])[1] and np.array_equal(one["counts"][0], tr["counts"][1])
    assert np.array_equal(_bits(fig["words"]), _bits(fig_blocks["words"])) and np.array_equal(fig["counts"], fig_blocks["counts"])
    # a strictly increasing map of the draws leaves the ranks and what is computed from z alone
    base = np.ascontiguousarray(table[:, :1, :])
    tr0, fig0 = run(engines, base)
    for label, mapped in (("exp", np.exp(base)), ("cube", base ** 3)):
        assert np.unique(mapped).size == np.unique(base).size
        tr1, fig1 = run(engines, np.ascontiguousarray(mapped))
        print(label, "r2", np.array_equal(tr1["rank2"], tr0["rank2"]), "z", np.array_equal(_bits(tr1["out"][:, 0, :]), _bits(tr0["out"][:, 0, :])), float(fig1["rhat_bulk"][0]), float(fig0["rhat_bulk"][0]))
        assert np.array_equal(tr1["rank2"], tr0["rank2"]) and np.array_equal(_bits(tr1["out"][:, 0, :]), _bits(tr0["out"][:, 0, :]))
        for name in ("rhat_bulk", "ess_bulk", "ess_lower", "ess_upper", "ess_tail"):
            assert _bits(fig1[name])[0] == _bits(fig0[name])[0], (label, name)
    # the chains in another order: the same multiset, every cell keeps its rank
    tr2, _ = run(engines, np.ascontiguousarray(base[:, :, ::-1]), figures=False)
    assert np.array_equal(tr2["rank2"][:, :, ::-1], tr0["rank2"]) and np.array_equal(_bits(tr2["out"][:, :, ::-1]), _bits(tr0["out"]))


def test_non_finite_cells_and_their_neighbours(engines):
    n, C = 61, 200
    cols = R.inputs(n * C, seed=17)
    medinf = cols["cauchy"].copy()
    medinf[np.random.default_rng(3).permutation(n * C)[:n * C // 2 + 40]] = np.inf          # more than half the cells: the median is +inf
    names = ["normal", "nans", "thirds", "infs", "medinf"]
    cols["medinf"] = medinf
    table = np.ascontiguousarray(np.stack([cols[k].reshape(n, C) for k in names], axis=1))
    tr, fig = run(engines, table)
    wants = check_transform(tr, fig, table, "non-finite")
    check_figures(tr, fig, table, "non-finite", wants)
    assert all(math.isnan(float(fig[w][1])) for w in R.WORD_NAMES) and fig["n_nan"][1] == int(np.isnan(cols["nans"]).sum()) > 0
    assert all(math.isfinite(float(fig[w][3])) for w in RHAT_WORDS + ESS_WORDS) and fig["n_pos_inf"][3] > 0 and fig["n_neg_inf"][3] > 0 and fig["n_nan_folded"][3] == 0
    print("median +inf:", {w: float(fig[w][4]) for w in R.WORD_NAMES}, "NaN folded cells", int(fig["n_nan_folded"][4]))
    assert fig["median"][4] == np.inf and fig["n_nan_folded"][4] == n * C // 2 + 40 and fig["n_nan"][4] == 0
    assert math.isnan(float(fig["rhat_folded"][4])) and math.isnan(float(fig["rhat_rank"][4])) and all(math.isfinite(float(fig[w][4])) for w in ("rhat_bulk", "ess_bulk", "ess_tail"))
    tr_clean, fig_clean = run(engines, np.ascontiguousarray(table[:, [0, 2], :]))
    assert np.array_equal(_bits(fig["words"][[0, 2]]), _bits(fig_clean["words"])) and np.array_equal(fig["counts"][[0, 2]], fig_clean["counts"])
    assert np.array_equal(_bits(tr["out"][:, [0, 1, 2, 3, 8, 9, 10, 11], :]), _bits(tr_clean["out"]))


def test_a_call_between_steps_changes_nothing_of_a_session(monkeypatch):
    monkeypatch.setenv("FG_JIT", "0")
    cp = E.compile_model(ZOO["hier"]())
    C, seen = 70, []
    for call in (False, True):
        eng = E.Engine(cp, C, seed=13)
        buf = eng.device_alloc(10 * cp.d * C * 8)
        eng.hmc_init(E.hmc_config(), 3)
        eng.hmc_step(3)
        eng.hmc_step(5, buf)
        if call:
            res = eng.diag_rank(buf, 5, cp.d)
            tr = eng.diag_rank_transform(buf, 5, cp.d, rank2=True)
            assert not res["n_nan"].any() and (res["n_cells"] == 5 * C).all() and np.isfinite(res["median"]).all() and tr["rank2"].min() >= 2 and tr["rank2"].max() <= 10 * C
        eng.hmc_step(5, buf + 5 * cp.d * C * 8)
        seen.append(dict(draws=eng.download(buf, (10, cp.d, C), dtype=np.int64), values=eng.get_values(), lj=eng.hmc_log_joint(), eps=eng.hmc_step_sizes(),
                         state=np.frombuffer(eng.state_export(), dtype=np.uint8), accept=np.float64(eng.hmc_stats().accept_rate)))
        eng.device_free(buf)
        eng.close()
    for k in seen[0]:
        a, b = (np.atleast_1d(np.ascontiguousarray(seen[j][k])) for j in (1, 0))
        print(f"{k}: equal {a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))}")
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), k


def test_end_to_end_on_three_normal_sites():
    """64 chains x 120 draws of `normal_sites(3)` at a fixed step size (four leapfrog steps of 0.2: close to independent draws; no
    warm-up, so nothing adapts).  `rank_diagnostics` equals `Engine.diag_rank` on the stored buffer; rhat_rank < 1.05.  Then the draws
    of the first 32 chains are stretched by 3 about their mean: the folded R-hat rises above 1.05 while the plain split R-hat stays
    below 1.01.  The restatement on the CPU oracle's run of this construction (seeds 7 and 8, three sites each) gave rhat_rank at most
    1.002, the folded R-hat of the stretched draws at least 1.139 and their plain split R-hat at most 1.0005."""
    cfg = I.HMCConfig(n_leapfrog=4, init_step_size=0.2)
    chains = I.hmc_chain(7, E.compile_model(W.normal_sites(3)), 120, 0, cfg, n_chains=64)
    rd = D.rank_diagnostics(chains)
    table = np.ascontiguousarray(np.stack([chains.get_f64(a) for a in rd.names], axis=1))
    eng = E.Engine(E.compile_model(W.normal_sites(1)), 64, seed=0)
    ptr = eng.upload(table)
    try:
        res = eng.diag_rank(ptr, 120, 3)
    finally:
        eng.device_free(ptr)
        eng.close()
    assert rd.names == [a for a, v in zip(chains.sites, chains.vtypes) if v == 0] and rd.d == 3 and rd.n_draws == 64 * 120
    for name in R.WORD_NAMES:
        assert np.array_equal(_bits(getattr(rd, name)), _bits(res[name])), name
    for name in R.COUNT_NAMES:
        assert np.array_equal(rd.counts[name], res[name]), name
    print("rhat_rank", rd.rhat_rank, "ess_bulk", rd.ess_bulk, "ess_tail", rd.ess_tail)
    assert (rd.rhat_rank < 1.05).all()
    a = rd.names[0]
    assert D.rank_r_hat_f64(chains, a) == rd.rhat_rank[0] and D.ess_bulk(chains, a) == rd.ess_bulk[0] and D.ess_tail(chains, a) == rd.ess_tail[0]
    wide = table.copy()
    for j in range(3):
        m = wide[:, j, :32].mean()
        wide[:, j, :32] = m + 3.0 * (wide[:, j, :32] - m)
    rw = D.rank_diagnostics(wide)
    plain = [float(D.ChainDiagnostics(D.HostMoments(np.ascontiguousarray(wide[:, j:j + 1, :]))).split_rhat()[0]) for j in range(3)]
    print("stretched: rhat_folded", rw.rhat_folded, "rhat_bulk", rw.rhat_bulk, "plain split R-hat", plain)
    assert (rw.rhat_folded > 1.05).all() and max(plain) < 1.01 and np.array_equal(_bits(rw.rhat_rank), _bits(np.maximum(rw.rhat_bulk, rw.rhat_folded)))
