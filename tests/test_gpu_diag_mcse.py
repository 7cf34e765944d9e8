"""GPU tests of the MCSE / ESS figures of the mean, the sd and quantiles (fg_diag_mcse.hip, `Engine.diag_mcse_transform`,
`Engine.diag_mcse`) against tests/mcse_restatement.py.  Bit for bit: mean, sd, rhat and ess_mean against
`Engine.diag_rhat_ess` of the same buffer; the rows |c|, c c and every I_p, the sorted cells, median, q, q7, mad and the counts against
the restatement; i_lo / i_hi against `fg_mcse_quantile_ranks` of the call's own ess_quantile word; th_lo / th_hi against the sorted cells
at the positions the call reports; mcse_mean, mcse_sd and mcse_quantile against their formulas in numpy on the call's own words (Evar
and std_B from `Engine.diag_rhat_ess` of the rows on the device, the call the library itself makes).  To a tolerance: ess_sd, ess_sq and
ess_quantile against the oracle's combination on the downloaded rows (rel 1e-8: tests/test_gpu_diag.py's tolerance for that combination),
Evar and V (rel 1e-10), and every figure against the full restatement (rel 1e-6, the wiring only).  The invariances bit for bit;
non-finite cells; a session is left as it was; the drivers end to end.  Every compared figure is printed before it is asserted."""
import math

import numpy as np
import pytest

from fugue_amd import diagnostics as D
from fugue_amd import engine as E
from fugue_amd import inference as I
from fugue_amd import workloads as W
from tests import mcse_restatement as M
from tests import rank_restatement as R
from tests.models import ZOO

pytestmark = pytest.mark.gpu

SHAPES = ((1, 1, 1), (7, 3, 2), (61, 200, 3), (97, 131, 3), (300, 1031, 1))
PROBS3 = (0.05, 0.5, 0.95)
PROBS8 = (0.0, 0.01, 0.25, 0.5, 0.5000001, 0.75, 0.99, 1.0)


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


def _equal(a, b):
    """bit-equal, every NaN equal to every NaN"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def _same(a, b):
    return _equal(np.float64(a), np.float64(b))


def _close(g, w, rel):
    g, w = float(g), float(w)
    return _same(g, w) or (math.isfinite(g) and math.isfinite(w) and abs(g - w) <= rel * abs(w))


def run(engines, table, probs=PROBS3, j0=0, n_j=None, max_out_bytes=0):
    """-> dict: `plain` (diag_rhat_ess of the buffer), `fig` (diag_mcse), `tr` (diag_mcse_transform of [j0, j0 + n_j) centred at the
    plain means, rows and sorted cells downloaded), `rows_comb` (diag_rhat_ess of the transform's rows on the device)"""
    table = np.ascontiguousarray(table, dtype=np.float64)
    n, d, C = table.shape
    n_j = d - j0 if n_j is None else n_j
    eng = engines.get(C)
    ptr = eng.upload(table)
    rows = 2 + len(probs)
    d_rows = eng.device_alloc(8 * n * rows * n_j * C)
    try:
        plain = eng.diag_rhat_ess(ptr, n, d)
        fig = eng.diag_mcse(ptr, n, d, probs=probs, max_out_bytes=max_out_bytes)
        tr = eng.diag_mcse_transform(ptr, n, d, plain["mean"][j0:j0 + n_j], j0=j0, n_j=n_j, probs=probs, d_out=d_rows, sorted_cells=True)
        tr["out"] = eng.download(d_rows, (n, rows * n_j, C))
        comb = eng.diag_rhat_ess(d_rows, n, rows * n_j)
        return dict(plain=plain, fig=fig, tr=tr, rows_comb=comb)
    finally:
        eng.device_free(d_rows)
        eng.device_free(ptr)


def check(res, table, label, probs=PROBS3, j0=0):
    """every comparison of one call; -> the restatements' order statistics per coordinate"""
    plain, fig, tr, comb = res["plain"], res["fig"], res["tr"], res["rows_comb"]
    n, _, C = table.shape
    S, Rw, misses, stats = n * C, 2 + len(probs), [], []
    for k in range(tr["median"].size):
        j = j0 + k
        x = table[:, j, :].reshape(-1)
        st = M.order_stats(x, probs)
        stats.append(st)
        nan = st["counts"]["n_nan"] > 0
        tag = f"{label} coordinate {j}"
        # the plain figures
        for word, key in (("mean", "mean"), ("sd", "std"), ("rhat", "r_hat"), ("ess_mean", "ess")):
            print(f"{tag} {word}: {float(fig[word][j])!r} / diag_rhat_ess {float(plain[key][j])!r}")
            assert math.isnan(float(fig[word][j])) if nan else _same(fig[word][j], plain[key][j]), (tag, word)
        # rows, sorted cells, order statistics, counts: the restatement, centred at the mean the device was given
        rows = tr["out"][:, Rw * k:Rw * k + Rw, :]
        want_rows = M.rows_of(x, plain["mean"][j], probs, st).reshape(Rw, n, C).transpose(1, 0, 2)
        for i in range(Rw):
            ok = _equal(rows[:, i, :], want_rows[:, i, :])
            print(f"{tag} row {i}: bit-equal {ok}")
            assert ok, (tag, "row", i)
        assert _equal(tr["sorted"][k], M.sorted_values(st)), (tag, "sorted")
        want_counts = [st["counts"][c] for c in M.COUNT_NAMES]
        print(f"{tag}: counts {fig['counts'][j].tolist()} / {want_counts} k_p {st['k_p']}; median {float(tr['median'][k])!r} / {st['median']!r}; mad {float(tr['mad'][k])!r} / {st['mad']!r}")
        assert fig["counts"][j, :6].tolist() == want_counts and tr["counts"][k, :6].tolist() == want_counts, (tag, "counts")
        assert fig["k_p"][j].tolist() == st["k_p"] and tr["k_p"][k].tolist() == st["k_p"], (tag, "k_p")
        assert _same(tr["median"][k], st["median"]) and _same(tr["mad"][k], st["mad"]), (tag, "median, mad of the transform")
        if nan:
            assert np.isnan(fig["words"][j]).all(), (tag, "a NaN cell makes every word NaN")
            continue
        assert _same(fig["median"][j], st["median"]) and _same(fig["mad"][j], st["mad"]), (tag, "median, mad")
        assert _equal(fig["q"][j], st["q"]) and _equal(fig["q7"][j], st["q7"]), (tag, "q, q7", fig["q"][j], st["q"], fig["q7"][j], st["q7"])
        # the ESS words are the device combination's of the device's rows; the oracle on the downloaded rows; Evar and V
        ess_rows, mean_rows, std_rows = (comb[key][Rw * k:Rw * k + Rw] for key in ("ess", "mean", "std"))
        got_ess = np.r_[fig["ess_sd"][j], fig["ess_sq"][j], fig["ess_quantile"][j]]
        assert _equal(got_ess, ess_rows), (tag, "the ESS words are fg_diag_rhat_ess's of the rows")
        orc_rows = [M.combination(rows[:, i, :]) for i in range(Rw)]
        for i, name in enumerate(["ess_sd", "ess_sq"] + [f"ess_quantile({p})" for p in probs]):
            print(f"{tag} {name}: {float(got_ess[i])!r}; the oracle on the device's rows {orc_rows[i]['ess']!r} (rel 1e-8)")
            if not _close(got_ess[i], orc_rows[i]["ess"], 1e-8):
                misses.append((tag, name, float(got_ess[i]), orc_rows[i]["ess"], 1e-8))
        with np.errstate(all="ignore"):
            evar, std_b = np.float64(mean_rows[1]), np.float64(std_rows[1])
            V = std_b * std_b * np.float64(S - 1) / np.float64(S)
            want_V = np.float64(orc_rows[1]["std"]) * np.float64(orc_rows[1]["std"]) * np.float64(S - 1) / np.float64(S)
            print(f"{tag} Evar {float(evar)!r} / {orc_rows[1]['mean']!r}, V {float(V)!r} / {float(want_V)!r} (rel 1e-10)")
            for name, g, w in (("Evar", evar, orc_rows[1]["mean"]), ("V", V, want_V)):
                if not _close(g, w, 1e-10):
                    misses.append((tag, name, float(g), float(w), 1e-10))
            # the formulas on the call's own words
            formulas = dict(mcse_mean=np.float64(fig["sd"][j]) / np.sqrt(np.float64(fig["ess_mean"][j])), mcse_sd=np.sqrt(V / np.float64(fig["ess_sq"][j]) / evar / np.float64(4.0)))
        for name, want in formulas.items():
            print(f"{tag} {name}: {float(fig[name][j])!r} / its formula {float(want)!r}")
            assert _same(fig[name][j], want), (tag, name)
        sv = tr["sorted"][k]
        for i, p in enumerate(probs):
            ess = float(fig["ess_quantile"][j, i])
            lo, hi = E.mcse_quantile_ranks(S, p, ess) if (math.isfinite(ess) and ess > 0.0) else (-1, -1)
            print(f"{tag} p = {p}: positions {int(fig['i_lo'][j, i])}, {int(fig['i_hi'][j, i])} / {lo}, {hi}; th {float(fig['th_lo'][j, i])!r}, {float(fig['th_hi'][j, i])!r}; "
                  f"mcse_quantile {float(fig['mcse_quantile'][j, i])!r}")
            assert (int(fig["i_lo"][j, i]), int(fig["i_hi"][j, i])) == (lo, hi), (tag, p, "positions")
            if lo < 0:
                assert all(math.isnan(float(fig[w][j, i])) for w in ("th_lo", "th_hi", "mcse_quantile")), (tag, p)
                continue
            assert _same(fig["th_lo"][j, i], sv[lo]) and _same(fig["th_hi"][j, i], sv[hi]), (tag, p, "th")
            with np.errstate(invalid="ignore"):
                assert _same(fig["mcse_quantile"][j, i], np.float64(0.5) * (np.float64(fig["th_hi"][j, i]) - np.float64(fig["th_lo"][j, i]))), (tag, p, "mcse_quantile")
        # the wiring: the full restatement
        full = M.coordinate(table, j, probs)
        for name in M.WORD_NAMES:
            print(f"{tag} {name}: {float(fig[name][j])!r}; the restatement {full['words'][name]!r} (rel 1e-6)")
            if not _close(fig[name][j], full["words"][name], 1e-6):
                misses.append((tag, name, float(fig[name][j]), full["words"][name], 1e-6))
        for i, p in enumerate(probs):
            names = ["ess_quantile"] + (["mcse_quantile", "th_lo", "th_hi"] if (full["prob_counts"]["i_lo"][i], full["prob_counts"]["i_hi"][i]) == (int(fig["i_lo"][j, i]), int(fig["i_hi"][j, i])) else [])
            if len(names) == 1:
                print(f"{tag} p = {p}: the restatement's own ESS puts the positions at {full['prob_counts']['i_lo'][i]}, {full['prob_counts']['i_hi'][i]}: not compared")
            for name in names:
                if not _close(fig[name][j, i], full["prob_words"][name][i], 1e-6):
                    misses.append((tag, name, p, float(fig[name][j, i]), full["prob_words"][name][i], 1e-6))
    assert not misses, misses
    return stats


def shape_table(n, C, d):
    cols = R.inputs(n * C, seed=1000 * n + C)
    return np.ascontiguousarray(np.stack([cols[k].reshape(n, C) for k in ("normal", "cauchy", "thirds")[:d]], axis=1))


@pytest.mark.parametrize("n,C,d", SHAPES)
def test_shapes_against_the_restatement(engines, n, C, d):
    """(1, 1, 1): one cell; (7, 3, 2); (61, 200, 3): odd n; (97, 131, 3): odd C, four radix tiles; (300, 1 031, 1): S = 309 300, 76 radix
    tiles, 1 024 blocks of the row kernel with a grid stride"""
    table = shape_table(n, C, d)
    check(run(engines, table), table, f"({n}, {C}, {d})")


def test_every_input_kind(engines):
    """n = 97, C = 131 (S = 12 707): normal, Cauchy, heavy ties, a constant column, a tie run longer than a radix tile and one across a
    block boundary, signed zeros and denormals, infinities, NaN cells.  The rank tests' two one-radix-pass columns are left to them: their
    cells differ in the last byte of the fraction only, their standard deviation lies below the rounding of their mean, and a figure
    that passes through the mean has no value there that two summation orders share."""
    n, C = 97, 131
    cols = R.inputs(n * C, seed=5)
    names = [k for k in cols if k not in ("low_byte", "top_byte")]
    table = np.ascontiguousarray(np.stack([cols[k].reshape(n, C) for k in names], axis=1))
    res = run(engines, table)
    stats = dict(zip(names, check(res, table, "inputs")))
    fig = res["fig"]
    k = names.index("constant")
    assert fig["mad"][k] == 0.0 and fig["sd"][k] == 0.0 and (fig["q7"][k] == -2.75).all() and fig["n_passes"][k] == 0
    assert stats["nans"]["counts"]["n_nan"] > 0 and fig["n_nan"][names.index("nans")] == stats["nans"]["counts"]["n_nan"]
    k = names.index("infs")
    print("infs:", {w: float(fig[w][k]) for w in M.WORD_NAMES}, fig["ess_quantile"][k], fig["q"][k])
    assert fig["n_pos_inf"][k] > 0 and fig["n_neg_inf"][k] > 0 and np.isfinite(fig["ess_quantile"][k]).all() and np.isfinite(fig["median"][k]) and np.isfinite(fig["mad"][k])
    assert not math.isfinite(float(fig["mean"][k]))


def test_eight_probabilities_with_both_ends(engines):
    n, C, d = 61, 200, 3
    table = shape_table(n, C, d)
    res = run(engines, table, probs=PROBS8)
    check(res, table, "eight probabilities", probs=PROBS8)
    fig = res["fig"]
    for j in range(d):
        x = table[:, j, :]
        assert fig["q"][j, 0] == x.min() and fig["q"][j, 7] == x.max() and fig["q7"][j, 0] == x.min() and fig["q7"][j, 7] == x.max()
        assert fig["k_p"][j, 0] == 0 and fig["k_p"][j, 7] == n * C - 1


def test_invariances_bit_for_bit(engines):
    n, C, d = 61, 200, 3
    table = shape_table(n, C, d)
    a, again = run(engines, table), run(engines, table)
    one = run(engines, table, j0=1, n_j=1)
    blocks = run(engines, table, max_out_bytes=1)
    for key in ("out", "sorted", "median", "mad"):
        assert _equal(a["tr"][key], again["tr"][key]), key
    assert _equal(a["fig"]["words"], again["fig"]["words"]) and np.array_equal(a["fig"]["counts"], again["fig"]["counts"]) and np.array_equal(a["tr"]["counts"], again["tr"]["counts"])
    Rw = 2 + len(PROBS3)
    print("coordinate 1 alone:", _equal(one["tr"]["out"], a["tr"]["out"][:, Rw:2 * Rw, :]), "one coordinate per block:", _equal(a["fig"]["words"], blocks["fig"]["words"]))
    assert _equal(one["tr"]["out"], a["tr"]["out"][:, Rw:2 * Rw, :]) and _equal(one["tr"]["sorted"][0], a["tr"]["sorted"][1])
    assert _same(one["tr"]["median"][0], a["tr"]["median"][1]) and _same(one["tr"]["mad"][0], a["tr"]["mad"][1]) and np.array_equal(one["tr"]["counts"][0], a["tr"]["counts"][1])
    assert _equal(a["fig"]["words"], blocks["fig"]["words"]) and np.array_equal(a["fig"]["counts"], blocks["fig"]["counts"])
    # the chains in another order: the same multiset, so every order statistic and the mad stay
    rev = run(engines, np.ascontiguousarray(table[:, :, ::-1]))
    for name in ("median", "mad", "q", "q7"):
        assert _equal(rev["fig"][name], a["fig"][name]), name
    ind = [Rw * k + 2 + i for k in range(d) for i in range(len(PROBS3))]                # the indicator rows do not pass through the mean
    assert _equal(rev["tr"]["sorted"], a["tr"]["sorted"]) and _equal(rev["tr"]["out"][:, ind, ::-1], a["tr"]["out"][:, ind, :])
    same_at = (rev["fig"]["i_lo"] == a["fig"]["i_lo"]) & (rev["fig"]["i_hi"] == a["fig"]["i_hi"])
    print("chains reversed: positions equal at", int(same_at.sum()), "of", same_at.size)
    for name in ("th_lo", "th_hi", "mcse_quantile"):
        assert _equal(rev["fig"][name][same_at], a["fig"][name][same_at]), name


def test_non_finite_cells_and_their_neighbours(engines):
    n, C = 61, 200
    cols = R.inputs(n * C, seed=17)
    medinf = cols["cauchy"].copy()
    medinf[np.random.default_rng(3).permutation(n * C)[:n * C // 2 + 40]] = np.inf          # more than half the cells: the median is +inf
    names = ["normal", "nans", "thirds", "infs", "medinf"]
    cols["medinf"] = medinf
    table = np.ascontiguousarray(np.stack([cols[k].reshape(n, C) for k in names], axis=1))
    res = run(engines, table)
    check(res, table, "non-finite")
    fig = res["fig"]
    assert np.isnan(fig["words"][1]).all() and fig["n_nan"][1] == int(np.isnan(cols["nans"]).sum()) > 0
    print("median +inf:", {w: float(fig[w][4]) for w in M.WORD_NAMES}, "NaN folded cells", int(fig["n_nan_folded"][4]))
    assert fig["median"][4] == np.inf and math.isnan(float(fig["mad"][4])) and fig["n_nan_folded"][4] == n * C // 2 + 40 and fig["n_nan"][4] == 0
    assert fig["q"][4, 1] == np.inf and fig["q"][4, 2] == np.inf and np.isfinite(fig["q"][4, 0])
    clean = run(engines, np.ascontiguousarray(table[:, [0, 2], :]))
    assert _equal(fig["words"][[0, 2]], clean["fig"]["words"]) and np.array_equal(fig["counts"][[0, 2]], clean["fig"]["counts"])


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
            res = eng.diag_mcse(buf, 5, cp.d)
            tr = eng.diag_mcse_transform(buf, 5, cp.d, res["mean"], sorted_cells=True)
            assert not res["n_nan"].any() and (res["n_cells"] == 5 * C).all() and np.isfinite(res["median"]).all() and (np.diff(tr["sorted"], axis=1) >= 0).all()
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
    """64 chains x 120 draws of `normal_sites(3)` at a fixed step size (four leapfrog steps of 0.2, no warm-up, as the rank test's run).
    `mcse_diagnostics` equals `Engine.diag_mcse` on the stored buffer; `summarise_draws` carries `rank_diagnostics`' and
    `mcse_diagnostics`' own numbers; mcse_mean < sd and ess_mean <= S log10(S)."""
    cfg = I.HMCConfig(n_leapfrog=4, init_step_size=0.2)
    chains = I.hmc_chain(7, E.compile_model(W.normal_sites(3)), 120, 0, cfg, n_chains=64)
    md = D.mcse_diagnostics(chains)
    rd = D.rank_diagnostics(chains)
    table = np.ascontiguousarray(np.stack([chains.get_f64(a) for a in md.names], axis=1))
    eng = E.Engine(E.compile_model(W.normal_sites(1)), 64, seed=0)
    ptr = eng.upload(table)
    try:
        res = eng.diag_mcse(ptr, 120, 3)
    finally:
        eng.device_free(ptr)
        eng.close()
    S = 64 * 120
    assert md.names == [a for a, v in zip(chains.sites, chains.vtypes) if v == 0] and md.d == 3 and md.n_draws == S and md.probs.tolist() == list(PROBS3)
    for name in M.WORD_NAMES + M.PROB_WORD_NAMES:
        assert _equal(getattr(md, name), res[name]), name
    for name in M.COUNT_NAMES + M.PROB_COUNT_NAMES:
        assert np.array_equal(md.counts[name], res[name]), name
    print("mcse_mean", md.mcse_mean, "sd", md.sd, "ess_mean", md.ess_mean, "mcse_sd", md.mcse_sd, "mcse_quantile", md.mcse_quantile)
    assert (md.mcse_mean < md.sd).all() and (md.ess_mean <= S * math.log10(S)).all() and (md.mcse_mean > 0).all() and (md.mcse_sd > 0).all() and (md.mcse_quantile > 0).all()
    table_rows = D.summarise_draws(chains)
    assert list(table_rows) == md.names
    for k, a in enumerate(md.names):
        row = table_rows[a]
        assert tuple(row) == D.SUMMARY_COLUMNS
        want = dict(mean=md.mean[k], median=md.median[k], sd=md.sd[k], mad=md.mad[k], q5=md.q7[k, 0], q95=md.q7[k, 2], rhat=rd.rhat_rank[k], ess_bulk=rd.ess_bulk[k], ess_tail=rd.ess_tail[k],
                    mcse_mean=md.mcse_mean[k], mcse_sd=md.mcse_sd[k], mcse_q5=md.mcse_quantile[k, 0], mcse_median=md.mcse_quantile[k, 1], mcse_q95=md.mcse_quantile[k, 2])
        for name in D.SUMMARY_COLUMNS:
            assert _same(row[name], want[name]), (a, name)
    a = md.names[0]
    assert D.mcse_mean(chains, a) == md.mcse_mean[0] and D.mcse_sd(chains, a) == md.mcse_sd[0] and D.mcse_median(chains, a) == md.mcse_quantile[0, 1] and D.mad(chains, a) == md.mad[0]
    assert D.ess_mean(chains, a) == md.ess_mean[0] and D.ess_sd(chains, a) == md.ess_sd[0] and D.ess_median(chains, a) == md.ess_quantile[0, 1]
    assert D.mcse_quantile(chains, a, 0.95) == md.mcse_quantile[0, 2] and D.ess_quantile(chains, a, 0.05) == md.ess_quantile[0, 0]
