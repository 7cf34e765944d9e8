"""GPU tests of the predictive checks and WAIC / IS-LOO of a weighted population (fg_wpop_eval.hip): device against
tests/wpop_eval_restatement.py -- units, counts, t_obs, p-values, the moments of the replicated statistics, the counters and every
word and figure no transcendental touches bit for bit; lppd, elpd_loo, is_ess, max_weight within the sum of the two bounds derived
in `wpop_eval_restatement.bounds`, and no more than (N + 8) 2^-52, (the restatement's glibc exp and the device's ocml exp, each within its bound of the exact figure,
which tests/test_wpop_eval_cpu.py holds the restatement to with mpmath); device against device (fg_ppc_stream at equal weights;
two calls; slices against whole); adaptive_smc_summary against the restatement of adaptive_smc's download; the engine untouched.
Every compared figure is printed before it is asserted."""
import functools
import math

import numpy as np
import pytest

from fugue_amd import checks as CK
from fugue_amd import comparison as CM
from fugue_amd import engine as E
from fugue_amd import inference as I
from fugue_amd import workloads as W
from tests import ppc_restatement as PR
from tests import wpop_eval_restatement as R

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 257, 65537)
LL3 = ("normal", "far", "neg_inf")
EXACT_WORDS = ("W", "W_fin", "W2", "mean", "ssd", "n_used", "mx", "mn")
EXACT_FIGURES = ("mean_ll", "p_waic")


def _kinds(N):
    return ("dirichlet", "quarter_zero") if N > 1000 else ("dirichlet", "uniform", "quarter_zero", "one_heavy", "below_unit", "bad")


def _checks(N):
    """three checks on the f64 rows -- all rows with five statistics, a marginal one, one sharing a row -- and the bool / u64 / i64 rows"""
    cells, vt, chk = R.check_table(N, N)
    return cells, vt, chk[:3] + [chk[4]]


def _tuples(chk):
    return [(rows, [st for st in range(PR.N_STATS) if (mask >> st) & 1], obs) for rows, mask, obs in chk]


@functools.lru_cache(maxsize=None)
def ref(N, wkind):
    w, _ = R.weights(wkind, N, N)
    cells, vt, chk = _checks(N)
    ll = R.ll_table(LL3 if N > 1000 else R.LL_KINDS, N, w, N)
    return w, cells, vt, chk, ll, R.checks(cells, vt, chk, w), R.loglik(ll, w)


class _Pool:
    def __init__(self):
        self.eng = E.Engine(E.compile_model(W.normal_sites(1)), 64, seed=1)
        self.bufs, self.pops = [], []

    def upload(self, a):
        self.bufs.append(self.eng.upload(np.ascontiguousarray(a)))
        return self.bufs[-1]

    def pop(self, w):
        self.pops.append(self.eng.wpop(len(w), self.upload(w)))
        return self.pops[-1]

    def close(self):
        for p in self.pops:
            p.close()
        for b in self.bufs:
            self.eng.device_free(b)
        self.eng.close()


@pytest.fixture(scope="module")
def pool():
    p = _Pool()
    yield p
    p.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same(a, b):
    """bit-equal doubles, any NaN equal to any NaN"""
    a, b = np.asarray(a, dtype=np.float64).ravel(), np.asarray(b, dtype=np.float64).ravel()
    return a.shape == b.shape and bool(np.all((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))))


def assert_checks(got, want, label):
    n_slots = len(want["t_obs"])
    assert len(got["slots"]) == n_slots
    for k in range(n_slots):
        mom = [got[name][k] for name in E.WPOP_MOMENTS[:5]] + [float(got["n_used"][k])]
        ok = (_same(got["t_obs"][k], want["t_obs"][k]) and [int(v) for v in got["units"][k]] == want["units"][k] and [int(v) for v in got["counts"][k]] == want["counts"][k] and
              _same(mom, want["moments"][k]) and _same([got["p_ge"][k], got["p_gt"][k], got["p_mid"][k]], want["p"][k]))
        print(f"{label} slot {k}: units {got['units'][k].tolist()} counts {got['counts'][k].tolist()} p_mid {got['p_mid'][k]!r} mean {got['mean'][k]!r} equal {ok}")
        assert ok, (label, k, want["units"][k], want["counts"][k], want["moments"][k], want["p"][k])


def assert_loglik(got, want, ll, w, label):
    worst = 0.0
    for k in range(len(ll)):
        words, counts, figs = want["words"][k], want["counts"][k], want["figures"][k]
        assert [int(got[n][k]) for n in E.WLL_COUNTS] == counts, (label, k, counts)
        for n in EXACT_WORDS:
            j = E.WLL_WORDS.index(n)
            assert _same(got["words"][k][j], words[j]), (label, k, n, got["words"][k][j], words[j])
        gf = {n: float(got[n][k]) for n in R.FIGURE_NAMES}
        wf = dict(zip(R.FIGURE_NAMES, figs))
        for n in EXACT_FIGURES:
            assert _same(gf[n], wf[n]), (label, k, n, gf[n], wf[n])
        for n in R.FIGURE_NAMES:
            assert (gf[n] != gf[n]) == (wf[n] != wf[n]) and (math.isinf(gf[n]) or math.isinf(wf[n])) <= (gf[n] == wf[n]), (label, k, n, gf[n], wf[n])
        if counts[0] == 0 or counts[3] > 0:
            continue
        scale = dict(wf, ln_p=wf["lppd"] - words[6], ln_n=words[7] - wf["elpd_loo"])         # the figures' own sizes for the relative parts of the bound
        if not all(math.isfinite(scale[n]) for n in ("ln_p", "ln_n", "lppd", "elpd_loo")):
            scale = dict(scale, **{n: (scale[n] if math.isfinite(scale[n]) else 0.0) for n in ("ln_p", "ln_n", "lppd", "elpd_loo", "is_ess", "max_weight")})
        b = R.bounds(ll[k], w, scale)
        for n in R.EXP_FIGURES:
            if not math.isfinite(wf[n]):
                continue
            err = abs(gf[n] - wf[n])
            bound = min(2 * b[n] * (1 + 1e-9), R.ceiling(len(w), scale)[n])        # each side within its bound of the exact figure; never past (N + 8) 2^-52
            worst = max(worst, err / bound)
            print(f"{label} row {k} {n}: {gf[n]!r} / {wf[n]!r}: err {err:.3e}, tolerance {bound:.3e}")
            assert err <= bound, (label, k, n, gf[n], wf[n])
    print(f"{label}: largest error / bound {worst:.3f}")


@pytest.mark.parametrize("N", NS)
def test_device_equals_the_restatement(pool, N):
    """A single particle, a partial wave, a full one, a partial block, two blocks, and a tree of three levels with a partial last
    block; f64, bool, u64 and i64 rows; n_sel = 1 and all rows; two calls give the same bytes; rows and checks one at a time give the
    bytes of the whole."""
    for wkind in _kinds(N):
        w, cells, vt, chk, ll, want_c, want_l = ref(N, wkind)
        wp, dc, dl = pool.pop(w), pool.upload(cells), pool.upload(ll)
        tup = _tuples(chk)
        got_c = wp.checks(dc, vt, tup)
        assert_checks(got_c, want_c, f"N {N} {wkind}")
        got_l = wp.loglik(dl, len(ll))
        assert_loglik(got_l, want_l, ll, w, f"N {N} {wkind}")
        again_c, again_l = wp.checks(dc, vt, tup), wp.loglik(dl, len(ll))
        for key in ("t_obs", "units", "counts", "p_mid") + E.WPOP_MOMENTS:
            assert np.array_equal(np.asarray(got_c[key]).view(np.uint64) if np.asarray(got_c[key]).dtype == np.float64 else got_c[key],
                                  np.asarray(again_c[key]).view(np.uint64) if np.asarray(again_c[key]).dtype == np.float64 else again_c[key]), key
        assert all(np.array_equal(_bits(got_l[n]), _bits(again_l[n])) for n in R.FIGURE_NAMES + ("words",))
        one = wp.loglik(dl + N * 8, 1)               # n_sel = 1: row 1 alone
        assert all(_bits(one[n])[0] == _bits(got_l[n])[1] for n in R.FIGURE_NAMES) and np.array_equal(_bits(one["words"][0]), _bits(got_l["words"][1]))
        k0 = 0
        for q, t in enumerate(tup):                  # every check alone: its slots' bytes
            alone = wp.checks(dc, vt, [t])
            ns = len(alone["slots"])
            assert np.array_equal(alone["units"], got_c["units"][k0:k0 + ns]) and np.array_equal(alone["counts"], got_c["counts"][k0:k0 + ns]), q
            assert all(np.array_equal(_bits(alone[n]), _bits(got_c[n][k0:k0 + ns])) for n in ("t_obs", "mean", "std", "mcse", "p_ge", "p_gt", "p_mid")), q
            k0 += ns


def test_slot_slices_of_a_large_population_equal_single_slots(pool):
    """N = 2^22 + 3: three slots fit the staging budget, so a check of five is cut into two slices, the second beginning inside the
    check; every slot asked for alone (a slice of its own) gives the same bytes.  Device against device."""
    N = (1 << 22) + 3
    rng = np.random.default_rng(11)
    cells = np.ascontiguousarray(rng.normal(0.0, 1.0, (2, N))).view(np.uint64)
    g = rng.gamma(0.7, size=N)
    wp, dc = pool.pop(g / g.sum()), pool.upload(cells)
    obs = [0.1, -0.2]
    whole = wp.checks(dc, [PR.F64, PR.F64], [([0, 1], list(range(5)), obs), ([1], [PR.MEAN], [0.0])])
    T = wp.units()["T"]
    assert all(int(sum(int(v) for v in row)) == T for row in whole["units"])
    for k, (q, st) in enumerate(whole["slots"]):
        alone = wp.checks(dc, [PR.F64, PR.F64], [([0, 1], [st], obs)] if q == 0 else [([1], [st], [0.0])])
        print(k, whole["units"][k].tolist(), whole["mean"][k], alone["mean"][0])
        assert np.array_equal(alone["units"][0], whole["units"][k]) and np.array_equal(alone["counts"][0], whole["counts"][k])
        assert all(_bits(alone[n])[0] == _bits(whole[n])[k] for n in ("t_obs", "mean", "std", "mcse", "p_mid"))


def test_row_slices_of_a_large_population_equal_single_rows(pool):
    """N = 2^22 + 3: three rows fit the staging budget, so fg_wpop_loglik takes five rows as slices of three and two; every row asked
    for alone gives the same figures, words and counters bit for bit.  A -inf and a NaN cell sit in rows of the second slice.  Device
    against device."""
    N, n_sel = (1 << 22) + 3, 5
    rng = np.random.default_rng(13)
    ll = rng.normal(-3.0, 1.0, (n_sel, N))
    ll[3, 12345], ll[4, 7] = -np.inf, np.nan
    g = rng.gamma(0.7, size=N)
    wp, dl = pool.pop(g / g.sum()), pool.upload(ll)
    whole = wp.loglik(dl, n_sel)
    assert whole["n_fin"].tolist() == [N, N, N, N - 1, N - 1] and whole["n_neg_inf"].tolist() == [0, 0, 0, 1, 0] and whole["n_nan"].tolist() == [0, 0, 0, 0, 1]
    for k in range(n_sel):
        alone = wp.loglik(dl + k * N * 8, 1)
        print(k, {n: float(whole[n][k]) for n in R.FIGURE_NAMES})
        assert all(_same(alone[n][0], whole[n][k]) for n in R.FIGURE_NAMES), k
        assert np.array_equal(_bits(alone["words"][0]), _bits(whole["words"][k])) and all(int(alone[n][0]) == int(whole[n][k]) for n in E.WLL_COUNTS), k
    assert np.isfinite(whole["lppd"][:4]).all() and whole["elpd_loo"][3] == -np.inf and np.isnan(whole["lppd"][4])


@pytest.mark.parametrize("N", (64, 1024))
def test_equal_weights_give_the_p_values_of_the_check_stream(N):
    """w = 1 / N, N a power of two: fg_wpop_checks on [R][N] against fg_ppc_stream with n_total = 1 and C = N chains -- the unit sums
    are the stream's counters times 2^52 / N and the p-values are bit-equal."""
    cells, vt, chk = _checks(N)
    tup = _tuples(chk)
    eng = E.Engine(E.compile_model(W.normal_sites(1)), N, seed=3)
    bufs, wp, stream = [], None, None
    try:
        bufs.append(eng.upload(np.full(N, 1.0 / N)))
        bufs.append(eng.upload(cells))
        wp = eng.wpop(N, bufs[0])
        got = wp.checks(bufs[1], vt, tup)
        stream = eng.ppc_stream(1, vt, tup)
        stream.update(bufs[1], 1)
        pooled = stream.pooled()
        p = CK._p_values(pooled["n_lt"], pooled["n_eq"], pooled["n_gt"])
        unit = 2 ** 52 // N
        for k in range(len(got["slots"])):
            counts = [int(pooled[n][k]) for n in ("n_lt", "n_eq", "n_gt", "n_nan")]
            print(f"N {N} slot {k}: units {got['units'][k].tolist()} = {unit} x {counts}; p_mid {got['p_mid'][k]!r} / {p['p_mid'][k]!r}")
            assert [int(v) for v in got["units"][k]] == [unit * c for c in counts] and got["counts"][k].tolist() == counts
        assert all(_same(got[n], p[n]) for n in CK.P_VALUES) and _same(got["t_obs"], stream.observed())
    finally:
        for h in (wp, stream):
            if h is not None:
                h.close()
        for b in bufs:
            eng.device_free(b)
        eng.close()


def _regression():
    X = np.array([[-1.0], [-0.3], [0.4], [1.1], [1.9]])
    y = 0.8 * X[:, 0] + np.array([0.1, -0.2, 0.05, 0.3, -0.15])
    return W.ridge_regression(X, y, sigma=0.5, lam=1.0)


@pytest.mark.parametrize("model", ("coin_flip", "regression"))
def test_adaptive_smc_summary_equals_the_restatement_of_the_download(model):
    """256 particles: `pointwise=True, checks=True` equals the restatement applied to adaptive_smc(predictive=True, pointwise=True)'s
    download (the split of the synthetic tests); log_evidence, betas and the existing summary fields are those of the summary without
    the options, bit for bit; weighted_predictive_check / weighted_model_comparison of the download give the summary's bytes; the
    engine's values, weights and state blob are the same before and after."""
    cp = E.compile_model(W.coin_flip() if model == "coin_flip" else _regression())
    N, seed, cfg = 256, 9, I.SMCConfig(rejuvenation_steps=1)
    full = I.adaptive_smc(seed, N, cp, cfg, predictive=True, pointwise=True)
    plain = I.adaptive_smc_summary(seed, N, cp, cfg)
    s = I.adaptive_smc_summary(seed, N, cp, cfg, pointwise=True, checks=True)
    assert plain.comparison is None and plain.checks is None
    assert s.log_evidence == plain.log_evidence == full.log_evidence and np.array_equal(s.betas, plain.betas) and (s.T, s.n_zero, s.ess) == (plain.T, plain.n_zero, plain.ess)
    for name in ("mean", "std", "mcse", "quantiles"):
        assert np.array_equal(_bits(getattr(s, name)), _bits(getattr(plain, name))), name
    w = full.weights
    names = full.predictive_names
    chk = [(list(range(len(names))), PR.ALL, [full.observe_values[a] for a in names])]
    want_c = R.checks(full.predictive.view(np.uint64), full.predictive_vtypes, chk, w)
    c = s.checks
    got_c = dict(slots=list(zip(c.names, c.statistics)), t_obs=c.t_obs, units=c.units, counts=c.counts, p_ge=c.p_ge, p_gt=c.p_gt, p_mid=c.p_mid, W=np.zeros(c.n_slots),
                 mean=c.t_rep_mean, var=c.t_rep_sd ** 2, std=c.t_rep_sd, mcse=c.t_rep_mcse, n_used=c.n_used)
    for k in range(c.n_slots):                       # W and var are not kept by the result: take the restatement's
        got_c["W"][k], got_c["var"][k] = want_c["moments"][k][0], want_c["moments"][k][2]
    assert_checks(got_c, want_c, model)
    assert c.names == ["all"] * 5 and c.statistics == list(CK.STATISTICS) and c.T == s.T and c.n_particles == N
    want_l = R.loglik(full.log_likelihood, w)
    m = s.comparison
    got_l = {n: getattr(m, n) for n in R.FIGURE_NAMES + E.WLL_COUNTS + ("words",)}
    assert_loglik(got_l, want_l, full.log_likelihood, w, model)
    assert m.names == names and m.n_draws == N
    sc, sm = CK.weighted_predictive_check(full), CM.weighted_model_comparison(full)
    for n in ("t_obs", "p_ge", "p_gt", "p_mid", "t_rep_mean", "t_rep_sd", "t_rep_mcse"):
        assert np.array_equal(_bits(getattr(sc, n)), _bits(getattr(c, n))), n
    assert np.array_equal(sc.units, c.units) and np.array_equal(sc.counts, c.counts) and sc.names == c.names
    for n in R.FIGURE_NAMES + ("words",):
        assert np.array_equal(_bits(getattr(sm, n)), _bits(getattr(m, n))), n
    d, se = CM.compare_models(sm, m)
    assert d == 0.0 and (se == 0.0 or se != se)
    # the summary reads the engine and changes nothing
    eng = E.Engine(cp, N, seed=seed)
    try:
        r = eng.smc_run(cfg.resampling_method, cfg.ess_threshold, cfg.rejuvenation_steps, download=False)
        v0, (lw0, w0), b0 = eng.get_values(), eng.smc_weights(), eng.state_export()
        s2 = I.population_summary(eng, r["log_evidence"], r["betas"], pointwise=True, checks=True, stage_words=N)      # one statement per slice
        v1, (lw1, w1), b1 = eng.get_values(), eng.smc_weights(), eng.state_export()
        assert np.array_equal(v0, v1) and np.array_equal(_bits(lw0), _bits(lw1)) and np.array_equal(_bits(w0), _bits(w1)) and b0 == b1
        assert np.array_equal(_bits(w0), _bits(w))
        for n in R.FIGURE_NAMES + ("words",):
            assert np.array_equal(_bits(getattr(s2.comparison, n)), _bits(getattr(m, n))), n
        assert np.array_equal(s2.checks.units, c.units) and np.array_equal(_bits(s2.checks.t_rep_mean), _bits(c.t_rep_mean))
    finally:
        eng.close()


def test_refusals_and_argument_errors(pool):
    """posterior_predictive_check still refuses a weighted population; the entries name their limits."""
    full = I.adaptive_smc(3, 64, W.coin_flip(), I.SMCConfig(rejuvenation_steps=1), predictive=True, pointwise=True)
    with pytest.raises(ValueError, match="weighted"):
        CK.posterior_predictive_check(full)
    w = np.full(64, 1.0 / 64)
    wp, dc = pool.pop(w), pool.upload(np.zeros((1, 64), dtype=np.uint64))
    for bad, text in (([([0], [7], [0.0])], "mask bit"), ([([3], [0], [0.0])], "outside [0, n_rows)"), ([([], [0], [])], "empty")):
        with pytest.raises(E.EngineError) as ei:
            wp.checks(dc, [PR.F64], bad)
        print(ei.value)
        assert ei.value.code == E.FG_E_BAD_ARG and text in str(ei.value) and "fg_wpop_checks" in str(ei.value)
    with pytest.raises(ValueError):
        wp.loglik(dc, 0)
    bad_w = w.copy()
    bad_w[5] = np.nan
    full.weights = bad_w
    for fn in (CK.weighted_predictive_check, CM.weighted_model_comparison):
        with pytest.raises(ValueError, match="n_bad"):
            fn(full)
