"""Exact Gibbs moves on the device (fugue_amd/csrc/fg_gibbs.hip) against the restatement (tests/gibbs_restatement.py) fed with a twin
engine's `Engine.log_joint`: scores bit for bit, conditionals within their derived bound, picks exactly (after the restatement alone
has shown that no pick is on a knife edge), closed-form conditionals, the invariance law, a live session's consistency, the bit-for-bit
invariances, the non-finite rules, the HMC-within-Gibbs driver against an exact 64-term posterior, and every refusal."""
import ctypes as C
import itertools
import math

import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import gibbs as GB
from fugue_amd import inference as I
from fugue_amd import model as M
from fugue_amd import workloads as W
from tests import gibbs_restatement as R
from tests.models import all_dists_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _oracle_built():
    from oracle import oracle as orc
    orc.build()                                               # the uniforms of the restatement come from the oracle's Philox


def _bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


def _twin_scorer(cp, Cn):
    """score(cells [S][Cn]) through Engine.log_joint of a second engine: (prior + likelihood) + factors"""
    twin = E.Engine(cp, Cn, seed=0)

    def score(cells):
        twin.set_values(cells)
        acc = twin.log_joint()
        return (acc[0] + acc[1]) + acc[2]
    return score, twin


@pytest.fixture(scope="module")
def alldists():
    return E.compile_model(all_dists_model())


# ---- scores and picks ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", R.PICK_SHAPES)
def test_scores_conditionals_and_picks_against_the_restatement(alldists, Cn):
    cp = alldists
    sites = R.pick_sites(cp.site_names)
    cell0, n_cells = R.layout(sites)
    eng = E.Engine(cp, Cn, seed=R.PICK_SEED)
    eng.prior_init()
    score, twin = _twin_scorer(cp, Cn)
    u = R.oracle_uniform(R.PICK_SEED)
    g = eng.gibbs(R.PICK_ADDRS)
    assert g.layout["sites"] == [s for s, _, _ in sites] and g.layout["lo"] == [lo for _, lo, _ in sites] and g.layout["K"] == [K for _, _, K in sites]
    assert g.layout["cell0"] == cell0 and g.n_cells == n_cells and g.layout["names"] == list(R.PICK_ADDRS)
    with pytest.raises(E.EngineError) as ei:
        g.probs()
    assert ei.value.code == E.FG_E_STATE
    counts, cond_sum = np.zeros((len(sites), R.COUNTS), dtype=np.int64), np.zeros((n_cells, Cn))
    for t in range(R.PICK_SWEEPS):
        before = eng.get_values()
        want = R.sweep(before, sites, score, u, t)
        # a condition on the inputs, from the restatement alone: no pick within the bound two evaluations can disagree by
        assert want["margin"].min() > 1.0, want["margin"].min()
        assert g.count == t
        out = g.sweep(1, rec_sites=list(range(cp.S)), scores=True, cond=True)
        assert np.array_equal(_bits(out.scores), _bits(want["scores"]))                       # bit for bit
        for (_, _, K), c0 in zip(sites, cell0):
            got, ref = out.cond[c0:c0 + K], want["cond"][c0:c0 + K]
            assert np.all(np.abs(got - ref) <= R.cond_tolerance(K) * ref), (K, np.max(np.abs(got - ref) / ref))
        after = eng.get_values()
        assert np.array_equal(after, want["cells"])                                          # the picks, exactly
        assert np.array_equal(out.rec[0], after)
        counts += want["counts"]
        cond_sum += out.cond
    st = g.stats()
    assert np.array_equal(np.stack([st[n] for n in GB.COUNT_NAMES], axis=1), counts)
    mean, n = g.probs()
    assert n.tolist() == [R.PICK_SWEEPS * Cn] * len(sites)
    pooled = R.pool_sum(cond_sum) / float(R.PICK_SWEEPS * Cn)                                # the fixed tree over the chains, bit for bit
    assert np.array_equal(_bits(np.concatenate(mean)), _bits(pooled))
    g.close(); twin.close(); eng.close()


# ---- conditionals in closed form -------------------------------------------------------------------------------------------------------------
def test_mixture_responsibilities_in_closed_form():
    """C5's pattern at 3 observations, K = 3, every chain at the same mu: probs() is r_ik within (K + 2 + ceil(log2 C)) 2^-52 relative
    (every chain adds the same p_k; the tree's depth is the rest) plus the scorer's 1e-12 (test_log_joint_matches_oracle's tolerance);
    the picks' frequencies within 5 binomial standard errors."""
    K, Cn = 3, 16384
    x, mu = np.array([-1.5, 0.4, 2.2]), np.array([-2.0, 0.5, 3.0])
    cp = E.compile_model(W.mixture(x, K=K))
    eng = E.Engine(cp, Cn, seed=3)
    eng.prior_init()
    v = eng.get_values()
    for k in range(K):
        v[cp.site_names.index(M.addr("mu", k))] = _bits(mu[k:k + 1])[0]
    eng.set_values(v)
    g = eng.gibbs()
    assert g.layout["names"] == [M.addr("z", i) for i in range(3)] and g.layout["K"] == [K] * 3
    g.sweep(1)
    mean, n = g.probs()
    assert n.tolist() == [Cn] * 3
    z = eng.get_values()
    for i in range(3):
        ll = -0.5 * (x[i] - mu) ** 2
        r = np.exp(ll - ll.max()); r /= r.sum()
        tol = (K + 2 + math.ceil(math.log2(Cn))) * R.EPS + 1e-12
        print(f"z#{i}: largest relative error {np.max(np.abs(mean[i] - r) / r):.3g}, bound {tol:.3g}")
        assert np.all(np.abs(mean[i] - r) <= tol * r), (mean[i], r)
        freq = np.bincount(z[cp.site_names.index(M.addr("z", i))], minlength=K) / Cn
        assert np.all(np.abs(freq - r) <= 5.0 * np.sqrt(r * (1.0 - r) / Cn)), (freq, r)
    g.close(); eng.close()


# ---- the invariance law ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["ab", "select"])
def test_invariance_law_on_the_device(which):
    cp = E.compile_model(R.law_program_ab() if which == "ab" else R.law_program_select())
    eng = E.Engine(cp, R.LAW_CHAINS, seed=R.LAW_SEED)
    eng.set_values(R.law_start(which))
    g = eng.gibbs()
    assert [(s, lo, K) for s, lo, K in zip(g.layout["sites"], g.layout["lo"], g.layout["K"])] == R.LAW_SITES
    g.sweep(1)
    assert g.stats()["moved"].min() > R.LAW_CHAINS // 10
    R.judge_law(which, eng.get_values())
    g.close(); eng.close()


# ---- a session stays consistent ----------------------------------------------------------------------------------------------------------------
def _mix8():
    return E.compile_model(W.mixture(W.mixture_data(8, means=(-2.0, 2.0), seed=4)[0], K=2))


def test_an_hmc_session_after_a_sweep_is_the_session_after_set_values():
    cp, Cn = _mix8(), 65
    A, B = E.Engine(cp, Cn, seed=5), E.Engine(cp, Cn, seed=5)
    for e in (A, B):
        e.hmc_init(E.hmc_config(n_leapfrog=4), 4)
        e.hmc_step(3)
    g = A.gibbs()
    g.sweep(1)
    assert g.stats()["moved"].sum() > 0
    B.set_values(A.get_values())
    assert np.array_equal(_bits(A.hmc_log_joint()), _bits(B.hmc_log_joint()))
    rows = []
    for e in (A, B):
        buf = e.device_alloc(2 * cp.d * Cn * 8)
        e.hmc_step(2, buf)
        rows.append(e.download(buf, (1, cp.d, Cn), dtype=np.int64))       # one post-warmup row
        e.device_free(buf)
    assert np.array_equal(rows[0], rows[1]) and np.array_equal(A.get_values(), B.get_values())
    assert np.array_equal(_bits(A.hmc_log_joint()), _bits(B.hmc_log_joint())) and np.array_equal(_bits(A.hmc_step_sizes()), _bits(B.hmc_step_sizes()))
    g.close(); A.close(); B.close()


def test_an_mh_session_after_a_sweep_is_the_session_after_set_values():
    cp, Cn = _mix8(), 65
    A, B = E.Engine(cp, Cn, seed=6), E.Engine(cp, Cn, seed=6)
    for e in (A, B):
        e.mh_init(2)
        e.mh_step(3)
    g = A.gibbs()
    g.sweep(1)
    B.set_values(A.get_values())
    assert np.array_equal(_bits(A.mh_log_weight()), _bits(B.mh_log_weight()))
    rows, rec = [], list(range(cp.S))
    for e in (A, B):
        buf = e.device_alloc(2 * cp.S * Cn * 8)
        e.mh_step(2, rec, buf)
        rows.append(e.download(buf, (2, cp.S, Cn), dtype=np.int64))
        e.device_free(buf)
    assert np.array_equal(rows[0], rows[1]) and np.array_equal(_bits(A.mh_log_weight()), _bits(B.mh_log_weight()))
    g.close(); A.close(); B.close()


# ---- invariances, bit for bit ------------------------------------------------------------------------------------------------------------------
def test_invariances_bit_for_bit(alldists):
    cp = alldists
    whole = E.Engine(cp, 130, seed=R.PICK_SEED)
    whole.prior_init()
    start = whole.get_values()
    parts = [E.Engine(cp, 65, seed=R.PICK_SEED, chain_offset=o) for o in (0, 65)]
    for e, o in zip(parts, (0, 65)):
        e.prior_init()
        assert np.array_equal(e.get_values(), start[:, o:o + 65])
    rec = list(range(cp.S))
    explicit = [a for a in cp.site_names if a in R.PICK_ADDRS]            # site order: what sites=None selects
    gw = whole.gibbs()                                                    # sites=None ...
    assert gw.layout["names"] == explicit
    ow = gw.sweep(3, rec_sites=rec, scores=True, cond=True)               # three sweeps in one call ...
    outs = []
    for e in parts:
        gp = e.gibbs(explicit)                                            # ... against the explicit list,
        assert gp.layout == gw.layout
        steps = [gp.sweep(1, rec_sites=rec, scores=True, cond=True) for _ in range(3)]      # three calls,
        outs.append(steps)
        assert gp.count == 3
        gp.close()
    for k in range(3):                                                    # and engines of 65 + 65 under their chain offsets
        assert np.array_equal(ow.rec[k], np.concatenate([outs[0][k].rec[0], outs[1][k].rec[0]], axis=1)), k
    assert np.array_equal(_bits(ow.scores), _bits(np.concatenate([outs[0][2].scores, outs[1][2].scores], axis=1)))
    assert np.array_equal(_bits(ow.cond), _bits(np.concatenate([outs[0][2].cond, outs[1][2].cond], axis=1)))
    assert np.array_equal(whole.get_values(), ow.rec[2])
    # seek(1) then one sweep against the second sweep of a fresh handle
    again = E.Engine(cp, 130, seed=R.PICK_SEED)
    again.set_values(ow.rec[0])
    ga = again.gibbs()
    ga.seek(1)
    oa = ga.sweep(1, rec_sites=rec)
    assert ga.count == 2 and np.array_equal(oa.rec[0], ow.rec[1])
    ga.seek(0)
    assert not np.array_equal(ga.sweep(1, rec_sites=rec).rec[0], ow.rec[2])       # the sweep index is in the stream
    for h in (gw, ga):
        h.close()
    for e in (whole, again, *parts):
        e.close()


# ---- non-finite ---------------------------------------------------------------------------------------------------------------------------------
def test_a_zero_probability_value_is_never_picked():
    P = M.Program()
    z = P.sample(M.addr("z"), M.Categorical([0.5, 0.0, 0.5]))
    P.observe(M.addr("y"), M.Normal(z, 1.0), 0.7)
    Cn = 4096
    eng = E.Engine(E.compile_model(P), Cn, seed=8)
    eng.prior_init()
    g = eng.gibbs()
    out = g.sweep(1, scores=True, cond=True)
    assert np.all(out.scores[1] == -np.inf) and np.all(out.cond[1] == 0.0) and np.isfinite(out.scores[[0, 2]]).all()
    assert not np.any(eng.get_values()[0] == 1) and set(np.unique(eng.get_values()[0])) == {0, 2}
    st = g.stats()
    assert st["neg_inf_cells"].tolist() == [Cn] and st["nan_cells"].tolist() == [0] and st["stuck"].tolist() == [0]
    mean, n = g.probs()
    assert mean[0][1] == 0.0 and n.tolist() == [Cn] and abs(mean[0].sum() - 1.0) < 1e-12
    g.close(); eng.close()


def test_a_site_without_a_possible_value_is_stuck():
    P = M.Program()
    k = P.sample(M.addr("k"), M.Bernoulli(0.5))
    P.observe(M.addr("y"), M.DiscreteUniform(5, 6), k)
    Cn = 130
    eng = E.Engine(E.compile_model(P), Cn, seed=9)
    eng.prior_init()
    before = eng.get_values()
    g = eng.gibbs()
    out = g.sweep(2, scores=True, cond=True)
    assert np.all(out.scores == -np.inf) and np.isnan(out.cond).all() and np.array_equal(eng.get_values(), before)
    st = g.stats()
    assert st["stuck"].tolist() == [2 * Cn] and st["moved"].tolist() == [0] and st["neg_inf_cells"].tolist() == [4 * Cn]
    mean, n = g.probs()
    assert n.tolist() == [0] and np.isnan(mean[0]).all()
    g.close(); eng.close()


def test_a_nan_score_has_no_weight_and_is_counted():
    P = M.Program()
    j = P.sample(M.addr("j"), M.Categorical([0.25, 0.25, 0.5]))
    P.factor(M.ln(1.0 - j))                                   # 0 at j = 0, -inf at j = 1, NaN at j = 2
    Cn = 65
    eng = E.Engine(E.compile_model(P), Cn, seed=10)
    eng.prior_init()
    g = eng.gibbs()
    out = g.sweep(1, scores=True, cond=True)
    assert np.isfinite(out.scores[0]).all() and np.all(out.scores[1] == -np.inf) and np.isnan(out.scores[2]).all()
    assert np.all(out.cond[0] == 1.0) and np.all(out.cond[1:] == 0.0) and np.all(eng.get_values()[0] == 0)
    st = g.stats()
    assert st["nan_cells"].tolist() == [Cn] and st["neg_inf_cells"].tolist() == [Cn] and st["stuck"].tolist() == [0]
    g.close(); eng.close()


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------------
DRV_X = [-3.4, 2.3, 1.6, -2.7, 2.9, 1.1]                     # six observations drawn once around -3 and 2
DRV_TAU2 = 25.0


def _driver_model():
    P = M.Program()
    mu = P.sample(M.addr("mu"), M.Normal(0.0, 5.0))
    zs = []
    for i, xi in enumerate(DRV_X):
        z = P.sample(M.addr("z", i), M.Bernoulli(0.5))
        P.observe(M.addr("x", i), M.Normal(M.select(z, [-3.0, mu]), 1.0), xi)
        zs.append(z)
    total = zs[0]
    for z in zs[1:]:
        total = total + z
    P.result = {"n1": total, "m0": M.select(zs[0], [-3.0, mu])}
    return P


def _driver_exact():
    """the 64-term enumeration over z, each term conjugate: E[mu], Var[mu], P(z_i = 1)"""
    x = np.array(DRV_X)
    logw, means, variances, zs = [], [], [], []
    for z in itertools.product((0, 1), repeat=6):
        z = np.array(z)
        a, b = x[z == 1], x[z == 0]
        n, s = a.size, a.sum()
        lm = -0.5 * np.sum((b + 3.0) ** 2) - 0.5 * math.log(1.0 + n * DRV_TAU2) - 0.5 * (np.sum(a * a) - DRV_TAU2 * s * s / (1.0 + n * DRV_TAU2))
        logw.append(lm); means.append(DRV_TAU2 * s / (1.0 + n * DRV_TAU2)); variances.append(DRV_TAU2 / (1.0 + n * DRV_TAU2)); zs.append(z)
    w = np.exp(np.array(logw) - max(logw)); w /= w.sum()
    means, variances, zs = np.array(means), np.array(variances), np.array(zs)
    e = float(np.sum(w * means))
    return e, float(np.sum(w * (variances + means ** 2)) - e * e), w @ zs


def test_hmc_gibbs_chain_against_the_exact_posterior():
    Cn = 4096
    prog = _driver_model()
    b = GB.hmc_gibbs_chain(21, prog, 20, 100, I.HMCConfig(), n_chains=Cn)
    e_mu, v_mu, p1 = _driver_exact()
    mu = b.get_f64("mu")
    assert mu.shape == (20, Cn)
    last = mu[-1]
    print(f"mean(mu) {last.mean():.4f} against {e_mu:.4f}, {abs(last.mean() - e_mu) / math.sqrt(v_mu / Cn):.2f} standard errors")
    assert abs(last.mean() - e_mu) <= 5.0 * math.sqrt(v_mu / Cn)
    # the per-chain conditionals of the last draw from the device itself: a handle on an engine that holds the last draw's cells (a label's
    # conditional reads mu and constants only, so a sweep from there returns p(z_i | mu of the last draw) for every chain)
    eng = E.Engine(E.compile_model(prog), Cn, seed=21)
    eng.set_values(np.ascontiguousarray(b.cells[-1]))
    gl = eng.gibbs()
    cond_last = gl.sweep(1, cond=True).cond
    cell0 = dict(zip(gl.layout["names"], gl.layout["cell0"]))
    gl.close(); eng.close()
    for i, xi in enumerate(DRV_X):
        z = b.get_int(M.addr("z", i))
        assert set(np.unique(z)) <= {0, 1}
        f = z[-1].mean()
        assert abs(f - p1[i]) <= 5.0 * math.sqrt(p1[i] * (1.0 - p1[i]) / Cn), (i, f, p1[i])
        # the Rao-Blackwell estimate; its standard error is the sample SE over chains of the device's conditionals at the last draw (the
        # mean over 20 sweeps of a chain varies no more than one sweep's value)
        pc = cond_last[cell0[M.addr("z", i)] + 1]
        assert np.all(np.abs(pc - 1.0 / (1.0 + np.exp(-0.5 * (xi + 3.0) ** 2 + 0.5 * (xi - last) ** 2))) <= 1e-9)
        se = pc.std(ddof=1) / math.sqrt(Cn)
        got = b.gibbs_probs[M.addr("z", i)]
        assert got.shape == (2,) and abs(got.sum() - 1.0) < 1e-12
        assert abs(got[1] - p1[i]) <= 5.0 * se, (i, got, p1[i], se)
        assert z.std(axis=0).max() > 0 or min(p1[i], 1 - p1[i]) < 1e-6      # the labels move over the draws
    assert b.gibbs_stats["sites"] == [M.addr("z", i) for i in range(6)] and b.gibbs_stats["n"].tolist() == [20 * Cn] * 6 and b.gibbs_stats["stuck"].sum() == 0
    # results that read z are right per draw
    zs = np.stack([b.get_int(M.addr("z", i)) for i in range(6)])
    assert np.array_equal(b.get_result("result.n1"), zs.sum(axis=0).astype(np.float64))
    assert np.array_equal(_bits(b.get_result("result.m0")), _bits(np.where(zs[0] == 1, mu, -3.0)))
    # hmc_chain holds the labels: the test tells the two drivers apart
    h = I.hmc_chain(21, prog, 5, 10, I.HMCConfig(), n_chains=130)
    for i in range(6):
        zi = h.get_int(M.addr("z", i))
        assert np.all(zi == zi[0:1])
    assert h.gibbs_probs is None


def test_gibbs_chain_on_a_purely_discrete_model():
    """sweeps only: the rows are the sweeps of a handle run by hand on an engine at the same seed, bit for bit"""
    Cn, prog = 130, R.law_program_ab()
    b = GB.gibbs_chain(R.LAW_SEED, prog, 3, 2, n_chains=Cn)
    assert b.cells.shape == (3, 2, Cn) and b.sites == ["a", "b"] and b.results is None
    eng = E.Engine(E.compile_model(prog), Cn, seed=R.LAW_SEED)
    eng.prior_init()
    g = eng.gibbs()
    g.sweep(2)
    want = g.sweep(3, rec_sites=[0, 1], cond=True)
    assert np.array_equal(b.cells, want.rec)
    g2 = eng.gibbs()                                          # the driver's sums cover the sampling sweeps only
    eng.set_values(np.ascontiguousarray(b.cells[1]))
    g2.seek(4)
    last = g2.sweep(1, cond=True)
    assert np.array_equal(_bits(last.cond), _bits(want.cond))
    assert b.gibbs_stats["n"].tolist() == [3 * Cn] * 2 and set(b.gibbs_probs) == {"a", "b"} and abs(b.gibbs_probs["a"].sum() - 1.0) < 1e-12
    g.close(); g2.close(); eng.close()
    b0 = GB.gibbs_chain(R.LAW_SEED, prog, 0, 2, n_chains=Cn)          # warmup only: no sampling sweep has contributed
    assert b0.cells.shape == (0, 2, Cn) and b0.gibbs_stats["n"].tolist() == [0, 0] and np.isnan(b0.gibbs_probs["b"]).all()


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_with_codes_and_messages(alldists, monkeypatch):
    cp = alldists
    eng = E.Engine(cp, 5, seed=1)
    eng.prior_init()

    def refused(sites, code, word):
        with pytest.raises(E.EngineError) as ei:
            eng.gibbs(sites)
        assert ei.value.code == code and word in str(ei.value), (sites, str(ei.value))
    refused(["a"], E.FG_E_BAD_ARG, "site `a` is not a discrete site")
    refused(["be", "po"], E.FG_E_BAD_ARG, "site `po` has no finite support known from constants")
    refused(["be", "du", "be"], E.FG_E_BAD_ARG, "site `be` is listed twice")
    refused([cp.S], E.FG_E_BAD_ARG, "outside [0, ")
    with pytest.raises(ValueError):
        eng.gibbs(["nope"])
    L = E.lib()
    h = C.c_void_p()
    assert L.fg_gibbs_new(eng.h, None, -1, C.byref(h)) == E.FG_E_BAD_ARG and "n_sites < 0" in E.last_error()
    assert L.fg_gibbs_new(eng.h, None, 2, C.byref(h)) == E.FG_E_BAD_ARG and "null site list" in E.last_error()
    big = M.Program()
    big.sample(M.addr("w"), M.DiscreteUniform(0, GB.K_CAP))
    big.sample(M.addr("ok"), M.DiscreteUniform(1, GB.K_CAP))
    cb = E.compile_model(big)
    eb = E.Engine(cb, 3, seed=1)
    eb.prior_init()
    with pytest.raises(E.EngineError) as ei:
        eb.gibbs(["w"])
    assert ei.value.code == E.FG_E_LIMIT and "site `w` has 4097 values" in str(ei.value)
    gb = eb.gibbs()                                           # the automatic list leaves `w` out and keeps the 4096 values of `ok`
    assert gb.layout["names"] == ["ok"] and gb.layout["K"] == [GB.K_CAP] and gb.layout["lo"] == [1]
    out = gb.sweep(1, cond=True)
    assert np.all(np.abs(out.cond * GB.K_CAP - 1.0) <= R.cond_tolerance(GB.K_CAP))      # uniform over its support
    gb.close(); eb.close()
    none = M.Program()
    none.sample(M.addr("x"), M.Normal(0.0, 1.0))
    none.sample(M.addr("p"), M.Poisson(2.0))
    en = E.Engine(E.compile_model(none), 2, seed=1)
    with pytest.raises(E.EngineError) as ei:
        en.gibbs()
    assert ei.value.code == E.FG_E_BAD_ARG and "no discrete site" in str(ei.value)
    en.close()
    g = eng.gibbs()
    one = (C.c_int32 * 1)(cp.S)
    assert L.fg_gibbs_sweep(g.h, -1, None, 0, None, None, None) == E.FG_E_BAD_ARG and "n_sweeps < 0" in E.last_error()
    assert L.fg_gibbs_sweep(g.h, 1, one, 1, None, None, None) == E.FG_E_BAD_ARG and "recorded site" in E.last_error()
    assert L.fg_gibbs_sweep(g.h, 1, None, 1, None, None, None) == E.FG_E_BAD_ARG
    buf = eng.device_alloc(64)
    assert L.fg_gibbs_sweep(g.h, 1, None, 0, buf, None, None) == E.FG_E_BAD_ARG and "d_rec without" in E.last_error()
    eng.device_free(buf)
    assert L.fg_gibbs_seek(g.h, -1) == E.FG_E_BAD_ARG and L.fg_gibbs_seek(g.h, 1 << 32) == E.FG_E_BAD_ARG
    g.seek((1 << 32) - 1)
    assert L.fg_gibbs_sweep(g.h, 2, None, 0, None, None, None) == E.FG_E_LIMIT and g.count == (1 << 32) - 1
    assert L.fg_gibbs_sweep(g.h, 0, None, 0, None, None, None) == 0 and L.fg_gibbs_probs(g.h, None, None) == E.FG_E_STATE
    assert L.fg_gibbs_stats(g.h, None) == E.FG_E_BAD_ARG
    g.close()
    with pytest.raises(ValueError):
        g.sweep(1)
    eng.close()
    monkeypatch.setenv("FG_GLOBAL_TILE", "1")                 # any program through the global-tile instantiations (fg_engine_new)
    gt = E.Engine(cp, 5, seed=1)
    try:
        gt.prior_init()
        with pytest.raises(E.EngineError) as ei:
            gt.gibbs()
        assert ei.value.code == E.FG_E_LIMIT and "global memory" in str(ei.value)
    finally:
        gt.close()
