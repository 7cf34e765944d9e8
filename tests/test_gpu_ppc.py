"""GPU tests of the posterior predictive check stream (fg_ppc_stream.hip): the pooled counters and moments and the per-chain counters
do not depend on the chunking, bit for bit; device against the Python restatement, exactly (counters, T_obs, mean and ssd bits: no
transcendental is involved); hmc_chain_summary / adaptive_mcmc_chain_summary(checks=...) against posterior_predictive_check of the
stored replicates of the same run, bit for bit; a selection; the Beta-Binomial law of the prior predictive number of heads; the call
order; a session is left as it was; weighted input is refused.

Synthetic cell tables (tests/ppc_restatement.py: N(0, 1), constant, Bernoulli bool cells, u64 cells at and above 2^53, negative i64,
rows with NaN / +inf / -inf cells) are uploaded once; a chunk is a slice of that buffer.  Every compared figure is printed before it is
asserted."""
import numpy as np
import pytest

from fugue_amd import checks as K
from fugue_amd import engine as E
from fugue_amd import inference as I
from fugue_amd import workloads as W
from tests import ppc_restatement as R
from tests.models import ZOO

pytestmark = pytest.mark.gpu

FG_E_BAD_ARG, FG_E_STATE = -3, -5
CS = (1, 63, 64, 65, 192, 600)          # a partial wave, a full one, pass-through in the tree, three waves, three blocks and a second level
NS = (1, 2, 40)                         # 40: three pieces of the scratch table (16, 16, 8)
KINDS = ("normal",) * 9 + ("bernoulli", "u64_big", "neg_i64", "nan", "pos_inf", "neg_inf", "constant")


class _Engines:
    """One engine per chain count for the whole module (the model does not matter to the stream)."""

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


def _configs(seed):
    """(label, checks as (rows, mask, observed)): one check of K = 1, 2, 9 members with all five statistics, and three checks with
    different masks, K = 9, 2 and 1 and a shared row, over the non-finite and discrete rows too."""
    rng = np.random.default_rng(seed)
    obs = [float(v) for v in rng.normal(0.0, 1.0, 9)]
    one = [(f"one check K {k}", [(list(range(k)), R.ALL, obs[:k])]) for k in (1, 2, 9)]
    three = [([0, 12, 1, 13, 2, 14, 3, 15, 4], R.ALL, obs),                                   # NaN, +inf, -inf cells and the constant row among normal ones
             ([9, 4], (1 << R.SUM) | (1 << R.MIN), [1.0, 0.25]),                              # a bool row and a row shared with the first check
             ([10], (1 << R.MEAN) | (1 << R.VAR) | (1 << R.MAX), [float(2 ** 53 + 2)])]       # u64 at and above 2^53; K = 1 with the variance bit
    more = [([11, 9, 11], (1 << R.MEAN) | (1 << R.MAX), [-2.0, 1.0, 0.0]), ([5], 1 << R.MEAN, [float("nan")]), ([15], R.ALL, [R.CONSTANT])]
    return one + [("three checks", three), ("i64 / NaN observed / constant", more)]


def _feed(eng, ptr, shape, vtypes, checks, chunks):
    n, n_rows, C = shape
    s = eng.ppc_stream(n, vtypes, [(rows, [st for st in range(5) if (mask >> st) & 1], obs) for rows, mask, obs in checks])
    try:
        at = 0
        for nc in chunks:
            s.update(ptr + at * n_rows * C * 8, nc)
            at += nc
            assert s.count() == at
        return dict(pooled=s.pooled(), t_obs=s.observed(), chains=[s.chains(k) for k in range(s.n_slots)], slots=list(s.slots))
    finally:
        s.free()


def _chunkings(n):
    return [(n,)] + ([(1, 7, n - 8)] if n > 8 else ([(1,) * n] if n > 1 else []))


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("C", CS)
def test_counters_and_moments_do_not_depend_on_the_chunking_and_equal_the_restatement(engines, C, n):
    """One chunk against (1, 7, rest) (n = 2: (1, 1)), device against device: pooled counters, mean and ssd, and chains(slot), bit-equal.
    Against the restatement everything is exact: T_obs, the counters pooled and per chain, the mean and ssd bits."""
    _check_configs(engines.get(C), C, n, _configs(C))


def test_a_tree_of_three_levels(engines):
    """C = 65 537 chains: 65 537 -> 257 -> 2 -> 1, the last block of every level partial.  One check of one N(0, 1) member, its mean,
    one draw; held to what the test above holds every configuration to."""
    _check_configs(engines.get(65537), 65537, 1, [("one member", [([0], 1 << R.MEAN, [0.25])])])


def _check_configs(eng, C, n, configs):
    x, vtypes = R.table(KINDS, n, C, seed=C)
    ptr = eng.upload(x)
    try:
        for label, checks in configs:
            runs = [_feed(eng, ptr, x.shape, vtypes, checks, ch) for ch in _chunkings(n)]
            got = runs[0]
            for other in runs[1:]:
                for f in R_COUNTS:
                    assert np.array_equal(other["pooled"][f], got["pooled"][f]), (label, f)
                for f in ("mean", "ssd"):
                    assert np.array_equal(_bits(other["pooled"][f]), _bits(got["pooled"][f])), (label, f, "differs between chunkings")
                for a, b in zip(other["chains"], got["chains"]):
                    assert all(np.array_equal(a[f], b[f]) for f in R_COUNTS), (label, "chains differ between chunkings")
            want = R.stream(x, vtypes, checks)
            assert got["slots"] == R.slots_of(checks)
            for k, (q, st) in enumerate(got["slots"]):
                counts = [int(got["pooled"][f][k]) for f in R_COUNTS]
                mom = [float(got["pooled"]["mean"][k]), float(got["pooled"]["ssd"][k])]
                print(f"C {C} n {n} {label} check {q} {R.STAT_NAMES[st]}: T_obs {float(got['t_obs'][k])!r} / {want['t_obs'][k]!r}; counts {counts} / {want['counts'][k]}; "
                      f"mean, ssd {mom} / {want['moments'][k]}")
                assert R.bits(got["t_obs"][k]) == R.bits(want["t_obs"][k])
                assert counts == want["counts"][k]
                assert [R.bits(v) for v in mom] == [R.bits(v) for v in want["moments"][k]]
                assert [got["chains"][k][f].tolist() for f in R_COUNTS] == want["chains"][k]
                assert sum(counts[:4]) == n * C
    finally:
        eng.device_free(ptr)


R_COUNTS = E.PPC_COUNTS


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
FIELDS = ("t_obs", "n_lt", "n_eq", "n_gt", "n_nan", "n_fin", "t_rep_mean", "t_rep_ssd", "chain_sd", "p_ge", "p_gt", "p_mid", "t_rep_sd")


def _view(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _same_check(label, a, b, slots_b=None):
    """Every field of a equals the field of b (at the slots `slots_b` of b), bit for bit."""
    idx = list(range(b.n_slots)) if slots_b is None else list(slots_b)
    assert a.names == [b.names[k] for k in idx] and a.statistics == [b.statistics[k] for k in idx], (label, a.names, a.statistics)
    assert (a.n_draws, a.n_chains) == (b.n_draws, b.n_chains)
    for f in FIELDS:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))[idx]
        print(f"{label} {f}: {x.tolist()}")
        assert x.dtype == y.dtype and np.array_equal(_view(x), _view(y)), (label, f, x, y)


def _same_summary(label, a, b, fields=("mean", "std", "r_hat", "ess")):
    assert a.sites == b.sites and (a.n_samples, a.n_chains, a.passes) == (b.n_samples, b.n_chains, b.passes)
    for f in fields:
        assert np.array_equal(_bits(getattr(a, f)), _bits(getattr(b, f))), (label, f)
    assert _bits(np.float64(a.accept_rate)) == _bits(np.float64(b.accept_rate)) and a.n_divergent == b.n_divergent


@pytest.mark.parametrize("model", ("readme", "hier"))
def test_hmc_chain_summary_checks_is_the_check_of_the_stored_replicates(monkeypatch, model):
    """readme_normal (one f64 observe) and hier (several): 40 draws in chunks of 16 from 128 chains."""
    monkeypatch.setenv("FG_JIT", "0")
    a = dict(seed=21, model_fn=E.compile_model(ZOO[model]()), n_samples=40, n_warmup=20, n_chains=128)
    summ = I.hmc_chain_summary(chunk=16, checks=True, **a)
    plain = I.hmc_chain_summary(chunk=16, **a)
    chains = I.hmc_chain(predictive=True, **a)
    assert plain.checks is None and summ.checks is not None
    stored = K.posterior_predictive_check(chains)
    _same_check(f"hmc {model}", summ.checks, stored)
    pc = summ.checks
    assert pc.names == ["all"] * 5 and pc.statistics == list(K.STATISTICS) and pc.n_draws == 40 * 128
    assert ((pc.n_lt + pc.n_eq + pc.n_gt + pc.n_nan) == 40 * 128).all() and (pc.n_nan[[0, 2, 3, 4]] == 0).all()
    # the host's own arithmetic on the stored replicates, for the in-order sum
    y = np.stack([chains.get_predictive(name) for name in chains.predictive_names], axis=1)          # [n][O][C] float64
    total = np.zeros((40, 128))
    for k in range(y.shape[1]):
        total = total + y[:, k, :]
    t_obs = 0.0
    for name in chains.predictive_names:
        t_obs += chains.observe_values[name]
    k = pc.slot("all", "sum")
    print(f"sum: T_obs {float(pc.t_obs[k])!r} / {t_obs!r}; n_gt {int(pc.n_gt[k])} / {int((total > t_obs).sum())}; p_ge {float(pc.p_ge[k])!r}")
    assert float(pc.t_obs[k]) == t_obs and int(pc.n_gt[k]) == int((total > t_obs).sum()) and int(pc.n_lt[k]) == int((total < t_obs).sum())
    assert 0.0 < pc.p_mid[k] < 1.0 and np.isfinite(pc.between_chain_sd(k))
    _same_summary(f"hmc {model}", summ, plain)
    assert summ.predictive is None and summ.comparison is None and summ.results is None


@pytest.fixture(scope="module")
def coin_runs():
    import os
    old = os.environ.get("FG_JIT")
    os.environ["FG_JIT"] = "0"
    try:
        a = dict(seed=22, model_fn=E.compile_model(W.coin_flip()), n_samples=40, n_warmup=20, n_chains=128)
        return dict(args=a, chains=I.adaptive_mcmc_chain(predictive=True, **a), plain=I.adaptive_mcmc_chain_summary(chunk=16, **a),
                    full=[I.adaptive_mcmc_chain_summary(chunk=c, checks=True, **a) for c in (16, 7)])
    finally:
        if old is None:
            del os.environ["FG_JIT"]
        else:
            os.environ["FG_JIT"] = old


def test_adaptive_mcmc_chain_summary_checks_with_bernoulli_observe_sites(coin_runs):
    """W.coin_flip(): ten Bernoulli observe sites (bool cells), nothing converted on the host; chunk sizes 16 and 7."""
    stored = K.posterior_predictive_check(coin_runs["chains"])
    assert coin_runs["chains"].predictive_vtypes == [1] * 10 and coin_runs["plain"].checks is None
    for summ, chunk in zip(coin_runs["full"], (16, 7)):
        _same_check(f"mh coin chunk {chunk}", summ.checks, stored)
        _same_summary(f"mh coin chunk {chunk}", summ, coin_runs["plain"])
    pc = coin_runs["full"][0].checks
    k = pc.slot("all", "sum")
    heads = coin_runs["chains"].predictive.sum(axis=1)                # [n][C] integers
    print(f"heads: T_obs {float(pc.t_obs[k])}, n_lt n_eq n_gt {int(pc.n_lt[k])} {int(pc.n_eq[k])} {int(pc.n_gt[k])}, p_ge {float(pc.p_ge[k])}, p_mid {float(pc.p_mid[k])}")
    assert float(pc.t_obs[k]) == 7.0
    assert [int(pc.n_lt[k]), int(pc.n_eq[k]), int(pc.n_gt[k])] == [int((heads < 7).sum()), int((heads == 7).sum()), int((heads > 7).sum())]
    assert 0.05 < pc.p_ge[k] < 0.95                                   # the tutorial's reading: the model that made the data is not rejected


def test_a_selection_by_check_spec_holds_the_slots_of_the_full_check(coin_runs):
    full = coin_runs["full"][0].checks
    names = coin_runs["chains"].predictive_names
    sel = I.adaptive_mcmc_chain_summary(chunk=16, checks=[K.CheckSpec("all", names, ("sum", "mean"))], **coin_runs["args"]).checks
    _same_check("selection", sel, full, [full.slot("all", "mean"), full.slot("all", "sum")])
    # marginal checks over two of the flips: the rows of the cell buffer are the union of the members, not all ten
    pick = [names[6], names[1]]
    marg = I.adaptive_mcmc_chain_summary(chunk=16, checks=K.marginal_checks(pick), **coin_runs["args"]).checks
    stored = K.posterior_predictive_check(coin_runs["chains"], K.marginal_checks(pick))
    _same_check("marginal", marg, stored)
    assert marg.names == pick and marg.t_obs.tolist() == [1.0, 0.0]
    with pytest.raises(ValueError):
        I.adaptive_mcmc_chain_summary(chunk=16, checks=[K.CheckSpec("c", ["nope"])], **coin_runs["args"])


def test_observed_values_that_read_a_site_need_an_override(monkeypatch):
    from tests.models import all_dists_model
    from fugue_amd import model as M
    pp = I.prior_predictive(5, all_dists_model(), n_chains=64)
    with pytest.raises(ValueError, match="o#0"):
        K.posterior_predictive_check(pp)
    o4, o1 = M.addr("o", 4), M.addr("o", 1)
    with pytest.raises(ValueError, match="o#4"):
        K.posterior_predictive_check(pp, K.marginal_checks([o1, o4]))
    pc = K.posterior_predictive_check(pp, K.marginal_checks([o1, o4]), observed={o4: 1.0})
    y1, y4 = pp.get_predictive(o1), pp.get_predictive(o4)
    print(pc.t_obs, pc.n_lt, pc.n_eq, pc.n_gt)
    assert pc.t_obs.tolist() == [0.25, 1.0]
    assert [int(pc.n_lt[0]), int(pc.n_gt[0])] == [int((y1 < 0.25).sum()), int((y1 > 0.25).sum())]
    assert [int(pc.n_lt[1]), int(pc.n_eq[1]), int(pc.n_gt[1])] == [int((y4 < 1).sum()), int((y4 == 1).sum()), 0]


# ---- a law --------------------------------------------------------------------------------------------------------------------------
def test_prior_predictive_number_of_heads_follows_the_beta_binomial():
    """4 096 independent prior predictive draws of W.coin_flip(): the number of heads is Beta-Binomial(10, 2, 2), the observed sum is 7,
    so (n_lt, n_eq, n_gt) is multinomial with probabilities 196 / 286, 32 / 286, 58 / 286; each count within 5 sqrt(C p (1 - p)) of C p.
    The mean slot compares s / 10 with 7 / 10: the same three counts."""
    C = 4096
    pp = I.prior_predictive(31, W.coin_flip(), n_chains=C)
    pc = K.posterior_predictive_check(pp, [K.CheckSpec("heads", pp.predictive_names, ("sum", "mean"))])
    ks, km = pc.slot("heads", "sum"), pc.slot("heads", "mean")
    got = [int(pc.n_lt[ks]), int(pc.n_eq[ks]), int(pc.n_gt[ks])]
    law = R.coin_law(C)
    print(f"T_obs {float(pc.t_obs[ks])}; n_lt n_eq n_gt {got}; expected {[round(m, 1) for m, _ in law]} +- {[round(h, 1) for _, h in law]}; "
          f"mean slot {[int(pc.n_lt[km]), int(pc.n_eq[km]), int(pc.n_gt[km])]}")
    assert float(pc.t_obs[ks]) == 7.0 and float(pc.t_obs[km]) == 0.7 and sum(got) == C and int(pc.n_nan[ks]) == 0
    for g, (m, h) in zip(got, law):
        assert abs(g - m) <= h
    assert [int(pc.n_lt[km]), int(pc.n_eq[km]), int(pc.n_gt[km])] == got
    heads = pp.predictive.sum(axis=0)
    assert got == [int((heads < 7).sum()), int((heads == 7).sum()), int((heads > 7).sum())]


# ---- call order, arguments, state ---------------------------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(E.EngineError) as ei:
        fn()
    print(ei.value)
    return ei.value.code


def test_call_order_and_arguments(engines):
    eng = engines.get(65)
    x, vtypes = R.table(["normal", "bernoulli"], 10, 65)
    checks = [([0, 1], ["mean", "sum"], [0.5, 1.0])]
    ptr = eng.upload(x)
    try:
        s = eng.ppc_stream(10, vtypes, checks)
        assert s.n_slots == 2 and s.slots == [(0, 0), (0, 4)] and s.observed().tolist() == [0.75, 1.5]
        s.update(ptr, 0)                                         # n_chunk == 0 is FG_OK and takes no draw (a launch cannot be seen from here)
        assert s.count() == 0
        s.update(ptr, 4)
        assert _code(s.pooled) == FG_E_STATE and _code(lambda: s.chains(0)) == FG_E_STATE
        assert _code(lambda: s.update(ptr, 7)) == FG_E_STATE and s.count() == 4
        s.update(ptr + 4 * 2 * 65 * 8, 0)
        s.update(ptr + 4 * 2 * 65 * 8, 6)
        assert s.count() == 10
        assert _code(lambda: s.update(ptr, 1)) == FG_E_STATE
        got, per_chain = s.pooled(), [s.chains(k) for k in range(2)]
        again = s.pooled()                                       # a read-out changes nothing
        assert all(np.array_equal(_view(got[f]), _view(again[f])) for f in got)
        s.update(ptr, 0)                                         # nor does an empty chunk at the end of the stream: the same bits, pooled and per chain
        assert s.count() == 10
        after = s.pooled()
        assert all(np.array_equal(_view(got[f]), _view(after[f])) for f in got)
        assert all(np.array_equal(per_chain[k][f], s.chains(k)[f]) for k in range(2) for f in per_chain[k])
        assert _code(lambda: s.chains(2)) == FG_E_BAD_ARG and _code(lambda: s.chains(-1)) == FG_E_BAD_ARG
        s.free()
        s.free()
        with pytest.raises(ValueError):
            s.count()
        one = _feed(eng, ptr, x.shape, vtypes, [([0, 1], (1 << R.MEAN) | (1 << R.SUM), [0.5, 1.0])], (10,))["pooled"]
        assert all(np.array_equal(_view(got[f]), _view(one[f])) for f in got)
    finally:
        eng.device_free(ptr)
    assert _code(lambda: eng.ppc_stream(0, vtypes, checks)) == FG_E_BAD_ARG
    assert _code(lambda: eng.ppc_stream(10, vtypes, [])) == FG_E_BAD_ARG
    assert _code(lambda: eng.ppc_stream(10, vtypes, [([], ["mean"], [])])) == FG_E_BAD_ARG
    assert _code(lambda: eng.ppc_stream(10, vtypes, [([0], [], [1.0])])) == FG_E_BAD_ARG
    assert _code(lambda: eng.ppc_stream(10, vtypes, [([0], [5], [1.0])])) == FG_E_BAD_ARG
    assert _code(lambda: eng.ppc_stream(10, vtypes, [([2], ["mean"], [1.0])])) == FG_E_BAD_ARG
    assert _code(lambda: eng.ppc_stream(10, [0, 9], checks)) == FG_E_BAD_ARG
    with pytest.raises(TypeError):
        eng.ppc_stream(1.5, vtypes, checks)
    with pytest.raises(ValueError):
        eng.ppc_stream(10, vtypes, [([0, 1], ["mean"], [1.0])])


def test_an_update_between_steps_changes_nothing_of_a_session(monkeypatch):
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
            y, _ = eng.predict_eval(buf, 5, loglik=False)
            s = eng.ppc_stream(5, cp.observe_vtypes, [(list(range(cp.O)), list(range(5)), cp.observe_values)])
            s.update(y, 5)
            res = s.pooled()
            assert (res["n_lt"] + res["n_eq"] + res["n_gt"] == 5 * C).all() and not res["n_nan"].any()
            s.free()
            eng.device_free(y)
        eng.hmc_step(5, buf + 5 * cp.d * C * 8)
        seen.append(dict(draws=eng.download(buf, (10, cp.d, C), dtype=np.int64), values=eng.get_values(), lj=eng.hmc_log_joint(), eps=eng.hmc_step_sizes(),
                         state=np.frombuffer(eng.state_export(), dtype=np.uint8), accept=np.float64(eng.hmc_stats().accept_rate)))
        eng.device_free(buf)
        eng.close()
    for k in seen[0]:
        a, b = (np.atleast_1d(np.ascontiguousarray(seen[j][k])) for j in (1, 0))
        print(f"{k}: equal {a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))}")
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), k


def test_weighted_input_is_refused():
    smc = I.adaptive_smc(7, 64, W.coin_flip(), predictive=True)
    assert smc.predictive is not None
    with pytest.raises(ValueError, match="weighted"):
        K.posterior_predictive_check(smc)
    with pytest.raises(ValueError):
        K.posterior_predictive_check(I.hmc_chain(3, W.readme_normal(), 4, 2, n_chains=8))     # no stored replicates
