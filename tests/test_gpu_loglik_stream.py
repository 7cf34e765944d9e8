"""GPU tests of the log-likelihood stream (fg_loglik_stream.hip): the pooled words do not depend on the chunking, bit for bit; device
against the Python restatement (counters, classes and the moment words exact, the figures through exp within (N + 8) 2^-52);
hmc_chain_summary / adaptive_mcmc_chain_summary(pointwise=...) against model_comparison of the stored table of the same run, bit for
bit; the selection; the call order; a session is left as it was.

Synthetic tables (tests/loglik_stream_restatement.py: N(-3, 1), a row near -1e4 with spread 800, monotone and constant rows, rows with
-inf / +inf / NaN cells) are uploaded once; a chunk is a slice of that buffer.  Every compared figure is printed before it is asserted."""
import numpy as np
import pytest

from fugue_amd import comparison as CMP
from fugue_amd import engine as E
from fugue_amd import inference as I
from fugue_amd import workloads as W
from tests import loglik_stream_restatement as L
from tests.models import ZOO

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
FG_E_BAD_ARG, FG_E_STATE = -3, -5
CS = (1, 63, 64, 65, 192, 600)          # a partial wave, a full one, pass-through in the tree, three waves, three blocks and a second level
NS = (1, 2, 40)
KINDS3 = (("normal", "far", "neg_inf"), ("increasing", "decreasing", "nan"), ("constant", "pos_inf", "all_neg_inf"), ("both_inf", "normal", "far"))


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


def _feed(eng, ptr, shape, chunks, read=("pooled", "result")):
    n, n_sel, C = shape
    s = eng.loglik_stream(n, n_sel)
    try:
        at = 0
        for nc in chunks:
            s.update(ptr + at * n_sel * C * 8, nc)
            at += nc
            assert s.count() == at
        return tuple(getattr(s, r)() for r in read)
    finally:
        s.free()


def _chunkings(n):
    return [(n,)] + ([(1, 7, n - 8)] if n > 8 else ([(1,) * n] if n > 1 else []))


def _tables(n, C):
    out = [(k, L.table(list(k), n, C, seed=C)) for k in KINDS3]
    out += [((k,), L.table([k], n, C, seed=C + 1)) for k in ("far", "neg_inf")]
    return out


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("C", CS)
def test_pooled_words_do_not_depend_on_the_chunking_and_match_the_restatement(engines, C, n):
    """n_sel = 3 and 1.  One chunk against (1, 7, rest) (n = 2: (1, 1)): bit-equal pooled words, device against device.  Against the
    restatement: counters exact; n_fin, mean, ssd bit-equal (no transcendental; -ffp-contract=off), so mean_ll and p_waic are exact;
    figures in the same class (NaN / +-inf / finite); lppd and elpd_loo within (N + 8) 2^-52 absolute, is_ess and max_weight within
    the same bound relative (ocml's exp against glibc's, each within an ulp or two, in a sum of N positive terms)."""
    _check_tables(engines.get(C), C, n, _tables(n, C))


def test_a_tree_of_three_levels(engines):
    """C = 65 537 chains: 65 537 -> 257 -> 2 -> 1, the last block of every level partial.  One statement with a -inf cell, one draw;
    held to what the test above holds every table to."""
    _check_tables(engines.get(65537), 65537, 1, [(("neg_inf",), L.table(["neg_inf"], 1, 65537, seed=3))])


def _check_tables(eng, C, n, tables):
    N = n * C
    bound = (N + 8) * EPS
    worst = dict(lppd=0.0, elpd_loo=0.0, is_ess=0.0, max_weight=0.0)
    for kinds, x in tables:
        ptr = eng.upload(x)
        try:
            runs = [_feed(eng, ptr, x.shape, ch) for ch in _chunkings(n)]
        finally:
            eng.device_free(ptr)
        pooled, res = runs[0]
        for other, _ in runs[1:]:
            assert np.array_equal(_bits(other["words"]), _bits(pooled["words"])), (kinds, "pooled words differ between chunkings")
            assert np.array_equal(other["counts"], pooled["counts"])
        want_e, want_f = L.stream(x)
        for k, kind in enumerate(kinds):
            we, wf = want_e[k], dict(zip(L.FIGURE_NAMES, want_f[k]))
            got = {name: float(res[name][k]) for name in L.FIGURE_NAMES}
            words = pooled["words"][k]
            print(f"C {C} n {n} {kind}: counts {pooled['counts'][k].tolist()} / {we[8:]}; n, mean, ssd {words[5:8].tolist()} / {we[5:8]}")
            print("   device      ", [f"{got[m]!r}" for m in L.FIGURE_NAMES])
            print("   restatement ", [f"{wf[m]!r}" for m in L.FIGURE_NAMES])
            assert pooled["counts"][k].tolist() == list(we[8:])
            assert [int(res[c][k]) for c in ("n_neg_inf", "n_pos_inf", "n_nan")] == list(we[8:])
            assert [L.bits(v) for v in words[5:8]] == [L.bits(v) for v in we[5:8]], "n_fin, mean, ssd"
            for m in L.FIGURE_NAMES:
                assert L.same_class(got[m], wf[m]), (kind, m, got[m], wf[m])
            for m in ("mean_ll", "p_waic"):
                assert L.bits(got[m]) == L.bits(wf[m]), (kind, m, got[m], wf[m])
            for m in ("lppd", "elpd_loo"):
                if np.isfinite(wf[m]):
                    err = abs(got[m] - wf[m])
                    worst[m] = max(worst[m], err / bound)
                    print(f"   {m} abs err {err:.3e} bound {bound:.3e}")
                    assert err <= bound, (kind, m, got[m], wf[m])
            for m in ("is_ess", "max_weight"):
                if np.isfinite(wf[m]):
                    err = abs(got[m] - wf[m]) / abs(wf[m])
                    worst[m] = max(worst[m], err / bound)
                    print(f"   {m} rel err {err:.3e} bound {bound:.3e}")
                    assert err <= bound, (kind, m, got[m], wf[m])
    print(f"C {C} n {n}: largest error / bound {worst}")


# ---- end to end ---------------------------------------------------------------------------------------------------------------------
COMPARED = CMP.POINTWISE + ("n_neg_inf", "n_pos_inf", "n_nan")


def _same_comparison(label, a, b):
    assert a.names == b.names and a.n_draws == b.n_draws, (label, a.names, b.names)
    for f in COMPARED:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        print(f"{label} {f}: {x.tolist()}")
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y), (label, f, x, y)


def _same_summary(label, a, b, fields=("mean", "std", "r_hat", "ess")):
    assert a.sites == b.sites and (a.n_samples, a.n_chains, a.passes) == (b.n_samples, b.n_chains, b.passes)
    for f in fields:
        assert np.array_equal(_bits(getattr(a, f)), _bits(getattr(b, f))), (label, f)
    assert _bits(np.float64(a.accept_rate)) == _bits(np.float64(b.accept_rate)) and _bits(np.float64(a.mean_step_size)) == _bits(np.float64(b.mean_step_size))
    assert a.n_divergent == b.n_divergent


@pytest.fixture(scope="module")
def hmc_runs():
    """hier (20 observe statements), 40 draws in chunks of 16 from 128 chains: the streamed summary, the plain one, the stored chains."""
    import os
    old = os.environ.get("FG_JIT")
    os.environ["FG_JIT"] = "0"
    try:
        a = dict(seed=11, model_fn=E.compile_model(ZOO["hier"]()), n_samples=40, n_warmup=20, n_chains=128)
        return dict(args=a, summ=I.hmc_chain_summary(chunk=16, pointwise=True, **a), plain=I.hmc_chain_summary(chunk=16, **a),
                    chains=I.hmc_chain(pointwise=True, **a))
    finally:
        if old is None:
            del os.environ["FG_JIT"]
        else:
            os.environ["FG_JIT"] = old


def test_hmc_chain_summary_pointwise_is_model_comparison_of_the_stored_table(hmc_runs):
    summ, plain, chains = hmc_runs["summ"], hmc_runs["plain"], hmc_runs["chains"]
    cmp_ = summ.comparison
    assert plain.comparison is None and cmp_ is not None and len(cmp_.names) >= 3 and cmp_.names == chains.predictive_names
    assert chains.log_likelihood.shape == (40, len(cmp_.names), 128) and cmp_.n_draws == 40 * 128
    stored = CMP.model_comparison(chains)
    _same_comparison("hmc hier", cmp_, stored)
    assert np.isfinite(cmp_.elpd_loo).all() and np.isfinite(cmp_.elpd_waic).all() and (cmp_.is_ess >= 1.0).all() and (cmp_.p_waic >= 0.0).all()
    # the host two-pass formulas on the stored table, loosely (the CPU tests hold the tight bounds): the figures are those of this table
    for k in (0, len(cmp_.names) - 1):
        want = dict(zip(L.FIGURE_NAMES, L.two_pass(chains.log_likelihood[:, k, :])))
        for f in ("lppd", "elpd_loo", "p_waic", "mean_ll"):
            print(f"{cmp_.names[k]} {f}: device {float(getattr(cmp_, f)[k])!r} two-pass {want[f]!r}")
            assert abs(float(getattr(cmp_, f)[k]) - want[f]) <= 1e-9 * max(1.0, abs(want[f]))
    total = 0.0
    for v in cmp_.elpd_loo.tolist():
        total += v
    assert cmp_.elpd_loo_total == total and cmp_.se("elpd_loo") > 0.0
    _same_summary("hmc hier", summ, plain)
    assert summ.results is None and summ.predictive is None and summ.discrete is None and summ.quantiles is None


def test_adaptive_mcmc_chain_summary_pointwise_with_discrete_observe_sites(monkeypatch):
    """hier_scale: Bernoulli and Poisson observe statements beside the f64 ones; discrete=True records every site."""
    monkeypatch.setenv("FG_JIT", "0")
    a = dict(seed=12, model_fn=E.compile_model(ZOO["hier_scale"]()), n_samples=40, n_warmup=20, n_chains=128)
    summ = I.adaptive_mcmc_chain_summary(chunk=16, discrete=True, pointwise=True, **a)
    plain = I.adaptive_mcmc_chain_summary(chunk=16, discrete=True, **a)
    chains = I.adaptive_mcmc_chain(pointwise=True, **a)
    cmp_ = summ.comparison
    assert plain.comparison is None and "flip#0" in cmp_.names and "count" in cmp_.names and cmp_.names == chains.predictive_names
    _same_comparison("mh hier_scale", cmp_, CMP.model_comparison(chains))
    _same_summary("mh hier_scale", summ, plain)
    assert summ.discrete.sites == plain.discrete.sites and all(np.array_equal(x, y) for x, y in zip(summ.discrete.counts, plain.discrete.counts))


def test_a_selection_holds_the_rows_of_the_full_comparison(hmc_runs):
    full = hmc_runs["summ"].comparison
    pick = [full.names[5], full.names[1]]
    sel = I.hmc_chain_summary(chunk=16, pointwise=pick, **hmc_runs["args"]).comparison
    assert sel.names == pick and sel.n_draws == full.n_draws
    idx = [full.names.index(p) for p in pick]
    for f in COMPARED:
        x, y = np.asarray(getattr(sel, f)), np.asarray(getattr(full, f))[idx]
        print(f"{f}: selected {x.tolist()} full {y.tolist()}")
        assert np.array_equal(x.view(np.uint64) if x.dtype == np.float64 else x, y.view(np.uint64) if y.dtype == np.float64 else y), f
    with pytest.raises(ValueError):
        I.hmc_chain_summary(chunk=16, pointwise=["nope"], **hmc_runs["args"])


# ---- call order, arguments ----------------------------------------------------------------------------------------------------------
def _code(fn):
    with pytest.raises(E.EngineError) as ei:
        fn()
    print(ei.value)
    return ei.value.code


def test_call_order_and_arguments(engines):
    eng = engines.get(65)
    x = L.table(["normal", "far"], 10, 65)
    ptr = eng.upload(x)
    try:
        s = eng.loglik_stream(10, 2)
        s.update(ptr, 0)                                         # a no-op
        assert s.count() == 0
        s.update(ptr, 4)
        assert _code(s.result) == FG_E_STATE and _code(s.pooled) == FG_E_STATE
        assert _code(lambda: s.update(ptr, 7)) == FG_E_STATE and s.count() == 4
        s.update(ptr + 4 * 2 * 65 * 8, 0)
        s.update(ptr + 4 * 2 * 65 * 8, 6)
        assert s.count() == 10
        assert _code(lambda: s.update(ptr, 1)) == FG_E_STATE
        s.update(ptr, 0)
        got = s.pooled()
        again = s.pooled()                                       # a read-out changes nothing
        assert np.array_equal(_bits(got["words"]), _bits(again["words"]))
        s.free()
        s.free()
        with pytest.raises(ValueError):
            s.count()
        one = _feed(eng, ptr, x.shape, (10,), read=("pooled",))[0]
        assert np.array_equal(_bits(got["words"]), _bits(one["words"]))
    finally:
        eng.device_free(ptr)
    assert _code(lambda: eng.loglik_stream(0, 1)) == FG_E_BAD_ARG
    assert _code(lambda: eng.loglik_stream(1, 0)) == FG_E_BAD_ARG
    with pytest.raises(TypeError):
        eng.loglik_stream(1.5, 1)
    with pytest.raises(ValueError):
        CMP.model_comparison(np.zeros((3, 2)))
    with pytest.raises(ValueError):
        CMP.model_comparison(x, names=["only one"])
    c = CMP.model_comparison(x)
    assert c.names == ["observe#0", "observe#1"] and c.n_draws == 650


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
            _, ll = eng.predict_eval(buf, 5, out=False)
            s = eng.loglik_stream(5, cp.O)
            s.update(ll, 5)
            res = s.result()
            assert np.isfinite(res["elpd_loo"]).all() and not res["n_nan"].any()
            s.free()
            eng.device_free(ll)
        eng.hmc_step(5, buf + 5 * cp.d * C * 8)
        seen.append(dict(draws=eng.download(buf, (10, cp.d, C), dtype=np.int64), values=eng.get_values(), lj=eng.hmc_log_joint(), eps=eng.hmc_step_sizes(),
                         state=np.frombuffer(eng.state_export(), dtype=np.uint8), accept=np.float64(eng.hmc_stats().accept_rate)))
        eng.device_free(buf)
        eng.close()
    for k in seen[0]:
        a, b = (np.atleast_1d(np.ascontiguousarray(seen[j][k])) for j in (1, 0))
        print(f"{k}: equal {a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))}")
        assert a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8)), k
