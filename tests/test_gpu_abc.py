"""ABC on the device (fg_abc.hip) against the sequential restatement (tests/abc_restatement.py): the distance kernel bit for bit, the
rounds of attempts against tables re-obtained through fg_prior_init / fg_predict_eval with the same stream words, batch invariance,
the stage round (base index, proposal, scoring, accept), the mixture kernel within 1e-9, the Python drivers, the law of a case with a
closed-form target, and that no ABC entry point moves a sampler session."""
import math
import warnings

import numpy as np
import pytest

import fugue_amd as F
from fugue_amd import abc as A
from fugue_amd import engine as E
from fugue_amd import model as M
from tests import abc_restatement as R
from tests.models import ZOO

pytestmark = pytest.mark.gpu
INF, NAN = float("inf"), float("nan")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_bits(label, got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    bad = ~((np.isnan(got) & np.isnan(want)) | (_bits(got) == _bits(want)))
    print(f"{label}: {int(bad.sum())} of {got.size} values differ in bits")
    assert got.shape == want.shape and not bad.any(), (label, np.argwhere(bad)[:5].tolist(), got[bad][:5], want[bad][:5])


def _readme():
    return M.sample(M.addr("mu"), M.Normal(0.0, 2.0)).bind(lambda mu: M.observe(M.addr("y"), M.Normal(mu, 1.0), 2.0).map(lambda _: mu))


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(E.compile_model(_readme()), 64, seed=5)
    yield e
    e.close()


# ---- 1. the distance kernel -----------------------------------------------------------------------------------------------------
def _dist_gpu(eng, sim, obs, kind, weights=()):
    sim = np.ascontiguousarray(sim, dtype=np.float64)
    K, B = sim.shape
    obs, w = np.ascontiguousarray(obs, dtype=np.float64), np.ascontiguousarray(weights, dtype=np.float64)
    guard = 16
    host = np.concatenate([np.full(guard, -77.0), np.full(B, 123.0), np.full(guard, -77.0)])
    d_sim, d_out = eng.upload(sim if sim.size else np.zeros(1)), eng.upload(host)
    try:
        E._check(E.lib().fg_abc_distance(eng.h, d_sim, K, B, E._dp(obs), obs.size, kind, E._dp(w), w.size, d_out + guard * 8))
        eng.synchronize()
        back = eng.download(d_out, (host.size,))
    finally:
        eng.device_free(d_sim), eng.device_free(d_out)
    assert (back[:guard] == -77.0).all() and (back[-guard:] == -77.0).all(), "guard words around the distances were written"
    return back[guard:-guard]


def _table(K, B, seed):
    """ties (values on a grid of quarters), both zeros, both infinities; one NaN column when B > 2"""
    rng = np.random.default_rng(seed)
    sim = np.round(rng.normal(0.0, 2.0, (K, B)) * 4.0) / 4.0
    flat = sim.reshape(-1)
    for v, k in ((0.0, 3), (-0.0, 3), (INF, 7), (-INF, 11)):
        flat[rng.integers(0, flat.size, max(1, flat.size // k // 4))] = v
    if B > 2:
        sim[rng.integers(0, K), 2] = NAN
    if B > 5 and K >= 2:
        sim[:, 5] = np.where(np.arange(K) % 2 == 0, 0.0, -0.0)      # a column of zeros of both signs: the median is a zero
    return sim


@pytest.mark.parametrize("B", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("K", [1, 2, 3, 64, 65])
def test_distances_equal_the_restatement_bit_for_bit(eng, K, B):
    sim = _table(K, B, 100 * K + B)
    obs = np.round(np.random.default_rng(K).normal(0.5, 1.0, K) * 8.0) / 8.0
    for kind, name in ((A.EUCLIDEAN, "Euclidean"), (A.MANHATTAN, "Manhattan")):
        want = [R.distance(kind, obs.tolist(), sim[:, b].tolist()) for b in range(B)]
        _same_bits(f"{name} K={K} B={B}", _dist_gpu(eng, sim, obs, kind), want)
        assert (_dist_gpu(eng, sim, np.append(obs, 1.0), kind) == INF).all()            # a length mismatch: +inf for every attempt
    for w in ([], [0.5, 2.0], [1.0, 0.25, 3.0], [1.0, 0.25, 3.0, 9.0, 9.0]):
        want = [R.summary_stats(obs.tolist(), sim[:, b].tolist(), w) for b in range(B)]
        got = _dist_gpu(eng, sim, obs, A.SUMMARY_STATS, w)
        _same_bits(f"SummaryStats K={K} B={B} weights={len(w)}", got, want)
        if B > 2:
            assert math.isnan(got[2])                       # a NaN among the simulated values: a NaN distance
    # SummaryStats has no length rule: the observed vector keeps its own statistics
    w3 = [1.0, 1.0, 1.0]
    _same_bits("SummaryStats, another observed length", _dist_gpu(eng, sim, [1.0, 4.0, 2.0, 8.0], A.SUMMARY_STATS, w3),
               [R.summary_stats([1.0, 4.0, 2.0, 8.0], sim[:, b].tolist(), w3) for b in range(B)])


def test_distance_refusals(eng):
    d = eng.device_alloc(64 * 8)
    try:
        L = E.lib()
        obs = np.array([1.0, NAN])
        assert L.fg_abc_distance(eng.h, d, 2, 4, E._dp(obs), 2, A.SUMMARY_STATS, E._dp(obs), 0, d) == E.FG_E_BAD_ARG      # a NaN in the observed vector
        assert L.fg_abc_distance(eng.h, d, 2, 4, E._dp(obs), 2, 7, None, 0, d) == E.FG_E_BAD_ARG
        assert L.fg_abc_distance(eng.h, d, -1, 4, E._dp(obs), 2, A.EUCLIDEAN, None, 0, d) == E.FG_E_BAD_ARG
        assert L.fg_abc_distance(eng.h, d, 2, 0, E._dp(obs), 2, A.EUCLIDEAN, None, 0, d) == 0
    finally:
        eng.device_free(d)


# ---- 2. the mixture kernel ------------------------------------------------------------------------------------------------------
def _mix_gpu(eng, x, centers, w, std):
    x, centers = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(centers, dtype=np.float64)
    d, m = x.shape
    n = centers.shape[1]
    w, std = np.ascontiguousarray(w, dtype=np.float64), np.ascontiguousarray(std if d else [1.0], dtype=np.float64)
    guard = 16
    host = np.concatenate([np.full(guard, -77.0), np.full(m, 123.0), np.full(guard, -77.0)])
    d_x, d_c, d_out = eng.upload(x if x.size else np.zeros(1)), eng.upload(centers if centers.size else np.zeros(1)), eng.upload(host)
    try:
        E._check(E.lib().fg_abc_mixture(eng.h, d_x, m, d_c, n, d, E._dp(w), E._dp(std), d_out + guard * 8))
        back = eng.download(d_out, (host.size,))
    finally:
        for p in (d_x, d_c, d_out):
            eng.device_free(p)
    assert (back[:guard] == -77.0).all() and (back[-guard:] == -77.0).all(), "guard words around log_denom were written"
    return back[guard:-guard]


MIX_CASES = [(1, 1, 1), (63, 65, 1), (64, 64, 3), (65, 257, 2), (130, 1000, 5), (64, 300, 33), (64, 10, 0)]
_mix_cache = {}


def _mix_case(m, n, d):
    """inputs and the restatement's values, computed once per case and shared by the split settings"""
    if (m, n, d) not in _mix_cache:
        rng = np.random.default_rng(1000 * m + n + d)
        centers = rng.normal(0.0, 1.5, (d, n))
        x = centers[:, rng.integers(0, n, m)] + rng.normal(0.0, 0.4, (d, m))
        w = rng.random(n)
        if n > 1:
            w[n // 2] = 0.0                                 # one w_j = 0 contributes nothing
        w = w / w.sum()
        std = 0.2 + rng.random(d)
        want = [R.kernel_mixture_log_density(x[:, i].tolist(), centers.T.tolist(), w.tolist(), std.tolist()) for i in range(m)]
        _mix_cache[(m, n, d)] = (x, centers, w, std, np.asarray(want))
    return _mix_cache[(m, n, d)]


def _check_mix(label, got, want, m):
    """|delta log_denom| <= 1e-9 max(1, |x|); weights normalised from them to rtol 1e-9 (the bound tests/test_gpu_smc.py holds SMC weights to)"""
    got, want = np.asarray(got), np.asarray(want)
    same_inf = np.isinf(want) & (got == want)
    with np.errstate(all="ignore"):
        err = np.where(same_inf, 0.0, np.abs(got - want))
    worst = float(np.nanmax(err / np.maximum(1.0, np.abs(np.where(np.isfinite(want), want, 1.0)))))
    print(f"{label}: largest |delta log_denom| / max(1, |x|) = {worst:.3e} (bound 1e-9)")
    assert not np.isnan(got).any() and worst <= 1e-9, label
    if np.isfinite(want).all():
        wg, ww = np.asarray(R.stage_weights([0.0] * m, got.tolist())), np.asarray(R.stage_weights([0.0] * m, want.tolist()))
        pos = ww > 0.0                                      # a weight that underflows to zero in the restatement is zero here too
        rel = float(np.max(np.abs(wg[pos] - ww[pos]) / ww[pos]))
        print(f"{label}: largest relative deviation of the normalised weights {rel:.3e} (bound 1e-9)")
        assert rel <= 1e-9 and abs(wg.sum() - 1.0) < 1e-12 and (wg[~pos] == 0.0).all()


@pytest.mark.parametrize("splits", [None, "1", "37"])
@pytest.mark.parametrize("m,n,d", MIX_CASES)
def test_mixture_matches_the_restatement(eng, monkeypatch, m, n, d, splits):
    if splits is None:
        monkeypatch.delenv("FG_ABC_MIX_SPLITS", raising=False)
    else:
        monkeypatch.setenv("FG_ABC_MIX_SPLITS", splits)    # 37 > n for the small cases: ranges without work
    x, centers, w, std, want = _mix_case(m, n, d)
    _check_mix(f"mixture m={m} n={n} d={d} splits={splits}", _mix_gpu(eng, x, centers, w, std), want, m)


@pytest.mark.parametrize("splits", [None, "1", "5"])
def test_mixture_edges(eng, monkeypatch, splits):
    if splits is None:
        monkeypatch.delenv("FG_ABC_MIX_SPLITS", raising=False)
    else:
        monkeypatch.setenv("FG_ABC_MIX_SPLITS", splits)
    # centers so far apart that only the maximum term survives
    centers = np.array([[0.0, 1000.0, -1000.0, 2000.0]])
    x = np.array([[0.1, 999.5, -1000.25, 1999.0, 500.0]])
    w, std = [0.25, 0.25, 0.25, 0.25], [1.0]
    want = [R.kernel_mixture_log_density([v], centers.T.tolist(), w, std) for v in x[0]]
    _check_mix("far centers", _mix_gpu(eng, x, centers, w, std), want, 5)
    # a degenerate component at the 1e-3 bandwidth (abc.rs:770), and a bandwidth below the 1e-12 floor (abc.rs:794)
    centers = np.full((2, 9), 0.75); centers[1] = np.linspace(-1.0, 1.0, 9)
    x = np.array([[0.75, 0.7501, 0.7495, 0.752], [0.1, -0.3, 0.9, 0.0]])
    w = (np.arange(9) + 1.0) / 45.0
    for std in ([1e-3, 0.5], [0.0, 0.5]):
        xx = x if std[0] else np.array([[0.75] * 4, x[1]])
        want = [R.kernel_mixture_log_density(xx[:, i].tolist(), centers.T.tolist(), w.tolist(), std) for i in range(4)]
        _check_mix(f"degenerate component std={std[0]}", _mix_gpu(eng, xx, centers, w, std), want, 4)
    # every weight zero: every term -inf, the result -inf
    got = _mix_gpu(eng, x, centers, np.zeros(9), [0.5, 0.5])
    assert (got == -INF).all()
    # a NaN coordinate is a NaN, for that particle alone
    xn = x.copy(); xn[1, 2] = NAN
    got = _mix_gpu(eng, xn, centers, w, [0.5, 0.5])
    assert math.isnan(got[2]) and np.isfinite(np.delete(got, 2)).all()
    # d = 0: LSE(ln w)
    got = _mix_gpu(eng, np.zeros((0, 3)), np.zeros((0, 9)), w, [])
    assert np.allclose(got, math.log(w.sum()), rtol=0, atol=1e-12)


# ---- 3. rejection rounds --------------------------------------------------------------------------------------------------------
def _cells_f64(cells, vtypes):
    """cells [K][B] -> doubles by the rule of fg_diag_cells_f64"""
    out = np.zeros(cells.shape)
    for k, vt in enumerate(vtypes):
        out[k] = cells[k].view(np.float64) if vt == M.F64 else (cells[k].view(np.uint64).astype(np.float64) if vt == M.U64 else cells[k].astype(np.float64))
    return out


def _prior_tables(cp, seed, chain_offset, B, n_rounds, sel):
    """what the rounds of the prior stage see, through the existing entry points: values [S][A], log_prior [A], simulated [K][A]"""
    vals, lps, sims = [], [], []
    for r in range(n_rounds):
        e2 = E.Engine(cp, B, seed=seed, chain_offset=chain_offset + r * B)
        acc = e2.prior_init(iteration=0)
        vals.append(e2.get_values()), lps.append(acc[0])
        y, _ = e2.predict_eval(None, 1, iter0=0, sel=sel, loglik=False)
        e2.synchronize()
        cells = e2.download(y, (len(sel), B), dtype=np.int64)
        e2.device_free(y)
        sims.append(_cells_f64(cells, [cp.observe_vtypes[k] for k in sel]))
        e2.close()
    return np.concatenate(vals, axis=1), np.concatenate(lps), np.concatenate(sims, axis=1)


REJECTION = {
    "coin": (lambda: ZOO["coin"](), [0, 2, 3, 7], A.MANHATTAN, 1.0),                       # a discrete observe: Bernoulli cells as 0.0 / 1.0
    "normal_mean": (_readme, [0], A.EUCLIDEAN, 0.7),
}


class _Dist:
    def __init__(self, kind, weights=()):
        self.kind, self.weights = kind, weights


@pytest.mark.parametrize("name", list(REJECTION))
def test_rejection_rounds_equal_the_restatement(name):
    make, sel, kind, tol = REJECTION[name]
    cp = E.compile_model(make())
    seed, c0, B, n_rounds = 31, 500, 64, 3
    obs = A._observed(cp, A.SIM_OBSERVE, sel, None)
    vals, lps, sims = _prior_tables(cp, seed, c0, B, n_rounds, sel)
    dist = np.asarray([R.distance(kind, obs.tolist(), sims[:, a].tolist()) for a in range(B * n_rounds)])
    accept = dist <= tol
    print(f"{name}: {int(accept.sum())} of {accept.size} attempts within {tol}")
    assert 10 < accept.sum() < accept.size - 10
    n_mid = int(accept[:100].sum())                        # its n_mid-th accept falls inside the second round
    eng = E.Engine(cp, B, seed=seed, chain_offset=c0)
    try:
        for label, n, budget in (("the n-th accept falls mid-round", n_mid, 192), ("the budget ends mid-round", 150, 100), ("one particle", 1, 192),
                                 ("a budget of one round exactly", 150, 64)):
            h = A.ABCHandle(eng, A.SIM_OBSERVE, sel, obs, _Dist(kind), n)
            acc, att = h.round_prior(tol, budget)
            want_idx, want_att = R.stop_rule(accept.tolist(), n, budget)
            print(f"{name}, {label}: accepted {acc} (restatement {len(want_idx)}), attempts {att} (restatement {want_att})")
            assert (acc, att) == (len(want_idx), want_att), label
            pop = h.get_population(0)
            assert pop["n"] == acc and pop["attempt"].tolist() == want_idx
            assert np.array_equal(pop["cells"], vals[:, want_idx])
            _same_bits(f"{label}: distances", pop["dist"], dist[want_idx])
            _same_bits(f"{label}: log-prior", pop["log_prior"], lps[want_idx])
            assert (pop["weights"] == 1.0 / acc).all()
            li, ld, llp, la = h.last_round()
            r_last = (att - 1) // B if acc == n else (budget - 1) // B
            lo = r_last * B
            live = min(B, budget - lo)
            assert (li == -1).all()
            _same_bits(f"{label}: the last round's distances", ld, dist[lo:lo + B])
            assert la[:live].tolist() == accept[lo:lo + live].astype(int).tolist() and (la[live:] == 0).all()   # attempts beyond the budget are masked
            h.close()
        # nothing accepted
        h = A.ABCHandle(eng, A.SIM_OBSERVE, sel, obs, _Dist(kind), 5)
        assert h.round_prior(-1.0, 130) == (0, 130) and h.get_population(0)["n"] == 0
        with pytest.raises(E.EngineError):
            h.stage_begin()                                 # no population
        with pytest.raises(E.EngineError):
            h.round_prior(1.0, 2 ** 32 - c0 + 1)            # the budget would wrap the chain word
        h.close()
        assert eng.get_values().shape == (cp.S, B)
    finally:
        eng.close()
    with pytest.raises(F.ABCError) as ei:
        F.abc_smc_weighted(seed, cp, [cp.observe_names[k] for k in sel], None, _Dist(kind), F.ABCSMCConfig(-1.0, [0.5], 5), 130, batch=B)
    assert (ei.value.kind, ei.value.tolerance, ei.value.attempts) == ("EmptyInitialPopulation", -1.0, 130)


# ---- 4. batch invariance --------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_batch():
    cp = E.compile_model(_readme())
    rej, smc = [], []
    for B in (64, 200, 1024):
        rej.append(F.abc_rejection(9, cp, "observe", None, F.EuclideanDistance(), 0.6, 150, batch=B))
        smc.append(F.abc_smc_weighted(9, cp, ["result"], [2.0], F.EuclideanDistance(), F.ABCSMCConfig(1.0, [0.5, 0.3], 120), 12000, batch=B))
    for got in (rej, smc):
        assert len(got[0]) in (150, 120)
        for other in got[1:]:
            assert np.array_equal(other.cells, got[0].cells) and np.array_equal(other.attempt_index, got[0].attempt_index)
            _same_bits("distances", other.distances, got[0].distances)
            _same_bits("weights", other.weights, got[0].weights)


# ---- 5. the stage round ---------------------------------------------------------------------------------------------------------
def _stage_model():
    P = M.Program()
    mu = P.sample(M.addr("mu"), M.Normal(0.0, 2.0))
    P.sample(M.addr("k"), M.Poisson(3.0))                   # a discrete site: carried over unchanged
    p = P.sample(M.addr("p"), M.Beta(2.0, 2.0))             # a bounded prior: proposals leave (0, 1)
    P.sample(M.addr("u"), M.Uniform(-1.0, 1.0))
    P.observe(M.addr("y"), M.Normal(mu + p, 1.0), 1.0)
    P.result = mu
    return P


@pytest.mark.parametrize("n", [1, 65, 300])
def test_stage_round_equals_the_restatement(oracle, n):
    """The base index exactly; the proposal v + bw z within 1e-11 (|v| + |bw z|): the Normal draw is held to the oracle's at 1e-11
    relative as tests/test_gpu_predict.py holds it (ocml against glibc inside the sampler), scaled by the bandwidth, and the sum adds
    half an ulp; discrete sites bit for bit; log_prior = the scoring run's first accumulator at the proposal; accept = isfinite(log_prior)
    and dist <= tol."""
    cp = E.compile_model(_stage_model())
    seed, c0, B, stage, tol = 17, 40, 200, 2, 1.5
    src = E.Engine(cp, n, seed=3)
    src.prior_init(iteration=1)
    cells = src.get_values()
    src.close()
    w = np.full(n, 0.01 / max(1, n - 1)); w[n // 3] = 0.99 if n > 1 else 1.0             # one dominating weight
    eng = E.Engine(cp, B, seed=seed, chain_offset=c0)
    h = A.ABCHandle(eng, A.SIM_OBSERVE, [0], [1.0], _Dist(A.EUCLIDEAN), 500)
    try:
        h.set_population(cells, w)
        back = h.get_population(0)
        assert back["n"] == n and np.array_equal(back["cells"], cells) and np.array_equal(back["weights"], w)
        h.stage_begin()
        acc, att = h.round_stage(stage, tol, B)             # one round
        idx, dist, lp, flag = h.last_round()
        prop = eng.get_values()
        f64 = [j for j in range(cp.S) if cp.site_vtypes[j] == M.F64]
        coords = [[float(cells[j, i:i + 1].view(np.float64)[0]) for j in f64] for i in range(n)]
        bw = R.kernel_bandwidths(coords, w.tolist())
        if n == 1:
            assert bw == [1e-3] * len(f64)
        want_idx = np.zeros(B, dtype=np.int64)
        for b in range(B):
            s = oracle.stream(seed, c0 + b, stage, A.RNG_ABC)
            want_idx[b] = R.sample_index(oracle.sample_dist("Uniform", [0.0, 1.0], s), w.tolist())
            for c, j in enumerate(f64):
                z = oracle.sample_dist("Normal", [0.0, 1.0], s)
                v = coords[want_idx[b]][c]
                got = float(prop[j, b:b + 1].view(np.float64)[0])
                assert abs(got - (v + bw[c] * z)) <= 1e-11 * (abs(v) + abs(bw[c] * z)) + 1e-300, (b, j, got, v + bw[c] * z)
        assert np.array_equal(idx, want_idx)
        print(f"n={n}: base indices equal; {int((want_idx == n // 3).sum())} of {B} proposals start from the dominating particle")
        for j in range(cp.S):
            if cp.site_vtypes[j] != M.F64:
                assert np.array_equal(prop[j], cells[j, want_idx])
        score = eng.log_joint()[0]                          # the scoring run at the proposals
        _same_bits("log_prior", lp, score)
        sims = np.zeros((1, B))
        y, _ = eng.predict_eval(None, 1, iter0=stage, sel=[0], loglik=False)
        eng.synchronize()
        sims[0] = eng.download(y, (1, B))
        eng.device_free(y)
        want_dist = [R.euclidean([1.0], [sims[0, b]]) for b in range(B)]
        _same_bits("distances of the stage", dist, want_dist)
        want_flag = np.isfinite(lp) & (np.asarray(want_dist) <= tol)
        assert flag.tolist() == want_flag.astype(int).tolist()
        outside = ~np.isfinite(lp)
        print(f"n={n}: {int(outside.sum())} proposals outside the support, {int(want_flag.sum())} accepted")
        if n > 1:
            assert outside.any() and (flag[outside] == 0).all()
        assert (acc, att) == (int(want_flag.sum()), B)
        nx = h.get_population(1)
        take = np.nonzero(want_flag)[0]
        assert nx["attempt"].tolist() == take.tolist() and np.array_equal(nx["cells"], prop[:, take])
        if acc:
            h.stage_end()
            cur = h.get_population(0)
            x = [[float(prop[j, b:b + 1].view(np.float64)[0]) for j in f64] for b in take]
            ld = [R.kernel_mixture_log_density(xi, coords, w.tolist(), bw) for xi in x]
            _check_mix(f"stage_end n={n}: log_denom", cur["log_denom"], ld, len(take))
            ww = np.asarray(R.stage_weights(lp[take].tolist(), ld))
            assert np.max(np.abs(cur["weights"] - ww) / ww) <= 1e-9 and abs(cur["weights"].sum() - 1.0) < 1e-12
    finally:
        h.close()
        eng.close()


def test_stage_exhausted_carries_the_references_fields():
    with pytest.raises(F.ABCError) as ei:
        F.abc_smc_weighted(4, _readme, ["result"], [2.0], F.EuclideanDistance(), F.ABCSMCConfig(1.0, [2.0, 1e-7], 20), 700, batch=256)
    e = ei.value
    assert (e.kind, e.tolerance, e.requested, e.attempts) == ("StageExhausted", 1e-7, 20, 700) and 0 <= e.accepted < 20   # (2.0 is skipped, abc.rs:566)
    cp = E.compile_model(_readme())
    eng = E.Engine(cp, 64, seed=1)
    h = A.ABCHandle(eng, A.SIM_RESULT, [0], [2.0], F.EuclideanDistance(), 4)
    try:
        h.set_population(np.zeros((1, 2), dtype=np.int64), [0.0, 0.0])
        with pytest.raises(E.EngineError) as ee:
            h.stage_begin()                                 # a weight total <= 0
        assert ee.value.code == E.FG_E_STATE
        with pytest.raises(E.EngineError):
            h.round_stage(1, 1.0, 10)                       # no open stage
    finally:
        h.close()
        eng.close()


# ---- 6. the drivers -------------------------------------------------------------------------------------------------------------
def test_abc_smc_weighted_equals_the_step_calls_composed_by_hand():
    cp = E.compile_model(_readme())
    cfg = F.ABCSMCConfig(1.0, [0.6, 0.9, 0.35], 100)
    res = F.abc_smc_weighted(12, cp, ["result"], [2.0], F.EuclideanDistance(), cfg, 20000, batch=128)
    eng = E.Engine(cp, 128, seed=12)
    h = A.ABCHandle(eng, A.SIM_RESULT, [0], [2.0], F.EuclideanDistance(), 100)
    try:
        assert h.round_prior(1.0, 20000)[0] == 100
        for t, tol in ((1, 0.6), (2, 0.35)):                # 0.9 is not below 0.6: skipped, and takes no stage index
            h.stage_begin()
            assert h.round_stage(t, tol, 20000)[0] == 100
            h.stage_end()
        pop = h.get_population(0)
    finally:
        h.close()
        eng.close()
    assert res.final_tolerance == 0.35 and np.array_equal(res.cells, pop["cells"]) and np.array_equal(res.attempt_index, pop["attempt"])
    _same_bits("weights", res.weights, pop["weights"])
    assert (res.distances <= 0.35).all() and abs(res.weights.sum() - 1.0) < 1e-12


def test_doc_examples_return_non_empty_results():
    model = lambda: M.sample(M.addr("mu"), M.Normal(0.0, 1.0)).map(lambda mu: mu)        # abc.rs:676-693
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = F.abc_smc(42, model, ["result"], [2.0], F.EuclideanDistance(), F.ABCSMCConfig(1.0, [0.5], 20), batch=256)
        assert len(out) == 20 and (np.abs(out.get_f64("mu") - 2.0) <= 0.5).all() and (out.weights == 1.0 / 20).all()
        model2 = lambda: M.sample(M.addr("mu"), M.Normal(0.0, 2.0)).map(lambda mu: mu)   # abc.rs:865-880
        got = F.abc_scalar_summary(42, model2, "result", 2.0, 0.5, 5, batch=64)
        assert len(got) == 5 and (np.abs(got.get_f64("mu") - 2.0) <= 0.5).all()
        rej = F.abc_rejection(42, model2, ["result"], [2.0], F.EuclideanDistance(), 0.5, 5, batch=64)   # abc.rs:262-281
        assert np.array_equal(rej.cells, got.cells)
    with pytest.warns(UserWarning, match="did not complete"):
        assert len(F.abc_smc(42, model, ["result"], [50.0], F.EuclideanDistance(), F.ABCSMCConfig(0.01, [0.005], 5), batch=64)) == 0
    with pytest.warns(UserWarning, match="No samples accepted"):
        assert len(F.abc_rejection(42, model, ["result"], [50.0], F.EuclideanDistance(), 0.01, 3, batch=64)) == 0


# ---- 7. the law -----------------------------------------------------------------------------------------------------------------
def test_law_of_a_truncated_normal_target():
    """mu ~ Normal(0, 2), simulator the result mu, observed 2.0, Euclidean, tolerances 1.0 -> 0.5 -> 0.25, n = 4 096: the target is exactly
    the prior truncated to [1.75, 2.25].  Every particle lies in the interval (the distance is bit-exact), the weights sum to 1 within
    1e-12, |weighted_mean - E_trunc| <= 5 sqrt(Var_trunc / ESS) with the closed forms, under the condition ESS >= n / 10 (a collapsed
    population cannot widen the bound).  The CPU restatement of this configuration (numpy over the oracle's streams and samplers, seed 2 024)
    gives ESS = 4 083.8 of 4 096 (weighted mean 1.98460 against E_trunc = 1.98962, bound 0.01126; 17 055, 10 596 and 11 047 attempts in
    the three stages): ten times the cap."""
    n = 4096
    res = F.abc_smc_weighted(2024, lambda: M.sample(M.addr("mu"), M.Normal(0.0, 2.0)).map(lambda mu: mu), ["result"], [2.0], F.EuclideanDistance(),
                             F.ABCSMCConfig(1.0, [0.5, 0.25], n), 100 * n, batch=8192)
    mu, w = res.get_f64("mu"), res.weights
    assert len(res) == n and (mu >= 1.75).all() and (mu <= 2.25).all() and abs(w.sum() - 1.0) <= 1e-12
    sig, a, b = 2.0, 1.75 / 2.0, 2.25 / 2.0
    phi = lambda t: math.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)
    Phi = lambda t: 0.5 * (1.0 + math.erf(t / math.sqrt(2.0)))
    Z = Phi(b) - Phi(a)
    e_trunc = sig * (phi(a) - phi(b)) / Z
    var_trunc = sig * sig * (1.0 + (a * phi(a) - b * phi(b)) / Z - ((phi(a) - phi(b)) / Z) ** 2)
    ess = 1.0 / float((w * w).sum())
    wm = res.weighted_mean("mu")
    print(f"law: weighted mean {wm:.6f}, E_trunc {e_trunc:.6f}, |diff| {abs(wm - e_trunc):.2e}, bound {5 * math.sqrt(var_trunc / ess):.2e}, ESS {ess:.1f} of {n}")
    assert ess >= n / 10
    assert abs(wm - e_trunc) <= 5.0 * math.sqrt(var_trunc / ess)


# ---- 8. sampler sessions are unchanged ------------------------------------------------------------------------------------------
def _abc_calls(eng):
    """every ABC entry point once, on an engine with a live session"""
    _dist_gpu(eng, np.ones((3, eng.C)), [1.0, 2.0, 3.0], A.SUMMARY_STATS, [1.0, 1.0, 1.0])
    _mix_gpu(eng, np.zeros((2, 5)), np.ones((2, 7)), np.full(7, 1.0 / 7), [0.5, 0.5])
    h = A.ABCHandle(eng, A.SIM_OBSERVE, list(range(eng.cp.O)), A._observed(eng.cp, A.SIM_OBSERVE, list(range(eng.cp.O)), None), _Dist(A.EUCLIDEAN), 8)
    try:
        assert h.round_prior(INF, 2 * eng.C)[0] == 8
        h.last_round()
        pop = h.get_population(0)
        h.set_population(pop["cells"], pop["weights"])
        h.stage_begin()
        h.round_stage(1, INF, 2 * eng.C)
        h.get_population(1)
        h.stage_end()
    finally:
        h.close()


@pytest.mark.parametrize("kind", ["hmc", "mh"])
def test_abc_calls_leave_a_sampler_session_what_it_was(kind):
    cp = E.compile_model(ZOO["readme"]() if kind == "hmc" else ZOO["coin"]())
    out = []
    for with_abc in (False, True):
        eng = E.Engine(cp, 128, seed=8)
        rows = cp.d if kind == "hmc" else cp.S
        d_draws = eng.device_alloc(6 * rows * 128 * 8)
        if kind == "hmc":
            eng.hmc_init(E.hmc_config(n_leapfrog=4, init_step_size=0.2), 2)
            eng.hmc_step(5)
        else:
            eng.mh_init(2)
            eng.mh_step(5)
        if with_abc:
            _abc_calls(eng)
        blob = eng.state_export()
        if kind == "hmc":
            eng.hmc_step(6, d_draws)
            lj = eng.hmc_log_joint()
        else:
            eng.mh_step(6, list(range(cp.S)), d_draws)
            lj = eng.mh_log_weight()
        eng.synchronize()
        out.append((blob, eng.download(d_draws, (6, rows, 128), dtype=np.int64), lj, eng.get_values()))
        eng.device_free(d_draws)
        eng.close()
    assert out[0][0] == out[1][0], "the state blob differs"
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][3], out[1][3])
    _same_bits("log-joint", out[0][2], out[1][2])
