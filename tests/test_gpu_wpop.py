"""GPU tests of the weighted-population summary (fg_wpop.hip): units, moments words, quantile bits and passes, tables against the
Python restatement (tests/wpop_restatement.py) bit for bit, on synthetic rows and weights uploaded once; the engine's own population
against the same weights uploaded again; adaptive_smc_summary against the restatement applied to adaptive_smc's download; the law
of the reference's doc model.  Every compared figure is printed before it is asserted."""
import functools
import math

import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import inference as I
from fugue_amd import model as M
from fugue_amd import workloads as W
from tests import wpop_restatement as R
from tests.models import ZOO

pytestmark = pytest.mark.gpu

NS = (1, 63, 64, 65, 192, 600)
WKINDS = R.WEIGHT_KINDS + ("bad",)
D3 = (0, 2)                                  # d = 3: rows 0..2 and 2..4 of the five kinds


def _weights(N, wkind):
    return R.bad_weights(N, N) if wkind == "bad" else (R.weights(wkind, N, N), 0)


@functools.lru_cache(maxsize=None)
def ref_units(N, wkind):
    return R.units(_weights(N, wkind)[0])


@functools.lru_cache(maxsize=None)
def ref_moments(N, wkind):
    x, w = R.rows(R.ROW_KINDS, N, N), _weights(N, wkind)[0]
    return [R.moments(x[k], w) for k in range(len(R.ROW_KINDS))]


@functools.lru_cache(maxsize=None)
def ref_quantiles(N, wkind, plan):
    x = R.rows(R.ROW_KINDS, N, N)
    q, T, _, _ = ref_units(N, wkind)
    return [R.quantiles(x[k], q, T, R.PROBS, *plan) for k in range(len(R.ROW_KINDS))]


class _Pool:
    """One engine for the module (its model does not matter: a caller's weights may have any n), every input uploaded once."""

    def __init__(self):
        self.eng = E.Engine(E.compile_model(W.normal_sites(1)), 64, seed=1)
        self.bufs, self.pops = {}, {}

    def upload(self, key, make):
        if key not in self.bufs:
            self.bufs[key] = self.eng.upload(np.ascontiguousarray(make()))
        return self.bufs[key]

    def rows(self, N):
        return self.upload(("x", N), lambda: R.rows(R.ROW_KINDS, N, N))

    def pop(self, N, wkind):
        if (N, wkind) not in self.pops:
            self.pops[(N, wkind)] = self.eng.wpop(N, self.upload(("w", N, wkind), lambda: _weights(N, wkind)[0]))
        return self.pops[(N, wkind)]

    def close(self):
        for p in self.pops.values():
            p.close()
        for b in self.bufs.values():
            self.eng.device_free(b)
        self.eng.close()


@pytest.fixture(scope="module")
def pool():
    p = _Pool()
    yield p
    p.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _moment_bits(m, k):
    return [R.bits(m[name][k]) for name in E.WPOP_MOMENTS[:5]] + [R.bits(float(m["n_used"][k]))]


@pytest.mark.parametrize("plan", R.PLANS)
@pytest.mark.parametrize("N", NS)
def test_device_equals_the_restatement_bit_for_bit(pool, N, plan):
    """A partial wave, a full one, pass-through in the tree, three waves, three blocks and a second level; every kind of row under
    every kind of weights; d = 1 (each row) and d = 3 (rows 0..2, 2..4); units, the six moments words, quantile bits, passes."""
    x = pool.rows(N)
    for wkind in WKINDS:
        wp = pool.pop(N, wkind)
        q, T, n_bad, n_zero = ref_units(N, wkind)
        u = wp.units()
        print(f"N {N} {wkind}: units {u} / T {T} n_bad {n_bad} n_zero {n_zero}")
        assert (u["T"], u["n_bad"], u["n_zero"]) == (T, n_bad, n_zero) and n_bad == _weights(N, wkind)[1]
        want_m, want_q = ref_moments(N, wkind), ref_quantiles(N, wkind, plan)
        for d, firsts in ((1, range(len(R.ROW_KINDS))), (3, D3)):
            for k0 in firsts:
                m = wp.moments(x + k0 * N * 8, d)
                vals, passes = wp.quantiles(x + k0 * N * 8, d, R.PROBS, *plan)
                for j in range(d):
                    k = k0 + j
                    ok_m = _moment_bits(m, j) == [R.bits(v) for v in want_m[k]]
                    ok_q = [int(b) for b in _bits(vals[j])] == [R.bits(v) for v in want_q[k][0]]
                    ok_p = passes[j].tolist() == want_q[k][1]
                    if d == 1 or not (ok_m and ok_q and ok_p):
                        print(f"  d {d} {R.ROW_KINDS[k]}: mean {m['mean'][j]!r} std {m['std'][j]!r} mcse {m['mcse'][j]!r} n_used {m['n_used'][j]} equal {ok_m}; "
                              f"quantiles {vals[j].tolist()} equal {ok_q}; passes {passes[j].tolist()} / {want_q[k][1]}")
                    assert ok_m and ok_q and ok_p, (wkind, d, R.ROW_KINDS[k])
        if T == 0:
            assert np.isnan(wp.quantiles(x, 1, R.PROBS, *plan)[0]).all()


def test_a_tree_of_three_levels_and_bins_flushed_by_many_blocks(pool):
    """N = 65 537: 65 537 -> 257 -> 2 -> 1 in the tree, the last block of every level partial; more particles than the capacity, so
    the first pass is a histogram pass that 257 blocks flush into the same bins, and the second collects."""
    N, plan = 65537, (12, 65536)
    x = R.row("normal", N, 5)
    w = R.weights("dirichlet", N, 5)
    dx, dw = pool.upload(("x", N), lambda: x), pool.upload(("w", N), lambda: w)
    wp = pool.eng.wpop(N, dw)
    try:
        q, T, n_bad, n_zero = R.units(w)
        u = wp.units()
        m = wp.moments(dx, 1)
        vals, passes = wp.quantiles(dx, 1, R.PROBS, *plan)
        want_m, (want_q, want_p) = R.moments(x, w), R.quantiles(x, q, T, R.PROBS, *plan)
        print(u, T, n_bad, n_zero)
        print([m[name][0] for name in E.WPOP_MOMENTS], want_m)
        print(vals[0].tolist(), want_q, passes[0].tolist(), want_p)
        assert (u["T"], u["n_bad"], u["n_zero"]) == (T, n_bad, n_zero)
        assert _moment_bits(m, 0) == [R.bits(v) for v in want_m]
        assert [int(b) for b in _bits(vals[0])] == [R.bits(v) for v in want_q] and passes[0].tolist() == want_p == [2] * 5
    finally:
        wp.close()


@pytest.mark.parametrize("N", (65, 600))
def test_tables_equal_the_restatement(pool, N):
    """bins 2, 8, 9 and 4 096, one row per value type (a u64 cell above 2^63 among them), cells below and above the bins."""
    rng = np.random.default_rng(3000 + N)
    vals = [[int(v) for v in rng.integers(0, 2, N)], [int(v) for v in rng.integers(0, 12, N)], [int(v) for v in rng.integers(2, 9, N)],
            [int(v) for v in rng.integers(-6, 7, N)]]
    vals[1][0] = 2 ** 63 + 5
    vt, lo, bins = [M.BOOL, M.U64, M.USIZE, M.I64], [0, 1, 2, -4], [2, 8, 9, 4096]
    cells = pool.upload(("cells", N), lambda: np.stack([R.encode(v, t == M.U64) for v, t in zip(vals, vt)]))
    for wkind in WKINDS:
        q, T, _, _ = ref_units(N, wkind)
        got = pool.pop(N, wkind).counts(cells, vt, lo, bins)
        for k in range(4):
            want = R.table(vals[k], q, T, lo[k], bins[k])
            g = dict(units=[int(v) for v in got["units"][k]], below=int(got["below"][k]), above=int(got["above"][k]), min=got["min"][k], max=got["max"][k])
            print(f"N {N} {wkind} row {k}: below {g['below']} above {g['above']} min {g['min']} max {g['max']} units in bins {sum(g['units'])} of T {T}: equal {g == want}")
            assert g == want and got["T"] == T
    one = pool.pop(N, "dirichlet").counts(cells + 3 * N * 8, [M.I64], [-6], [13])            # a single row, every cell inside
    assert int(one["below"][0]) == int(one["above"][0]) == 0 and int(one["units"][0].sum()) == one["T"]


def test_the_engines_own_population():
    """smc_run(download=False) on smc_normal at 4 096 particles: Engine.wpop() equals Engine.wpop(n, d_w) fed the weights of
    smc_weights() uploaded again, bit for bit, and both equal the restatement; without a population FG_E_STATE; n != C is refused."""
    cp = E.compile_model(W.smc_normal())
    N = 4096
    eng = E.Engine(cp, N, seed=11)
    bufs, pops = [], []
    try:
        with pytest.raises(E.EngineError) as ei:
            eng.wpop()
        print("no population:", ei.value)
        assert ei.value.code == E.FG_E_STATE
        r = eng.smc_run(rejuvenation_steps=1, download=False)
        with pytest.raises(E.EngineError) as ei:
            eng.wpop(n=100)
        print("n != C:", ei.value)
        assert ei.value.code == E.FG_E_BAD_ARG
        own = eng.wpop()
        pops.append(own)
        _, w = eng.smc_weights()
        bufs.append(eng.upload(w))
        again = eng.wpop(N, bufs[-1])
        pops.append(again)
        x = eng.cells_f64(E.lib().fg_engine_values_device(eng.h), 1, cp.S, cp.f64_sites, [M.F64] * cp.d)
        bufs.append(x)
        xh = eng.get_values()[0].view(np.float64)
        q, T, n_bad, n_zero = R.units(w)
        want_m, (want_q, want_p) = R.moments(xh, w), R.quantiles(xh, q, T, R.PROBS, 12, 65536)
        for name, wp in (("own", own), ("uploaded", again)):
            u, m = wp.units(), wp.moments(x, 1)
            vals, passes = wp.quantiles(x, 1, R.PROBS)
            print(f"{name}: {u}; moments {[m[k][0] for k in E.WPOP_MOMENTS]}; quantiles {vals[0].tolist()} passes {passes[0].tolist()}; betas {r['betas']}")
            assert (u["T"], u["n_bad"], u["n_zero"]) == (T, n_bad, n_zero) and n_bad == 0
            assert _moment_bits(m, 0) == [R.bits(v) for v in want_m]
            assert [int(b) for b in _bits(vals[0])] == [R.bits(v) for v in want_q] and passes[0].tolist() == want_p
    finally:
        for p in pops:
            p.close()
        for b in bufs:
            eng.device_free(b)
        eng.close()


def _mixture_with_a_result():
    """tests/models.py's mixture (four f64 means, ten Categorical assignments, ten f64 observe sites) with a return value added"""
    P = ZOO["mixture"]()
    mu = [M.Expr("site", a=h) for h in range(4)]
    P.result = {"spread": mu[0] - mu[1], "lift": mu[2] * 0.5 + 1.0}
    return P


def test_adaptive_smc_summary_equals_the_restatement_of_the_download():
    """4 096 particles of the mixture with results, predictive replicates and discrete sites: every figure of the summary equals the
    restatement applied to adaptive_smc's downloaded SMCResult of the same seed, bit for bit; log_evidence and betas are equal; the
    engine's values and weights after population_summary are those before it."""
    cp = E.compile_model(_mixture_with_a_result())
    N, seed, cfg = 4096, 5, I.SMCConfig(rejuvenation_steps=1)
    full = I.adaptive_smc(seed, N, cp, cfg, predictive=True)
    s = I.adaptive_smc_summary(seed, N, cp, cfg, results=True, predictive=True, discrete=True)
    print(s.names, s.log_evidence, full.log_evidence, s.betas, s.ess, s.T, s.n_zero)
    assert s.log_evidence == full.log_evidence and np.array_equal(s.betas, full.betas) and s.n_particles == N
    w = full.weights
    q, T, n_bad, n_zero = R.units(w)
    assert (s.T, s.n_zero, n_bad) == (T, n_zero, 0)
    assert abs(s.ess - 1.0 / float(np.sum(w * w))) <= 2 * (N + 8) * 2.0 ** -52 * s.ess          # two sums of N positive terms, each within N ulps
    f64 = [a for a, v in zip(full.sites, full.vtypes) if v == M.F64]
    assert s.sites == f64 and s.result_names == full.result_names and s.predictive_names == full.predictive_names
    assert s.names == f64 + full.result_names + full.predictive_names
    rows = [full.get_f64(a) for a in f64] + [full.get_result(a) for a in full.result_names] + [full.get_predictive(a) for a in full.predictive_names]
    for k, (name, x) in enumerate(zip(s.names, rows)):
        W_, mean, var, std, mcse, n_used = R.moments(x, w)
        qv, qp = R.quantiles(x, q, T, s.probs, 12, 65536)
        ok = (R.bits(s.mean[k]), R.bits(s.std[k]), R.bits(s.mcse[k]), int(s.n_used[k])) == (R.bits(mean), R.bits(std), R.bits(mcse), int(n_used))
        ok_q = [int(b) for b in _bits(s.quantiles[k])] == [R.bits(v) for v in qv] and s.passes[k].tolist() == qp
        print(f"  {name}: mean {s.mean[k]!r} / {mean!r}, std {s.std[k]!r}, mcse {s.mcse[k]!r}, quantiles {s.quantiles[k].tolist()}: equal {ok and ok_q}")
        assert ok and ok_q, name
    t = s.tables
    disc = [(a, v) for a, v in zip(full.sites, full.vtypes) if v != M.F64]
    assert t is not None and t.names == [a for a, _ in disc] and t.T == T
    for k, (a, v) in enumerate(disc):
        cells = [int(c) for c in full.cells[full.sites.index(a)]]
        want = R.table(cells, q, T, t.lo[k], t.bins[k])
        got = dict(units=[int(u) for u in t.units[k]], below=int(t.below[k]), above=int(t.above[k]), min=t.min[k], max=t.max[k])
        print(f"  table {a}: lo {t.lo[k]} bins {t.bins[k]} probs {t.probs()[k].tolist()} equal {got == want}")
        assert got == want and (t.lo[k], t.bins[k]) == (0, 4)
    # the summary changes nothing: the same engine before and after
    eng = E.Engine(cp, N, seed=seed)
    try:
        r = eng.smc_run(cfg.resampling_method, cfg.ess_threshold, cfg.rejuvenation_steps, download=False)
        v0, (lw0, w0) = eng.get_values(), eng.smc_weights()
        s2 = I.population_summary(eng, r["log_evidence"], r["betas"], results=True, predictive=True, discrete=True)
        v1, (lw1, w1) = eng.get_values(), eng.smc_weights()
        assert np.array_equal(v0, v1) and np.array_equal(_bits(lw0), _bits(lw1)) and np.array_equal(_bits(w0), _bits(w1))
        assert np.array_equal(v0, full.cells) and np.array_equal(_bits(w0), _bits(w))
        for name in ("mean", "std", "mcse", "quantiles"):
            assert np.array_equal(_bits(getattr(s2, name)), _bits(getattr(s, name))), name
    finally:
        eng.close()


def test_law_of_the_doc_model():
    """mu ~ N(0, 1), y ~ N(mu, 0.5) observed at 1.8 (smc.rs:445-453): the posterior is N(1.44, 0.2).  65 536 particles,
    rejuvenation_steps = 1: |mean - 1.44| <= 5 sqrt(0.2 / ess) under the condition ess >= N / 10 (tests/test_gpu_abc.py's rule); the
    median lies inside the weighted 2.5 % - 97.5 % interval, which contains 1.44.  The seed was chosen on the CPU with
    oracle.OracleModel(...).smc_run(65536, seed, rejuvenation_steps=1), whose own population meets both:
      seed 7: ess 36883.1, mean 1.4391995, |mean - 1.44| 8.0e-4, bound 1.164e-2, 2 betas, log_evidence -2.3201150
    (seeds 2025 and 42 as well: ess 36806.8 / 36827.9, |mean - 1.44| 3.8e-3 / 1.5e-3)."""
    N = 65536
    s = I.adaptive_smc_summary(7, N, W.readme_normal(y=1.8, sigma=0.5), I.SMCConfig(rejuvenation_steps=1))
    k = s.row("mu")
    lo, med, hi = s.quantiles[k][0], s.quantiles[k][2], s.quantiles[k][4]
    bound = 5.0 * math.sqrt(0.2 / s.ess)
    print(f"law: mean {s.mean[k]:.6f}, |mean - 1.44| {abs(s.mean[k] - 1.44):.2e}, bound {bound:.2e}, ess {s.ess:.1f} of {N}, std {s.std[k]:.4f} (sqrt 0.2 = {math.sqrt(0.2):.4f}), "
          f"mcse {s.mcse[k]:.2e}, interval [{lo:.4f}, {hi:.4f}], median {med:.4f}, log_evidence {s.log_evidence:.6f}, betas {s.betas.tolist()}")
    assert s.ess >= N / 10
    assert abs(s.mean[k] - 1.44) <= bound
    assert lo <= med <= hi and lo <= 1.44 <= hi


def test_a_population_with_bad_weights_raises():
    cp = E.compile_model(W.smc_normal())
    eng = E.Engine(cp, 64, seed=3)
    try:
        eng.smc_prior_particles()
        lw = np.zeros(64)
        lw[3] = np.nan
        eng.smc_set_log_weights(lw)
        eng.smc_normalize()
        with pytest.raises(ValueError) as ei:
            I.population_summary(eng)
        print(ei.value)
        assert "not normalised" in str(ei.value)
    finally:
        eng.close()


def test_an_empty_population_is_an_empty_summary():
    s = I.adaptive_smc_summary(1, 0, W.smc_normal())
    assert s.log_evidence == 0.0 and s.n_particles == 0 and s.names == ["mu"] and np.isnan(s.mean).all() and s.betas.size == 0
