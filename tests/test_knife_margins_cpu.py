"""The CPU twin of the free-running parity tests: for every row of tests/parity_cases.py, with the oracle alone,

  - the traced runs of tests/oracle_margins.py ARE the runs the GPU tests compare with: mh_run_from's draws equal mh_run's, hmc_replay's equal
    hmc_run's, eps_search's step size equals find_reasonable_epsilon's, all bit for bit;
  - no chain has a decision inside the band (1e-6) of its boundary.  This is a condition on the inputs: with it, tests/knife.excused excuses no
    chain on the device, and a change of seed or model that breaks it fails HERE -- pick another seed; the band is never widened.

Each row's smallest margin is printed (-s); DESIGN.md's test table quotes them.  Also knife.excused itself on made-up arrays, and the
falsification the rule exists for: the oracle's draws with one chain replaced by its neighbour's must fail test_gpu_mh._compare, by name."""
import warnings

import numpy as np
import pytest

from tests import knife
from tests import oracle_margins as OM
from tests import parity_cases as PC


@pytest.mark.parametrize("cid", list(PC.MH_CASES))
def test_mh_rows_are_traced_exactly_and_have_no_knife_edge(oracle, cid):
    k = PC.MH_CASES[cid]
    om = oracle.OracleModel(k.make())
    ov = k.overrides_for(om.site_names)
    draws, final, scales, st = om.mh_run(k.seed, k.C, k.nw, k.ns, ov, chain0=k.chain0, n_threads=8)
    dist, o = OM.mh_margins(om, k.seed, k.C, k.nw, k.ns, ov, k.chain0)
    assert dist.shape == (k.nw + k.ns, k.C)
    assert np.array_equal(o["draws"][k.nw:], draws) and np.array_equal(o["final"], final) and np.array_equal(o["scales"], scales)
    decided = np.isfinite(dist)
    la, u = o["log_alpha"], o["u"]
    assert np.array_equal(decided, ~np.isnan(u) & np.isfinite(la)) and (la[decided] < 0.0).all()
    assert np.array_equal(o["accept"].astype(bool)[decided], u[decided] < np.exp(la[decided]))   # the decision the distance is about: mh.rs:733
    margin = dist.min(axis=0)
    t, c = np.unravel_index(dist.argmin(), dist.shape)
    print(f"[margins] MH {cid}: {int(decided.sum())} decisions, smallest |ln u - log_alpha| = {dist.min():.2e} (step {t}, chain {c})")
    assert decided.sum() > 100
    assert int((margin < PC.MH_BAND).sum()) == 0, (cid, np.nonzero(margin < PC.MH_BAND)[0], margin.min())


@pytest.mark.parametrize("cid", list(PC.HMC_CASES))
def test_hmc_rows_are_replayed_exactly_and_have_no_knife_edge(oracle, cid):
    k = PC.HMC_CASES[cid]
    om = oracle.OracleModel(k.make())
    cfg = oracle.HmcConfig.default(n_leapfrog=k.n_leapfrog, init_step_size=k.step_size)
    odraws, _, _, _ = om.hmc_run(k.seed, k.C, k.nw, k.ns, cfg, chain0=k.chain0, n_threads=8)
    draws, dist, search = OM.hmc_replay(om, k.seed, k.C, k.nw, k.ns, cfg, k.chain0)
    assert np.array_equal(draws, odraws)
    assert np.isfinite(search).all() == (k.step_size is None) and np.isinf(search).all() == (k.step_size is not None)
    margin = np.minimum(dist.min(axis=0), search)
    print(f"[margins] HMC {cid}: {int(np.isfinite(dist).sum())} decisions, smallest |u - alpha| = {dist.min():.2e}"
          + (f", smallest step-size-search distance {search.min():.2e}" if k.step_size is None else ""))
    assert np.isfinite(dist).sum() > 100
    assert int((margin < PC.HMC_BAND).sum()) == 0, (cid, np.nonzero(margin < PC.HMC_BAND)[0], margin.min())


@pytest.mark.parametrize("cid", list(PC.EPS_CASES))
def test_eps_search_rows_are_restated_exactly_and_have_no_knife_edge(oracle, cid):
    k = PC.EPS_CASES[cid]
    om = oracle.OracleModel(k.make())
    cells, p0 = PC.eps_inputs(om, k)
    dist = np.zeros(k.C)
    for c in range(k.C):
        q = np.ascontiguousarray(cells[om.f64_sites, c]).view(np.float64)
        lj = om.log_joint_at(cells[:, c], q)
        eps, dist[c] = OM.eps_search(om, cells[:, c], q, lj, p0[:, c])
        assert eps == om.find_reasonable_epsilon(cells[:, c], q, lj, p0[:, c]), (cid, c)
    print(f"[margins] step-size search {cid}: smallest |log-ratio - threshold| = {dist.min():.2e}")
    assert int((dist < PC.HMC_BAND).sum()) == 0, (cid, np.nonzero(dist < PC.HMC_BAND)[0], dist.min())


def test_eps_search_counts_every_threshold_it_compared_with(oracle):
    """The distance covers EVERY comparison made: a search that doubles twice compared three log-ratios with -ln 2 (ln 0.5: Alg. 4's
    (ratio)^a > 2^-a puts the ratio against 1/2 whether it doubles or halves).  Recomputed here from the returned step size alone."""
    om = oracle.OracleModel(PC.EPS_CASES["readme"].make())
    cells, p0 = PC.eps_inputs(om, PC.EPS_CASES["readme"])
    seen = set()
    for c in range(PC.EPS_CASES["readme"].C):
        q = np.ascontiguousarray(cells[om.f64_sites, c]).view(np.float64)
        lj = om.log_joint_at(cells[:, c], q)
        eps, dist = OM.eps_search(om, cells[:, c], q, lj, p0[:, c])
        seen.add(eps)
        h0 = -lj + 0.5 * float(p0[:, c] @ p0[:, c])
        lrs = []
        e = 1.0
        assert 2.0 ** -19 < eps < 2.0 ** 9                   # a power of two inside the clamps, reached by the loop's own exit
        while True:                                          # the log-ratios at 1, and at every step size up to and including the returned one
            q1, p1, div = om.leapfrog(cells[:, c], q, p0[:, c], e, 1)
            lrs.append(-np.inf if div else h0 - (-om.log_joint_at(cells[:, c], q1) + 0.5 * float(p1 @ p1)))
            if e == eps: break
            e = e * 2.0 if eps > 1.0 else e / 2.0
        want = min(abs(x - np.log(0.5)) for x in lrs)        # (ratio)^a > 2^-a compares the ratio with 1/2 in either direction
        assert dist == pytest.approx(want, rel=1e-9), (c, eps, lrs)
    assert len(seen) >= 2                                    # the chains do not all stop at the same step size


# ---------------------------------------------------------------------------------- the rule itself
def test_excused_refuses_a_parted_chain_with_a_wide_margin():
    parted = np.zeros(70, dtype=bool); parted[67] = True
    margin = np.full(70, 0.5); margin[67] = 1e-3
    with pytest.raises(AssertionError) as ei:
        knife.excused("made-up", parted, margin, 1e-6, first_bad={67: dict(step=4, site="x", device=1.0, oracle=2.0)}, chain0=5)
    msg = str(ei.value)
    assert "chain 67 (global id 72, lane 3 of wave 1)" in msg and "1.000e-03" in msg and "'step': 4" in msg and "'site': 'x'" in msg


def test_excused_excuses_a_parted_chain_on_a_knife_edge_and_warns():
    parted = np.zeros(70, dtype=bool); parted[67] = True
    margin = np.full(70, 0.5); margin[67] = 1e-8
    with pytest.warns(knife.KnifeEdge, match="chain=67, global_id=72, lane=3, wave=1"):
        mask = knife.excused("made-up", parted, margin, 1e-6, chain0=5)
    assert np.array_equal(mask, parted)
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # nothing parted: nothing excused, nothing said
        assert not knife.excused("made-up", np.zeros(70, dtype=bool), margin, 1e-6).any()
    margin[67] = np.nan                                      # an unknown margin excuses nothing
    with pytest.raises(AssertionError):
        knife.excused("made-up", parted, margin, 1e-6)


def test_a_chain_replaced_by_its_neighbour_fails_the_hmc_comparison(oracle):
    """The same for free-running hmc_chain (test_gpu_parity._excuse_hmc_chains): only the chain that differs is replayed, from its global id."""
    from tests.test_gpu_parity import _excuse_hmc_chains
    k = PC.HMC_CASES["adaptive-normal32"]
    om = oracle.OracleModel(k.make())
    cfg = oracle.HmcConfig.default(n_leapfrog=k.n_leapfrog, init_step_size=k.step_size)
    odraws, _, _, _ = om.hmc_run(k.seed, k.C, k.nw, k.ns, cfg, chain0=k.chain0, n_threads=8)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert not _excuse_hmc_chains("made-up", oracle, om, k, odraws.copy(), odraws, rtol=1e-4, atol=1e-5).any()
    wrong = odraws.copy()
    wrong[1:, :, 65] = odraws[1:, :, 64]                     # from the second recorded transition on
    with pytest.raises(AssertionError) as ei:
        _excuse_hmc_chains("made-up", oracle, om, k, wrong, odraws, rtol=1e-4, atol=1e-5)
    msg = str(ei.value)
    assert "1 of 96 chains" in msg and "chain 65 (global id 72, lane 1 of wave 1)" in msg and "'recorded_transition': 1, 'transition': 4" in msg, msg


def test_a_chain_replaced_by_its_neighbour_fails_the_mh_comparison(oracle):
    """What the rule is for.  The oracle's own draws with chain 70 (lane 6 of the ragged second wave) holding chain 69's -- a wrong chain offset
    in one lane -- passed the comparison that allowed one chain; now it fails, naming the chain and recorded step 0."""
    from tests.test_gpu_mh import _compare

    class Sites:
        pass
    k = PC.MH_CASES["zoo-normal32"]
    om = oracle.OracleModel(k.make())
    cp = Sites()
    cp.S, cp.site_vtypes, cp.site_names = om.S, om.site_vtypes, om.site_names
    dist, o = OM.mh_margins(om, k.seed, k.C, k.nw, k.ns, None, k.chain0)
    odraws = o["draws"][k.nw:]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert not _compare(cp, odraws.copy(), odraws, dist, chain0=k.chain0).any()
    wrong = odraws.copy()
    wrong[:, :, 70] = odraws[:, :, 69]
    with pytest.raises(AssertionError) as ei:
        _compare(cp, wrong, odraws, dist, chain0=k.chain0)
    msg = str(ei.value)
    assert "1 of 96 chains" in msg and "chain 70 (global id 73, lane 6 of wave 1)" in msg and "'recorded_step': 0" in msg, msg
