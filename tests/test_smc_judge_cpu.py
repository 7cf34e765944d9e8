"""The judge of next_beta's answers (tests/smc_judge.py) on the CPU: the oracle's own answers pass it, answers moved off the root fail it,
and its 40-digit root agrees with the closed form of a two-point likelihood."""
import math

import mpmath
import numpy as np
import pytest

from tests import smc_judge as J

CASES = J.step_cases(max_n=100_000)


def _oracle_beta(oracle, c, ll):
    return oracle.next_beta(c.beta, np.full(c.n, -math.log(c.n)), ll, c.target)


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_oracle_next_beta_passes_the_judge(oracle, c):
    ll = c.ll()
    b = _oracle_beta(oracle, c, ll)
    if c.kind == "steep":                      # the corner these cases are built for: beta + 1e-9 wins (smc.rs:621)
        assert b == c.beta + 1e-9, b
        return
    if J.clamped(c.beta, b):
        return
    ok, e_hi, e_lo, D = J.is_root(J.Curve(ll, c.beta), c.target, b, reference=True)
    assert ok, (b, e_hi, e_lo, D)


def test_judge_rejects_answers_off_the_root(oracle):
    moved = 0
    for c in CASES:
        if c.n != 2049 or c.kind != "smooth" or c.name.startswith("halfneginf") or c.thr > 0.5:
            continue                           # (near thr = 1 the curve is flat: a move of 1e-6 stays within rounding of the target)
        ll = c.ll()
        b = _oracle_beta(oracle, c, ll)
        if J.clamped(c.beta, b):
            continue
        curve = J.Curve(ll, c.beta)
        assert J.accept(curve, c.target, b, b)
        for d in (1e-6, -1e-6):
            bm = b + d
            if c.beta < bm < 1.0:
                assert not J.accept(curve, c.target, bm, b, case=c.name), (c, b, d)
                moved += 1
    assert moved >= 20, moved
    # a steep curve: 64 ulps either way is no root
    c = next(c for c in CASES if c.name == "smooth1e+06-n2049-b0.3-t0.5")
    ll = c.ll()
    b = _oracle_beta(oracle, c, ll)
    curve = J.Curve(ll, c.beta)
    assert not J.clamped(c.beta, b)
    for k in (64, -64):
        bm = b + k * math.ulp(b)
        assert not J.accept(curve, c.target, bm, b, case=c.name), (b, bm)
    # a clamp the oracle did not take, away from the crossing, is no root
    assert not J.accept(curve, c.target, c.beta + 1e-9, b)
    assert not J.accept(curve, c.target, 1.0, b)


@pytest.mark.parametrize("n,k,c,thr,beta", [(2, 1, 3.0, 0.6, 0.0), (65, 1, 5.0, 0.5, 0.0), (2049, 683, 4.0, 0.5, 0.3),
                                            (2049, 10, 1e4, 0.01, 0.0), (131073, 13107, 0.5, 0.999, 0.3)])
def test_two_point_root_matches_the_closed_form(oracle, n, k, c, thr, beta):
    ll = J.two_point(n, k, c)
    curve = J.Curve(ll, beta)
    target = thr * n
    exact = J.two_point_root(n, k, c, target, beta)
    with mpmath.workdps(J.DPS):
        assert abs(curve.root(target) - exact) <= mpmath.mpf(10) ** -30 * (1 - mpmath.mpf(beta))
        assert abs(curve.ess(float(exact)) / target - 1) < 1e-12       # (at the double nearest the root)
    if n <= 2049:                              # the reference's answer passes the judge on this exact curve (its sums of tied terms round
        b = _oracle_beta(oracle, J.StepCase("twopoint", n, lambda rng, m: ll, beta, thr, "tie"), ll)     # one way: not within a bracket)
        ok, e_hi, e_lo, D = J.is_root(curve, target, b, reference=True)
        assert ok, (b, float(exact), e_hi, e_lo, D)
