"""One tempering step of smc_run's ladder (fg_device_smc_temper: the kernels fg_smc_run launches, in its order) against the oracle on
adversarial log-likelihoods: sizes at every grain of the passes, smooth curves from flat to steep, ties, the beta + 1e-9 corner reached
naturally, non-finite values, roots on both sides of where the bisection's bracket reaches adjacent doubles.  Each case runs with the zoom
passes, with the plain passes only, and with the separate-kernels reweight forced.

  * beta': bit-identical to the oracle's next_beta or a root to working precision (tests/smc_judge.py);
  * log_norm: the exact log_sum_exp(lw0 + (beta' - beta) ll) at the device's own beta' within smc_judge.log_norm_tol -- ~64 eps
    (1 + max |(beta' - beta)(ll_i - max ll)|) for the product form E R^j of the pass sums, plus rounding of the maximum and summation --
    and, where the betas agree, the oracle's log_sum_exp of the same array within the same tolerance;
  * log_w / w: comb - log_norm from the device's beta' and log_norm, to a few ulps; the weights sum to one;
  * non-finite inputs: the class of beta', of the evidence (finite / -inf / +inf / NaN) and of the weights (the uniform fallback) is the
    oracle's."""
import math

import numpy as np
import pytest

from fugue_amd import engine as E
from tests import smc_judge as J

pytestmark = pytest.mark.gpu

CASES = J.step_cases()
RUNS = (("zoom", True, False), ("plain", False, False), ("force_sum", True, True))


def _cls(x):
    return "nan" if math.isnan(x) else ("-inf" if x == -math.inf else ("+inf" if x == math.inf else "finite"))


def _check_weights(r, ll, beta, n, where):
    lw0 = -math.log(n)
    b, ln = r["beta"], r["log_norm"]
    if math.isfinite(ln):
        with np.errstate(invalid="ignore"):
            comb = lw0 + (b - beta) * ll
        want = comb - ln
        fin = np.isfinite(want)
        assert np.array_equal(fin, np.isfinite(r["log_w"])), where
        assert (r["log_w"][~fin] == -np.inf).all() and (r["w"][~fin] == 0.0).all(), where
        # the same operations as the device's (built with -ffp-contract=off); a few ulps of the larger operand allowed
        scale = np.maximum(np.abs(comb[fin]), abs(ln))
        err = np.abs(r["log_w"][fin] - want[fin])
        assert (err <= 4.0 * np.spacing(scale)).all(), (where, float((err / np.spacing(scale)).max()))
        np.testing.assert_allclose(r["w"][fin], np.exp(r["log_w"][fin]), rtol=1e-15, atol=0, err_msg=where)   # (the device's exp)
        assert abs(math.fsum(r["w"].tolist()) - 1.0) < 1e-12, where
    else:                                      # the uniform fallback (smc.rs:524-528)
        np.testing.assert_allclose(r["log_w"], lw0, rtol=4e-16, atol=0, err_msg=where)    # (-ln n by the device's log)
        np.testing.assert_allclose(r["w"], 1.0 / n, rtol=1e-15, atol=0, err_msg=where)


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_tempering_step_matches_the_oracle(oracle, c):
    ll = c.ll()
    n, beta, target = c.n, c.beta, c.target
    lw0 = -math.log(n)
    want_b = oracle.next_beta(beta, np.full(n, lw0), ll, target)
    with np.errstate(invalid="ignore"):
        want_ln = oracle.log_sum_exp(lw0 + (want_b - beta) * ll)
    curve = J.Curve(ll, beta)
    got = {name: E.device_smc_temper(beta, ll, target, zoom=zoom, force_sum=fs) for name, zoom, fs in RUNS}
    betas = {name: r["beta"] for name, r in got.items()}
    for name, r in got.items():
        where = f"{c.name} [{name}]"
        b, ln = r["beta"], r["log_norm"]
        # beta'
        if c.kind == "nonfinite":
            assert b == want_b, (where, b, want_b)
        else:
            assert J.accept(curve, target, b, want_b, case=where), (where, repr(b), repr(want_b), J.is_root(curve, target, b))
        # the path: beta + 1e-9 is no candidate of any pass -- the separate kernels take the step (and always when forced)
        if name == "force_sum":
            assert r["need_sum"], where
        elif c.kind == "steep":
            assert b == beta + 1e-9 and r["need_sum"], (where, b, r["need_sum"])
        # the log-normaliser
        assert _cls(ln) == _cls(want_ln) or b != want_b, (where, ln, want_ln)
        if c.kind == "nonfinite":
            assert _cls(ln) == _cls(want_ln), (where, ln, want_ln)
        if math.isfinite(ln):
            tol = J.log_norm_tol(ll, beta, b)
            exact = J.exact_log_norm(ll, beta, b)
            assert abs(ln - exact) <= tol, (where, ln, exact, tol)
            if b == want_b:                    # (the oracle's own sequential sum adds up to (n - 1) eps: tied terms round alike)
                tol_ref = tol + J.EPS * (n - 1)
                assert abs(ln - want_ln) <= tol_ref, (where, ln, want_ln, tol_ref)
        _check_weights(r, ll, beta, n, where)
    # the three runs agree, or each passed the judge above
    if len(set(betas.values())) > 1:
        assert c.kind not in ("nonfinite", "steep"), (c.name, betas)


@pytest.mark.parametrize("name", ["root0.0001edge-n65-b0.3-t0.5", "smooth1e+06-n2049-b0.3-t0.01", "smooth1e+06-n65-b0.999999-t0.5"])
def test_candidates_are_evaluated_where_they_are_recorded(oracle, name):
    """Regression: the passes' product form E R^k evaluated grid point k at lo + k dl, up to half an ulp of b from the double the bracket
    records (the reference's midpoint chain, wl + k wd).  Near beta = 0.3 with b - beta ~ 1e-8 that moved the exponent by ~3e-9: beta'
    came out one ulp below the crossing (ESS(beta') / target - 1 = 2e-10) and log_norm, taken from the same sums, 1e-10 off."""
    c = next(c for c in CASES if c.name == name)
    ll = c.ll()
    curve = J.Curve(ll, c.beta)
    want = oracle.next_beta(c.beta, np.full(c.n, -math.log(c.n)), ll, c.target)
    for zoom in (True, False):
        r = E.device_smc_temper(c.beta, ll, c.target, zoom=zoom)
        assert J.accept(curve, c.target, r["beta"], want, case=f"{name} zoom={zoom}"), (zoom, r["beta"], want, J.is_root(curve, c.target, r["beta"]))
        assert abs(r["log_norm"] - J.exact_log_norm(ll, c.beta, r["beta"])) <= J.log_norm_tol(ll, c.beta, r["beta"]), zoom
