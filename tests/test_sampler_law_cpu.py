"""The law of the rejection samplers, judged on the CPU oracle alone (no GPU): every check of tests/sampler_cases.py over
oracle.sample_dist / OracleModel.run_prior draws from the streams the device tests use.  The oracle (oracle/orc_numerics.c) restates the
algorithms of fugue_amd/csrc/fg_math.h line for line, so this file is what shows that the thresholds of
tests/test_gpu_sampler_branches.py are met by a correct sampler at these seeds -- and a case that fails here is a finding about the
algorithm, not a reason to pick another seed.  Every figure goes into the assertion message.

Figures of this file at N = 16384: discrete cases, smallest chi-square p-value 0.075 (binom_20_0.5; 0.185 without the Binomial(20, .)
pair), largest mean z 1.44; continuous cases, largest KS D 0.0094 against the critical value 0.0152, largest mean z 1.70; mixed model, PIT
KS D 0.0059 (Poisson), 0.0083 (Binomial), 0.0086 (Gamma), 0.0065 (e_z).

The edge parameters are pinned too: which of them draw nothing from the stream, what the invalid ones return (a non-finite Binomial p:
0 without a draw, as Bernoulli; a Poisson rate whose draws lie above 2^63: the saturated cast), and the host build of fg_sample_dist
runs them and 1e5 random valid parameter sets per family under the undefined-behaviour and float-cast sanitizers."""
import math
import os
import subprocess

import numpy as np
import pytest

from tests import sampler_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", SC.CASES, ids=[c.name for c in SC.CASES])
def test_table_cases_take_the_code_path_they_name(case):
    got = SC.branch_reached(case)
    print(f"{case.name} [{case.branch}]: table path '{case.path}', the samplers' own comparisons give '{got}'")
    assert got == case.path
    if case.name in ("binom_25_0.4", "binom_20_0.5"):
        assert float(case.params[0]) * case.params[1] == 10.0          # the product rounds to exactly 10: `n q < 10` is false


@pytest.mark.parametrize("case", SC.CASES, ids=[c.name for c in SC.CASES])
def test_law_of_the_oracle_draws(oracle, case):
    x, blocks = SC.oracle_draws(oracle, case)
    print(f"{case.name}: Philox blocks per draw min {blocks.min()}, mean {blocks.mean():.2f}, max {blocks.max()}")
    SC.check_case(case, x)
    assert blocks.min() >= 1 and blocks.max() < 1000              # far from the caps of the rejection loops


@pytest.mark.parametrize("case", SC.LARGE, ids=[c.name for c in SC.LARGE])
def test_large_sample_law_of_the_transformed_rejection_branches(oracle, case):
    """2^20 draws of every PTRS / BTRS case.  Measured with the oracle's constants changed by 5 % (never committed): PTRS vr * 1.05 leaves
    every draw of Poisson(30) and all but a few of Poisson(100.5) unchanged and passes all three Poisson cases at N = 16384 (p = 0.19, 0.93,
    0.51); at 2^20 draws Poisson(5000) fails (chi-square 719 on 558 df).  BTRS alpha * 1.05 and * 0.95 pass every Binomial case at N = 16384
    (smallest p 0.06 and 0.02); at 2^20 draws Binomial(10^6, 0.37) fails both (3721 and 3836 on 3315 df) and Binomial(1000, 0.5) the
    second (204 on 134 df).  Unchanged, the smallest p-value of the nine cases at 2^20 draws is 0.050."""
    x, blocks = SC.oracle_draws(oracle, case, SC.N_LARGE)
    assert np.array_equal(x[:SC.N], SC.oracle_draws(oracle, case)[0]) and blocks.max() < 1000
    SC.check_case(case, x)


def _mixed_cells(oracle, n):
    om = oracle.OracleModel(SC.mixed_program())
    assert om.site_names == SC.MIXED_SITES
    return np.stack([om.run_prior(SC.SEED_MIXED, c, 0)[0] for c in range(n)], axis=1)


def test_law_of_the_mixed_model_given_the_parent(oracle):
    cells = _mixed_cells(oracle, SC.N)
    SC.check_mixed(cells)
    # the site-fed parameters are the restated ones: the oracle's own draw at those parameters, from a stream advanced as run_prior's
    u, k, b, g, z = SC.mixed_decode(cells)
    par = SC.mixed_params(u)
    for c in range(0, 512):
        s = oracle.stream(SC.SEED_MIXED, c, 0, 1)
        assert oracle.sample_dist("Uniform", [0.0, 1.0], s) == u[c]
        assert oracle.sample_dist("Poisson", [par["lam"][c]], s) == k[c]
        assert oracle.sample_dist("Binomial", [30, par["p"][c]], s) == b[c]
        assert oracle.sample_dist("Gamma", [par["shape"][c], 2.0], s) == g[c]
        assert oracle.sample_dist("Normal", [0.0, 1.0], s) == z[c]


@pytest.mark.parametrize("edge", SC.EDGES, ids=[e[0] for e in SC.EDGES])
def test_edge_parameters(oracle, edge):
    name, family, params, want, want_blocks = edge
    for chain in range(64):
        s = oracle.stream(5, chain, 0, 1)
        got = oracle.sample_dist(family, params, s)
        if chain == 0:
            print(f"{name}: {family}{tuple(params)} -> {got} after {s.c1} blocks")
        assert got == want, (name, chain, got)
        if want_blocks is None:
            assert 1 <= s.c1 < 1000, (name, chain, s.c1)
        else:
            assert s.c1 == want_blocks, (name, chain, s.c1)
        if want_blocks is not None:                              # the next site starts where this one stopped
            s2 = oracle.stream(5, chain, 0, 1)
            s2.c1 = want_blocks
            assert oracle.sample_dist("Normal", [0.0, 1.0], s) == oracle.sample_dist("Normal", [0.0, 1.0], s2)
    if name == "binom_nan":
        for p in (math.inf, -math.inf):
            s = oracle.stream(5, 0, 0, 1)
            assert oracle.sample_dist("Binomial", [10, p], s) == 0 and s.c1 == 0
    if name == "pois_1e19":
        for lam in (1e300, 1.7976931348623157e308):
            s = oracle.stream(5, 0, 0, 1)
            assert oracle.sample_dist("Poisson", [lam], s) == SC.I64_MAX
        s = oracle.stream(5, 0, 0, 1)                             # below 2^63 nothing saturates
        k = oracle.sample_dist("Poisson", [1e18], s)
        assert abs(k - 10 ** 18) < 12 * 10 ** 9 and k < SC.I64_MAX


def test_samplers_on_the_host_under_the_sanitizers(tmp_path):
    """tests/cpp/test_sampler_edges.cpp: fg_sample_dist of fg_math.h itself (host build) on the edge list and on 1e5 random valid
    parameter sets per family, with -fsanitize=undefined,float-cast-overflow and no recovery: a float-to-integer conversion out of
    range (what Binomial(n, NaN) and Poisson(1e19) ran into) ends the program."""
    exe = str(tmp_path / "test_sampler_edges")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=undefined,float-cast-overflow", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "cpp", "test_sampler_edges.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sampler edges ok" in r.stdout and "runtime error" not in r.stderr
