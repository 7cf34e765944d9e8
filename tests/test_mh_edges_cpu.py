"""The oracle's single-site MH on the edge cases of tests/mh_edge_cases.py, checked against expectations written from the reference by hand
(src/inference/mh.rs:180-295, 339-358, 698-744; src/inference/mcmc_utils.rs:88-150), not from the oracle: the proposals are recomputed
here from the step's own random numbers and the state before the step.  Also the two conditions tests/test_gpu_mh_edges.py leans on, for
its exact seeds, models and starts: no accept decision closer than MARGIN to its uniform, and every listed branch taken often enough."""
import ctypes
import math

import numpy as np
import pytest

from tests import mh_edge_cases as K

T = K.NW + K.NS


def _f(cells):
    return np.asarray(cells, dtype=np.int64).view(np.float64)


def _same_cell(a: float, b: float) -> bool:
    return K.f64_cell(a) == K.f64_cell(b) or (math.isnan(a) and math.isnan(b))


def _round_half_away(x: float) -> int:                     # f64::round (mh.rs:287)
    return int(math.copysign(math.floor(abs(x) + 0.5), x))


class Run:
    """One oracle run of a model from the table's starts, with every step's random numbers drawn again from its stream."""

    def __init__(self, orc, which):
        self.orc, self.which = orc, which
        self.om = om = orc.OracleModel(K.MODELS[which]())
        self.seed = K.SEEDS[which]
        self.names, self.vt, self.S = om.site_names, om.site_vtypes, om.S
        self.ov = K.overrides(self.names)
        self.start = K.start_cells(om, self.seed)
        self.o = om.mh_run_from(self.seed, K.C, K.NW, K.NS, start=self.start, overrides=self.ov, chain0=K.CHAIN0, n_threads=8)
        L = orc.lib()
        # the step's stream again (mh.rs:716 the target from block 0; then gaussian_z or nothing; then the accept uniform)
        self.pick = np.zeros((T, K.C), dtype=np.int64)
        self.z = np.zeros((T, K.C))                        # gaussian_z from the block after the target's
        self.u_after_z = np.zeros((T, K.C))                # the uniform after that Gaussian
        self.u_first = np.zeros((T, K.C))                  # the uniform straight after the target's block (a proposal that drew nothing)
        ra, rb = ctypes.c_uint64(), ctypes.c_uint64()
        for t in range(T):
            for c in range(K.C):
                s = orc.stream(self.seed, K.CHAIN0 + c, t, K.RNG_MH)
                L.orc_stream_block(ctypes.byref(s), ctypes.byref(ra), ctypes.byref(rb))
                self.pick[t, c] = (ra.value * self.S) >> 64
                s2 = orc.Stream.from_buffer_copy(s)
                self.u_first[t, c] = L.orc_stream_u01(ctypes.byref(s2))
                self.z[t, c] = L.orc_stream_gaussian_z(ctypes.byref(s))
                self.u_after_z[t, c] = L.orc_stream_u01(ctypes.byref(s))
        # state and scale BEFORE each step
        self.before = np.concatenate([self.start[None], self.o["draws"][:-1]], axis=0)          # [T][S][C]
        self.scale_before = np.ones((T, K.C))
        sc = np.ones((self.S, K.C))
        cols = np.arange(K.C)
        for t in range(T):
            tg = self.o["target"][t]
            self.scale_before[t] = sc[tg, cols]
            sc[tg, cols] = self.o["scale"][t]
        self.final_scales = sc

    def kind(self, j, c):
        o = self.ov[j]
        return o[0] if o is not None else int(self.o["kinds"][j, c])

    def steps(self):
        tg = self.o["target"]
        for t in range(T):
            for c in range(K.C):
                yield t, c, int(tg[t, c])

    def lw(self, cells):
        acc, _ = self.om.run_score(cells)
        return acc[0] + acc[1] + acc[2]


@pytest.fixture(scope="module", params=["A", "B"])
def run(request, oracle):
    return Run(oracle, request.param)


def _bounces(pr, lo, hi):
    n = 0
    while pr < lo or pr > hi:                               # mh.rs:247-254
        if pr < lo: pr = 2.0 * lo - pr
        if pr > hi: pr = 2.0 * hi - pr
        n += 1
    return min(max(pr, lo), hi), n


def test_the_models_are_what_the_table_says(oracle):
    a, b = oracle.OracleModel(K.model_a()), oracle.OracleModel(K.model_b())
    assert a.site_names == sorted("bcegknruvw") and b.site_names == sorted("bcdegknruvw")
    assert [b.site_vtypes[b.site_names.index(s)] for s in "bcdk"] == [K.BOOL, K.USIZE, K.I64, K.U64]
    assert len(K.CASES) * 3 <= K.C and K.C % 64 != 0        # every case in several lanes, a part-filled last tile
    for case in K.CASES:                                    # the reflection budget of the module's docstring
        for name, x in case.items():
            if name in K.REFLECT and math.isfinite(x):
                lo, hi = K.REFLECT[name]
                assert hi - lo >= 1.0 and lo - 40 * (hi - lo) <= x <= hi + 40 * (hi - lo)


def test_run_from_the_prior_state_reproduces_mh_run(oracle):
    om = oracle.OracleModel(K.model_a())
    ov = K.overrides(om.site_names)
    draws, final, scales, st = om.mh_run(K.SEEDS["A"], 40, K.NW, K.NS, ov, chain0=K.CHAIN0)
    prior = np.stack([om.run_prior(K.SEEDS["A"], K.CHAIN0 + c)[0] for c in range(40)], axis=1)
    for start in (None, prior):
        o = om.mh_run_from(K.SEEDS["A"], 40, K.NW, K.NS, start=start, overrides=ov, chain0=K.CHAIN0)
        assert np.array_equal(o["draws"][K.NW:], draws) and np.array_equal(o["final"], final)
        assert np.array_equal(o["scales"], scales) and o["stats"].accept_rate == st.accept_rate
        assert o["stats"].n_model_evals == st.n_model_evals
        assert int(o["accept"].sum()) == round(st.accept_rate * 40 * T)


def test_every_step_picks_its_target_from_block_0(run):
    assert np.array_equal(run.o["target"], run.pick)        # sites[rng.gen_range(0..len)]: mh.rs:716


def test_the_accept_rule_and_its_uniform(run):
    """mh.rs:733: log_alpha >= 0 accepts without a uniform; otherwise -- NaN included -- one uniform is drawn, from the block after the
    proposal's, and NaN rejects.  The state moves to the proposal exactly on acceptance."""
    o = run.o
    la, u, acc = o["log_alpha"], o["u"], o["accept"].astype(bool)
    assert np.array_equal(np.isnan(u), la >= 0.0)
    assert acc[la >= 0.0].all() and not acc[np.isnan(la)].any()
    dec = ~(la >= 0.0) & ~np.isnan(la)
    assert np.array_equal(acc[dec], u[dec] < np.exp(la[dec]))
    drew_nothing = np.zeros((T, K.C), dtype=bool)
    for t, c, j in run.steps():
        cur = _f(run.before[t, j, c:c + 1])[0]
        drew_nothing[t, c] = run.vt[j] == K.BOOL or (run.vt[j] == K.F64 and run.kind(j, c) == K.PROP_LOGSPACE and cur <= 0.0)
        after = run.o["draws"][t, :, c]
        want = run.before[t, :, c].copy()
        if acc[t, c]: want[j] = o["proposed"][t, c]
        assert np.array_equal(after, want), (t, c, run.names[j])
    walk = np.isin(run.o["target"], [j for j in range(run.S) if run.vt[j] != K.USIZE])
    m = walk & ~np.isnan(u)
    assert np.array_equal(u[m], np.where(drew_nothing, run.u_first, run.u_after_z)[m])
    assert (m & drew_nothing).sum() >= K.MIN_TAKES


def test_logspace_walk_corners(run):
    """LogSpaceWalkProposal, mh.rs:201-224."""
    n_nonpos = n_over = n_under = n_block1_decides = n_block2_would_differ = 0
    for t, c, j in run.steps():
        if run.vt[j] != K.F64 or run.kind(j, c) != K.PROP_LOGSPACE: continue
        cur = _f(run.before[t, j, c:c + 1])[0]
        prop = _f(run.o["proposed"][t, c:c + 1])[0]
        where = (run.which, t, c, run.names[j], cur, prop)
        if cur <= 0.0:                                      # :203-206, and both log_proposal_prob are 0 (:218-220)
            assert K.f64_cell(prop) == K.f64_cell(K.MIN_POSITIVE), where
            state = run.before[t, :, c].copy()
            lw0 = run.lw(state)
            state[j] = run.o["proposed"][t, c]
            with np.errstate(invalid="ignore"):
                want = run.lw(state) - lw0 + (0.0 - 0.0)
            assert _same_cell(run.o["log_alpha"][t, c], want), where
            n_nonpos += 1
            la = run.o["log_alpha"][t, c]
            if math.isfinite(la) and la < 0.0:              # no z was drawn: the uniform is the first value after the target's block (:733)
                assert run.o["u"][t, c] == run.u_first[t, c] and bool(run.o["accept"][t, c]) == (run.u_first[t, c] < math.exp(la)), where
                n_block1_decides += 1
                n_block2_would_differ += bool(run.o["accept"][t, c]) != (run.u_after_z[t, c] < math.exp(la))
            continue
        with np.errstate(all="ignore"):
            raw = float(np.exp(np.log(np.float64(cur)) + run.scale_before[t, c] * run.z[t, c]))
        if not math.isfinite(raw):                          # :209-214 (a NaN or +inf current lands here too)
            assert K.f64_cell(prop) == K.f64_cell(K.F64_MAX), where
            n_over += 1
        elif raw < K.MIN_POSITIVE * (1 - 1e-9):             # :210
            assert K.f64_cell(prop) == K.f64_cell(K.MIN_POSITIVE), where
            n_under += 1
        elif raw > K.MIN_POSITIVE * (1 + 1e-9):
            assert prop == pytest.approx(raw, rel=1e-12), where
    assert min(n_nonpos, n_over, n_under, n_block1_decides) >= K.MIN_TAKES, (n_nonpos, n_over, n_under, n_block1_decides)
    assert n_block2_would_differ >= 5, n_block2_would_differ          # a kernel that took the uniform of the block after z's parts ways that often


def test_reflection_corners(run):
    """ReflectionWalkProposal, mh.rs:237-257: range <= 0 returns the current value after the Gaussian was drawn."""
    n_degenerate = n_u_after_z = n_multi = n_outside = 0
    for t, c, j in run.steps():
        if run.vt[j] != K.F64 or run.kind(j, c) != K.PROP_REFLECT: continue
        lo, hi = run.ov[j][1], run.ov[j][2]
        cur = _f(run.before[t, j, c:c + 1])[0]
        where = (run.which, t, c, run.names[j], cur)
        if hi - lo <= 0.0:
            assert run.o["proposed"][t, c] == run.before[t, j, c], where
            n_degenerate += 1
            if not np.isnan(run.o["u"][t, c]):              # the stream still advanced by one Gaussian
                assert run.o["u"][t, c] == run.u_after_z[t, c] != run.u_first[t, c], where
                n_u_after_z += 1
            continue
        prop = _f(run.o["proposed"][t, c:c + 1])[0]
        if math.isnan(cur):
            assert math.isnan(prop), where
            continue
        want, nb = _bounces(cur + run.scale_before[t, c] * run.z[t, c], lo, hi)
        assert nb < 1000 and lo <= prop <= hi and prop == pytest.approx(want, rel=1e-12, abs=1e-12), where
        n_multi += nb > 1
        n_outside += cur < lo or cur > hi
    assert min(n_degenerate, n_u_after_z, n_multi, n_outside) >= K.MIN_TAKES, (n_degenerate, n_u_after_z, n_multi, n_outside)


def test_kind_of_a_positive_support_site_is_decided_once(run):
    """f64_kind, mh.rs:339-358: the first visit decides -- LogSpace where the current value is > 0 (NaN is not), Gaussian otherwise, for good."""
    n_gauss = n_gauss_from_positive = 0
    for name in K.POSITIVE_AUTO:
        j = run.names.index(name)
        first = np.full(K.C, -1)
        for t in range(T - 1, -1, -1): first[run.o["target"][t] == j] = t
        for c in range(K.C):
            k = int(run.o["kinds"][j, c])
            if first[c] < 0: assert k == K.PROP_AUTO; continue
            cur0 = _f(run.before[first[c], j, c:c + 1])[0]
            assert k == (K.PROP_LOGSPACE if cur0 > 0.0 else K.PROP_GAUSSIAN), (name, c, cur0)
            if name in K.case_of_chain(c): assert cur0 == K.case_of_chain(c)[name] or math.isnan(cur0)
        for t, c, jj in run.steps():
            if jj != j: continue
            cur, prop = _f(run.before[t, j, c:c + 1])[0], _f(run.o["proposed"][t, c:c + 1])[0]
            if run.o["kinds"][j, c] == K.PROP_GAUSSIAN:         # mh.rs:183-187, whatever the site's value has become since
                assert prop == pytest.approx(cur + run.scale_before[t, c] * run.z[t, c], rel=1e-12, abs=1e-300, nan_ok=True)
                n_gauss += 1
                n_gauss_from_positive += cur > 0.0
            else:
                assert prop > 0.0
    assert n_gauss >= K.MIN_TAKES and n_gauss_from_positive >= 1, (n_gauss, n_gauss_from_positive)


def test_discrete_walks(run):
    """DiscreteWalkProposal, mh.rs:285-294: k + delta < 0 reflects about -1/2; the i64 walk has no boundary (mh.rs:566-567); the flip."""
    n_reflected = {0: 0, 1: 0}
    for t, c, j in run.steps():
        cur, prop = int(run.before[t, j, c]), int(run.o["proposed"][t, c])
        if run.vt[j] == K.BOOL: assert prop == (0 if cur else 1)
        if run.vt[j] not in (K.U64, K.I64): continue
        k = cur + _round_half_away(run.scale_before[t, c] * run.z[t, c])
        if run.vt[j] == K.I64: assert prop == k; continue
        assert prop == (k if k >= 0 else -k - 1), (run.which, t, c, cur, k, prop)
        if k < 0 and cur in n_reflected: n_reflected[cur] += 1
    assert min(n_reflected.values()) >= K.MIN_TAKES, n_reflected


def test_non_finite_accept_operands(run):
    """mh.rs:731-733 with a -inf current log-weight: a finite proposal gives +inf and accepts, a -inf proposal gives NaN and rejects;
    a NaN cell keeps its chain where it is; the chains whose Categorical index has no probability never move at all."""
    la, acc = run.o["log_alpha"], run.o["accept"].astype(bool)
    n_posinf, n_nan = int(np.isposinf(la).sum()), int(np.isnan(la).sum())
    assert acc[np.isposinf(la)].all()
    assert n_posinf >= K.MIN_TAKES and n_nan >= K.MIN_TAKES, (n_posinf, n_nan)
    jc = run.names.index("c")
    stuck = [c for c in range(K.C) if "c" in K.case_of_chain(c)]
    nan_cell = [c for c in range(K.C) if any(isinstance(x, float) and math.isnan(x) for x in K.case_of_chain(c).values())]
    assert len(stuck) >= 12 and len(nan_cell) >= 9
    for c in stuck + nan_cell:
        assert np.isnan(la[:, c]).all() and not acc[:, c].any()
        assert np.array_equal(run.o["final"][:, c], run.start[:, c])
    assert all(run.start[jc, c] == K.case_of_chain(c)["c"] for c in stuck)
    # (a NaN value scores -inf, not NaN: every log_prob of the reference guards its argument, as Normal's does at distribution.rs:189-208)
    assert np.isneginf(run.o["log_weight"][stuck + nan_cell]).all()


def test_no_decision_is_closer_than_the_margin(run):
    """What lets the device test allow no parted chain: over every decided step, |ln u - log_alpha| >= MARGIN -- seven orders above the
    error of exp / log in either library, three above the multi-wave kernels' own decision margin."""
    la, u = run.o["log_alpha"], run.o["u"]
    dec = np.isfinite(la) & (la < 0.0)
    assert dec.sum() > 1000
    with np.errstate(divide="ignore"):
        gap = np.abs(np.log(u[dec]) - la[dec])
    assert gap.min() >= K.MARGIN, gap.min()


def test_frozen_steps_leave_the_oracle_adaptation_alone(run):
    sc = np.ones((run.S, K.C))
    cols = np.arange(K.C)
    for t in range(K.NW): sc[run.o["target"][t], cols] = run.o["scale"][t]
    assert np.array_equal(sc, run.o["scales"])
    for t in range(K.NW, T): assert np.array_equal(run.o["scale"][t], sc[run.o["target"][t], cols])


# ---------------------------------------------------------------------------------- DiminishingAdaptation::update
def _adapt_by_hand(accepts):
    """mcmc_utils.rs:88-150 for one site, target rate 0.44, gamma 0.7: the scale after every update."""
    scale, log_scale, acc, tot, out = 1.0, 0.0, 0, 0, []
    for a in accepts:
        tot += 1; acc += int(a)
        if tot >= 10:                                       # :112-114
            log_scale += (1.0 / tot ** 0.7) * (acc / tot - 0.44)
            ns = math.exp(log_scale)
            scale = min(max(ns, 0.001), 100.0) if math.isfinite(ns) and ns > 0.0 else 1.0
            log_scale = 0.0 if scale == 1.0 else math.log(scale)
        out.append(scale)
    return np.array(out)


@pytest.mark.parametrize("name", sorted(K.ADAPT))
def test_adaptation_gate_and_clamps(oracle, name):
    make, x0, steps, clamp = K.ADAPT[name]
    om = oracle.OracleModel(make())
    o = om.mh_run_from(K.ADAPT_SEED, K.ADAPT_C, steps, 0, start=K.adapt_start(x0), chain0=K.ADAPT_CHAIN0)
    sc = o["scale"]
    assert (sc[:9] == 1.0).all()                            # total_count < 10: mcmc_utils.rs:112-114
    assert (sc[9] != 1.0).all()
    assert (sc[-1] == clamp).all(), (sc[-1].min(), sc[-1].max())      # the clamp: mcmc_utils.rs:139
    assert np.array_equal(o["scales"][0], sc[-1])
    first = (sc == clamp).argmax(axis=0)
    assert (first > 30).all() and first.max() < steps - 20            # reached step by step, and held for a while
    for c in range(0, K.ADAPT_C, 7):
        np.testing.assert_allclose(sc[:, c], _adapt_by_hand(o["accept"][:, c]), rtol=1e-13)


# ---------------------------------------------------------------------------------- the compiled kernels of the two models
@pytest.mark.parametrize("which", ["A", "B"])
@pytest.mark.parametrize("unit", ["FG_DEBUG_JIT_MHMW", "FG_DEBUG_JIT_MH", None])
def test_units_of_a_program_with_a_zero_probability_compile(which, unit, monkeypatch):
    """ln 0 = -inf in a Categorical's constant table has to be a constant expression in the generated unit (fg_jit.cpp, lit_static): a
    table initialised through a call does not compile, and the engine then runs the hand-written kernels without a word -- the compiled
    multi-wave MH kernel (both models), the statement-segment MH kernel and the HMC kernel were out of reach of any such program."""
    from fugue_amd import engine as E
    lib = E.lib()
    lib.fg_debug_jit_compile.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_longlong, ctypes.c_char_p, ctypes.c_longlong, ctypes.POINTER(ctypes.c_longlong)]
    for k in ("FG_DEBUG_JIT_MHMW", "FG_DEBUG_JIT_MH"): monkeypatch.delenv(k, raising=False)
    if unit: monkeypatch.setenv(unit, "1")
    cp = E.compile_model(K.MODELS[which]())
    src = ctypes.create_string_buffer(8 << 20); log = ctypes.create_string_buffer(1 << 20); n = ctypes.c_longlong()
    rc = lib.fg_debug_jit_compile(cp.h, src, len(src), log, len(log), ctypes.byref(n))
    assert rc == 0 and n.value > 0, log.value.decode()[:2000]
    assert "(-__builtin_huge_val())" in src.value.decode()
