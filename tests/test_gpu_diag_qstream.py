"""GPU tests of the streamed quantile selector (fg_diag_qstream.hip): result bits, passes and per-slot passes against the numpy
restatement (tests/qstream_restatement.py), result bits against a sort by key and against Engine.diag_quantiles on the same stored
buffer, under every chunking; adversarial columns; the edges; the protocol and the integrity error as error returns; the two
summary drivers against the stored-draws drivers.

Synthetic draws are uploaded once with Engine.upload; a chunk is a slice [n_c][d][C] of that buffer.  Every compared figure is
printed before it is asserted."""
import ctypes
import math

import numpy as np
import pytest

from fugue_amd import engine as E
from fugue_amd import inference as I
from fugue_amd import workloads as W
from tests import qstream_restatement as Q

pytestmark = pytest.mark.gpu

CHUNKINGS = {"one": [97], "mixed": [5, 31, 1, 60], "ones": [1] * 97}
SETTINGS = [(12, 0), (12, 8), (12, 7000), (5, 0)]


class _Engines:
    """One engine per chain count for the whole module (the model does not matter to the diagnostics calls), and every input
    uploaded once with its Engine.diag_quantiles."""

    def __init__(self):
        self.cp, self.by_c, self.bufs = E.compile_model(W.normal_sites(1)), {}, {}

    def get(self, C: int):
        if C not in self.by_c:
            self.by_c[C] = E.Engine(self.cp, C, seed=1)
        return self.by_c[C]

    def upload(self, name: str, x: np.ndarray):
        if name not in self.bufs:
            x = np.ascontiguousarray(x, dtype=np.float64)
            self.bufs[name] = (self.get(x.shape[2]), x, self.get(x.shape[2]).upload(x))
        return self.bufs[name]

    def close(self):
        for eng, _, ptr in self.bufs.values():
            eng.device_free(ptr)
        for e in self.by_c.values():
            e.close()


@pytest.fixture(scope="module")
def engines():
    pool = _Engines()
    yield pool
    pool.close()


def stream_select(eng, ptr, shape, probs, digit_bits, capacity, chunkings, replay_ptr=None):
    """Pass k is fed in chunkings[k mod len] from `ptr` (passes after the first from `replay_ptr` when given):
    (values, slot passes, passes)."""
    n, d, C = shape
    s = eng.diag_qstream(n, d, probs, digit_bits, capacity)
    try:
        k = 0
        while True:
            base, at = (ptr if k == 0 or replay_ptr is None else replay_ptr), 0
            for nc in chunkings[k % len(chunkings)]:
                s.update(base + at * d * C * 8, nc)
                at += nc
                assert s.count == at
            assert at == n and s.passes == k
            k += 1
            if s.end_pass():
                break
            assert s.count == 0
        vals, sp = s.result()
        return vals, sp, s.passes
    finally:
        eng.synchronize()
        s.close()


def check(label, engines, name, x, probs, digit_bits, capacity, chunkings, stored=True):
    """Every slot of x: stream == restatement == key sort (== diag_quantiles of the stored buffer), with the restatement's passes."""
    eng, x, ptr = engines.upload(name, x)
    want, want_sp, want_passes = Q.select_all(x, probs, digit_bits, capacity)
    ref = Q.reference_all(x, probs)
    got, got_sp, got_passes = stream_select(eng, ptr, x.shape, probs, digit_bits, capacity, chunkings)
    dq = eng.diag_quantiles(ptr, x.shape[0], x.shape[1], probs) if stored else ref
    for i in range(x.shape[1]):
        for q, p in enumerate(probs):
            print(f"{label} bits {digit_bits} cap {capacity} [{i}] p={p}: stream {int(Q.bits(got)[i, q]):016x} ({got_sp[i, q]} passes) restatement "
                  f"{int(Q.bits(want)[i, q]):016x} ({want_sp[i, q]}) sort {int(Q.bits(ref)[i, q]):016x} diag_quantiles {int(Q.bits(dq)[i, q]):016x}")
    print(f"{label}: passes stream {got_passes} restatement {want_passes}")
    assert np.array_equal(Q.bits(got), Q.bits(want))
    assert np.array_equal(Q.bits(got), Q.bits(ref))
    assert np.array_equal(Q.bits(got), Q.bits(dq))
    assert np.array_equal(got_sp, want_sp) and got_passes == want_passes


# ---- 1. normal draws -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", list(CHUNKINGS))
@pytest.mark.parametrize("digit_bits,capacity", SETTINGS)
def test_normal_draws_under_every_chunking(engines, digit_bits, capacity, first):
    """97 x 3 x 70 N(0, 1) draws (C = 70: a full wave and a partial one); the first pass in one chunking, the later passes in the
    other two in turn."""
    names = list(CHUNKINGS)
    order = [CHUNKINGS[names[(names.index(first) + k) % 3]] for k in range(3)]
    check(f"normal first={first}", engines, "normal", Q.normal_input(), Q.DEFAULT_PROBS, digit_bits, capacity, order)


# ---- 2. adversarial columns ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [0, 8])
@pytest.mark.parametrize("C", [70, 65])
def test_adversarial_columns(engines, C, capacity):
    """d = 3: special values (-inf, -1.5, +-0.0, +-5e-324, 1, 1 + 2^-52, +inf, NaN), values that differ in their last four bits,
    a constant; eight probabilities including 0 and 1.  The coordinates finish after different numbers of passes."""
    check(f"adversarial C={C}", engines, f"adversarial{C}", Q.adversarial_input(C), Q.PROBS8, 12, capacity, [[97], [5, 31, 1, 60]])


# ---- 3. edges --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("capacity", [0, 1])
def test_a_single_draw_of_a_single_chain(engines, capacity):
    check("n=1 C=1", engines, "single", np.full((1, 1, 1), -0.0), Q.PROBS8, 12, capacity, [[1]])


@pytest.mark.parametrize("probs", [(0.5,), Q.PROBS8], ids=["one_prob", "eight_probs"])
def test_one_full_wave_of_chains(engines, probs):
    x = np.random.default_rng(64).standard_normal((33, 2, 64))
    for capacity in (0, 8):
        check("C=64", engines, "c64", x, probs, 12, capacity, [[33], [32, 1]])


def test_two_probabilities_that_select_the_same_element(engines):
    """Equal ranks: the two slots share one group through every pass; with six groups wanted at 12 bits some count in global
    memory past the LDS histograms."""
    x = Q.normal_input()
    for probs in ((0.5, 0.5, 0.25), (0.1, 0.2, 0.3, 0.4, 0.4, 0.6, 0.7, 0.8)):
        for capacity in (0, 8):
            check("shared group", engines, "normal", x, probs, 12, capacity, [[97], [5, 31, 1, 60]])


# ---- 4. the protocol -------------------------------------------------------------------------------------------------------------
def test_call_order_and_arguments_are_error_returns(engines):
    eng, x, ptr = engines.upload("normal", Q.normal_input())
    n, d, C = x.shape
    s = eng.diag_qstream(n, d, Q.DEFAULT_PROBS, 12, 0)
    try:
        s.update(ptr, 90)
        for call, what in ((s.end_pass, "end_pass before n_total draws"), (s.result, "result before done"), (lambda: s.update(ptr, 8), "update past n_total")):
            with pytest.raises(E.EngineError) as err:
                call()
            print(f"{what}: {err.value}")
            assert err.value.code == E.FG_E_STATE, what
        assert s.count == 90 and s.passes == 0
        with pytest.raises(E.EngineError) as err:
            s.update(ptr, 0)
        assert err.value.code == E.FG_E_BAD_ARG
        s.update(ptr + 90 * d * C * 8, 7)
        while not s.end_pass():
            with pytest.raises(E.EngineError) as err:
                s.result()
            assert err.value.code == E.FG_E_STATE
            s.update(ptr, n)
        with pytest.raises(E.EngineError) as err:                          # an update after the stream is done
            s.update(ptr, 1)
        print(f"update after done: {err.value}")
        assert err.value.code == E.FG_E_STATE
        assert np.array_equal(Q.bits(s.result()[0]), Q.bits(Q.reference_all(x, Q.DEFAULT_PROBS)))
    finally:
        eng.synchronize()
        s.close()
    out = ctypes.c_void_p()
    pr = np.array(Q.DEFAULT_PROBS)
    bad_pr = [np.array([0.5, 1.5]), np.array([-0.1]), np.array([float("nan")])]
    dp = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    cases = [(0, 3, pr, 5, 12, 8), (97, 0, pr, 5, 12, 8), (97, 65536, pr, 5, 12, 8), (97, 3, pr, 0, 12, 8), (97, 3, np.full(9, 0.5), 9, 12, 8),
             (97, 3, pr, 5, 0, 8), (97, 3, pr, 5, 13, 8), (97, 3, pr, 5, 12, -1)] + [(97, 3, b, b.size, 12, 8) for b in bad_pr]
    for n_total, dd, probs, n_probs, digit_bits, capacity in cases:         # the library's own checks, below the Python ones
        rc = E.lib().fg_diag_qstream_new(eng.h, n_total, dd, dp(probs), n_probs, digit_bits, capacity, ctypes.byref(out))
        print(f"new({n_total}, {dd}, {probs.tolist()}, {n_probs}, {digit_bits}, {capacity}) -> {rc}: {E.last_error()}")
        assert rc == E.FG_E_BAD_ARG and not out.value


@pytest.mark.parametrize("capacity", [0, 8, 1000])
def test_a_replay_that_differs_by_one_element_is_reported(engines, capacity):
    """The second pass comes from a buffer in which the element at the median has left its bucket: FG_E_STATE at end_pass (a
    histogram total or a collect cursor one short), never a quantile; the stream stays failed."""
    eng, x, ptr = engines.upload("normal", Q.normal_input())
    y = x.copy()
    t, c = np.argwhere(x[:, 0, :] == Q.reference(x[:, 0, :], (0.5,))[0])[0]
    y[t, 0, c] = 1e300
    _, _, yptr = engines.upload("normal_one_replaced", y)
    with pytest.raises(Q.ReplayDiverged):
        Q.select(x[:, 0, :], Q.DEFAULT_PROBS, 12, capacity, replays=[y[:, 0, :]])
    with pytest.raises(E.EngineError) as err:
        stream_select(eng, ptr, x.shape, Q.DEFAULT_PROBS, 12, capacity, [[97]], replay_ptr=yptr)
    print(f"cap {capacity}: {err.value}")
    assert err.value.code == E.FG_E_STATE and "did not reproduce the previous one" in str(err.value)


def test_a_collect_cursor_past_the_capacity_writes_nothing_and_is_reported(engines):
    """The median's first bucket (sign and exponent of a value near 0) holds far fewer than 1 000 of the 6 790 elements, so pass 2
    collects it; the replay is the constant column of the median's value, so all 6 790 elements match and the cursor runs far past
    the 1 000 keys of the buffer: an error return, nothing written past the buffer."""
    eng, x, ptr = engines.upload("normal", Q.normal_input())
    y = x.copy()
    y[:, 0, :] = Q.reference(x[:, 0, :], (0.5,))[0]
    _, _, yptr = engines.upload("normal_flooded", y)
    with pytest.raises(E.EngineError) as err:
        stream_select(eng, ptr, x.shape, Q.DEFAULT_PROBS, 12, 1000, [[97]], replay_ptr=yptr)
    print(err.value)
    assert err.value.code == E.FG_E_STATE and "did not reproduce the previous one" in str(err.value)


# ---- 5. the drivers --------------------------------------------------------------------------------------------------------------
def _check_driver(label, summ, plain, chains):
    draws = np.ascontiguousarray(np.stack([chains.get_f64(a) for a in summ.sites], axis=1))         # [n][d][C]
    want = Q.reference_all(draws, I.QUANTILE_PROBS)
    for i, site in enumerate(summ.sites):
        for q, p in enumerate(summ.quantile_probs):
            print(f"{label} {site} p={p}: summary {summ.quantiles[i, q]!r} sort of the stored draws {want[i, q]!r}")
    print(f"{label}: passes {summ.passes}")
    for k in ("mean", "std", "r_hat", "ess"):
        print(f"{label} {k}: with quantiles {getattr(summ, k).tolist()} without {getattr(plain, k).tolist()}")
    assert summ.quantile_probs == I.QUANTILE_PROBS and summ.quantiles.shape == (len(summ.sites), 5)
    assert np.array_equal(Q.bits(summ.quantiles), Q.bits(want)) and (summ.quantiles == want).all()
    assert summ.passes >= 2
    assert plain.quantiles is None and plain.passes == 1
    for k in ("mean", "std", "r_hat", "ess"):
        assert np.array_equal(Q.bits(getattr(summ, k)), Q.bits(getattr(plain, k))), k


def test_hmc_chain_summary_with_quantiles():
    """Replaying the sampling phase into the same engine (state_import of the blob taken after warmup) reproduces the draws: the
    quantiles are the host sort's elements of hmc_chain's stored draws, everything else is what quantiles=False gives."""
    a = dict(seed=7, model_fn=W.normal_sites(4), n_samples=60, n_warmup=20, n_chains=128)
    chains = I.hmc_chain(**a)
    plain = I.hmc_chain_summary(chunk=16, **a)
    summ = I.hmc_chain_summary(chunk=16, quantiles=True, quantile_capacity=8, **a)
    print(f"hmc: accept_rate {summ.accept_rate!r} / {chains.accept_rate!r}, step size {summ.mean_step_size!r} / {chains.mean_step_size!r}, divergent {summ.n_divergent} / {chains.n_divergent}")
    _check_driver("hmc", summ, plain, chains)
    assert (summ.accept_rate, summ.mean_step_size, summ.n_divergent) == (chains.accept_rate, chains.mean_step_size, chains.n_divergent)


def test_adaptive_mcmc_chain_summary_with_quantiles():
    a = dict(seed=7, model_fn=W.reference_model(4), n_samples=60, n_warmup=20, n_chains=128)
    chains = I.adaptive_mcmc_chain(**a)
    plain = I.adaptive_mcmc_chain_summary(chunk=16, **a)
    summ = I.adaptive_mcmc_chain_summary(chunk=16, quantiles=True, quantile_capacity=8, **a)
    print(f"mh: accept_rate {summ.accept_rate!r} / {chains.accept_rate!r}")
    _check_driver("mh", summ, plain, chains)
    assert summ.accept_rate == chains.accept_rate and math.isnan(summ.mean_step_size) and summ.n_divergent == 0
