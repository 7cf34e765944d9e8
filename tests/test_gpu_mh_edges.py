"""Every MH kernel family against the oracle on the edge cases of tests/mh_edge_cases.py, step by step and with no chain allowed to part
ways (tests/test_mh_edges_cpu.py asserts, for these seeds, models and starts, that no accept decision of the oracle's run is closer than
1e-6 to its uniform): the LogSpace walk at and beyond the ends of its domain, reflections with many bounces, from outside the bounds and
with an empty range, kinds decided on a first visit at <= 0, the u64 walk at 0 and 1, log-weights of -inf and NaN cells in the accept
rule, and DiminishingAdaptation's gate and clamps step by step."""
import numpy as np
import pytest

from fugue_amd import engine as E
from tests import mh_edge_cases as K

pytestmark = pytest.mark.gpu

T = K.NW + K.NS
SWITCHES = ("FG_JIT", "FG_MH_MW", "FG_MH_PIPE", "FG_MH_SPLIT", "FG_HMC_WAVES", "FG_HMC_INTERP_MW", "FG_MH_INTERP_WAVES", "FG_MH_INTERP_OCC", "FG_MH_NOSTREAM_MW")

# (the kernel mh_last_kernel must name, the switches that select it); two wave counts where the family has them
FAMILIES = {
    "A": [("k_mh_steps W=1", dict(FG_JIT=0, FG_MH_MW=0)),
          ("k_mh_mw2_steps W=2", dict(FG_JIT=0, FG_MH_MW=1, FG_MH_PIPE=1, FG_MH_SPLIT=0, FG_HMC_WAVES=2)),
          ("k_mh_mw2_steps W=16", dict(FG_JIT=0, FG_MH_MW=1, FG_MH_PIPE=1, FG_MH_SPLIT=1, FG_HMC_WAVES=16)),
          ("k_mh_mw_steps W=2", dict(FG_JIT=0, FG_MH_MW=1, FG_MH_PIPE=0, FG_MH_SPLIT=0, FG_HMC_WAVES=2)),
          ("k_mh_mw_steps W=16", dict(FG_JIT=0, FG_MH_MW=1, FG_MH_PIPE=0, FG_MH_SPLIT=1, FG_HMC_WAVES=16)),
          ("k_mh_mw2_jit_steps W=2", dict(FG_JIT=1, FG_MH_MW=1, FG_MH_PIPE=1, FG_MH_SPLIT=0, FG_HMC_WAVES=2)),
          ("k_mh_mw2_jit_steps W=16", dict(FG_JIT=1, FG_MH_MW=1, FG_MH_PIPE=1, FG_MH_SPLIT=1, FG_HMC_WAVES=16)),
          ("k_mh_mw_jit_steps W=2", dict(FG_JIT=1, FG_MH_MW=1, FG_MH_PIPE=0, FG_MH_SPLIT=0, FG_HMC_WAVES=2)),
          ("k_mh_mw_jit_steps W=16", dict(FG_JIT=1, FG_MH_MW=1, FG_MH_PIPE=0, FG_MH_SPLIT=1, FG_HMC_WAVES=16))],
    "B": [("k_mh_steps W=1", dict(FG_JIT=0, FG_HMC_INTERP_MW=0)),
          ("k_mh_interp_mw_steps W=2", dict(FG_JIT=0, FG_HMC_INTERP_MW=1, FG_MH_INTERP_WAVES=2)),
          ("k_mh_interp_mw_steps W=", dict(FG_JIT=0, FG_HMC_INTERP_MW=1, FG_MH_INTERP_WAVES=16)),       # (as many of the 16 as the program's statements allow)
          ("k_mh_jit_steps W=2", dict(FG_JIT=1, FG_HMC_INTERP_MW=1, FG_MH_NOSTREAM_MW=0, FG_MH_INTERP_WAVES=2, FG_MH_INTERP_OCC=2)),
          ("k_mh_jit_steps W=8", dict(FG_JIT=1, FG_HMC_INTERP_MW=1, FG_MH_NOSTREAM_MW=0, FG_MH_INTERP_WAVES=8, FG_MH_INTERP_OCC=2)),
          ("k_mh_mw_jit_steps W=2 (a program without a record stream", dict(FG_JIT=1, FG_HMC_INTERP_MW=1, FG_MH_SPLIT=0, FG_HMC_WAVES=2)),
          ("k_mh_mw_jit_steps W=16 (a program without a record stream", dict(FG_JIT=1, FG_HMC_INTERP_MW=1, FG_MH_SPLIT=1, FG_HMC_WAVES=16))],
}


def _switch(monkeypatch, env):
    for k in SWITCHES: monkeypatch.delenv(k, raising=False)
    for k, v in env.items(): monkeypatch.setenv(k, str(v))


def _f(cells):
    return np.ascontiguousarray(cells, dtype=np.int64).view(np.float64)


_EXACT = [K.f64_cell(x) for x in (K.MIN_POSITIVE, K.F64_MAX, 0.0, -0.0)]


def _f64_cells_agree(g_cells, o_cells):
    """Bit-equal where both are non-finite or the oracle's value is exactly MIN_POSITIVE, f64::MAX or +-0; |g - o| <= 1e-9 |o| elsewhere
    (no absolute floor: it would hide everything near 1e-308)."""
    g, o = _f(g_cells), _f(o_cells)
    exact = (~np.isfinite(g) & ~np.isfinite(o)) | np.isin(o_cells, _EXACT)
    with np.errstate(invalid="ignore", over="ignore"):
        close = np.abs(g - o) <= 1e-9 * np.abs(o)
    return np.where(exact, np.asarray(g_cells) == np.asarray(o_cells), close)


def _weights_agree(g, o, rtol):
    fin = np.isfinite(o)
    with np.errstate(invalid="ignore"):
        close = np.abs(g - o) <= rtol * np.abs(o)
    return np.where(fin, close, (np.isnan(g) & np.isnan(o)) | (g == o))


@pytest.fixture(scope="module")
def oracle_runs(oracle):
    out = {}
    for which, make in K.MODELS.items():
        prog = make()
        om = oracle.OracleModel(prog)
        start = K.start_cells(om, K.SEEDS[which])
        ov = K.overrides(om.site_names)
        with np.errstate(invalid="ignore"):
            lw_start = np.array([np.sum(om.run_score(start[:, c])[0]) for c in range(K.C)])       # what set_values has to re-score
        out[which] = (prog, start, ov, lw_start, om.mh_run_from(K.SEEDS[which], K.C, K.NW, K.NS, start=start, overrides=ov, chain0=K.CHAIN0, n_threads=8))
    return out


@pytest.mark.parametrize("which", ["A", "B"])
def test_mh_edge_states_match_the_oracle(oracle_runs, which, monkeypatch):
    prog, start, ov, lw_start, o = oracle_runs[which]
    cp = E.compile_model(prog)
    assert (E.PROP_LOGSPACE, E.PROP_REFLECT) == (K.PROP_LOGSPACE, K.PROP_REFLECT) and list(cp.site_names) == sorted("bcegknruvw" if which == "A" else "bcdegknruvw")
    assert (cp.stream_records[1] > 0) == (which == "A")                       # A has a score stream, B's expression parameter leaves it none
    rec = list(range(cp.S))
    row = cp.S * K.C * 8
    results = []
    for want, env in FAMILIES[which]:
        _switch(monkeypatch, env)
        eng = E.Engine(cp, K.C, seed=K.SEEDS[which], chain_offset=K.CHAIN0)
        eng.mh_init(K.NW, ov)
        eng.mh_set_recording(True)
        eng.set_values(start)
        lw0 = eng.mh_log_weight()
        d = eng.device_alloc(T * row)
        eng.mh_step(K.NW, rec, d)
        scales_warm = eng.mh_scales()
        eng.mh_step(K.NS, rec, d + K.NW * row)
        kernel = eng.mh_last_kernel()
        draws = eng.download(d, (T, cp.S, K.C), dtype=np.int64)
        eng.device_free(d)
        st = eng.mh_stats()
        res = (draws, eng.get_values(), eng.mh_scales(), eng.mh_log_weight(), round(st.accept_rate * st.n_steps))
        eng.close()
        assert kernel.startswith(want), (want, kernel)
        results.append((kernel, res))

        # ---- against the oracle, step by step
        parted = np.zeros(K.C, dtype=bool)
        first_bad = {}
        for j in range(cp.S):
            ok = _f64_cells_agree(draws[:, j, :], o["draws"][:, j, :]) if cp.site_vtypes[j] == 0 else draws[:, j, :] == o["draws"][:, j, :]
            for c in np.nonzero(~ok.all(axis=0))[0]:
                t = int((~ok[:, c]).argmax())
                if c not in first_bad or t < first_bad[c][0]:
                    first_bad[int(c)] = (t, cp.site_names[j], K.case_of_chain(int(c)), int(draws[t, j, c]), int(o["draws"][t, j, c]), float(o["log_alpha"][t, c]))
            parted |= ~ok.all(axis=0)
        print(f"[mh edges] model {which} {kernel}: {int(parted.sum())} parted chains", dict(list(first_bad.items())[:6]))
        assert not parted.any(), (kernel, dict(list(first_bad.items())[:6]))
        assert np.array_equal(res[1], draws[-1])
        sc_bad = ~np.isclose(res[2], o["scales"], rtol=1e-10, atol=0.0)
        assert not sc_bad.any(), (kernel, np.argwhere(sc_bad)[:5], res[2][sc_bad][:5], o["scales"][sc_bad][:5])
        # the log-weight set_values scored (-inf in the chains whose injected state has no density), and the one the chain ends with
        lw0_bad = ~_weights_agree(lw0, lw_start, 1e-9)
        assert not lw0_bad.any() and np.isneginf(lw_start).sum() >= 20, (kernel, np.nonzero(lw0_bad)[0][:5], lw0[lw0_bad][:5], lw_start[lw0_bad][:5])
        lw_bad = ~_weights_agree(res[3], o["log_weight"], 1e-9)
        assert not lw_bad.any(), (kernel, np.nonzero(lw_bad)[0][:5], res[3][lw_bad][:5], o["log_weight"][lw_bad][:5])
        assert res[4] == int(o["accept"].sum()), (kernel, res[4], int(o["accept"].sum()))
        # test_mh_frozen_steps_leave_the_adaptation_alone: after warmup the scales stay (mh.rs:989-1001); the decided kinds show in the draws
        assert np.array_equal(scales_warm, res[2]), kernel
    # ---- the families against each other, bit for bit
    for kernel, res in results[1:]:
        for a, b in zip(results[0][1], res):
            assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), kernel


ADAPT_KERNELS = [("k_mh_steps W=1", dict(FG_JIT=0, FG_MH_MW=0, FG_HMC_INTERP_MW=0)),
                 ("k_mh_mw_steps W=2", dict(FG_JIT=0, FG_MH_MW=1, FG_MH_PIPE=0, FG_MH_SPLIT=0, FG_HMC_WAVES=2))]


@pytest.mark.parametrize("name", sorted(K.ADAPT))
def test_mh_adaptation_gate_and_clamps(oracle, name, monkeypatch):
    """DiminishingAdaptation::update (mcmc_utils.rs:88-150) watched after every step: nothing moves before a site's 10th proposal, then
    the oracle's scale step by step, up to the clamp at 100 (every move accepted) or down to the clamp at 0.001 (none accepted)."""
    make, x0, steps, clamp = K.ADAPT[name]
    prog = make()
    om = oracle.OracleModel(prog)
    start = K.adapt_start(x0)
    o = om.mh_run_from(K.ADAPT_SEED, K.ADAPT_C, steps, 0, start=start, chain0=K.ADAPT_CHAIN0)
    assert (o["scale"][-1] == clamp).all()
    cp = E.compile_model(prog)
    for want, env in ADAPT_KERNELS:
        _switch(monkeypatch, env)
        eng = E.Engine(cp, K.ADAPT_C, seed=K.ADAPT_SEED, chain_offset=K.ADAPT_CHAIN0)
        eng.mh_init(steps)
        if start is not None: eng.set_values(start)
        for t in range(steps):
            eng.mh_step(1)
            g, want_sc = eng.mh_scales()[0], o["scale"][t]
            assert np.allclose(g, want_sc, rtol=1e-12, atol=0.0), (want, t, np.abs(g / want_sc - 1).max())
            if t < 9: assert (g == 1.0).all(), (want, t)                      # total_count < 10: mcmc_utils.rs:112-114
            at_clamp = want_sc == clamp
            assert (g[at_clamp] == clamp).all(), (want, t)
        assert eng.mh_last_kernel().startswith(want), (want, eng.mh_last_kernel())
        st = eng.mh_stats()
        assert round(st.accept_rate * st.n_steps) == int(o["accept"].sum())
        eng.close()
