"""GPU tests of the discrete-site streams (fg_diag_cstream.hip): k_diag_cstream_count against the numpy restatement exactly and
under every chunking, at the block / wave / form boundaries, both forms against each other; k_diag_cells_f64 against the numpy
conversion bit for bit; adaptive_mcmc_chain_summary(discrete=True) against the stored draws of adaptive_mcmc_chain from the same
seed; the errors.

Synthetic cells are uploaded once with Engine.upload; a chunk is a slice [n_c][n_rec][C] of that buffer.  Integer sums are exact, so
tables are compared for equality.  Every compared figure is printed before it is asserted."""
import math

import numpy as np
import pytest

from fugue_amd import diagnostics as D
from fugue_amd import engine as E
from fugue_amd import inference as I
from fugue_amd import model as M
from fugue_amd import workloads as W
from tests import cstream_restatement as T
from tests import diag_reference as R
from tests import qstream_restatement as Q
from tests import reference_suite as S

pytestmark = pytest.mark.gpu

FIGURES = ("r_hat", "ess", "mean", "std")
ABS_TOL = dict(r_hat=0.0, ess=0.0, mean=1e-12, std=0.0)          # as tests/test_gpu_diag_stream.py and tests/test_gpu_result.py


class _Engines:
    """One engine per chain count for the whole module (the model does not matter to the diagnostics calls)."""

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


def _tables(res):
    return [dict(counts=res["counts"][k], below=int(res["below"][k]), above=int(res["above"][k]), min=res["min"][k], max=res["max"][k])
            for k in range(len(res["counts"]))]


def _stream(eng, ptr, shape, watch, chunks):
    """The tables of the uploaded cells at `ptr` ([n][n_rec][C]) fed in `chunks`."""
    n, n_rec, C = shape
    s = eng.diag_cstream(n, n_rec, watch["rows"], watch["vtypes"], watch["lo"], watch["bins"])
    try:
        at = 0
        for nc in chunks:
            s.update(ptr + at * n_rec * C * 8, nc)
            at += nc
            assert s.count == at
        return _tables(s.result())
    finally:
        s.close()


# ---- 1. state against the restatement ---------------------------------------------------------------------------------------------
def test_tables_equal_the_restatement_under_every_chunking(engines):
    cells, watch = T.mixed_input()
    want = T.tabulate(cells, **watch)
    T.show("restatement", want)
    eng = engines.get(cells.shape[2])
    ptr = eng.upload(cells)
    try:
        first = None
        for chunks in T.CHUNKINGS:
            got = _stream(eng, ptr, cells.shape, watch, chunks)
            T.show(f"device {len(chunks)} chunks", got)
            assert T.same_tables(got, want)
            first = first or got
            assert T.same_tables(got, first)
    finally:
        eng.device_free(ptr)


# ---- 2. edges -------------------------------------------------------------------------------------------------------------------
BINS = (1, 2, 8, 9, 64, 4096)


def _edge_cells(C, n=3):
    """[n][4][C]: an all-equal usize row (5), a u64 row uniform over [0, 4096), an i64 row entirely below 0, an i64 row entirely
    above 4096."""
    rng = np.random.default_rng(100 + C)
    cells = np.zeros((n, 4, C), dtype=np.int64)
    cells[:, 0, :] = 5
    cells[:, 1, :] = rng.integers(0, 4096, size=(n, C))
    cells[:, 2, :] = rng.integers(-7, 0, size=(n, C))
    cells[:, 3, :] = rng.integers(4096, 9000, size=(n, C))
    return cells


EDGE_VTYPES = [T.FG_USIZE, T.FG_U64, T.FG_I64, T.FG_I64]


@pytest.mark.parametrize("C", [1, 63, 64, 65, 257, 1025])
def test_edges_of_blocks_waves_and_forms(engines, C):
    """Every bin count at which the form or the flush changes, one and three watched rows, chunks of one draw and of two; the
    all-equal row (the greatest contention in either form), the row uniform over 4096 bins, rows entirely outside the range."""
    cells = _edge_cells(C)
    eng = engines.get(C)
    ptr = eng.upload(cells)
    try:
        for bins in BINS:
            lo_equal = 5 - min(bins - 1, 3)                       # the all-equal value falls into bin min(bins - 1, 3)
            for rows in ([0], [1], [2], [3], [3, 0, 1]):
                watch = dict(rows=rows, vtypes=[EDGE_VTYPES[r] for r in rows], lo=[lo_equal if r == 0 else 0 for r in rows], bins=[bins] * len(rows))
                want = T.tabulate(cells, **watch)
                got = _stream(eng, ptr, cells.shape, watch, [1, 2])
                print(f"C {C} bins {bins} rows {rows}: below {[t['below'] for t in got]} above {[t['above'] for t in got]} "
                      f"in range {[int(t['counts'].sum()) for t in got]} min {[t['min'] for t in got]} max {[t['max'] for t in got]} "
                      f"equal {T.same_tables(got, want)}")
                assert T.same_tables(got, want)
                for r, t in zip(rows, got):
                    if r == 0:
                        assert int(t["counts"][min(bins - 1, 3)]) == 3 * C and t["min"] == t["max"] == 5
                    if r == 2:
                        assert t["below"] == 3 * C
                    if r == 3:
                        assert t["above"] == 3 * C
                    if r == 1 and bins == 4096:
                        assert t["below"] == 0 and t["above"] == 0
    finally:
        eng.device_free(ptr)


def _many_trips_input(n=40, C=1025, n_watch=64):
    """[n][2 + n_watch][C]: two unwatched f64 rows, then watched rows in turn usize at K = 4, bool, i64 on both sides of [-5, 4), u64
    uniform over 4096 values (tabulated in 4096 bins, and once in 64)."""
    rng = np.random.default_rng(77)
    cells = np.zeros((n, 2 + n_watch, C), dtype=np.int64)
    cells[:, :2, :] = rng.standard_normal((n, 2, C)).view(np.int64)
    watch = dict(rows=[], vtypes=[], lo=[], bins=[])
    for i in range(n_watch):
        kind = i % 4
        size = (n, C)
        v, vt, lo, bins = ((rng.integers(0, 4, size=size), T.FG_USIZE, 0, 4), (rng.integers(0, 2, size=size), T.FG_BOOL, 0, 2),
                           (rng.integers(-20, 20, size=size), T.FG_I64, -5, 9), (rng.integers(0, 4096, size=size), T.FG_U64, 0, 64 if i == 3 else 4096))[kind]
        cells[:, 2 + i, :] = v
        for key, x in (("rows", 2 + i), ("vtypes", vt), ("lo", lo), ("bins", bins)):
            watch[key].append(x)
    return cells, watch


def test_several_trips_of_the_grid_stride_loop_in_both_forms(engines, monkeypatch):
    """64 watched rows of [40][66][1025] cells: the plan gives each row 32 blocks, so a thread takes 5 or 6 elements of the launch of
    40 draws (and 2 to 4 of the launches of 13 and 27) and the stride of 8 192 elements advances (draw, chain) by (7, 1017) with a
    wrap on most trips: the counters a wave carries across trips, the LDS histogram accumulated across trips and the division-free
    advance, in the default forms and with every row WIDE, equal to the restatement."""
    cells, watch = _many_trips_input()
    n, n_rec, C = cells.shape
    assert -(-2048 // len(watch["rows"])) * 256 * 5 < n * C                   # more than five trips' worth of elements per row
    want = T.tabulate(cells, **watch)
    eng = engines.get(C)
    ptr = eng.upload(cells)
    try:
        for form in (None, "wide"):
            if form:
                monkeypatch.setenv("FG_DIAG_CSTREAM_FORM", form)
            for chunks in ([40], [13, 27]):
                got = _stream(eng, ptr, cells.shape, watch, chunks)
                bad = [k for k in range(len(want)) if not T.same_tables([got[k]], [want[k]])]
                print(f"form {form or 'default'} chunks {chunks}: rows that differ {bad}; row 0 {got[0]['counts'].tolist()} / {want[0]['counts'].tolist()}; "
                      f"row 2 below {got[2]['below']} / {want[2]['below']} above {got[2]['above']} / {want[2]['above']}; "
                      f"row 7 in range {int(got[7]['counts'].sum())} / {int(want[7]['counts'].sum())} max {got[7]['max']} / {want[7]['max']}")
                assert not bad
                assert all(int(t["counts"].sum()) + t["below"] + t["above"] == n * C for t in got)
    finally:
        eng.device_free(ptr)


# ---- 3. the forms agree -----------------------------------------------------------------------------------------------------------
def test_narrow_and_wide_forms_give_identical_tables(engines, monkeypatch):
    """Rows of at most 8 bins under FG_DIAG_CSTREAM_FORM=wide (read at fg_diag_cstream_new) and under the default."""
    cells, watch = T.mixed_input()
    narrow_rows = [k for k, b in enumerate(watch["bins"]) if b <= 8]
    watch = {key: [v[k] for k in narrow_rows] for key, v in watch.items()}
    extra = _edge_cells(257)
    eng, eng2 = engines.get(cells.shape[2]), engines.get(257)
    ptr, ptr2 = eng.upload(cells), eng2.upload(extra)
    watch2 = dict(rows=[0, 1, 2], vtypes=EDGE_VTYPES[:3], lo=[2, 0, 0], bins=[8, 8, 2])
    try:
        default = _stream(eng, ptr, cells.shape, watch, [5, 31, 1, 60]), _stream(eng2, ptr2, extra.shape, watch2, [3])
        monkeypatch.setenv("FG_DIAG_CSTREAM_FORM", "wide")
        wide = _stream(eng, ptr, cells.shape, watch, [5, 31, 1, 60]), _stream(eng2, ptr2, extra.shape, watch2, [3])
        monkeypatch.setenv("FG_DIAG_CSTREAM_FORM", "narrow")
        narrow = _stream(eng, ptr, cells.shape, watch, [5, 31, 1, 60]), _stream(eng2, ptr2, extra.shape, watch2, [3])
    finally:
        eng.device_free(ptr)
        eng2.device_free(ptr2)
    for d, w, nr, cl, wt in zip(default, wide, narrow, (cells, extra), (watch, watch2)):
        T.show("default", d)
        T.show("wide", w)
        assert T.same_tables(d, w) and T.same_tables(d, nr) and T.same_tables(d, T.tabulate(cl, **wt))


# ---- 4. cells_f64 ---------------------------------------------------------------------------------------------------------------
def _gather_input(C):
    """[7][5][C]: an f64 row with a NaN payload, -0.0 and inf; a bool row; a u64 row with cells >= 2^63; an i64 row with -1 and the
    ends of the type; a usize row."""
    rng = np.random.default_rng(5)
    cells = np.zeros((7, 5, C), dtype=np.int64)
    f = rng.standard_normal((7, C))
    f[0, 0], f[1, C - 1], f[2, 0] = -0.0, np.inf, np.nan
    fb = f.view(np.int64).copy()
    fb[3, C // 2] = np.int64(0x7ff8dead0000beef)             # a NaN that carries a payload
    cells[:, 0, :] = fb
    cells[:, 1, :] = rng.integers(0, 2, size=(7, C))
    u = rng.integers(0, 2 ** 64, size=(7, C), dtype=np.uint64)
    u[0, 0], u[6, C - 1] = np.uint64(2 ** 63), np.uint64(2 ** 64 - 1)
    cells[:, 2, :] = u.view(np.int64)
    i = rng.integers(-2 ** 62, 2 ** 62, size=(7, C))
    i[0, 0], i[1, 0], i[2, 0] = -1, np.iinfo(np.int64).min, np.iinfo(np.int64).max
    cells[:, 3, :] = i
    cells[:, 4, :] = rng.integers(0, 64, size=(7, C))
    return cells, [T.FG_F64, T.FG_BOOL, T.FG_U64, T.FG_I64, T.FG_USIZE]


def _convert(cells, rows, vtypes):
    out = np.zeros((cells.shape[0], len(rows), cells.shape[2]))
    for k, r in enumerate(rows):
        c = np.ascontiguousarray(cells[:, r, :])
        out[:, k, :] = c.view(np.float64) if vtypes[r] == T.FG_F64 else c.view(np.uint64).astype(np.float64) if vtypes[r] == T.FG_U64 else c.astype(np.float64)
    return out


@pytest.mark.parametrize("C", [65, 64])
def test_cells_f64_equals_the_numpy_conversion_bit_for_bit(engines, C):
    """C = 65: the one-cell form; C = 64: the 16-byte form.  Rows in permuted order, a row taken twice, a subset; n = 0."""
    cells, vt = _gather_input(C)
    eng = engines.get(C)
    ptr = eng.upload(cells)
    guard = 64
    try:
        for rows in ([3, 0, 4, 2, 1], [2], [0, 0, 3], [4, 1]):
            want = _convert(cells, rows, vt)
            host = np.concatenate([np.full(guard, -1234.5), np.full(want.size, 777.0), np.full(guard, -1234.5)])
            out = eng.upload(host)
            try:
                eng.cells_f64(ptr, 7, 5, rows, [vt[r] for r in rows], out=out + guard * 8)
                eng.synchronize()
                back = eng.download(out, (host.size,))
            finally:
                eng.device_free(out)
            got = back[guard:-guard].reshape(want.shape)
            diff = int((got.view(np.int64) != want.view(np.int64)).sum())
            print(f"C {C} rows {rows}: {diff} of {want.size} values differ in bits; NaN {int(np.isnan(want).sum())}")
            assert np.array_equal(back[:guard], host[:guard]) and np.array_equal(back[-guard:], host[-guard:]), "guard words around d_out were written"
            assert diff == 0
        got = _convert(cells, [0, 2, 3], vt)
        print("payload NaN passes through:", hex(int(got[3, 0, C // 2].view(np.int64))), "2^63 ->", got[0, 1, 0], "-1 ->", got[0, 2, 0])
        assert got[0, 1, 0] == 2.0 ** 63 and got[0, 2, 0] == -1.0
        eng.cells_f64(ptr, 0, 5, [0, 1], [vt[0], vt[1]], out=ptr)            # n = 0: FG_OK, nothing is launched or written
        eng.synchronize()
        assert np.array_equal(eng.download(ptr, cells.shape, dtype=np.int64), cells)
        for bad in (dict(rows=[5], vtypes=[T.FG_I64]), dict(rows=[-1], vtypes=[T.FG_I64]), dict(rows=[0], vtypes=[7])):
            with pytest.raises(E.EngineError) as ei:
                eng.cells_f64(ptr, 7, 5, bad["rows"], bad["vtypes"], out=ptr)
            assert ei.value.code == E.FG_E_BAD_ARG
    finally:
        eng.device_free(ptr)


def test_cells_f64_with_more_selected_rows_than_one_launch_carries(engines):
    """250 selected rows (repeats allowed) of [3][5][C]: the selection travels 120 rows per launch, so three launches with their own
    offsets into the output."""
    for C in (65, 64):
        cells, vt = _gather_input(C)
        cells = cells[:3]
        rows = np.random.default_rng(9).integers(0, 5, size=250).tolist()
        want = _convert(cells, rows, vt)
        eng = engines.get(C)
        ptr = eng.upload(cells)
        out = eng.upload(np.full(want.size + 64, -1234.5))
        try:
            eng.cells_f64(ptr, 3, 5, rows, [vt[r] for r in rows], out=out)
            eng.synchronize()
            back = eng.download(out, (want.size + 64,))
        finally:
            eng.device_free(ptr)
            eng.device_free(out)
        got = back[:want.size].reshape(want.shape)
        per_row = (got.view(np.int64) != want.view(np.int64)).sum(axis=(0, 2))
        print(f"C {C}: {int(per_row.sum())} of {want.size} values differ in bits; output rows that differ {np.nonzero(per_row)[0].tolist()[:10]}")
        assert per_row.sum() == 0 and np.all(back[want.size:] == -1234.5)


def test_a_diagnostics_stream_over_gathered_rows_equals_one_over_the_same_doubles(engines):
    cells, _ = T.mixed_input()
    n, n_rec, C = cells.shape
    rows, vt = [4, 0, 3], [T.FG_U64, T.FG_F64, T.FG_I64]
    x = _convert(cells, rows, {4: T.FG_U64, 0: T.FG_F64, 3: T.FG_I64})
    eng = engines.get(C)
    ptr, direct = eng.upload(cells), eng.upload(x)
    gathered = eng.cells_f64(ptr, n, n_rec, rows, vt)
    figs = []
    try:
        for buf in (gathered, direct):
            s = eng.diag_stream(n, len(rows), 128)
            try:
                at = 0
                for nc in (5, 31, 1, 60):
                    s.update(buf + at * len(rows) * C * 8, nc)
                    at += nc
                figs.append(s.rhat_ess())
            finally:
                s.close()
    finally:
        for b in (ptr, direct, gathered):
            eng.device_free(b)
    for k in FIGURES:
        print(f"{k}: gathered {figs[0][k].tolist()} direct {figs[1][k].tolist()}")
        assert np.array_equal(Q.bits(figs[0][k]), Q.bits(figs[1][k])), k


# ---- 5. the driver against stored draws, same seed --------------------------------------------------------------------------------
RUN = dict(n_samples=96, n_warmup=40, n_chains=130)


def _same(got: float, want: float, rel: float, abs_: float = 0.0) -> bool:
    if math.isnan(want) or math.isinf(want):
        return (math.isnan(got) and math.isnan(want)) or got == want
    return math.isfinite(got) and abs(got - want) <= max(rel * abs(want), abs_)


def _assert_figures(label, summ, stored_draws):
    """summ: a ChainSummary; stored_draws [n][d][C] float64: streamed against stored, the comparison of tests/test_gpu_result.py."""
    stored = D.ChainDiagnostics(D.HostMoments(np.ascontiguousarray(stored_draws))).summary()
    for i, nm in enumerate(summ.sites):
        for k in FIGURES:
            print(f"{label} {nm} {k}: streamed {float(getattr(summ, k)[i])!r} stored {float(stored[k][i])!r}")
    for i, nm in enumerate(summ.sites):
        for k in FIGURES:
            assert _same(float(getattr(summ, k)[i]), float(stored[k][i]), R.FIGURE_TOL[k], ABS_TOL[k]), (label, nm, k)


def _assert_tables(label, disc, stored, n_cells):
    """disc: a DiscreteSummary; stored: a ChainBatch of the same run."""
    for k, nm in enumerate(disc.sites):
        v = stored.get_int(nm)
        lo, nb = disc.lo[k], len(disc.counts[k])
        inside = v[(v >= lo) & (v < lo + nb)] - lo
        want = np.bincount(inside.reshape(-1), minlength=nb)
        print(f"{label} {nm}: counts {disc.counts[k].tolist()} bincount {want.tolist()} below {int(disc.below[k])} above {int(disc.above[k])} "
              f"min {disc.min[k]} / {int(v.min())} max {disc.max[k]} / {int(v.max())}")
        assert np.array_equal(disc.counts[k].astype(np.int64), want)
        assert int(disc.below[k]) == int((v < lo).sum()) and int(disc.above[k]) == int((v >= lo + nb).sum())
        assert disc.min[k] == int(v.min()) and disc.max[k] == int(v.max())
        assert int(disc.counts[k].sum()) + int(disc.below[k]) + int(disc.above[k]) == n_cells


def test_categorical_site_against_stored_draws(monkeypatch):
    monkeypatch.setenv("FG_JIT", "0")
    P, _ = S.categorical_k(8)
    stored = I.adaptive_mcmc_chain(5, P, **RUN)
    summ = I.adaptive_mcmc_chain_summary(5, P, chunk=25, max_lag=96, discrete=True, **RUN)
    disc = summ.discrete
    assert summ.sites == [] and disc.sites == ["z"] and disc.vtypes == [T.FG_USIZE] and disc.lo == [0] and len(disc.counts[0]) == 8 and disc.numeric is None
    _assert_tables("categorical_k(8)", disc, stored, 96 * 130)
    assert int(disc.below[0]) == 0 and int(disc.above[0]) == 0                  # the bins cover the support
    print("probs", disc.probs()[0].tolist())
    assert abs(disc.probs()[0].sum() - 1.0) < 1e-12


def test_poisson_site_against_stored_draws(monkeypatch):
    monkeypatch.setenv("FG_JIT", "0")
    stored = I.adaptive_mcmc_chain(6, S.poisson1(), **RUN)
    summ = I.adaptive_mcmc_chain_summary(6, S.poisson1(), chunk=25, max_lag=96, discrete=True, **RUN)
    disc = summ.discrete
    assert disc.sites == ["k"] and disc.vtypes == [T.FG_U64] and disc.lo == [0] and len(disc.counts[0]) == 64
    _assert_tables("poisson1", disc, stored, 96 * 130)
    assert int(disc.below[0]) == 0 and int(disc.above[0]) == 0
    k = stored.get_int("k")
    _assert_figures("poisson1 numeric", disc.numeric, k.astype(np.float64)[:, None, :])
    assert disc.numeric.sites == ["k"]
    two = I.adaptive_mcmc_chain_summary(6, S.poisson1(), chunk=25, max_lag=96, discrete=True, discrete_bins={"k": (0, 2)}, **RUN).discrete
    print(f"bins (0, 2): counts {two.counts[0].tolist()} above {int(two.above[0])} stored >= 2: {int((k >= 2).sum())}")
    _assert_tables("poisson1 (0, 2)", two, stored, 96 * 130)
    assert len(two.counts[0]) == 2 and int(two.above[0]) == int((k >= 2).sum()) and two.max[0] == int(k.max())


def _mixture3():
    """workloads.mixture(data, K=3) over 6 points, returning select(z#0, mus) and the indicator of z#1 == 2."""
    data = [-4.1, -3.7, 0.2, 0.4, 3.9, 4.3]
    P = M.Program()
    mus = [P.sample(M.addr("mu", k), M.Normal(0.0, 5.0)) for k in range(3)]
    zs = []
    for i, xi in enumerate(data):
        z = P.sample(M.addr("z", i), M.Categorical([1.0 / 3] * 3))
        P.observe(M.addr("x", i), M.Normal(M.select(z, mus), 1.0), float(xi))
        zs.append(z)
    P.result = {"mu_of_z0": M.select(zs[0], mus), "z1_is_2": M.select(zs[1], [0.0, 0.0, 1.0])}
    return P


def test_mixture_against_stored_draws_with_results_and_quantiles(monkeypatch):
    monkeypatch.setenv("FG_JIT", "0")
    cp = E.compile_model(_mixture3())
    assert cp.R == 2
    stored = I.adaptive_mcmc_chain(7, cp, **RUN)
    plain = I.adaptive_mcmc_chain_summary(7, cp, chunk=25, max_lag=96, quantiles=True, **RUN)
    summ = I.adaptive_mcmc_chain_summary(7, cp, chunk=25, max_lag=96, quantiles=True, results=True, discrete=True, **RUN)
    disc = summ.discrete
    assert plain.discrete is None and disc.sites == [f"z#{i}" for i in range(6)] and disc.numeric is None
    _assert_tables("mixture", disc, stored, 96 * 130)
    assert not disc.below.any() and not disc.above.any() and all(len(c) == 3 for c in disc.counts)
    for k in ("mean", "std", "r_hat", "ess", "quantiles"):
        print(f"f64 sites {k}: discrete=True {getattr(summ, k).tolist()} discrete=False {getattr(plain, k).tolist()}")
        assert np.array_equal(Q.bits(getattr(summ, k)), Q.bits(getattr(plain, k))), k
    assert summ.sites == plain.sites and (summ.accept_rate, summ.passes) == (plain.accept_rate, plain.passes)
    # the two results read discrete sites: figures against the stored ChainBatch.results, quantiles the exact order statistics
    rs = summ.results
    assert rs.sites == stored.result_names == ["result.mu_of_z0", "result.z1_is_2"]
    ind = (stored.get_int("z#1") == 2).astype(np.float64)
    assert np.array_equal(stored.get_result("result.z1_is_2"), ind)
    _assert_figures("mixture results", rs, stored.results)
    want_q = Q.reference_all(np.ascontiguousarray(stored.results), I.QUANTILE_PROBS)
    print(f"result quantiles: summary {rs.quantiles.tolist()} sort of the stored results {want_q.tolist()}")
    assert np.array_equal(Q.bits(rs.quantiles), Q.bits(want_q))
    # without discrete=True the refusal stands
    with pytest.raises(ValueError):
        I.adaptive_mcmc_chain_summary(7, cp, chunk=25, max_lag=96, results=True, **RUN)


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------
def test_refused_arguments_and_call_order(engines):
    cells, watch = T.mixed_input(n=6, C=64)
    eng = engines.get(64)
    ptr = eng.upload(cells)
    try:
        with pytest.raises(E.EngineError) as ei:
            eng.diag_cstream(6, 5, [0, 1], [T.FG_F64, T.FG_BOOL], [0, 0], [2, 2])
        print("a watched f64 row:", ei.value)
        assert ei.value.code == E.FG_E_BAD_ARG
        with pytest.raises(E.EngineError) as ei:
            eng.diag_cstream(6, 5, [1, 2, 1], [T.FG_BOOL, T.FG_USIZE, T.FG_BOOL], [0, 0, 0], [2, 4, 2])
        print("a duplicate row:", ei.value)
        assert ei.value.code == E.FG_E_BAD_ARG
        s = eng.diag_cstream(6, 5, watch["rows"], watch["vtypes"], watch["lo"], watch["bins"])
        try:
            s.update(ptr, 4)
            with pytest.raises(E.EngineError) as ei:
                s.result()
            print("result() early:", ei.value)
            assert ei.value.code == E.FG_E_STATE
            with pytest.raises(E.EngineError) as ei:
                s.update(ptr + 4 * 5 * 64 * 8, 3)
            print("update past n_total:", ei.value)
            assert ei.value.code == E.FG_E_STATE and s.count == 4
            s.update(ptr + 4 * 5 * 64 * 8, 2)
            assert T.same_tables(_tables(s.result()), T.tabulate(cells, **watch))
        finally:
            s.close()
    finally:
        eng.device_free(ptr)
