"""A numpy restatement of the chunked diagnostics state (fugue_amd/csrc/fg_diag_stream.hip), one IEEE operation at a time: numpy's
elementwise add / subtract / multiply / divide round once each, and the loops below run over the draw index, so every column sees
exactly the sequence of operations a kernel thread performs.  Not a test, and nothing here calls the engine.

State per column, over y_t = x_t - pivot with pivot = x_0: the in-order sums S1, S2 of the full chain and of the two halves, the
in-order lag products P_t = sum_i y_i y_{i + t} (t < K), head (the first K values of y) and ring (the last K, slot u mod K).
`update` takes chunks of any length; the state after the last one does not depend on how the draws were cut."""
import numpy as np


class StreamRestatement:
    def __init__(self, n_total: int, d: int, C: int, max_lag: int):
        assert n_total >= 1 and 1 <= max_lag <= 2048
        self.n, self.d, self.C = int(n_total), int(d), int(C)
        self.K = (int(max_lag) + 31) // 32 * 32
        self.count = 0
        z = lambda *shape: np.zeros(shape + (d, C))
        self.pivot = z()
        self.s1, self.s2 = z(3), z(3)                     # full chain, first half, second half
        self.P, self.head, self.ring = z(self.K), z(self.K), z(self.K)
        self._y = []                                       # only to form the lagged products; the kernel reads ring and chunk

    def update(self, chunk: np.ndarray):
        chunk = np.asarray(chunk, dtype=np.float64)
        assert chunk.shape[1:] == (self.d, self.C) and self.count + len(chunk) <= self.n
        half = self.n // 2
        with np.errstate(invalid="ignore", over="ignore"):
            for x in chunk:
                u = self.count
                if u == 0:
                    self.pivot = x.copy()
                y = x - self.pivot
                self._y.append(y)
                for t in range(min(u + 1, self.K)):        # P_t gains y_{u - t} y_u: ascending u is ascending i = u - t
                    self.P[t] = self.P[t] + self._y[u - t] * y
                yy = y * y
                segs = [0] + ([1] if u < half else [2] if u < 2 * half else [])
                for k in segs:
                    self.s1[k] = self.s1[k] + y
                    self.s2[k] = self.s2[k] + yy
                if u < self.K:
                    self.head[u] = y
                self.ring[u % self.K] = y
                self.count += 1

    def moments(self) -> np.ndarray:
        """[d][6][C]: mu = S1 / n_seg, mean = pivot + mu, ssd = S2 - S1 mu (n_seg = 0: mean NaN, ssd 0, as k_diag_moments)."""
        assert self.count == self.n
        out = np.zeros((self.d, 6, self.C))
        with np.errstate(invalid="ignore", over="ignore"):
            for k, nseg in enumerate((self.n, self.n // 2, self.n // 2)):
                if nseg == 0:
                    out[:, 2 * k], out[:, 2 * k + 1] = np.nan, 0.0
                    continue
                mu = self.s1[k] / float(nseg)
                out[:, 2 * k] = self.pivot + mu
                out[:, 2 * k + 1] = self.s2[k] - self.s1[k] * mu
        return out

    def resid(self) -> np.ndarray:
        """[d][C]: n (pivot + S1 / n - mean), the row the pooled std's cross term wants (two-sum of pivot + mu, then the
        division's remainder; the kernel forms the latter with one fused multiply-add, so this row is close, not bit-equal)."""
        n = float(self.n)
        mu = self.s1[0] / n
        mean = self.pivot + mu
        bb = mean - self.pivot
        err = (self.pivot - (mean - bb)) + (mu - bb)
        return n * err + (self.s1[0] - n * mu)

    def chain_autocov(self, lag: int) -> np.ndarray:
        """[d][C]: (P_t - mu (2 S1 - head_sum_t - tail_sum_t) + (n - t) mu^2) / n, head_sum_t / tail_sum_t the sums of the first /
        last t values of y added from the ends inwards; 0 for lag >= n."""
        assert self.count == self.n
        n, K = self.n, self.K
        if lag >= n:
            return np.zeros((self.d, self.C))
        assert lag < K, "the stream does not keep this lag"
        hs, ts = np.zeros((self.d, self.C)), np.zeros((self.d, self.C))
        with np.errstate(invalid="ignore", over="ignore"):
            for t in range(1, lag + 1):
                hs = hs + self.head[t - 1]
                ts = ts + self.ring[(n - t) % K]
            s1, nf = self.s1[0], float(n)
            mu = s1 / nf
            cross = mu * ((2.0 * s1 - hs) - ts)
            return ((self.P[lag] - cross) + (float(n - lag) * mu) * mu) / nf

    def autocov_sums(self, lag0: int, n_lags: int) -> np.ndarray:
        """[d][n_lags]: the per-column values summed over chains (numpy's order: a restatement of the value, not of the tree)."""
        return np.stack([self.chain_autocov(lag0 + k).sum(axis=1) for k in range(n_lags)], axis=1)


class RestatementMoments:
    """MomentProvider (fugue_amd.diagnostics) over a finished StreamRestatement."""

    def __init__(self, st: StreamRestatement):
        self.st, self.n, self.d = st, st.n, st.d

    def moments(self) -> np.ndarray:
        return self.st.moments()

    def autocov_sums(self, lag0: int, n_lags: int) -> np.ndarray:
        return self.st.autocov_sums(lag0, n_lags)


def restate(x: np.ndarray, max_lag: int, chunks=None) -> StreamRestatement:
    """The state after all of x [n][d][C], cut into `chunks` (lengths; default: one chunk)."""
    x = np.asarray(x, dtype=np.float64)
    st = StreamRestatement(x.shape[0], x.shape[1], x.shape[2], max_lag)
    at = 0
    for n in (chunks or [len(x)]):
        st.update(x[at:at + n])
        at += n
    assert at == len(x)
    return st


# ---- seeded inputs shared by tests/test_diag_stream_cpu.py and tests/test_gpu_diag_stream.py -------------------------------
def ar1_input(seed: int, n: int, C: int, d: int, phi: float) -> np.ndarray:
    """[n][d][C]: d independent AR(1) columns from numpy.random.default_rng(seed)."""
    from tests.diag_helpers import ar1
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack([ar1(rng, n, C, phi) for _ in range(d)], axis=1))


def oracle_figures(oracle, x: np.ndarray) -> list:
    """Per column of x [n][d][C]: the oracle's split R-hat, multi-chain ESS, pooled mean and std."""
    rows = []
    for i in range(x.shape[1]):
        ch = np.ascontiguousarray(x[:, i, :].T)
        s = oracle.summarize(ch)
        rows.append(dict(r_hat=oracle.split_rhat(ch), ess=oracle.ess_multichain(ch), mean=s["mean"], std=s["std"]))
    return rows
