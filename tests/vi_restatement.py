"""Plain-Python restatement of the reference's mean-field VI (src/inference/vi.rs:104-923) from what the CPU oracle exports --
`orc.stream`, `orc.sample_dist`, `orc.logpdf` for the guide, `OracleModel.run_score` for the model -- plus the engine's two
summation orders in numpy, the common-random-numbers finite-difference pair and the optimizer loop.  A helper, not a test:
tests/test_vi_cpu.py and tests/test_gpu_vi.py check fugue_amd.vi / fg_vi.hip against it.

A guide is a row of factors (family, site, a, b) in address-sorted order: family 0 Normal {mu, log_sigma}, 1 LogNormal
{mu, log_sigma}, 2 Beta {log_alpha, log_beta}; site = sorted site index of the model, or -1 for an address the model never visits."""
import math

import numpy as np

FG_RNG_VI = 8
FAMILY = ("Normal", "LogNormal", "Beta")
LOG_SCALE_MIN, LOG_SCALE_MAX, MU_ABS_MAX = -20.0, 20.0, 1.0e6


def dist_params(family, a, b):
    """VariationalParam -> distribution parameters (vi.rs:294-323)."""
    return [math.exp(a), math.exp(b)] if family == 2 else [a, math.exp(b)]


def sample_terms(orc, om, row, seed, n_samples, stream_id, sample0=0):
    """elbo_with_guide's per-sample quantity (vi.rs:647-666): -> (terms [N], draws [N][n_factors]).  Sample n draws the factors in
    row order from stream (seed, sample0 + n, stream_id, FG_RNG_VI); a factor with site -1 is drawn and adds nothing to log q."""
    terms, draws = np.zeros(n_samples), np.zeros((n_samples, len(row)))
    params = [dist_params(f, a, b) for f, _, a, b in row]
    for n in range(n_samples):
        s = orc.stream(seed, sample0 + n, stream_id, FG_RNG_VI)
        cells = np.zeros(max(1, om.S), dtype=np.int64)
        log_q = 0.0
        for k, (fam, site, _, _) in enumerate(row):
            x = orc.sample_dist(FAMILY[fam], params[k], s)
            lq = orc.logpdf(FAMILY[fam], x, params[k])
            draws[n, k] = x
            if site >= 0:
                log_q += lq
                cells[site:site + 1].view(np.float64)[0] = x
        acc, _ = om.run_score(cells[:om.S])
        terms[n] = ((acc[0] + acc[1]) + acc[2]) - log_q
    return terms, draws


def wave_sums(terms):
    """The wave order: 64 consecutive terms (the tail padded with +0.0), v[i] = v[i] + v[i + s] for s = 32, 16, .., 1."""
    t = np.asarray(terms, dtype=np.float64)
    nb = (t.size + 63) // 64
    v = np.zeros(nb * 64)
    v[:t.size] = t
    v = v.reshape(nb, 64)
    with np.errstate(invalid="ignore"):
        for s in (32, 16, 8, 4, 2, 1):
            v = v[:, :s] + v[:, s:2 * s]
    return v[:, 0]


def block_sum(partial):
    """The block order: 256 accumulators from +0.0, accumulator t adds partial[t], partial[t + 256], ...; then a[t] = a[t] + a[t + s]
    for s = 128, 64, .., 1."""
    p = np.asarray(partial, dtype=np.float64)
    rows = (p.size + 255) // 256
    q = np.zeros(max(1, rows) * 256)
    q[:p.size] = p
    a = np.zeros(256)
    with np.errstate(invalid="ignore"):
        for r in q.reshape(-1, 256):
            a = a + r
        for s in (128, 64, 32, 16, 8, 4, 2, 1):
            a = a[:s] + a[s:2 * s]
    return a[0]


def elbo_of_terms(terms):
    """The engine's ELBO of one evaluation's terms: both orders, then / N."""
    return block_sum(wave_sums(terms)) / float(len(terms))


def elbo(orc, om, row, seed, n_samples, stream_id):
    return elbo_of_terms(sample_terms(orc, om, row, seed, n_samples, stream_id)[0])


def shifted(row, k, coord, delta):
    out = list(row)
    f, s, a, b = out[k]
    out[k] = (f, s, a + delta, b) if coord == 0 else (f, s, a, b + delta)
    return out


def gradient_fd(orc, om, row, k, coord, eps, seed, n_samples, stream_id):
    """elbo_gradient_fd (vi.rs:687-725): both signs from ONE stream id."""
    ep = elbo(orc, om, shifted(row, k, coord, eps), seed, n_samples, stream_id)
    em = elbo(orc, om, shifted(row, k, coord, -eps), seed, n_samples, stream_id)
    with np.errstate(invalid="ignore"):
        return (ep - em) / (2.0 * eps)


def apply_update(fac, coord, delta):
    f, s, a, b = fac
    if coord == 0:
        lo, hi = (LOG_SCALE_MIN, LOG_SCALE_MAX) if f == 2 else (-MU_ABS_MAX, MU_ABS_MAX)
        return (f, s, min(max(a + delta, lo), hi), b)
    return (f, s, a, min(max(b + delta, LOG_SCALE_MIN), LOG_SCALE_MAX))


def plateau_statistic(history, w):
    """|recent - previous| / max(|previous|, 1e-8) over the two latest windows (vi.rs:809-817), or None before 2 w estimates."""
    n = len(history)
    if w <= 0 or n < 2 * w:
        return None
    recent = previous = 0.0
    for x in history[n - w:]:
        recent += x
    for x in history[n - 2 * w:n - w]:
        previous += x
    recent, previous = recent / w, previous / w
    with np.errstate(invalid="ignore"):
        return abs(recent - previous) / max(abs(previous), 1e-8)


def optimize(orc, om, row, seed, n_samples, n_iterations=1000, base_learning_rate=0.1, fd_eps=0.01, convergence_tol=1e-4,
             convergence_window=20, step_decay_exponent=0.6):
    """optimize_meanfield_vi_with_config (vi.rs:784-864) with the engine's stream ids: iteration t draws the monitor from
    t (2P + 1) and both signs of coordinate j = 2 factor + coord from t (2P + 1) + 1 + j.  -> (row, history, converged, iterations,
    dict(plateau = the plateau statistics, max_grad = the largest finite |gradient|))."""
    row, P = list(row), len(row)
    history, stats, converged, iterations, max_grad = [], [], False, 0, 0.0
    for t in range(n_iterations):
        iterations = t + 1
        s0 = t * (2 * P + 1)
        history.append(elbo(orc, om, row, seed, n_samples, s0))
        st = plateau_statistic(history, convergence_window)
        if st is not None:
            stats.append(st)
            if st < convergence_tol:
                converged = True
                break
        step = base_learning_rate * math.pow(float(t + 1), -step_decay_exponent)
        snapshot = list(row)
        for j in range(2 * P):
            grad = gradient_fd(orc, om, snapshot, j // 2, j & 1, fd_eps, seed, n_samples, s0 + 1 + j)
            if math.isfinite(grad):
                max_grad = max(max_grad, abs(grad))
            if math.isfinite(grad) and math.isfinite(step * grad):
                row[j // 2] = apply_update(row[j // 2], j & 1, step * grad)
    return row, np.array(history), converged, iterations, dict(plateau=stats, max_grad=max_grad)
