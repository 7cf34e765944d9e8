"""A sequential restatement of the reference's ABC module (src/inference/abc.rs) in plain Python over IEEE doubles and the oracle's
scalar numerics: what the device kernels of fugue_amd/csrc/fg_abc.hip are held to.  Python floats are IEEE doubles and every line
below is one rounded operation in the reference's order, so the distances are comparable bit for bit.  No GPU, no engine.

    euclidean / manhattan / summary_stats   abc.rs:132-145, 168-180, 183-226
    kernel_bandwidths                       abc.rs:751-773
    sample_index                            abc.rs:816-830 (the uniform is handed in)
    kernel_mixture_log_density              abc.rs:776-799, the reference's own operations, its division included
    stop_rule                               the accept loop of abc.rs:295-316 / :534-547 over a table of per-attempt decisions

Divergences kept on purpose (the kernels document the same): a NaN among the simulated values of SummaryStats gives NaN where the
reference panics in `partial_cmp().unwrap()`; sums start from +0.0.
"""
from __future__ import annotations

import math

from oracle import oracle as orc

INF = float("inf")
LN_2PI_HALF = 0.5 * math.log(2.0 * math.pi)                # abc.rs:796: 0.5 * (2.0 * PI).ln()


def euclidean(observed, simulated) -> float:
    if len(observed) != len(simulated):
        return INF
    s = 0.0
    for o, x in zip(observed, simulated):
        dv = float(o) - float(x)
        s = s + dv * dv
    return _sqrt(s)


def manhattan(observed, simulated) -> float:
    if len(observed) != len(simulated):
        return INF
    s = 0.0
    for o, x in zip(observed, simulated):
        s = s + abs(float(o) - float(x))
    return s


def _sqrt(x: float) -> float:
    return math.sqrt(x) if x >= 0.0 else float("nan")      # (NaN and negative arguments: NaN, as f64::sqrt)


def compute_stats(data):
    """abc.rs:192-210: [mean, population std, median]; None when a NaN is among the data (the reference panics)."""
    data = [float(v) for v in data]
    if not data:
        return [0.0, 0.0, 0.0]
    if any(v != v for v in data):
        return None
    k = len(data)
    s = 0.0
    for v in data:
        s = s + v
    mean = s / float(k)
    ss = 0.0
    for v in data:
        dv = v - mean                                      # (inf - inf = NaN, as in the reference)
        ss = ss + dv * dv
    var = ss / float(k)
    srt = sorted(data)                                     # no NaN: a total order up to the sign of zero
    med = (srt[k // 2 - 1] + srt[k // 2]) / 2.0 if k % 2 == 0 else srt[k // 2]
    return [mean, _sqrt(var), med]


def summary_stats(observed, simulated, weights) -> float:
    o_st, s_st = compute_stats(observed), compute_stats(simulated)
    if o_st is None:
        raise ValueError("NaN in the observed vector")
    if s_st is None:
        return float("nan")
    s = 0.0
    for o, x, w in zip(o_st, s_st, weights):
        dv = o - x
        s = s + float(w) * (dv * dv)
    return _sqrt(s)


def distance(kind: int, observed, simulated, weights=()) -> float:
    return (euclidean, manhattan, lambda o, s: summary_stats(o, s, weights))[kind](observed, simulated)


def kernel_bandwidths(coords, weights):
    """coords [n][d] (one row per particle), weights [n] -> [d]"""
    d = len(coords[0]) if len(coords) else 0
    total = 0.0
    for w in weights:
        total = total + float(w)
    if total <= 0.0:
        return [1e-3] * d
    out = []
    for c in range(d):
        mean = 0.0
        for row, w in zip(coords, weights):
            mean = mean + float(w) * float(row[c])
        mean = mean / total
        var = 0.0
        for row, w in zip(coords, weights):
            dv = float(row[c]) - mean
            var = var + float(w) * dv * dv
        var = var / total
        bw = _sqrt(2.0 * var)
        out.append(bw if bw > 1e-12 else 1e-3)
    return out


def sample_index(u: float, weights) -> int:
    """abc.rs:816-830 with the uniform handed in (total <= 0 draws an index uniformly in the reference: not restated, the engine
    refuses such a population)."""
    total = 0.0
    for w in weights:
        total = total + float(w)
    if total <= 0.0:
        raise ValueError("weights without mass")
    ut = u * total
    cum = 0.0
    for i, w in enumerate(weights):
        cum = cum + float(w)
        if ut <= cum:
            return i
    return len(weights) - 1


def gaussian_log_density(x, mean, std) -> float:
    lp = 0.0
    for xi, mi, si in zip(x, mean, std):
        s = max(float(si), 1e-12)
        z = (float(xi) - float(mi)) / s
        lp = lp + (-0.5 * z * z - math.log(s) - LN_2PI_HALF)
    return lp


def kernel_mixture_log_density(x, centers, weights, kernel_std) -> float:
    """x [d], centers [n][d], weights [n], kernel_std [d]"""
    terms = [(math.log(w) if w > 0.0 else -INF) + gaussian_log_density(x, c, kernel_std) for c, w in zip(centers, weights)]
    return orc.log_sum_exp(terms)


def stage_weights(log_prior, log_denom):
    """abc.rs:612-616, 632-640: normalised importance weights of a stage"""
    lw = [p - q for p, q in zip(log_prior, log_denom)]
    log_norm = orc.log_sum_exp(lw)
    n = len(lw)
    return [math.exp(v - log_norm) if math.isfinite(log_norm) else 1.0 / n for v in lw]


def stop_rule(accept, n: int, budget: int):
    """accept[a] for attempts a = 0, 1, ...: the sequential loop stops right after the n-th accept or at its budget.
    -> (indices of the accepted attempts, attempts made)"""
    taken, a = [], 0
    while len(taken) < n and a < budget:
        if accept[a]:
            taken.append(a)
        a += 1
    return taken, a
