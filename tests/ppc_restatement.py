"""The posterior predictive check stream (fugue_amd/csrc/fg_ppc_stream_plan.h) restated operation by operation in Python floats and
ints: the five statistics of a data set in member order, the counters and pivoted sums of a (slot, chain) column, the leaf
identities, the pair merge and the fixed tree on the chain index.  No transcendental is involved, so the device, the host driver and
this file agree bit for bit.  No numpy arithmetic on the path of a compared figure.  Also the inputs the CPU and GPU tests share.

A column is [n_lt, n_eq, n_gt, n_nan, n_fin, pivot, s1, s2]; a tree element is [n, mean, ssd, n_lt, n_eq, n_gt, n_nan]."""
import struct

import numpy as np

F64, BOOL, U64, USIZE, I64 = range(5)
MEAN, VAR, MIN, MAX, SUM, N_STATS = 0, 1, 2, 3, 4, 5
STAT_NAMES = ("mean", "var", "min", "max", "sum")
ALL = 31
INF = float("inf")
NAN = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]
WORDS = 6


def bits(v):
    return struct.unpack("<Q", struct.pack("<d", float(v)))[0]


def cell(u, vtype):
    """One raw 8-byte cell (a Python int, unsigned) as the double `x as f64`."""
    u = int(u) & 0xFFFFFFFFFFFFFFFF
    if vtype == F64:
        return struct.unpack("<d", struct.pack("<Q", u))[0]
    if vtype == U64:
        return float(u)                                 # int -> float rounds to nearest, ties to even, as the cast does
    return float(u - (1 << 64) if u >> 63 else u)


def stats(xs, want_var=True):
    """The five statistics of one data set (a list of floats, member order)."""
    K = len(xs)
    x = xs[0]
    total, mn, mx, nan = 0.0 + x, x, x, x != x
    for x in xs[1:]:
        total = total + x
        mn = x if x < mn else mn
        mx = x if x > mx else mx
        nan = nan or x != x
    mean = total / float(K)
    var = NAN
    if want_var:
        ss = 0.0
        for x in xs:
            d = x - mean
            ss = ss + d * d
        var = ss / float(K - 1) if K > 1 else NAN       # 0/0 and ss/0 with ss = NaN: K = 1 leaves ss = +0.0 or NaN, never a non-zero
    T = [mean, var, mn, mx, total]
    return [NAN if (nan or v != v) else v for v in T]


def new_column():
    return [0, 0, 0, 0, 0, 0.0, 0.0, 0.0]


def update(s, T, t_obs):
    if T != T or t_obs != t_obs:
        s[3] += 1
    elif T < t_obs:
        s[0] += 1
    elif T == t_obs:
        s[1] += 1
    else:
        s[2] += 1
    if T != T or T == INF or T == -INF:
        return
    if s[4] == 0:
        s[5], s[6], s[7] = T, 0.0, 0.0
    d = T - s[5]
    s[6] = s[6] + d
    s[7] = s[7] + d * d
    s[4] += 1


def state_words(s):
    """The six 8-byte words of a column as unsigned ints (bit patterns)."""
    return [s[0] | (s[1] << 32), s[2] | (s[3] << 32), s[4], bits(s[5]), bits(s[6]), bits(s[7])]


def leaf(s):
    e = [0.0, 0.0, 0.0, s[0], s[1], s[2], s[3]]
    if s[4] == 0:
        return e
    n = float(s[4])
    mu = s[6] / n
    e[0], e[1], e[2] = n, s[5] + mu, s[7] - s[6] * mu
    return e


def merge(a, b):
    if a[0] == 0.0:
        r = list(b)
    elif b[0] == 0.0:
        r = list(a)
    else:
        r = list(a)
        n = a[0] + b[0]
        delta = b[1] - a[1]
        r[0] = n
        r[1] = a[1] + delta * (b[0] / n)
        r[2] = a[2] + b[2] + delta * delta * (a[0] * b[0] / n)
    for i in (3, 4, 5, 6):
        r[i] = a[i] + b[i]
    return r


def tree(elems):
    """The fixed tree on the chain index: stride s = 1, 2, 4, ...; element i (a multiple of 2 s) takes in i + s when that exists."""
    e = [list(v) for v in elems]
    s = 1
    while s < len(e):
        for i in range(0, len(e) - s, 2 * s):
            e[i] = merge(e[i], e[i + s])
        s *= 2
    return e[0]


def slots_of(checks):
    """checks: [(rows, mask, observed)] -> [(check, statistic)] in check order, then statistic order."""
    return [(q, st) for q, (_, mask, _) in enumerate(checks) for st in range(N_STATS) if (mask >> st) & 1]


def observed_stats(checks):
    out = []
    for rows, mask, obs in checks:
        T = stats([float(v) for v in obs], bool((mask >> VAR) & 1))
        out += [T[st] for st in range(N_STATS) if (mask >> st) & 1]
    return out


def statistics_table(table, vtypes, checks):
    """table uint64 [n][n_rows][C] -> T_rep as nested lists [n][n_slots][C]."""
    n, n_rows, C = table.shape
    used = sorted({r for rows, _, _ in checks for r in rows})
    conv = {}                                             # row -> [n][C] floats; an f64 row is a view of the same bits, no arithmetic
    for r in used:
        if vtypes[r] == F64:
            conv[r] = np.ascontiguousarray(table[:, r, :]).view(np.float64).tolist()
        else:
            conv[r] = [[cell(u, vtypes[r]) for u in line] for line in table[:, r, :].tolist()]
    out = []
    for t in range(n):
        draw = {r: conv[r][t] for r in used}
        per_slot = []
        for rows, mask, _ in checks:
            cols = [[draw[r][c] for r in rows] for c in range(C)]
            T = [stats(xs, bool((mask >> VAR) & 1)) for xs in cols]
            per_slot += [[T[c][st] for c in range(C)] for st in range(N_STATS) if (mask >> st) & 1]
        out.append(per_slot)
    return out


def stream(table, vtypes, checks):
    """-> dict(t_obs [n_slots], T [n][n_slots][C], columns [n_slots][C], state uint64 words [6][n_slots][C], counts [n_slots][5] (lt eq gt
    nan fin), moments [n_slots][2] (mean, ssd), chains [n_slots][5][C])."""
    n, _, C = table.shape
    t_obs = observed_stats(checks)
    T = statistics_table(table, vtypes, checks)
    n_slots = len(t_obs)
    cols = [[new_column() for _ in range(C)] for _ in range(n_slots)]
    for draw in T:
        for k in range(n_slots):
            ck, tk, ob = cols[k], draw[k], t_obs[k]
            for c in range(C):
                update(ck[c], tk[c], ob)
    words = [[[state_words(cols[k][c])[w] for c in range(C)] for k in range(n_slots)] for w in range(WORDS)]
    counts, moments, chains = [], [], []
    for k in range(n_slots):
        e = tree([leaf(s) for s in cols[k]])
        counts.append([e[3], e[4], e[5], e[6], int(e[0])])
        moments.append([NAN, NAN] if e[0] == 0.0 else [e[1], e[2]])
        chains.append([[s[i] for s in cols[k]] for i in range(5)])
    return dict(t_obs=t_obs, T=T, columns=cols, state=words, counts=counts, moments=moments, chains=chains)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
ROW_KINDS = ("normal", "constant", "bernoulli", "u64_big", "neg_i64", "nan", "pos_inf", "neg_inf", "far")
ROW_VTYPES = dict(normal=F64, constant=F64, bernoulli=BOOL, u64_big=U64, neg_i64=I64, nan=F64, pos_inf=F64, neg_inf=F64, far=F64)
CONSTANT = -1.25


def row(kind, n, C, seed=0):
    """One table row's raw cells uint64 [n][C] of the given kind."""
    rng = np.random.default_rng([seed, ROW_KINDS.index(kind), n, C])
    N = n * C
    if kind == "bernoulli":
        u = (rng.random(N) < 0.6).astype(np.uint64)
    elif kind == "u64_big":                              # at and above 2^53: the conversion rounds (odd values, ties)
        u = (np.uint64(1) << np.uint64(53)) + rng.integers(0, 9, N).astype(np.uint64)
        u[::7] = (np.uint64(1) << np.uint64(63)) + rng.integers(0, 4097, len(u[::7])).astype(np.uint64)
    elif kind == "neg_i64":
        u = rng.integers(-6, 3, N).astype(np.int64).view(np.uint64)
    else:
        if kind == "constant":
            x = np.full(N, CONSTANT)
        elif kind == "far":                              # a mean far from the first draw's neighbourhood in units of the spread
            x = 1e6 + rng.normal(0.0, 1.0, N)
        else:
            x = rng.normal(0.0, 1.0, N)
        at = rng.integers(0, N, 1 + N // 9)
        if kind == "nan":
            x[at] = np.nan
        elif kind == "pos_inf":
            x[at] = np.inf
        elif kind == "neg_inf":
            x[at] = -np.inf
        u = x.view(np.uint64)
    return np.ascontiguousarray(u.reshape(n, C))


def table(kinds, n, C, seed=0):
    """Rows of the given kinds (a repeated kind gets a stream of its own) -> (uint64 [n][len(kinds)][C], vtypes)."""
    rows = [row(k, n, C, seed + 1000 * j) for j, k in enumerate(kinds)]
    return np.ascontiguousarray(np.stack(rows, axis=1)), [ROW_VTYPES[k] for k in kinds]


def standard_checks(K, seed=0):
    """The row kinds and checks of the sweeps: K rows of every kind, kind j in rows [j K, (j + 1) K).  -> (kinds, checks, labels)."""
    rng = np.random.default_rng([seed, K])
    kinds = [k for k in ROW_KINDS for _ in range(K)]
    rows = {k: list(range(j * K, (j + 1) * K)) for j, k in enumerate(ROW_KINDS)}
    normal_obs = [float(v) for v in rng.normal(0.0, 1.0, K)]
    checks = [
        (rows["normal"], ALL, normal_obs),                                           # N(0, 1) f64, all five (K = 1: the variance slot is all n_nan)
        (rows["constant"], ALL, [CONSTANT] * K),                                     # every draw lands in n_eq
        (rows["bernoulli"], (1 << SUM) | (1 << MEAN), [float(v) for v in rng.integers(0, 2, K)]),
        (rows["u64_big"], ALL, [float(2 ** 53 + 2 * i) for i in range(K)]),
        (rows["neg_i64"], (1 << MIN) | (1 << MAX) | (1 << SUM), [float(v) for v in rng.integers(-6, 3, K)]),
        (rows["nan"], ALL, normal_obs),
        (rows["pos_inf"], ALL, normal_obs),
        (rows["neg_inf"], ALL, normal_obs),
        (rows["pos_inf"], (1 << MEAN) | (1 << MAX), [INF] + normal_obs[1:]),         # T_obs = +inf: inf == inf counts in n_eq
        (rows["normal"], 1 << MAX, normal_obs),                                      # rows shared with the first check, a single bit
        (rows["far"], ALL, [NAN] + normal_obs[1:]),                                  # a NaN in the observed vector: all n_nan, the moments stay
        (rows["neg_inf"][:1] + rows["pos_inf"][:1] + rows["normal"][:1], ALL, [0.0, 0.5, -0.5]),   # -inf and +inf in one data set
    ]
    labels = ["normal", "constant", "bernoulli", "u64_big", "neg_i64", "nan", "pos_inf", "neg_inf", "obs_inf", "shared_max", "obs_nan", "mixed_inf"]
    return kinds, checks, labels


def coin_law(C):
    """The prior predictive number of heads of workloads.coin_flip (10 flips, bias ~ Beta(2, 2)) is Beta-Binomial(10, 2, 2), pmf(s) =
    (s + 1)(11 - s) / 286; against the observed 7 heads a draw is below / equal / above with probability 196 / 32 / 58 over 286.  ->
    [(expected count, 5 sigma half-width)] for n_lt, n_eq, n_gt of C independent draws: a false alarm below 1e-6 per count."""
    pmf = [(s + 1) * (11 - s) / 286.0 for s in range(11)]
    ps = [sum(pmf[:7]), pmf[7], sum(pmf[8:])]
    return [(C * p, 5.0 * (C * p * (1.0 - p)) ** 0.5) for p in ps]
