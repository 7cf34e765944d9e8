"""The result expressions and synthetic draws shared by tests/test_result_cpu.py (conditioning of the oracle comparison) and
tests/test_gpu_result.py (device identity, oracle parity, shapes).  Sites, in address order:
    b#0 .. b#8   Normal          the nine terms of the linear predictor (FG_OP_DOT: two groups of four and a tail)
    f            Bernoulli       a bool site
    k            Categorical     a usize site, three categories
    s            Uniform         sin / cos arguments, kept inside [0.5, 1.5]
    u            Normal          exp / tanh / pow arguments
EXACT expressions use only + - x / sqrt abs floor min max clamp neg select: one correctly rounded operation each, so the oracle
(glibc) and the device agree bit for bit.  TRANSCENDENTAL expressions end in ONE transcendental whose argument comes from exactly
rounded operations and nothing follows it, so a one-ulp difference between ocml and glibc stays one ulp in the result."""
import numpy as np

from fugue_amd import model as M

COEF = [0.5, -0.25, 1.5, 0.125, -2.0, 0.75, 3.0, -0.375, 0.0625]
TRANSCENDENTAL_OPS = ("exp", "ln", "sin", "cos", "tanh", "pow")


def base_program():
    """-> (program, dict of site expressions)"""
    P = M.Program()
    b = [P.sample(M.addr("b", j), M.Normal(0.0, 1.0)) for j in range(9)]
    f = P.sample(M.addr("f"), M.Bernoulli(0.5))
    k = P.sample(M.addr("k"), M.Categorical([0.25, 0.25, 0.5]))
    s = P.sample(M.addr("s"), M.Uniform(0.5, 1.5))
    u = P.sample(M.addr("u"), M.Normal(0.0, 1.0))
    P.observe(M.addr("y"), M.Normal(b[0], 1.0), 0.3)
    return P, dict(b=b, f=f, k=k, s=s, u=u)


def expressions(v):
    """name -> expression over the sites `v` of base_program(); between them every opcode of the expression switch."""
    b, f, k, s, u = v["b"], v["f"], v["k"], v["s"], v["u"]
    lin = M.as_expr(0.25)
    for j in range(9):
        lin = lin + b[j] * COEF[j]
    exact = {
        "lin9": lin,                                                        # LOAD, 9 MACs -> DOT (4 + 4 + tail)
        "select": M.select(k, [b[0], 2.0, b[1] * b[2]]),                    # STORE x 3, GATHER; k outside 0..2 gives NaN
        "clamp": M.fmax(M.clamp(b[0] * 2.0, M.fmin(b[1], b[2]), 1.5), -b[3]),   # MUL, MIN, STORE, CLAMP, NEG, MAX
        "quot": (b[0] - b[1]) / (b[2] + 3.0),                               # SUB, ADD, STORE, DIV
        "rsub_rdiv": (1.0 - b[0] * b[1]) + 2.0 / (b[2] * b[2] + 1.0),       # RSUB, RDIV
        "sqrt_abs_floor": M.sqrt(M.fabs(b[0])) + M.floor(b[1] * 4.0),       # SQRT, ABS, FLOOR
        "no_site": M.as_expr(2.5) * 3.0 - 0.5,                              # folded on the host: a result reading no site
        "bool_site": b[4] + f * 3.0,                                        # MAC with an integer slot (not fused)
        "int_sites": f + k * 2.0,                                           # integer sites converted as FG_T_SITE says
    }
    transcendental = {
        "exp": M.exp(u),
        "ln": M.ln(M.fabs(b[5]) + 1.0),
        "sin": M.sin(s),
        "cos": M.cos(s),
        "tanh": M.tanh(b[6] * 0.5),
        "pow": M.powf(M.fabs(b[7]) + 0.5, 1.5),                             # POW: leaf exponent
        "rpow": M.powf(2.0, u * 0.5),                                       # RPOW: leaf base
    }
    return exact, transcendental


def draws(n: int, C: int, seed: int = 11):
    """cells [n][S][C] int64 in address order (b#0..b#8, f, k, s, u) with -0.0, +-inf and NaN placed in the b sites and in u, and
    category 7 (outside 0..2) in k."""
    rng = np.random.default_rng(seed)
    x = np.zeros((n, 13, C))
    x[:, :9] = rng.standard_normal((n, 9, C))
    x[:, 11] = rng.uniform(0.5, 1.5, (n, C))
    x[:, 12] = rng.standard_normal((n, C))
    special = [-0.0, np.inf, -np.inf, np.nan, 0.0]
    for q in range(min(n * C, 40)):                                          # every special value in every b site and in u, spread over draws and chains
        t, c = q % n, (q * 7 + 3) % C
        x[t, q % 9, c] = special[q % 5]
        x[(t + 1) % n, 12, (c + 1) % C] = special[(q + 2) % 5]
    cells = np.ascontiguousarray(x).view(np.int64).copy()
    cells[:, 9] = rng.integers(0, 2, (n, C))
    cells[:, 10] = rng.integers(0, 3, (n, C))
    cells[n - 1, 10, C // 2] = 7                                             # an index no option answers to
    cells[0, 10, 0] = -1
    return cells


def evaluate(expr, site_values, nudge=None):
    """numpy evaluation of an expression tree at site_values (handle -> array); nudge(op, value) may move a transcendental's
    result (the CPU test moves it by one ulp each way)."""
    def ev(e):
        if e.op == "const":
            return np.float64(e.value)
        if e.op == "site":
            return site_values[e.a]
        a = [ev(x) for x in e.args]
        with np.errstate(all="ignore"):
            if e.op == "select":
                idx, opts = a[0], np.stack(np.broadcast_arrays(*a[1:]))
                ok = (idx >= 0) & (idx < len(opts)) & (idx == np.floor(idx))
                return np.where(ok, np.take_along_axis(opts, np.where(ok, idx, 0).astype(int)[None], 0)[0], np.nan)
            fn = {"neg": np.negative, "exp": np.exp, "ln": np.log, "sqrt": np.sqrt, "abs": np.abs, "floor": np.floor, "sin": np.sin, "cos": np.cos,
                  "tanh": np.tanh, "add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide, "pow": np.power, "min": np.fmin,
                  "max": np.fmax, "clamp": lambda x, lo, hi: np.where(x < lo, lo, np.where(x > hi, hi, x))}[e.op]
            r = fn(*a)
        return nudge(e.op, r) if nudge and e.op in TRANSCENDENTAL_OPS else r
    return ev(expr)
