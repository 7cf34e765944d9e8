"""One table of single-site MH edge cases, shared by tests/test_mh_edges_cpu.py (the oracle alone, against src/inference/mh.rs read by
hand) and tests/test_gpu_mh_edges.py (every MH kernel family against the oracle, step by step).  Data and small helpers only.

Model A has a score stream, so every operand is a constant or a site; model B has an expression parameter, so it has none and runs on
the interpreter kernels and the kernels compiled at run time.  Sites, in address order:

  b  Bernoulli(0.3)                 flip (mh.rs:263-269)
  c  Categorical(0.2, 0, 0.5, 0.3)  prior resample, a zero entry in the table (mh.rs:516-530)
  d  DiscreteUniform(-3, 3)         i64 walk (mh.rs:557-567) -- model B only: a DiscreteUniform site has no score-stream record
  e  Exponential(1)                 automatic kind (mh.rs:339-358)
  g  Gamma(2, 1)                    automatic kind
  k  Poisson(0.7)                   u64 walk reflected about -1/2 (mh.rs:285-294)
  n  Normal(0, 1)                   LogSpace by override: a real-line site on the log walk, current <= 0 in half of the prior starts
  r  Normal(0, 3)                   Reflect(-1, 1)
  u  Uniform(0, 2)                  Reflect(0, 2)
  v  Normal(0, 1)                   Reflect(0.5, 0.5): range == 0 returns the current value, z still consumed (mh.rs:241-244)
  w  Normal(0, 1)                   Reflect(1, -1):   range < 0, the same
  A: observe Normal(n, g) = -2.5, Normal(u, 0.5) = Normal(r, 2) = 0.7     (a sum of sites as an operand would cost A its stream)
  B: observe Normal(n + u + r, 0.5 + g) = -2.5

Chain c starts from the prior draw of chain c with case c mod len(CASES) written over it (a case = {site: value}); the empty case is the
control group.  C = 150 chains: every case sits in several lanes, the last tile is part-filled.

The one deliberate deviation of the device: it caps the reflection loop at 100 000 iterations where mh.rs:247-254 has no cap
(fugue_amd/csrc/fg_interp.h, fg_mh_walk_proposal).  Every Reflect case here stays below 1 000 bounces: a Reflect site with a positive
range has range 2 (>= 1, the scale is clamped at 100 and |z| < 7), and no start lies more than 40 ranges outside its bounds.

The adaptation models have one latent site: `flat` accepts essentially every move (the scale climbs to the clamp at 100), `peaked`
rejects almost every move (the scale sinks to the clamp at 0.001)."""
import math

import numpy as np

from fugue_amd import model as M

PROP_AUTO, PROP_GAUSSIAN, PROP_LOGSPACE, PROP_REFLECT, PROP_PRIOR_RESAMPLE = range(5)   # SiteProposal, mh.rs:145-161 (oracle and engine)
F64, BOOL, U64, USIZE, I64 = range(5)
RNG_PRIOR, RNG_MH = 1, 4                                # stream purposes (oracle/fugue_oracle.h)

MIN_POSITIVE = 2.2250738585072014e-308                  # f64::MIN_POSITIVE
F64_MAX = 1.7976931348623157e308                        # f64::MAX
INF, NAN = math.inf, math.nan

C, NW, NS = 150, 40, 20                                 # chains, adapting steps, frozen steps
CHAIN0 = 5
SEEDS = {"A": 47, "B": 55}                              # chosen so that test_mh_edges_cpu.py's margin and branch-count conditions hold
MARGIN = 1e-6                                           # |ln u - log_alpha| of every decided step (tests/test_mh_edges_cpu.py)
MIN_TAKES = 20

CAT_TABLE = (0.2, 0.0, 0.5, 0.3)
OBSERVED = 0.7
OBSERVED_N = -2.5                                       # what n is observed at: below 0, so that the log walk's nudge from n <= 0 up to MIN_POSITIVE often
                                                        # LOSES likelihood -- log_alpha < 0, and the accept uniform of block 1 (no z drawn) decides
REFLECT = {"r": (-1.0, 1.0), "u": (0.0, 2.0), "v": (0.5, 0.5), "w": (1.0, -1.0)}
LOGSPACE_FORCED = ("n",)
POSITIVE_AUTO = ("e", "g")

LOGSPACE_STARTS = (1e308, F64_MAX, INF, NAN, 2.3e-308, 5e-324, 0.0, -0.0, -3.0)

CASES = (
    [{}]                                                                    # control: the untouched prior start
    + [{"n": x} for x in LOGSPACE_STARTS]                                   # the forced log walk at every corner of its domain
    + [{"g": x} for x in LOGSPACE_STARTS] + [{"g": -1.0}]                   # automatic kind: LogSpace where > 0, else Gaussian for good
    + [{"e": x, "k": 1} for x in (F64_MAX, INF, 5e-324, 0.0, -1.0)]
    + [{"k": 0}, {"k": 1}, {"k": 10 ** 15}]
    # r at and outside its bounds (k = 1 rides along here and above: a reflection from state 1 needs delta <= -2, rare from the prior starts alone)
    + [{"r": -1.0, "k": 1}, {"r": 1.0, "k": 1}, {"r": -1.0 - 40 * 2.0 + 0.5, "k": 1}, {"r": 1.0 + 40 * 2.0 - 0.25, "k": 1}, {"r": 7.5, "k": 1}, {"r": NAN}]
    # outside the support and the bounds: the log-weight is -inf until the site moves, and that move's log_alpha is +inf
    + [{"u": 5.0, "k": 1}, {"u": -3.0, "k": 1}, {"u": 2.5, "k": 1}, {"u": -0.5, "k": 1}, {"e": -2.5}]
    + [{"c": -1}, {"c": len(CAT_TABLE)}, {"c": len(CAT_TABLE) + 3}, {"c": 1}]   # out of range / on the zero entry: every proposal's log_alpha is NaN
)


def _program(stream: bool) -> M.Program:
    P = M.Program()
    P.sample(M.addr("b"), M.Bernoulli(0.3))
    P.sample(M.addr("c"), M.Categorical(list(CAT_TABLE)))
    if not stream: P.sample(M.addr("d"), M.DiscreteUniform(-3, 3))
    P.sample(M.addr("e"), M.Exponential(1.0))
    g = P.sample(M.addr("g"), M.Gamma(2.0, 1.0))
    P.sample(M.addr("k"), M.Poisson(0.7))
    n = P.sample(M.addr("n"), M.Normal(0.0, 1.0))
    r = P.sample(M.addr("r"), M.Normal(0.0, 3.0))
    u = P.sample(M.addr("u"), M.Uniform(0.0, 2.0))
    P.sample(M.addr("v"), M.Normal(0.0, 1.0))
    P.sample(M.addr("w"), M.Normal(0.0, 1.0))
    if stream:
        P.observe(M.addr("y", 0), M.Normal(n, g), OBSERVED_N)
        P.observe(M.addr("y", 1), M.Normal(u, 0.5), OBSERVED)
        P.observe(M.addr("y", 2), M.Normal(r, 2.0), OBSERVED)
    else:
        P.observe(M.addr("y"), M.Normal(n + u + r, 0.5 + g), OBSERVED_N)
    return P


def model_a() -> M.Program:
    return _program(True)


def model_b() -> M.Program:
    return _program(False)


MODELS = {"A": model_a, "B": model_b}


def overrides(site_names):
    """Per sorted site: None or (kind, lower, upper)."""
    ov = [None] * len(site_names)
    for name, (lo, hi) in REFLECT.items():
        ov[site_names.index(name)] = (PROP_REFLECT, lo, hi)
    for name in LOGSPACE_FORCED:
        ov[site_names.index(name)] = (PROP_LOGSPACE, 0.0, 0.0)
    return ov


def f64_cell(x: float) -> int:
    return int(np.array([x], dtype=np.float64).view(np.int64)[0])


def case_of_chain(c: int) -> dict:
    return CASES[c % len(CASES)]


def start_cells(om, seed: int, n_chains: int = C, chain0: int = CHAIN0) -> np.ndarray:
    """[S][n_chains] cells: the oracle's prior draw of every chain (what mh_init draws, mh.rs:950-957) with the chain's case written in."""
    out = np.zeros((om.S, n_chains), dtype=np.int64)
    for c in range(n_chains):
        cells, _, _ = om.run_prior(seed, chain0 + c, 0, RNG_PRIOR)
        out[:, c] = cells
        for name, x in case_of_chain(c).items():
            j = om.site_names.index(name)
            out[j, c] = f64_cell(x) if om.site_vtypes[j] == F64 else int(x)
    return out


# ---------------------------------------------------------------------------------- adaptation models
def flat_model() -> M.Program:
    P = M.Program()
    P.sample(M.addr("x"), M.Uniform(-1e6, 1e6))
    return P


PEAK = 0.25


def peaked_model() -> M.Program:
    P = M.Program()
    x = P.sample(M.addr("x"), M.Normal(0.0, 1.0))
    P.observe(M.addr("y"), M.Normal(x, 1e-7), PEAK)
    return P


# name -> (program, start of x or None for the prior draw, steps, the clamp the scale ends at).  The peaked chains start ON the peak: from
# the prior a chain first climbs to it, accepting about every second move, and needs twice the steps to sink to the clamp.
ADAPT = {"flat": (flat_model, None, 180, 100.0), "peaked": (peaked_model, PEAK, 620, 0.001)}
ADAPT_C, ADAPT_SEED, ADAPT_CHAIN0 = 64, 41, 2


def adapt_start(x0):
    """[1][ADAPT_C] start cells of an adaptation model, or None for the prior draw."""
    return None if x0 is None else np.full((1, ADAPT_C), f64_cell(x0), dtype=np.int64)
