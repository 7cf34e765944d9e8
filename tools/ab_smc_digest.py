"""SHA-256 of what adaptive_smc computes for a fixed list of small runs, one line per run: betas, log_evidence, values, log_weights,
weights and n_model_runs of fg_smc_run; values, weights and the accept rate of the standalone smc_prior_particles -> smc_resample ->
smc_rejuvenate sequence.  Two builds compute the same thing when their outputs are the same, line for line
(FG_LIB_PATH=<other build's libfugue_amd.so> selects the library).  The list covers every rejuvenation kernel and launcher path: score
classes 0 / 3 / 2 / -1, the compiled sweep, sequential adaptation, the global tile, the population rule of large runs, the three
resampling methods, the separate-kernels reweight and the importance-sampling branch.

    python tools/ab_smc_digest.py [> profiles/...]
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fugue_amd import engine as E, workloads as W      # noqa: E402
from tests.models import ZOO                           # noqa: E402


def digest(*parts):
    h = hashlib.sha256()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes())
    return h.hexdigest()


def run(label, prog, n, seed=17, env=(), **kw):
    for k, v in env:
        os.environ[k] = v
    try:
        eng = E.Engine(E.compile_model(prog), n, seed=seed)
        r = eng.smc_run(**kw)
        eng.close()
    finally:
        for k, _ in env:
            del os.environ[k]
    print(label, len(r["betas"]), "steps", *(digest(np.asarray(r[k], dtype=None if k == "values" else np.float64)) for k in ("betas", "log_evidence", "values", "log_w", "weights")),
          int(r["n_model_runs"]), flush=True)


def standalone(label, prog, n, env=()):
    for k, v in env:
        os.environ[k] = v
    try:
        eng = E.Engine(E.compile_model(prog), n, seed=23)
        eng.smc_prior_particles()
        idx = eng.smc_resample(E.RESAMPLE_SYSTEMATIC, step=1)
        acc = eng.smc_rejuvenate(0.37, 2)
        print(label, digest(idx), digest(eng.get_values()), digest(*eng.smc_weights()), digest(np.float64(acc)), flush=True)
        eng.close()
    finally:
        for k, _ in env:
            del os.environ[k]


def main():
    jit0, jit1 = (("FG_JIT", "0"),), (("FG_JIT", "1"),)
    run("smc_normal 4096", W.smc_normal(), 4096, rejuvenation_steps=3)
    run("refmodel8 4096 sequential", ZOO["refmodel8"](), 4096, rejuvenation_steps=2, sequential_adaptation=True)
    run("refmodel8 4096 batched", ZOO["refmodel8"](), 4096, rejuvenation_steps=2)
    for name in ("mixture", "hier_scale", "poisson_glm"):
        run(f"{name} 3000 FG_JIT=0", ZOO[name](), 3000, env=jit0, rejuvenation_steps=2)
        run(f"{name} 3000 FG_JIT=1", ZOO[name](), 3000, env=jit1, rejuvenation_steps=2)
    run("normal_sites(400) 512 batched", W.normal_sites(400), 512, rejuvenation_steps=2)
    run("normal_sites(400) 64 sequential", W.normal_sites(400), 64, rejuvenation_steps=2, sequential_adaptation=True)
    run("refmodel8 262144 FG_JIT=1", ZOO["refmodel8"](), 1 << 18, seed=19, env=jit1, rejuvenation_steps=2)
    for method, mname in ((E.RESAMPLE_SYSTEMATIC, "systematic"), (E.RESAMPLE_STRATIFIED, "stratified"), (E.RESAMPLE_MULTINOMIAL, "multinomial")):
        run(f"smc_normal 5000 {mname}", W.smc_normal(), 5000, resampling_method=method, rejuvenation_steps=2)
    run("smc_normal 4096 FG_SMC_FORCE_SUM=1", W.smc_normal(), 4096, env=(("FG_SMC_FORCE_SUM", "1"),), rejuvenation_steps=2)
    run("smc_normal 4096 rejuvenation_steps=0", W.smc_normal(), 4096, rejuvenation_steps=0)
    for jit in (jit0, jit1):
        standalone(f"standalone normal_sites(400) 128 FG_JIT={jit[0][1]}", W.normal_sites(400), 128, env=jit)
        standalone(f"standalone mixture 3000 FG_JIT={jit[0][1]}", ZOO["mixture"](), 3000, env=jit)


if __name__ == "__main__":
    main()
