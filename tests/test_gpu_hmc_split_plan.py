"""The wave splits of the HMC launchers (fugue_amd/csrc/fg_hmc_split_plan.h) on the device, at the chain counts where the rules that
production runs take apply: several tiles per CU (four or eight waves per tile by the residency rule), the one-barrier gradient chosen
by the host, a split re-planned on a used engine, the interpreter kernel's program in LDS or in global memory.  Whatever the split,
the arithmetic per chain is the same: every comparison is bit for bit.  The W and the program's place a kernel name must show come from
the CPU plan for the same inputs (tests/cpp/split_plan_driver.cpp), not from a literal."""
import numpy as np
import pytest

from fugue_amd import engine as E
from tests.models import ZOO
from tests.test_hmc_split_plan_cpu import FAST, SPARSE, U, build_driver, jit_case, mwi_case, run_plans

pytestmark = pytest.mark.gpu

L, NW, NS = 3, 4, 2


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return build_driver(tmp_path_factory.mktemp("split_plan"))


@pytest.fixture(scope="module")
def n_simd():
    """SIMDs of device 0 (four per CU), asked of the HIP runtime the library itself runs on (no second runtime in this process)."""
    import ctypes
    E.lib()
    cus = ctypes.c_int(0)
    for path in sorted({ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64" in ln}):      # (a process that also imported PyTorch holds the wheel's runtime too, which may see no device)
        if ctypes.CDLL(path).hipDeviceGetAttribute(ctypes.byref(cus), 63, 0) == 0 and cus.value > 0:    # 63: hipDeviceAttributeMultiprocessorCount
            return 4 * cus.value
    raise AssertionError("no HIP runtime of this process reports device 0")


def run(cp, C, monkeypatch, env, mode=E.GRAD_FD_SPARSE, eng=None):
    """One short run under `env` (the switches not named are unset): (results, kernel name)."""
    for k in ("FG_JIT", "FG_HMC_INTERP_WAVES", "FG_JIT_TASKS", "FG_JIT_FUSED", "FG_HMC_INTERP_OCC", "FG_HMC_INTERP_LDSPROG", "FG_HMC_JIT_OCC", "FG_HMC_WAVES"):
        if k in env: monkeypatch.setenv(k, str(env[k]))
        else: monkeypatch.delenv(k, raising=False)
    own = eng is None
    if own: eng = E.Engine(cp, C, seed=41, chain_offset=5)
    d = eng.device_alloc(NS * cp.d * C * 8)
    st = eng.hmc_run(E.hmc_config(n_leapfrog=L, grad_mode=mode), NS, NW, d)
    name = eng.hmc_last_kernel()
    draws = eng.download(d, (NS, cp.d, C))
    eng.device_free(d)
    out = (draws, eng.hmc_step_sizes(), eng.hmc_log_joint(), eng.get_values(), st.accept_rate, st.n_divergent)
    if own: eng.close()
    return out, name


def same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


def cpu_jit_plan(driver, tmp_path, cp, C, n_simd, mode=SPARSE, sw=(U, U, U), tasks=U, sub=FAST):
    """fg_jit_task_plan / fg_jit_launch_shape for this program.  W does not depend on the task costs; the one-barrier form does (`sub`)."""
    return run_plans(driver, [jit_case(d=cp.d, S=cp.S, n_simd=n_simd, tiles0=(C + 63) // 64, sw0=sw, tasks=tasks, mode=mode, sub=sub)], tmp_path)[0]


@pytest.mark.parametrize("name,C,W", [("refmodel8", 65536, 4), ("hier", 16448, 8), ("hier_scale", 16448, 8)])
def test_the_several_tiles_per_cu_rule_is_bit_identical_to_the_stream_kernel(name, C, W, driver, n_simd, tmp_path, monkeypatch):
    """Four resident tiles of at most sixteen tasks: four waves; otherwise eight.  `W` is what the rule gives on 256 CUs; the assertion is
    against the CPU plan for the device at hand."""
    cp = E.compile_model(ZOO[name]())
    plan = cpu_jit_plan(driver, tmp_path, cp, C, n_simd)
    assert "resident" in plan["say"] and (n_simd != 1024 or plan["W"] == W), plan["say"]      # the rule was taken, not W = wcap
    ref, k0 = run(cp, C, monkeypatch, {"FG_JIT": 0})
    by_rule, k1 = run(cp, C, monkeypatch, {"FG_JIT": 1})
    forced, k2 = run(cp, C, monkeypatch, {"FG_JIT": 1, "FG_HMC_INTERP_WAVES": 16})
    assert k0.startswith("k_hmc_stream_steps") and k1.startswith("k_hmc_jit_steps W=%d " % plan["W"]), (k0, k1, plan["W"])
    assert k2.startswith("k_hmc_jit_steps W=%d " % cpu_jit_plan(driver, tmp_path, cp, C, n_simd, sw=(16, U, U))["W"]), k2
    assert np.isfinite(ref[0]).all() and same(ref, by_rule) and same(ref, forced)


def test_one_engine_replans_when_the_gradient_mode_changes(monkeypatch):
    """sparse -> dense -> analytic -> sparse on one engine against four fresh engines of the same seed."""
    cp = E.compile_model(ZOO["hier"]())
    C = 150
    modes = [E.GRAD_FD_SPARSE, E.GRAD_FD_DENSE, E.GRAD_ANALYTIC, E.GRAD_FD_SPARSE]
    fresh = [run(cp, C, monkeypatch, {}, mode=m) for m in modes]
    eng = E.Engine(cp, C, seed=41, chain_offset=5)
    used = [run(cp, C, monkeypatch, {}, mode=m, eng=eng) for m in modes]
    eng.close()
    assert [k for _, k in used] == [k for _, k in fresh]
    assert fresh[0][1].startswith("k_hmc_jit_steps") and "dense" in fresh[1][1]
    for (a, _), (b, _) in zip(fresh, used):
        assert same(a, b)


def test_tasks_and_one_barrier_switches_at_several_tiles_per_cu(driver, n_simd, tmp_path, monkeypatch):
    """FG_JIT_TASKS=0 (the task list in memory), FG_JIT_FUSED=0 / 1 against the host's own choice; "one barrier per gradient" is in the name
    exactly when it is forced on or chosen -- chosen as the CPU plan chooses for this program's costs."""
    cp = E.compile_model(ZOO["refmodel8"]())
    C = 16448
    sub = [(0, 0, E.lib().fg_program_dep_count(cp.h, k), 0) for k in range(cp.d)]        # (every instruction of its sub-programs is a fast Normal)
    ref, _ = run(cp, C, monkeypatch, {})
    for env, sw, tasks, one_barrier in [({}, (U, U, U), U, None), ({"FG_JIT_TASKS": 0}, (U, U, U), 0, False), ({"FG_JIT_FUSED": 0}, (U, U, 0), U, False), ({"FG_JIT_FUSED": 1}, (U, U, 1), U, True)]:
        out, k = run(cp, C, monkeypatch, env)
        want = cpu_jit_plan(driver, tmp_path, cp, C, n_simd, sw=sw, tasks=tasks, sub=sub)
        assert k == want["name"] and same(ref, out), (env, k, want["name"])
        assert ("one barrier per gradient" in k) == (bool(want["cb"]) if one_barrier is None else one_barrier), (env, k)


@pytest.mark.parametrize("name", ["alldists", "poisson_glm"])
def test_the_interpreter_kernel_at_several_tiles_per_cu(name, driver, n_simd, tmp_path, monkeypatch):
    cp = E.compile_model(ZOO[name]())
    C = 16448
    prog_bytes = 96 * (cp.n_instructions + sum(E.lib().fg_program_dep_count(cp.h, k) for k in range(cp.d)))      # (sub-programs + the program, 96 bytes an instruction)
    outs = []
    for waves in (U, 2, 8):
        out, k = run(cp, C, monkeypatch, {"FG_JIT": 0} if waves == U else {"FG_JIT": 0, "FG_HMC_INTERP_WAVES": waves})
        plan = run_plans(driver, [mwi_case(d=cp.d, S=cp.S, n_slots=cp.n_slots, n_simd=n_simd, tiles=(C + 63) // 64, prog_bytes=prog_bytes, sw=(waves, U, U))], tmp_path)[0]
        assert plan["rc"] == 0 and k == plan["name"] and ("(program in global memory)" in k) == (not plan["pl"]), (k, plan)
        outs.append(out)
    assert np.isfinite(outs[0][0]).all() and same(outs[0], outs[1]) and same(outs[0], outs[2])
