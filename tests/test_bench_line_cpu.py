"""The line bench.py prints must fit the driver's record: contract keys first, `roofline` + `cpu_baseline`, `legs` LAST, <= 6 KB."""
import glob
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONTRACT = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config")


def _bench():
    spec = importlib.util.spec_from_file_location("fg_bench_module", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_compact_line_of_every_committed_verbose_document():
    bench = _bench()
    docs = sorted(glob.glob(os.path.join(ROOT, "profiles", "round*_bench_full.json")))
    assert docs
    for path in docs[-1:]:
        full = json.load(open(path))
        line = bench.compact(full)
        text = json.dumps(line, separators=(",", ":"))
        assert len(text) <= 6144, (path, len(text))
        keys = list(line)
        assert keys[: len(CONTRACT)] == list(CONTRACT)
        assert keys[-1] == "legs" and "roofline" in line and "workload" in line["config"] and "model" not in line["config"]
        for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
            assert k in line["roofline"]
        if "cpu_baseline" in full:
            for k in ("value", "unit", "cores", "kind", "sample"):
                assert k in line["cpu_baseline"]
        for leg in ("mh", "c5", "smc", "c3_65536", "c3_8192", "hmc_fd_dense"):
            e = line["legs"][leg]
            assert e["value"] > 0 and 0 < e["frac"] < 1.5 and e["kernel"]
        assert line["legs"]["mh"]["cpu"]["value"] > 0 and line["legs"]["smc"]["cpu"]["value"] > 0
        assert json.loads(text) == json.loads(json.dumps(line))


def test_default_arguments_fit_the_contract():
    bench = _bench()
    a = bench.parse([])
    assert a.gpus == 1 and a.steps > 0 and a.warmup >= 0 and not a.full


def test_a_plain_run_times_exactly_the_steps_asked_for(monkeypatch):
    bench = _bench()
    monkeypatch.delenv("FG_BENCH_FULL_OUT", raising=False)
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert a.steps == 7 and a.warmup == 3 and a.repeats == 1 and not a.full and a.full_out == "" and a.dump_outputs is None
    f = bench.parse(["--full", "--dump-outputs", "out"])
    assert f.full and f.repeats == 5 and f.full_out and f.dump_outputs == "out"


def test_the_line_of_a_plain_run_keeps_the_contract_without_the_full_legs():
    bench = _bench()
    full = json.load(open(sorted(glob.glob(os.path.join(ROOT, "profiles", "round*_bench_full.json")))[-1]))
    for k in ("check", "validity", "cpu_baseline", "mh", "smc", "c3", "c5", "hmc_fd_dense", "hmc_8192", "extras", "full_document"):
        full.pop(k, None)
    line = bench.compact(full)
    assert list(line)[: len(CONTRACT)] == list(CONTRACT)
    assert "roofline" in line and "legs" not in line and "check" not in line and "cpu_baseline" not in line
    assert line["ms_per_step"] > 0 and line["unit"] == "leapfrog-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f64"


def test_dumped_outputs_are_float64_and_fit_in_64_mb(tmp_path):
    import numpy as np
    bench = _bench()
    rng = np.random.default_rng(5)
    d, C = 32, 4096
    draws, lj, eps = rng.standard_normal((d, C)), rng.standard_normal(C), rng.random(C)
    assert bench.dump_outputs(str(tmp_path / "small"), draws, lj, eps) == ["draws_last_step", "log_joint", "step_size"]
    assert np.array_equal(np.load(tmp_path / "small" / "draws_last_step.npy"), draws)
    assert np.array_equal(np.load(tmp_path / "small" / "log_joint.npy"), lj) and np.array_equal(np.load(tmp_path / "small" / "step_size.npy"), eps)
    # 8 ranks of 65 536 chains would write 146 MB in all: each rank writes the same seeded sample of its chains
    C, world = 65536, 8
    draws, lj, eps = rng.standard_normal((d, C)), rng.standard_normal(C), rng.random(C)
    for rank in (0, 5):
        bench.dump_outputs(str(tmp_path / "big"), draws, lj, eps, world=world, rank=rank)
    files = sorted((tmp_path / "big").iterdir())
    assert len(files) == 8 and all(np.load(f).dtype == np.float64 for f in files)
    assert sum(f.stat().st_size for f in files) * world / 2 <= 64 << 20
    ids0, ids5 = np.load(tmp_path / "big" / "chain_id_rank0.npy"), np.load(tmp_path / "big" / "chain_id_rank5.npy")
    assert np.array_equal(ids5 - 5 * C, ids0) and np.all(np.diff(ids0) > 0)
    idx = ids0.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "big" / "draws_last_step_rank0.npy"), draws[:, idx])
    assert np.array_equal(np.load(tmp_path / "big" / "log_joint_rank5.npy"), lj[idx])


def test_a_draw_slab_smaller_than_the_region_ends_with_its_last_rows_in_order():
    torch = __import__("torch")
    bench = _bench()

    class Eng:                                      # writes the transition number into each row it is handed
        def __init__(self, slab):
            self.slab, self.s, self.calls = slab, 0, []

        def hmc_step(self, n, ptr):
            r = (ptr - self.slab.data_ptr()) // (self.slab[0].numel() * 8)
            assert 0 <= r and r + n <= self.slab.shape[0]
            for i in range(n):
                self.slab[r + i] = self.s
                self.s += 1
            self.calls.append(n)

    for K, rows, launch in ((103, 10, 4), (100, 100, 25), (57, 57, 25), (1000, 999, 25)):
        slab = torch.full((rows, 2, 3), -1.0, dtype=torch.float64)
        eng, done = Eng(slab), 0
        while done < K:
            n = min(launch, K - done)
            bench.ring_step(eng, n, done, slab, (-K) % rows)
            done += n
        assert eng.s == K and slab[:, 0, 0].tolist() == list(range(K - rows, K))
