"""`python bench.py --gpus N` must really start N ranks: the launcher / rendezvous / max-over-ranks skeleton
of bench.py is run here on CPU with gloo and a stub step (ADVCHAIN_BENCH_STUB=1); the GPU step itself is covered by
tests/test_dist_gpu.py and the -m gpu bench test."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(argv, extra_env=None, drop=("WORLD_SIZE", "RANK", "LOCAL_RANK")):
    env = {k: v for k, v in os.environ.items() if k not in drop}
    env["ADVCHAIN_BENCH_STUB"] = "1"
    env.update(extra_env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, env=env, capture_output=True,
                          text=True, timeout=300)


def test_gpus_2_self_spawns_two_ranks():
    r = _run(["--gpus", "2", "--steps", "3", "--warmup", "1"])
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout          # rank 0 prints ONE JSON line
    rec = json.loads(lines[0])
    assert rec["n_gpus"] == 2 and rec["rccl_ranks"] == 2
    assert rec["config"]["global_batch"] == 64 and rec["steps"] == 3 and rec["scaling"] == "weak"
    # load imbalance and collective count in the same line
    spread = rec["rank_ms_per_step"]
    assert len(spread["by_rank"]) == 2 and spread["min"] <= spread["max"] and abs(spread["max"] - rec["ms_per_step"]) < 0.5
    assert "all_reduces_per_step" in rec


def test_world_size_mismatch_fails_loudly():
    """A launcher that started 1 rank for --gpus 2 must not print n_gpus: 1."""
    r = _run(["--gpus", "2"], extra_env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"}, drop=())
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr
    assert not any(ln.startswith("{") for ln in r.stdout.splitlines())


def test_too_few_gpus_fails_loudly():
    """Without the stub the spawn path checks the visible devices first: no GPU here -> rc != 0, no JSON."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "ADVCHAIN_BENCH_STUB")}
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= 8:
        return
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8"], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode != 0 and "GPU(s) visible" in r.stderr
    assert not any(ln.startswith("{") for ln in r.stdout.splitlines())


def test_stub_refuses_dump_outputs(tmp_path):
    """--dump-outputs writes what the GPU path computed; the stub computes nothing and must say so, not write empty files."""
    r = _run(["--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / "out")])
    assert r.returncode != 0 and "--dump-outputs" in r.stderr
    assert not (tmp_path / "out").exists()


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_outputs(tmp_path):
    """A plain run: the headline line only (no roofline, no secondary legs), `steps` timed steps, and --dump-outputs writes
    the last step's loss (float64), the solver's outputs and every transform's parameters (float32), within 64 MB; arrays
    larger than bench.DUMP_MAX_ELEMS as a sample of that many elements.  A second run with the same arguments starts from
    the same inputs and writes the same arrays up to rounding."""
    import numpy as np
    import bench
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "ADVCHAIN_BENCH_STUB")}
    out, again = tmp_path / "out", tmp_path / "again"
    for d in (out, again):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                            "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0 and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert rec["solver_calls_in_process"] == 1 + 2           # a plain run makes the warm-up and the timed calls, no more
    assert abs(rec["value"] * rec["ms_per_step"] / 1e3 - 32) < 0.05        # cfg-2: 32 images per step
    for key in ("roofline", "kernel_time_ms_first_step", "other_workloads", "roofline_grid_sample3d", "cpu_baseline",
                "replayed_ms_per_step", "model_ms_per_step"):
        assert key not in rec, key
    files = {p.stem: np.load(p) for p in out.glob("*.npy")}
    assert sum(p.stat().st_size for p in out.glob("*.npy")) <= 64 << 20
    assert files["loss"].dtype == np.float64 and files["loss"].shape == () and np.isfinite(files["loss"])
    assert {"param_0_noise", "param_1_bias", "param_2_morph", "param_3_affine"} <= set(files), sorted(files)
    for nm in ("adv_data", "adv_predict", "warped_back_adv_output", "init_output"):
        assert files[nm].dtype == np.float32 and np.isfinite(files[nm]).all(), nm
    assert files["adv_data"].shape == (bench.DUMP_MAX_ELEMS,)           # 32 x 1 x 256 x 256: a sample
    assert rec["config"]["deterministic"] is True
    # identical inputs: the model's prediction on the clean data is the same bit for bit; what the timed path computed
    # from them agrees within rounding (the timed solver runs in its deterministic mode)
    assert np.array_equal(files["init_output"], np.load(again / "init_output.npy"))
    for p in sorted(out.glob("*.npy")):
        a, b = np.load(p), np.load(again / p.name)
        err = float(np.abs(a.astype(np.float64) - b).max()) if a.size else 0.0
        assert err <= 1e-6 + 1e-5 * float(np.abs(a).max()), (p.name, err, r.stderr[-1000:])
