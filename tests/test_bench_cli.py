"""bench.py's command line at the tiny CPU shape: a plain run does the timed steps only and its
``--dump-outputs`` files repeat exactly from run to run; ``--full`` adds the round and the AUC."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4", "--preset", "tiny", "--backbone", "tiny"]


def _bench(*extra):
    env = dict(os.environ, OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *TINY, *extra], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    return d, _bench("--dump-outputs", str(d / "a"))


def test_plain_run_times_the_steps_only(plain):
    _, r = plain
    assert r["steps"] == 3 and r["warmup"] == 1 and r["full"] is False
    assert r["timed_step_kinds"]["eager_steps"] == 3  # --steps is the number of timed steps
    assert r["unit"] == "impressions/s" and r["higher_is_better"] is True and r["dtype"] == "fp32"
    assert r["ms_per_step"] > 0
    assert abs(r["value"] - 4 / (r["ms_per_step"] / 1000)) / r["value"] < 0.01
    for k in ("valid_auc", "learning_probe", "ipc_allreduce", "grad_allreduce_ms"):
        assert r[k] is None, k
    assert "round_s" not in r


def test_dump_outputs_are_the_last_step_and_repeat(plain):
    d, r = plain
    a = {n: np.load(d / "a" / f"{n}.npy") for n in ("loss", "losses", "params")}
    assert sorted(os.listdir(d / "a")) == ["loss.npy", "losses.npy", "params.npy"]
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert a["losses"].shape == (3,) and a["loss"].shape == (1,) and a["loss"][0] == a["losses"][-1]
    assert abs(float(a["losses"].mean()) - r["train_loss"]) < 1e-4
    assert a["params"].ndim == 1 and a["params"].size > 100_000 and float(np.abs(a["params"]).max()) > 0
    _bench("--dump-outputs", str(d / "b"))  # same arguments: same inputs, same outputs
    for n, v in a.items():
        assert np.array_equal(v, np.load(d / "b" / f"{n}.npy")), n


def test_full_run_adds_round_and_auc():
    r = _bench("--full", "--round", "on", "--no-probe", "--valid-limit", "16")
    assert r["full"] is True and r["round_steps"] > 0 and r["round_s"] > 0
    assert 0.0 <= r["valid_auc"] <= 1.0


def test_dump_sample_is_fixed_and_within_budget(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    try:
        import bench
    finally:
        sys.path.remove(ROOT)
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 2 * 1000)  # 1000 elements per array
    big = np.arange(5000, dtype=np.float64)
    for sub in ("x", "y"):
        bench.dump_outputs(str(tmp_path / sub), {"small": np.ones(7), "big": big})
    x, y = np.load(tmp_path / "x" / "big.npy"), np.load(tmp_path / "y" / "big.npy")
    assert x.dtype == np.float32 and x.shape == (1000,) and np.array_equal(x, y)
    assert np.all(np.diff(x) >= 0) and x.max() < 5000 and len(np.unique(x)) > 800  # a spread of big's entries
    assert np.array_equal(np.load(tmp_path / "x" / "small.npy"), np.ones(7, dtype=np.float32))
