"""bench.py's inputs and outputs: the pre-generated action pool is bitwise sharding.synthetic_actions step by step,
--dump-outputs writes the last timed step's obs / reward / done as float32 .npy within its size budget, and a plain run
(no --full) times exactly --steps steps and reports ms_per_step."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402
from trex_gym import sharding  # noqa: E402


def _limits(J=25):
    lo = np.linspace(-1.5, -0.2, J)
    hi = np.linspace(0.1, 2.0, J)
    return lo, hi


@pytest.mark.parametrize("n, draws, first_id", [(4096, 40, 0), (37, 500, 2048)])
def test_action_pool_is_synthetic_actions_step_by_step(n, draws, first_id):
    lo, hi = _limits()
    ids = torch.arange(first_id, first_id + n)
    pool = bench.action_pool(ids, draws, lo, hi, "cpu")
    want = torch.stack([sharding.synthetic_actions(ids, t, lo, hi, seed=0, device="cpu") for t in range(draws)])
    assert pool.dtype == torch.float32 and pool.shape == (draws, n, 25)
    assert torch.equal(pool, want)


def _fake_env(n, J=25, seed=0):
    g = torch.Generator().manual_seed(seed)
    rows = torch.rand(n, 3 * J + 2, generator=g)
    rows[:, 3 * J + 1] = (rows[:, 3 * J + 1] > 0.9).float()
    return types.SimpleNamespace(J=J, obs=rows[:, :3 * J], rew=rows[:, 3 * J], done=rows[:, 3 * J + 1] != 0), rows


def test_dump_outputs_writes_the_callers_arrays_as_float32(tmp_path):
    env, rows = _fake_env(64)
    bench.dump_outputs(str(tmp_path / "a"), env)
    got = {k: np.load(str(tmp_path / "a" / (k + ".npy"))) for k in ("obs", "reward", "done")}
    assert all(a.dtype == np.float32 for a in got.values())
    np.testing.assert_array_equal(got["obs"], rows[:, :75].numpy())
    np.testing.assert_array_equal(got["reward"], rows[:, 75].numpy())
    np.testing.assert_array_equal(got["done"], rows[:, 76].numpy())
    # the row block of a step_many launch gives the same files
    bench.dump_outputs(str(tmp_path / "b"), types.SimpleNamespace(J=25), rows)
    for k, a in got.items():
        np.testing.assert_array_equal(np.load(str(tmp_path / "b" / (k + ".npy"))), a)


def test_dump_outputs_samples_rows_beyond_the_budget(tmp_path, monkeypatch):
    env, rows = _fake_env(1000)
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 100 * 77 * 4)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), env)
    sizes = 0
    for k in ("obs", "reward", "done"):
        a, b = (np.load(str(tmp_path / d / (k + ".npy"))) for d in ("a", "b"))
        assert a.shape[0] == 100
        np.testing.assert_array_equal(a, b)           # the sample is fixed
        sizes += a.nbytes
    assert sizes <= 100 * 77 * 4
    obs = np.load(str(tmp_path / "a" / "obs.npy"))
    full = rows[:, :75].numpy()
    idx = [int(np.flatnonzero((full == r).all(1))[0]) for r in obs]
    assert idx == sorted(set(idx))                    # distinct env rows, in env order


@pytest.mark.gpu
def test_plain_run_times_its_steps_and_dumps_the_last_one(tmp_path):
    out = tmp_path / "out"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2",
                        "--preroll", "40", "--envs-per-gpu", "256", "--dump-outputs", str(out)],
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 7 and d["warmup"] == 2 and d["unit"] == "env-steps/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(256 * 1e3 / d["ms_per_step"], rel=1e-9)
    assert "cpu_baseline" not in d                     # measured with --full only
    obs, rew, done = (np.load(str(out / (k + ".npy"))) for k in ("obs", "reward", "done"))
    assert obs.shape == (256, 75) and rew.shape == (256,) and done.shape == (256,)
    assert obs.dtype == rew.dtype == done.dtype == np.float32
    assert np.isfinite(obs).all() and np.isfinite(rew).all() and set(np.unique(done)) <= {0.0, 1.0}
