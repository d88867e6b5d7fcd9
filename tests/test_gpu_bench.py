"""bench.py on one GPU: a plain run reports the timed steps and nothing that needs runs of its own (those come with --full),
`--steps` sets the timed step count, and `--dump-outputs DIR` writes what the last timed step computed -- the same arrays,
bit for bit, from two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + args, env=env, capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_plain_line_and_dumped_outputs(tmp_path):
    args = ["--workload", "state", "--n-steps", "16", "--steps", "2", "--warmup", "1"]
    a = _bench(args + ["--dump-outputs", str(tmp_path / "a")])
    assert a["steps"] == 2 and a["warmup"] == 1 and a["ms_per_step"] > 0 and a["value"] > 0
    assert a["unit"] == "env-steps/s" and a["higher_is_better"] is True and a["dtype"] == "f32"
    assert not {"cpu_baseline", "gpu_over_cpu", "secondary", "optional_paths"} & set(a)
    b = _bench(args + ["--dump-outputs", str(tmp_path / "b")])
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"actor_params.npy", "critic_params.npy", "returns.npy", "advantages.npy", "Train_surrogate_loss.npy"} <= set(names)
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64), (n, x.dtype)
        assert np.array_equal(x, y), n
    assert np.load(tmp_path / "a" / "returns.npy").shape == (16, 4096, 1)
    assert float(np.load(tmp_path / "a" / "Train_value_function_loss.npy")[0]) == a["config"]["train_scalars"]["Train/value_function_loss"]
