"""The benchmark's contract: a plain ``bench.py --gpus 1 --steps K --warmup W`` times exactly K steps, reports ``ms_per_step`` and
nothing of what ``--full`` adds, and ``--dump-outputs DIR`` writes what the last timed step returned — the same arrays run after run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *extra):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "AOG_FORCE_DIST", "AOG_BENCH_SHARE_GPU"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "5", "--batch", "128",
                        "--no-spinup", "--dump-outputs", str(out_dir), *extra], capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_plain_bench_line_and_dumped_outputs_are_reproducible(tmp_path):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    res = _bench(tmp_path / "a")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in res, k
    assert res["metric"] == "env_steps_per_sec" and res["unit"] == "env-steps/s" and res["higher_is_better"] is True
    assert res["steps"] == 40 and res["config"]["batch_per_gpu"] == 128
    # value = envs x steps / wall time, ms_per_step = wall time / steps: their product is the batch
    assert res["value"] > 0 and res["ms_per_step"] > 0
    np.testing.assert_allclose(res["value"] * res["ms_per_step"] * 1e-3, 128, rtol=1e-9)
    for k in ("roofline", "roofline_dominant", "value_pipelined", "parity", "cpu_baseline"):
        assert k not in res, k                        # --full only
    names = {"obs", "reward", "done", "trunc", "power", "obs_raw", "strehl"}
    assert {f[:-4] for f in os.listdir(tmp_path / "a")} == names
    first = {n: np.load(tmp_path / "a" / f"{n}.npy") for n in names}
    for n, a in first.items():
        assert a.dtype == np.float32 and a.shape[0] == 128 and np.isfinite(a).all(), n
    assert first["obs_raw"].shape == (128, 4) and ((first["strehl"] > 0) & (first["strehl"] <= 1)).all()
    # 40 steps of 30-step episodes after 5 of warm-up: the last timed step is step 15 of an episode, not its end
    assert not first["done"].any()
    _bench(tmp_path / "b")
    for n, a in first.items():
        np.testing.assert_allclose(np.load(tmp_path / "b" / f"{n}.npy"), a, rtol=1e-6, atol=0, err_msg=n)
