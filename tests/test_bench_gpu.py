"""bench.py's contract on one GPU: a plain run (no --full) prints the headline line without any side object, --steps / --warmup are the
counts it times and warms up, value and ms_per_step describe the same timed steps, and --dump-outputs writes the last step's outputs
as float32 .npy files, 64 MB at most in all."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDE_OBJECTS = {"roofline", "roofline_gemm", "roofline_hiera_attention", "cpu_baseline", "train_iteration", "train_iteration_frozen_encoder",
                "f16", "bf16", "volume_3d"}


@pytest.mark.gpu
def test_plain_run_dumps_last_step(tmp_path):
    out = tmp_path / "outputs"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "MSAM2_LIB_PATH")}
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["metric"] == "slices/sec @1024^2 (Hiera-S)" and line["unit"] == "slices/s" and line["higher_is_better"] is True
    assert line["dtype"] == "bf16" and line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(4 * 1e3 / line["ms_per_step"], rel=1e-9)   # 4 slices per step
    assert not SIDE_OBJECTS & set(line), sorted(SIDE_OBJECTS & set(line))
    names = sorted(os.listdir(out))
    assert names == ["iou_predictions.npy", "low_res_masks.npy", "maskmem_features.npy"], names
    for name in names:
        a = np.load(out / name)
        assert a.dtype == np.float32 and a.shape[0] == 4 and np.isfinite(a).all(), (name, a.dtype, a.shape)
    assert sum(os.path.getsize(out / n) for n in names) <= 64e6
