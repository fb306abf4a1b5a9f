"""GPU: the plain benchmark line (no sub-records of --full) and the outputs it writes with --dump-outputs, at a small size."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_bench_plain_run_times_its_steps_and_dumps_the_last_step(tmp_path):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = tmp_path / "out"
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "2", "--imgsz", "320",
           "--dump-outputs", str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "images/sec" and d["higher_is_better"] is True and d["dtype"] == "bf16"
    # value and ms_per_step describe the same timed steps: images/s = batch / (ms per step)
    assert d["ms_per_step"] > 0 and abs(d["value"] * d["ms_per_step"] / 1e3 - 2) <= 2e-2, d
    assert not {"roofline", "sustained", "forward", "cpu_baseline"} & set(d), sorted(d)
    assert sorted(os.listdir(out)) == ["ema.npy", "loss_items.npy", "model.npy"]
    arrays = {f: np.load(out / f) for f in os.listdir(out)}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["model.npy"].size == arrays["ema.npy"].size > 1 << 20
    np.testing.assert_allclose(arrays["loss_items.npy"], d["loss_items"], rtol=0, atol=1e-4)
