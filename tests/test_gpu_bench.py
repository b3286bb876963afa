"""bench.py as a command: a plain run prints the headline line only and
--dump-outputs writes what the timed path returned; the legs behind --full
stay off the plain line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dumped_output(tmp_path):
    B, K = 8, 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", "1",
                        "--batch", str(B), "--settle-ms", "0", "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["metric"] == bench.METRIC and d["unit"] == "seq/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["steps"] == K and d["full"] is False
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(B / d["ms_per_step"] * 1e3, rel=5e-3)  # both are rounded on the line
    for k in ("roofline", "kernel_ms_per_step_event_bracketed", "cpu_baseline", "variant_t75", "exact_fp32",
              "eval_b32", "train_b32"):
        assert k not in d  # --full only
    assert os.listdir(tmp_path) == ["y.npy"]
    y = np.load(tmp_path / "y.npy")
    assert y.dtype == np.float32 and y.shape == (B, 35, 22, 3)
    # the same seeded input through the same call in this process: the same array
    model, opts, _ = bench.load_model("h36m", torch.device("cuda", 0))
    x = bench.synth_input(B, 35, 22, opts["input_time_frame"], 1234).to("cuda:0")
    with torch.no_grad():
        ref = model(x).cpu().numpy()
    np.testing.assert_array_equal(y, ref)
