"""bench.py's plain run: the result line without the --full measurements, and
--dump-outputs DIR writing the last timed step's outputs as float32 .npy files."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_dumps_last_step_outputs(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    out = tmp_path / "dump"
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--batch", "16", "--steps", "2",
           "--warmup", "1", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0
    assert abs(d["value"] - 16 / (d["ms_per_step"] * 1e-3)) <= 0.01 * d["value"]
    assert d["unit"] == "QA-samples/s" and d["higher_is_better"] is True and d["dtype"] == "fp32"
    # what --full measures in runs of its own is absent from a plain line
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["comm"] is None
    arrays = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(arrays) == {"loss", "logits_concat", "logits_vis", "logits_syb", "mil_nce_obj",
                           "params_sample", "grads_sample"}
    for name, a in arrays.items():
        assert a.dtype == np.float32 and np.isfinite(a).all(), name
    for name in ("logits_concat", "logits_vis", "logits_syb"):
        assert arrays[name].shape == (16, 914) and np.abs(arrays[name]).max() > 0
    assert arrays["loss"].shape == (1,) and abs(float(arrays["loss"][0]) - d["loss"]) < 1e-4
    assert arrays["params_sample"].shape == arrays["grads_sample"].shape
    assert np.count_nonzero(arrays["grads_sample"]) > 0.25 * arrays["grads_sample"].size
    assert sum(a.nbytes for a in arrays.values()) <= 64 * 2 ** 20
