"""`bench.py --gpus 1 --steps K --warmup W` as the driver runs it: a plain run prints the headline only (the diagnostics are `--full`'s),
`--steps` is the number of timed steps and `ms_per_step` their mean, and `--dump-outputs DIR` writes what the timed step computes from the
seeded initial state.  Two runs see the same inputs, dropout masks and state, so their dumps agree to the rounding of the float atomics
in the backward kernels -- whatever number of steps ran before the dumped one."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILES = ["gradients.npy", "loss.npy", "loss_terms.npy"]


def _bench(out_dir, steps, warmup):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    tail = (r.stdout + r.stderr)[-3000:]
    assert r.returncode == 0, tail
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, tail
    return json.loads(lines[0])


def _load(d):
    files = sorted(os.listdir(d))
    assert files == FILES, files
    assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
    arr = {f[:-4]: np.load(d / f) for f in files}
    for k, v in arr.items():
        assert v.dtype in (np.float32, np.float64) and v.size > 0 and np.isfinite(v).all(), k
    return arr


def _rel(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / np.linalg.norm(b.astype(np.float64)))


def test_plain_run_steps_and_dump(tmp_path):
    out = _bench(tmp_path / "c", 3, 2)
    assert out["steps"] == 3 and len(out["step_series"]["timed_ms"]) == 3 and out["warmup_effective"] >= 2
    assert out["value"] > 0 and abs(out["value"] - 256 / (out["ms_per_step"] * 1e-3)) < 0.02 * out["value"]
    assert out["unit"] == "windows/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert out["roofline"] is None and out["secondary"] is None and out["cpu_baseline"] is None and out["dp"] is None
    c = _load(tmp_path / "c")
    assert c["loss_terms"].shape == (5,) and c["loss"].shape == (1,)
    assert abs(c["loss_terms"][4] - c["loss"][0]) < 1e-4 * max(1.0, abs(c["loss"][0]))  # (the step's loss is terms[4])
    assert c["gradients"].shape == (1 << 22,)  # 11.8 M parameters: the fixed sample
    assert np.count_nonzero(c["gradients"]) > (1 << 21)


def test_same_arguments_same_outputs(tmp_path):
    _bench(tmp_path / "a", 1, 0)
    _bench(tmp_path / "b", 1, 0)
    _bench(tmp_path / "c", 3, 2)
    a, b, c = _load(tmp_path / "a"), _load(tmp_path / "b"), _load(tmp_path / "c")
    # observed between two runs (20 / 5 steps against 20 / 5 and 3 / 2): loss terms 3e-7, gradients 1.0e-4 (relative)
    for other in (b, c):
        assert np.allclose(a["loss_terms"], other["loss_terms"], rtol=1e-5, atol=1e-6), (a["loss_terms"], other["loss_terms"])
        assert _rel(a["gradients"], other["gradients"]) < 2e-3
