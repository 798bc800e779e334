"""bench.py's command line on the GPU: a plain run times exactly --steps steps, leaves
everything beside the headline to --full, and --dump-outputs writes the last timed step's
outputs (GPU only; one short child process)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def test_plain_run_is_lean_and_dumps_last_step(dev, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                          "--dump-outputs", str(tmp_path / "dump")],
                         capture_output=True, text=True, timeout=300, env=env, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1                                      # ONE result line
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "rays/s" and d["higher_is_better"] is True and d["dtype"] == "f32 (f16x3 emulation)"
    assert d["ms_per_step"] > 0
    assert d["value"] == pytest.approx(1024 / (d["ms_per_step"] * 1e-3), rel=1e-9)
    # one timed pass only: the mode that ran has a time, the other has none
    assert (d["ms_per_step_graph"] is None) != (d["ms_per_step_eager"] is None)
    for key in ("roofline", "cpu_baseline", "alt_gemm", "render_cfg4", "full_cfg3"):
        assert d[key] is None, key                              # measured with --full only
    files = sorted(os.listdir(tmp_path / "dump"))
    assert "loss.npy" in files and "l2_mean.npy" in files
    params = [f for f in files if f.startswith("param.")]
    assert len(params) == 24                                    # the field's twelve linears, weight + bias
    total = 0
    for f in files:
        a = np.load(tmp_path / "dump" / f)
        assert a.dtype == np.float32 and np.isfinite(a).all(), f
        total += a.nbytes
    assert 595_844 * 4 <= total <= 64 * 2 ** 20
    assert float(np.load(tmp_path / "dump" / "loss.npy")) == pytest.approx(d["final_loss"], rel=1e-6)
