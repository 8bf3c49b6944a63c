"""bench.py without --full: the headline step only, its line, and --dump-outputs (the outputs of the last timed step)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=str(tmp_path), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line, k
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["dtype"] == "f32"
    assert line["value"] == pytest.approx(128 * 200 / (line["ms_per_step"] * 1e-3), rel=1e-4)
    for k in ("roofline", "cpu_baseline", "full_length", "cfg5", "plugin_path", "detail"):      # --full only
        assert k not in line, k
    got = {p[:-4]: np.load(out / p) for p in os.listdir(out)}
    assert sorted(got) == ["adam_m", "adam_v", "grads", "params", "step_metrics"]
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got["params"].shape == got["grads"].shape == (2316120,)          # cfg 2: the whole flat buffers
    assert got["step_metrics"][4] == pytest.approx(line["final_total_loss"], rel=1e-4)
