"""-m gpu: bench.py's plain run -- exactly --steps timed steps in one region, one JSON line whose value and ms_per_step agree, none
of the --full legs, and --dump-outputs writing the same arrays from two runs with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", *extra]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_times_its_steps_and_dumps_repeatable_outputs(tmp_path):
    runs = [_bench("--dump-outputs", str(tmp_path / d)) for d in ("a", "b")]
    for out in runs:
        assert out["metric"] == "ELBO train-step samples/sec" and out["unit"] == "samples/s" and out["higher_is_better"] is True
        assert out["dtype"] == "f32" and out["steps"] == 20 and out["timed_regions"]["count"] == 1
        assert out["ms_per_step"] > 0 and out["value"] == pytest.approx(out["config"]["global_batch"] * 1e3 / out["ms_per_step"], rel=1e-9)
        assert out["roofline"] is None and out["cpu_baseline"] is None
        assert out["per_sample_path"] is None and out["fresh_inputs_each_step"] is None
    names = {"params", "grads", "adam_m", "adam_v", "adam_step"}
    assert {f[:-4] for f in os.listdir(str(tmp_path / "a"))} == names
    for n in names:
        a, b = np.load(str(tmp_path / "a" / f"{n}.npy")), np.load(str(tmp_path / "b" / f"{n}.npy"))
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all()
        np.testing.assert_array_equal(a, b, err_msg=n)
    P = runs[0]["config"]["params"]
    grads = np.load(str(tmp_path / "a" / "grads.npy"))
    assert grads.shape == (P + 4,) and float(grads[P]) == runs[0]["config"]["final_loss"]
