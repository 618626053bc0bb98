"""bench.py's own contract on one GPU: `--steps` is the number of timed steps, `ms_per_step` is their time, `--dump-outputs DIR`
writes what the last timed step returned, and a plain run carries nothing of what only `--full` measures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _line(args, tmp_path):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    return json.loads([ln for ln in r.stdout.split("\n") if ln.startswith("{")][-1])


def test_plain_run_times_the_given_steps_and_dumps_the_last_log_likelihood(tmp_path):
    common = ["--gpus", "1", "--workload", "mg94_64x1250", "--warmup", "2", "--preheat-s", "0"]
    a = _line(common + ["--steps", "5", "--dump-outputs", str(tmp_path / "a")], tmp_path)
    b = _line(common + ["--steps", "7", "--dump-outputs", str(tmp_path / "b")], tmp_path)
    for line, steps, d in ((a, 5, "a"), (b, 7, "b")):
        assert line["steps"] == steps and line["ms_per_step"] > 0
        assert line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-9)
        assert line["value_cold"] is None and "cpu_baseline" not in line and "parity" not in line
        assert line["roofline"]["expm_ms"] is None
        dump = np.load(tmp_path / d / "logl.npy")
        assert dump.dtype == np.float64 and dump.shape == (1,)
        assert dump[0] == line["logl_last"]
    assert a["logl_last"] != b["logl_last"]      # the last timed step's sweep point follows --steps
