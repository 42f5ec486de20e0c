"""GPU: what a plain `bench.py` run does and what it leaves to `--full`.  A plain run sets up, warms up, times its window and prints the line
with the headline keys; the measurements that take runs of their own (CPU baseline, the `also` windows, the box calibration around the
window, the FLF gate cost) appear with `--full` only.  Run on a 2-layer DiT at 9 frames of 64 x 64 (a debug size: the line says so)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--layers", "2", "--frames", "9", "--height", "64", "--width", "64"]
FULL_ONLY = ("cpu_baseline", "also", "also_s", "box_calib_tflops", "value_normalised", "flf_gate_ms")


def _line(extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_line_and_nothing_that_takes_runs_of_its_own():
    out = _line([])
    assert out["unit"] == "steps/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
    assert out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0
    assert abs(out["value"] * out["ms_per_step"] - 1e3) < 1e-6 * 1e3
    assert out["roofline"]["launches"] > 0 and "tracked_body_avg_launch_ms" not in out["roofline"]   # in-window events stay
    assert not [k for k in FULL_ONLY if k in out], sorted(out)


def test_full_run_adds_the_measurements_beside_the_window():
    out = _line(["--full"])   # (the `also` windows belong to the production size and take minutes: not run here)
    assert out["steps"] == 2 and out["warmup"] == 1 and out["value"] > 0
    assert set(out["flf_gate_ms"]) == {"farneback", "tdiff"}
    assert out["box_calib_tflops"]["before"] > 0 and out["box_calib_tflops"]["after"] > 0
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["unit"] == "steps/s"
