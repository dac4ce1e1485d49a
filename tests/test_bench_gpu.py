"""bench.py's two kinds of run on a small configuration: a plain run reports the timed steps and nothing else, `--full`
adds the legs measured after them (here `--full --lean`: the roofline only)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--arch", "dino_vits16", "--img", "32", "--batch", "64"]
EXTRAS = ("roofline", "cpu_baseline", "parity", "residual_alt", "parity_mode_rate", "dp_proxy", "configs",
          "cls_only_last_block")


def _line(*extra):
    r = subprocess.run([sys.executable, "bench.py", *SMALL, *extra], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_reports_the_timed_steps_only():
    d = _line()
    assert d["metric"] == "images/sec fwd+bwd dino_vits16 32^2 bs=64/GPU" and d["unit"] == "images/sec"
    assert d["higher_is_better"] is True and d["dtype"] == "bf16" and d["steps"] == 3 and d["warmup"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert abs(d["value"] - 64 / d["ms_per_step"] * 1e3) <= 1e-3 * d["value"] + 0.01
    assert {k: d[k] for k in EXTRAS} == dict.fromkeys(EXTRAS)


def test_full_run_adds_the_legs_after_the_timed_steps():
    d = _line("--full", "--lean", "--no-cpu-baseline")
    r = d["roofline"]
    assert r is not None and r["launches_per_step"] > 0 and r["achieved"] > 0
    assert r["step_frac"] == d["step_mfma_frac"]
    assert {k: d[k] for k in EXTRAS if k != "roofline"} == dict.fromkeys(set(EXTRAS) - {"roofline"})
