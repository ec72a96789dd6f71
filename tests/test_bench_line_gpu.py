"""bench.py's line on the GPU: a plain run carries the headline and the dominant kernel's roofline and nothing that needs a run
of its own; --full adds those legs after the same timed steps."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline_conv", "roofline_conv_family", "extra", "cpu_baseline", "cfg4_ms_per_fragment")


def _line(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", *args],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


def test_plain_line_is_the_headline_and_full_adds_its_legs():
    plain = _line()
    assert plain["metric"] == "fragments_per_sec" and plain["unit"] == "fragments/s" and plain["dtype"] == "f32"
    assert plain["higher_is_better"] is True and plain["steps"] == 3 and plain["warmup"] == 1
    assert plain["value"] == pytest.approx(1e3 / plain["ms_per_step"])
    assert plain["roofline"]["avg_launch_ms"] > 0
    assert not [k for k in FULL_ONLY if k in plain]
    full = _line("--full", "--no-extra", "--no-cpu-baseline")
    assert full["roofline_conv"]["launches_timed"] >= 1 and full["roofline_conv_family"]["shapes"] == 30
    assert "extra" not in full and "cpu_baseline" not in full
