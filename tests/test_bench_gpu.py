"""bench.py at N = 1 on a small batch: a plain run measures the timed steps and nothing else, `--full` adds the side measurements it names."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what only --full measures at N = 1 (large_batch needs the default batch of 256, other_configs / end_to_end / cpu_baseline are left out below to keep the test short)
FULL_ONLY = ("pcie_inclusive", "small_batch", "large_batch", "large_batch_chain_form", "other_configs", "end_to_end", "end_to_end_one_group",
             "end_to_end_homogeneous", "end_to_end_8_host_threads", "end_to_end_8_host_threads_two_groups", "cpu_baseline")


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8", *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    r = json.loads(lines[0])
    assert r["steps"] == 3 and r["warmup"] == 1 and r["n_gpus"] == 1 and r["higher_is_better"] is True
    assert r["unit"] == "window-solves/s (each with its tracker frame)" and r["value"] > 0
    assert abs(r["value"] * r["ms_per_step"] * 1e-3 - 8) < 1e-6        # 8 window-solves per step
    return r, out.stderr


@pytest.mark.gpu
def test_plain_run_measures_the_timed_steps_only():
    r, err = _bench()
    assert not [k for k in FULL_ONLY if k in r]
    assert r["value_200_steps"] is None and r["gpu_ms_isolated"] == {}
    assert r["roofline_jtj"] is None and r["roofline_step"] is None and r["roofline_jtj_split"] is None
    assert r["roofline"]["frac"] > 0 and r["roofline"]["frac_isolated"] is None       # the LK roofline of the timed region itself stays
    assert "200-step run" not in err and "isolated passes" not in err


@pytest.mark.gpu
def test_full_run_adds_the_side_measurements():
    r, err = _bench("--full", "--no-other-configs", "--no-e2e", "--no-cpu-baseline")
    assert r["value_200_steps"] > 0 and r["gpu_ms_isolated"]["lk_ms"] > 0 and r["roofline"]["frac_isolated"] > 0
    assert r["roofline_jtj"]["frac"] > 0 and r["roofline_step"]["frac"] > 0 and r["roofline_jtj_split"]["launch_ms"] > 0
    assert r["pcie_inclusive"]["steps"] > 0 and sorted(r["small_batch"]) == ["1", "64", "8"]
    assert "large_batch" not in r                          # the default batch of 256 only
    assert "200-step run" in err and "isolated passes" in err
