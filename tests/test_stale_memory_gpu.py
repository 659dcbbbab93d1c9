"""Nothing the back end returns may depend on device memory the handle has not written itself, nor on what an earlier window left in a slot.

Round 4 found a group member and a stand-alone estimator disagreeing once earlier handles of the process had used the device memory, cured it by zeroing every
buffer at creation and never located the read.  Zeroing makes every handle look like the first one of a process -- it says nothing about a
long-running handle whose buffers hold the PREVIOUS batch's tables.  These tests take both covers away (scripts/stale_probe.py in sub-processes):
  * every fresh device buffer of gf_ba filled with plausible stale data (GF_BA_POISON=4: ordinary doubles, small ints and -1 markers -- what hipMalloc hands back
    behind another handle; 0x5A garbage, GF_BA_POISON=2, turns a stray read into NaN or a crash, plausible data into a slightly different result) must give the
    bits of the zero-initialised run, in every scenario;
  * a window solved / marginalised behind OTHER windows in the same handle (different sizes, factor families, priors; slots that sit batches out, never-packed
    slots) must give the bits of the same window in a fresh handle."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = ["plain", "plain_after", "gnss", "gnss_after", "gnss_thinned", "gnss_thinned_after", "slots", "slots_fresh", "group", "group_gnss"]


def _probe(**env):
    e = dict(os.environ, GF_NO_TORCH_PRELOAD="1")
    for k in ("GF_BA_POISON", "GF_BA_POISON_RANGE", "GF_BA_POISON_ELEMS"):
        e.pop(k, None)
    e.update({k: str(v) for k, v in env.items()})
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "stale_probe.py")] + SCENARIOS, capture_output=True, text=True, cwd=ROOT, env=e)
    assert out.returncode == 0, out.stderr[-1500:]
    res = dict(ln.split() for ln in out.stdout.splitlines() if len(ln.split()) == 2)
    assert sorted(res) == sorted(SCENARIOS), out.stdout
    return res


@pytest.fixture(scope="module")
def zeroed():
    return _probe()


def test_a_window_behind_other_windows_in_the_same_handle_gives_the_same_bits(zeroed):
    assert zeroed["plain_after"] == zeroed["plain"]
    assert zeroed["gnss_after"] == zeroed["gnss"]
    assert zeroed["gnss_thinned_after"] == zeroed["gnss_thinned"]      # a shorter GNSS list behind a longer one in the same slot
    assert zeroed["slots"] == zeroed["slots_fresh"]


@pytest.mark.parametrize("mode", [4, 5, 2])
def test_stale_device_memory_changes_nothing(zeroed, mode):
    """mode 4: plausible stale data (doubles, ints, and each other's bit patterns), mode 5: 0xFF (every double a NaN, every int -1 -- the pattern behind which round 5
    located the read of pri_c: a value "masked" by a multiplication with zero), mode 2: 0x5A garbage in every fresh gf_ba device buffer"""
    got = _probe(GF_BA_POISON=mode)
    moved = [k for k in SCENARIOS if got[k] != zeroed[k]]
    assert not moved, moved
