"""The recording stage of the track image without a GPU: tests/native/track_host_draw.cpp runs the CPU tracker of tests/native/track_host.cpp (the library's own
stage functions of csrc/gf_track_host.hpp) with SHOW_TRACK on and prints, for every frame, the state before the call, the state after it and the recorded
primitive list.  Here the list is rebuilt from the two states alone -- a dot per feature at its point, coloured by its track_cnt; an arrow for every feature
whose id was in the state before the call, back to the point it had there -- with tests/track_draw_ref.py, and compared.  Stand-alone, under the sanitizers."""
import os
import subprocess

import numpy as np
import pytest

import roi_ref as RR
import track_draw_ref as TD
from test_track_host import frame_file  # noqa: F401  (the frames file of the sibling test)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("track_host_draw") / "track_host_draw"
    flags = [f for f in RR._makefile_flags() if f not in ("-O3", "-fPIC")]
    subprocess.check_call([os.environ.get("CXX", "g++")] + flags + ["-O1", "-g", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "oracle"), "-o", str(out), os.path.join(ROOT, "tests", "native", "track_host_draw.cpp"),
                           os.path.join(ROOT, "tests", "roi_tracker_ref.cpp")])
    return str(out)


def _frames(text):
    frames = []
    for line in text.splitlines():
        f = line.split()
        if f[0] == "frame":
            frames.append(dict(show=int(f[3]), before={}, after=[], prims=[], removed=0))
        elif f[0] == "before":
            frames[-1]["before"][int(f[1])] = (np.float32(f[2]), np.float32(f[3]))
        elif f[0] == "after":
            frames[-1]["after"].append((int(f[1]), int(f[2]), np.float32(f[3]), np.float32(f[4])))
        elif f[0] == "prim":
            frames[-1]["prims"].append(tuple(int(v) for v in f[1:]))
        elif f[0] == "removed":
            frames[-1]["removed"] = int(f[1])
    return frames


def expected_prims(before, after):
    """the list of DESIGN.md section 4 from the two states: all dots in list order, then three strokes per carried feature"""
    cur = [(a[2], a[3]) for a in after]
    has = [a[0] in before for a in after]
    prev = [before.get(a[0], (0, 0)) for a in after]
    dots = [(TD.rnd(x), TD.rnd(y), 0, 0, 0, TD.C0[min(a[1], 20)], TD.C2[min(a[1], 20)]) for a, (x, y) in zip(after, cur)]
    ss, margin = TD.strokes(cur, prev, has)
    assert margin > 1e-9, "an arrow tip within 1e-9 of a tie of lrint"
    return dots + [s + (1, 0, 255) for s in ss], sum(has)


@pytest.mark.parametrize("on_at,feedback", [(0, 0), (2, 0), (0, 1)], ids=["from_the_start", "switched_on_at_frame_2", "with_removeOutliers_and_setPrediction"])
def test_recorded_list_is_what_the_states_imply(exe, frame_file, on_at, feedback):  # noqa: F811
    case = RR.SIZES[0]
    out = subprocess.run([exe, frame_file(case, 0), str(case[2]), str(case[3]), "on_at=%d" % on_at, "feedback=%d" % feedback], capture_output=True, text=True)
    assert out.returncode == 0 and "all: ok" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    frames = _frames(out.stdout)
    assert len(frames) >= 6
    arrows = new = 0
    for k, f in enumerate(frames):
        if k < on_at:
            assert not f["show"] and not f["prims"]
            continue
        want, carried = expected_prims(f["before"], f["after"])
        assert f["prims"] == want, "frame %d" % k
        if k == 0:
            assert carried == 0 and len(want) == len(f["after"])   # the first frame: dots only
        arrows += carried
        new += len(f["after"]) - carried
    assert arrows >= 50 and new >= 20   # carried and newly detected features both occurred
    if feedback:
        assert sum(f["removed"] for f in frames) >= 10
        # a frame after removeOutliers: the removed ids are in neither state, so they have neither dot nor arrow (checked above); the picture before them stayed (the program's own check)
