"""The host bookkeeping of a tracker sequence without a GPU: tests/native/track_host.cpp is a CPU tracker made of the stage functions of csrc/gf_track_host.hpp,
with the oracle's LK, circle and corner primitives in the place of the kernels.  It runs next to the oracle's Tracker (gfo_tracker_*; in the region case tests/roi_tracker_ref.cpp's, which adds
a region of interest) on the frames of tests/roi_ref.py and demands ids, observations, n_out and state bit for bit after every frame.  A stand-alone program under
the address and undefined-behaviour sanitizers; nothing is loaded into Python."""
import os
import subprocess

import numpy as np
import pytest

import roi_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 8
RANDOMS = 512   # per frame and stream; the program walks them modulo this


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("track_host") / "track_host"
    flags = [f for f in RR._makefile_flags() if f not in ("-O3", "-fPIC")]   # the oracle's own: -ffp-contract=off -fno-fast-math decide its bits
    subprocess.check_call([os.environ.get("CXX", "g++")] + flags + ["-O1", "-g", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "oracle"), "-o", str(out), os.path.join(ROOT, "tests", "native", "track_host.cpp"),
                           os.path.join(ROOT, "tests", "roi_tracker_ref.cpp")])
    return str(out)


@pytest.fixture(scope="module")
def frame_file(tmp_path_factory):
    made = {}

    def get(case, seed=0):
        if (case, seed) not in made:
            w, h = case[:2]
            path = tmp_path_factory.mktemp("frames") / ("%dx%d_%d.bin" % (w, h, seed))
            rng = np.random.default_rng(9)
            with open(path, "wb") as f:
                f.write(np.array([w, h, FRAMES, RANDOMS], np.int32).tobytes())
                f.write(np.stack(RR.frames(w, h, n=FRAMES, seed=seed)).astype(np.uint8).tobytes())
                f.write(np.stack([RR.depth(k, w, h) for k in range(FRAMES)]).tobytes())
                f.write(RR.region("A", w, h).tobytes())
                for _ in range(FRAMES):
                    f.write(np.concatenate([rng.random(RANDOMS), rng.random(RANDOMS), rng.normal(0, 1, RANDOMS)]).astype(np.float64).tobytes())
            made[(case, seed)] = str(path)
        return made[(case, seed)]
    return get


SMALL, TINY = RR.SIZES[0], RR.SIZES[2]   # TINY tracks 20 points: the 30 % of them that keep their own pixel as the prediction are fewer than 10
# (size, seed of the frames, options).  The seeds are those of tests/test_roi_host.py (0, and 3 with feedback) where the program's conditions on its own inputs hold
# with them -- tracks carried over, a covered point dropped, the fallback taken, a track dropped by the region -- and another one where they do not.
CASES = {
    "plain": (SMALL, 0, ["flow_back=0", "depth_cam=0", "depth=none"]),
    "flow_back": (SMALL, 0, ["flow_back=1", "depth_cam=0", "depth=none"]),
    "feedback": (TINY, 3, ["feedback=1", "depth_cam=0", "depth=none"]),
    "distortion": (TINY, 3, ["distort=1", "feedback=1", "depth_cam=0", "depth=none"]),
    "depth_in_the_kernels": (SMALL, 0, ["depth_cam=1", "depth=kernel"]),
    "depth_on_the_host": (SMALL, 0, ["depth_cam=1", "depth=host"]),
    "depth_cam_without_an_image": (SMALL, 0, ["depth_cam=1", "depth=none"]),
    "host_depth_without_a_depth_cam": (SMALL, 0, ["depth_cam=0", "depth=host"]),   # the image is not read: every sample is 0
    "region": (SMALL, 0, ["roi=1", "depth_cam=1", "depth=kernel"]),
    "two_sequences": (SMALL, 2, ["two=1", "depth_cam=1", "depth=host"]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_stage_functions_are_the_oracle(exe, frame_file, name):
    case, seed, opts = CASES[name]
    out = subprocess.run([exe, frame_file(case, seed), str(case[2]), str(case[3])] + opts, capture_output=True, text=True)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "all: ok" in out.stdout
