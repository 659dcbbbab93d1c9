"""A frame size per sequence in the host bookkeeping, without a GPU: tests/native/seq_size_track_host.cpp runs the CPU tracker of tests/native/track_host.cpp
(the stage functions of csrc/gf_track_host.hpp around the oracle's primitives) for a 64 x 48 sequence with w, h = 64, 48 next to a 640 x 480 neighbour, each
against the oracle's Tracker on frames of its own size, bit for bit; a point at x = 100 is out of border for the small one while the neighbour keeps it.
A stand-alone program under the address and undefined-behaviour sanitizers; nothing is loaded into Python."""
import os
import subprocess

import numpy as np

import roi_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES, RANDOMS = 3, 64
SMALL, LARGE = (64, 48, 30, 3), (640, 480, 150, 30)   # the rows of tests/test_tracker_sizes_gpu.py's SIZES


def _write(path, w, h):
    rng = np.random.default_rng(9)
    with open(path, "wb") as f:
        f.write(np.array([w, h, FRAMES, RANDOMS], np.int32).tobytes())
        f.write(np.stack(RR.frames(w, h, n=FRAMES)).astype(np.uint8).tobytes())
        f.write(np.stack([RR.depth(k, w, h) for k in range(FRAMES)]).tobytes())
        f.write(RR.region("A", w, h).tobytes())
        for _ in range(FRAMES):
            f.write(np.concatenate([rng.random(RANDOMS), rng.random(RANDOMS), rng.normal(0, 1, RANDOMS)]).astype(np.float64).tobytes())
    return str(path)


def test_small_sequence_beside_a_640_wide_neighbour(tmp_path):
    exe = tmp_path / "seq_size_track_host"
    flags = [f for f in RR._makefile_flags() if f not in ("-O3", "-fPIC")]   # the oracle's own: -ffp-contract=off -fno-fast-math decide its bits
    subprocess.check_call([os.environ.get("CXX", "g++")] + flags + ["-O1", "-g", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "oracle"), "-o", str(exe), os.path.join(ROOT, "tests", "native", "seq_size_track_host.cpp"),
                           os.path.join(ROOT, "tests", "roi_tracker_ref.cpp")])
    small, large = _write(tmp_path / "small.bin", *SMALL[:2]), _write(tmp_path / "large.bin", *LARGE[:2])
    out = subprocess.run([str(exe), small, str(SMALL[2]), str(SMALL[3]), large, str(LARGE[2]), str(LARGE[3])], capture_output=True, text=True)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "all: ok" in out.stdout
    assert "the point at x = 100: dropped by the 64-wide sequence, kept by the 640-wide one" in out.stdout
