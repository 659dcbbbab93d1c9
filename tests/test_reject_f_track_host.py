"""rejectWithF in the host bookkeeping, without a GPU: tests/native/reject_f_track_host.cpp runs the CPU tracker of tests/native/track_host.cpp (the stage
functions of csrc/gf_track_host.hpp around the oracle's primitives) twice on a stream in which a patch moves against the scene -- with the switch on, and with it
off but fed a status row edited between LK and after_lk -- and holds the two to each other bit for bit.  Every edit is written out, and held here to the numpy
restatement of tests/reject_f_ref.py.  A stand-alone program under the address and undefined-behaviour sanitizers; nothing is loaded into Python."""
import os
import subprocess

import numpy as np

import reject_f_ref as RF
import roi_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, FRAMES, RANDOMS = 160, 120, 6, 8


def test_stage_on_equals_switch_off_fed_the_restatements_status(tmp_path):
    exe = tmp_path / "reject_f_track_host"
    flags = [f for f in RR._makefile_flags() if f not in ("-O3", "-fPIC")]   # the oracle's own: -ffp-contract=off -fno-fast-math decide its bits
    subprocess.check_call([os.environ.get("CXX", "g++")] + flags + ["-O1", "-g", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "oracle"), "-o", str(exe), os.path.join(ROOT, "tests", "native", "reject_f_track_host.cpp"),
                           os.path.join(ROOT, "tests", "roi_tracker_ref.cpp")])
    path = tmp_path / "frames.bin"
    with open(path, "wb") as f:
        f.write(np.array([W, H, FRAMES, RANDOMS], np.int32).tobytes())
        f.write(np.stack(RF.stream(W, H, FRAMES)).astype(np.uint8).tobytes())
        f.write(np.zeros((FRAMES, H, W), np.uint16).tobytes())
        f.write(np.full((H, W), 255, np.uint8).tobytes())
        f.write(np.zeros(FRAMES * 3 * RANDOMS, np.float64).tobytes())
    dump = tmp_path / "edits.bin"
    out = subprocess.run([str(exe), str(path), "60", "8", "1.0", "5", str(dump)], capture_output=True, text=True)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "all: ok" in out.stdout
    raw = open(dump, "rb").read()
    at, edits, rejected = 0, 0, 0
    while at < len(raw):
        n, seed = int(np.frombuffer(raw, np.int32, 1, at)[0]), int(np.frombuffer(raw, np.uint32, 1, at + 4)[0])
        thr = float(np.frombuffer(raw, np.float64, 1, at + 8)[0])
        at += 16
        pairs = np.frombuffer(raw, np.float32, 4 * n, at).reshape(n, 4)
        at += 16 * n
        before, after = np.frombuffer(raw, np.uint8, n, at), np.frombuffer(raw, np.uint8, n, at + n)
        at += 2 * n
        res = tuple(int(v) for v in np.frombuffer(raw, np.int32, 4, at))
        at += 16
        st, want, _ = RF.reject(pairs, before, thr, seed)
        assert st.tobytes() == after.tobytes() and want == res, "edit %d: the program's status differs from the restatement's (%s, %s)" % (edits, res, want)
        edits += 1
        rejected += res[1]
    assert edits >= FRAMES - 2 and rejected > 0
