"""Exclusion boxes without a GPU.  tests/native/roi_boxes_host.cpp holds the shared functions of csrc/gf_roi.hpp (the table word under a box list, the point test of
setMask's walk) and the frame primitive of csrc/gf_track_draw.hpp to brute force on the hard lists of tests/roi_boxes_ref.py; a stand-alone program under the
address and undefined-behaviour sanitizers, nothing is loaded into Python.  Then the header, the binding and the refusals that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import roi_boxes_ref as BR
import roi_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("roi_boxes_host") / "roi_boxes_host"
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(out), os.path.join(ROOT, "tests", "native", "roi_boxes_host.cpp")])
    return str(out)


@pytest.mark.parametrize("size", BR.HOST_SIZES, ids=lambda s: "%dx%d" % s)
def test_shared_functions_against_brute_force(exe, tmp_path, size):
    w, h = size
    lists = BR.hard_lists(w, h)
    assert len(lists["cap"]) == BR.CAP and lists["none"] == []
    path = tmp_path / "lists.bin"
    with open(path, "wb") as f:
        f.write(np.array([w, h, len(lists)], np.int32).tobytes())
        for l in lists.values():
            f.write(np.array([len(l)], np.int32).tobytes())
            f.write(np.array(l, np.int64).reshape(-1, 4).astype(np.int32).tobytes())
        f.write(RR.region("A", w, h).tobytes())
        f.write(RR.region("B", w, h).tobytes())
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "all: ok" in out.stdout


def test_python_raster_is_the_per_pixel_statement():
    """tests/roi_boxes_ref.py's slices against the definition, pixel by pixel, at the smallest size"""
    w, h = 64, 61
    for name, l in BR.hard_lists(w, h).items():
        R = BR.raster(l, w, h, RR.region("B", w, h))
        base = RR.region("B", w, h)
        for y in range(0, h, 3):
            for x in range(0, w, 3):
                inside = any(b[0] <= x <= b[2] and b[1] <= y <= b[3] for b in l)
                assert R[y, x] == (0 if inside or base[y, x] == 0 else 255), (name, x, y)


def test_header_is_plain_c_and_a_box_is_16_bytes(tmp_path):
    import gfamd
    src = tmp_path / "t.c"
    src.write_text('#include "include/groundfusion_hip.h"\ntypedef char box_is_16[sizeof(gf_box) == 16 ? 1 : -1];\n'
                   "int main(void) { gf_box b = {1, 2, 3, 4}; box_is_16 c; (void)c; return GF_MAX_BOXES_PER_SEQ >= 256 && b.xmin == 1 ? 0 : 1; }\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-fsyntax-only", "-I", ROOT, str(src)])
    assert C.sizeof(gfamd.Box) == 16 and gfamd.MAX_BOXES_PER_SEQ >= 256
    hdr = open(os.path.join(ROOT, "include", "groundfusion_hip.h")).read()
    assert "#define GF_MAX_BOXES_PER_SEQ %d" % gfamd.MAX_BOXES_PER_SEQ in hdr
    assert "sizeof(gf_box) == 16" in hdr


def test_exports_and_refusals_without_a_device():
    import gfamd
    L = gfamd.lib()
    for name in ("gf_tracker_set_boxes_some", "gf_tracker_get_boxes", "gf_roi_boxes_batch", "gf_estimator_set_boxes", "gf_draw_track_boxes_batch"):
        assert name in gfamd.EXPORTS and hasattr(L, name), name
    seq, first, n = (C.c_int * 1)(0), (C.c_int * 2)(0, 1), C.c_int(0)
    box = (gfamd.Box * 1)(gfamd.Box(1, 2, 3, 4))
    assert L.gf_tracker_set_boxes_some(None, 1, seq, first, box) == -1 and b"null handle" in L.gf_last_error()
    assert L.gf_tracker_get_boxes(None, 0, box, 1, C.byref(n)) == -1
    assert L.gf_estimator_set_boxes(None, box, 1) == -1 and b"without a tracker" in L.gf_last_error()
    out = np.zeros((4, 4), np.uint8)
    p = out.ctypes.data_as(C.POINTER(C.c_uint8))
    assert L.gf_roi_boxes_batch(1, 4, 4, (C.c_int * 2)(1, 1), box, None, p) == -1     # first[0] != 0
    assert L.gf_roi_boxes_batch(1, 4, 4, (C.c_int * 2)(0, 300), box, None, p) == -1   # longer than the cap
    assert L.gf_roi_boxes_batch(0, 4, 4, first, box, None, p) == -1


def test_replay_tool_refuses_a_malformed_boxes_file(tmp_path):
    exe = os.path.join(ROOT, "bin", "gf_replay")
    assert os.path.exists(exe), "bin/gf_replay is missing: run `python __graft_entry__.py` (build)"
    bad = tmp_path / "boxes.txt"
    bad.write_text("0.5 1 2 3 4\n0.6 1 2 3\n")
    r = subprocess.run([exe, "--boxes", str(bad), "config.yaml", "nowhere"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--boxes" in r.stderr and "line 2" in r.stderr, r.stderr
    late = tmp_path / "late.txt"
    late.write_text("0.5 1 2 3 4\n\n0.4 1 2 3 4\n")
    r = subprocess.run([exe, "--boxes", str(late), "config.yaml", "nowhere"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "line 3" in r.stderr, r.stderr
    r = subprocess.run([exe, "--ranks", "2", "--boxes", str(bad), "config.yaml", "nowhere"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--boxes" in r.stderr, r.stderr
