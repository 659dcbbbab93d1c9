"""gf_stereo_from_yaml on config files the test writes: `num_of_cam: 2` and `cam1_calib` (parameters.cpp:424-436) -> the switch and the right camera.  Host code only.
The setter's own refusals are not here: gf_tracker_set_seq_stereo needs a handle, and gf_tracker_create needs a device (tests/test_stereo_tracker_gpu.py holds them)."""
import os

import pytest

import gfamd

CALIB = """%YAML:1.0
---
model_type: PINHOLE
camera_name: right
image_width: 752
image_height: 480
distortion_parameters:
   k1: -2.8e-01
   k2: 7.4e-02
   p1: 1.9e-04
   p2: 1.8e-05
projection_parameters:
   fx: 457.587
   fy: 456.134
   cx: 379.999
   cy: 255.238
"""


def _config(tmp_path, body, calib=CALIB):
    if calib is not None:
        (tmp_path / "cam1_pinhole.yaml").write_text(calib)
    path = tmp_path / "config.yaml"
    path.write_text("%YAML:1.0\n---\n" + body)
    return str(path)


def test_two_cameras(tmp_path):
    c = gfamd.stereo_from_yaml(_config(tmp_path, 'num_of_cam: 2\ncam0_calib: "cam0_pinhole.yaml"\ncam1_calib: "cam1_pinhole.yaml"\n'))
    assert c.enable == 1 and c.reserved == 0 and c.right.model == gfamd.CAMERA_PINHOLE
    assert list(c.right.proj) == [457.587, 456.134, 379.999, 255.238] and list(c.right.dist)[:4] == [-2.8e-01, 7.4e-02, 1.9e-04, 1.8e-05]


def test_one_camera_reads_no_second_file(tmp_path):
    c = gfamd.stereo_from_yaml(_config(tmp_path, 'num_of_cam: 1\ncam1_calib: "nowhere.yaml"\n', calib=None))
    assert c.enable == 0 and c.right.model == 0 and list(c.right.proj) == [0.0] * 4


def test_refusals_name_the_file_and_the_key(tmp_path):
    with pytest.raises(gfamd.GfError, match="cam1_calib is missing"):
        gfamd.stereo_from_yaml(_config(tmp_path, "num_of_cam: 2\n"))
    with pytest.raises(gfamd.GfError, match="nowhere.yaml"):
        gfamd.stereo_from_yaml(_config(tmp_path, 'num_of_cam: 2\ncam1_calib: "nowhere.yaml"\n'))
    with pytest.raises(gfamd.GfError, match="model_type"):
        gfamd.stereo_from_yaml(_config(tmp_path, 'num_of_cam: 2\ncam1_calib: "cam1_pinhole.yaml"\n', calib=CALIB.replace("PINHOLE", "FISHEYE9")))


def test_declared_and_exported():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "groundfusion_hip.h")).read()
    for name in ("gf_tracker_set_seq_stereo", "gf_tracker_get_seq_stereo", "gf_tracker_get_stereo_stats", "gf_stereo_from_yaml", "gf_stereo_match_batch", "gf_stereo_match_batch_device"):
        assert "int %s(" % name in header and name in gfamd.EXPORTS and hasattr(gfamd.lib(), name), name
