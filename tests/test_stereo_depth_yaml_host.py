"""gf_stereo_depth_from_yaml and gf_estimator_cfg_from_yaml_stereo on config files the test writes: `num_of_cam: 2` with body_T_cam0 / body_T_cam1
(parameters.cpp:445-463) -> the rig inverse(body_T_cam0) * body_T_cam1, depth_threshold as max_depth, the default gates; the old readers keep refusing two cameras.
Host code only."""
import os

import numpy as np
import pytest

import gfamd
import stereo_depth_ref as ref
from test_camera_wide_host import CONFIG_YAML, FULL_YAML, PINHOLE_YAML


def _mat(name, R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = np.asarray(R).reshape(3, 3), t
    return "%s: !!opencv-matrix\n   rows: 4\n   cols: 4\n   dt: d\n   data: [%s]\n" % (name, ", ".join(repr(float(v)) for v in T.reshape(-1)))


R0, T0 = ref.rot(0.02, -0.01, 0.03), (0.01, 0.02, -0.03)
R1, T1 = ref.rot(0.025, -0.02, 0.028), (0.06, 0.021, -0.031)


def _config(tmp_path, num_of_cam=2, depth_threshold=3, cam1=True):
    body = CONFIG_YAML.replace("num_of_cam: 1", "num_of_cam: %d" % num_of_cam)
    body = body[:body.index("body_T_cam0")] + _mat("body_T_cam0", R0, T0) + (_mat("body_T_cam1", R1, T1) if cam1 else "")
    body += 'cam1_calib: "cam1.yaml"\ndepth_threshold: %d\n' % depth_threshold
    (tmp_path / "cam.yaml").write_text(PINHOLE_YAML)
    (tmp_path / "cam1.yaml").write_text(FULL_YAML)
    path = tmp_path / "config.yaml"
    path.write_text(body)
    return str(path)


def test_two_cameras_give_the_rig_and_the_default_gates(tmp_path):
    c = gfamd.stereo_depth_from_yaml(_config(tmp_path))
    A, B = np.asarray(R0).reshape(3, 3), np.asarray(R1).reshape(3, 3)
    assert c.enable == 1 and c.right_obs == 1
    assert np.abs(np.asarray(c.R).reshape(3, 3) - A.T @ B).max() < 1e-12 and np.abs(np.asarray(c.t) - A.T @ (np.asarray(T1) - np.asarray(T0))).max() < 1e-12
    assert (c.min_parallax, c.max_epipolar, c.min_depth, c.max_depth) == (1e-3, 10.0 / 460.0, 0.1, 3.0)
    assert (gfamd.STEREO_DEPTH_MIN_PARALLAX, gfamd.STEREO_DEPTH_MAX_EPIPOLAR, gfamd.STEREO_DEPTH_MIN_DEPTH) == (1e-3, 10.0 / 460.0, 0.1)
    # what the setter checks, the reader has checked: the configuration passes the building block
    mm, why = gfamd.stereo_depth_host([ref.gf(ref.PIN_PLAIN)], [ref.gf(ref.PIN_PLAIN)], [c], [[[200.0, 130.0]]], [[[186.0, 130.0]]], [[1]])
    assert why[0][0] in ref.NAMES


def test_one_camera_is_switched_off(tmp_path):
    c = gfamd.stereo_depth_from_yaml(_config(tmp_path, num_of_cam=1, cam1=False))
    assert bytes(c) == bytes(gfamd.StereoDepthCfg())


def test_refusals_name_the_key_or_the_field(tmp_path):
    with pytest.raises(gfamd.GfError, match="body_T_cam1"):
        gfamd.stereo_depth_from_yaml(_config(tmp_path, cam1=False))
    with pytest.raises(gfamd.GfError, match="max_depth.*depth_threshold"):
        gfamd.stereo_depth_from_yaml(_config(tmp_path, depth_threshold=0))
    with pytest.raises(gfamd.GfError, match="65.535"):
        gfamd.stereo_depth_from_yaml(_config(tmp_path, depth_threshold=66))


def test_estimator_reader_accepts_two_cameras_and_the_old_ones_keep_refusing(tmp_path):
    path = _config(tmp_path)
    cfg, left, st, sd = gfamd.estimator_cfg_from_yaml_stereo(path)
    assert cfg.depth == 1 and cfg.tracker.depth_cam == 0 and cfg.with_tracker == 1 and cfg.depth_threshold == 3
    assert left.model == gfamd.CAMERA_PINHOLE and st.enable == 1 and st.right.model == gfamd.CAMERA_PINHOLE_FULL
    assert bytes(sd) == bytes(gfamd.stereo_depth_from_yaml(path)) and bytes(st) == bytes(gfamd.stereo_from_yaml(path))
    for reader in (gfamd.estimator_cfg_from_yaml, gfamd.estimator_cfg_from_yaml_camera, gfamd.estimator_cfg_from_yaml_camera_ex):
        with pytest.raises(gfamd.GfError, match=r"num_of_cam must be 1 \(RGB-D\), got 2"):
            reader(path)
    one = _config(tmp_path, num_of_cam=1, cam1=False)
    cfg1, left1, st1, sd1 = gfamd.estimator_cfg_from_yaml_stereo(one)
    ref_cfg, ref_cam = gfamd.estimator_cfg_from_yaml_camera_ex(one)
    assert bytes(cfg1) == bytes(ref_cfg) and bytes(left1) == bytes(ref_cam) and st1.enable == 0 and sd1.enable == 0 and cfg1.tracker.depth_cam == 1


def test_declared_and_exported():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "groundfusion_hip.h")).read()
    for name in ("gf_stereo_depth_from_yaml", "gf_estimator_set_stereo_depth", "gf_estimator_input_image_refs", "gf_estimator_cfg_from_yaml_stereo"):
        assert "int %s(" % name in header and name in gfamd.EXPORTS and hasattr(gfamd.lib(), name), name
    for name in ("set_stereo_depth", "inputImageRefs"):
        assert hasattr(gfamd.SlidingWindowEstimator, name)
    for path, words in (("feature_tracker.h", ("setStereoDepth", "const gf_stereo_depth_cfg& rig")), ("estimator.h", ("setStereoDepth", "gf_estimator_input_image_refs"))):
        text = open(os.path.join(os.path.dirname(gfamd.__file__), "host", path)).read()
        assert all(w in text for w in words), path
