"""Camera models without a GPU: csrc/gf_camera_models.hpp -- the header the lift kernel and the tracker's host code compile -- in tests/native/camera_models_host.cpp, a
stand-alone program under the address and undefined-behaviour sanitizers, against the 60-digit values of tests/golden/camera_models.json.gz; the YAML readers on
files written here; gf_camera_model through a C99 compile; gfamd's mirror of it; and gf_estimator_cfg_from_yaml, which keeps refusing what it refused."""
import ctypes as C
import gzip
import json
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "camera_models.json.gz")


def load_fixture():
    return json.loads(gzip.open(GOLDEN).read())


def write_fixture_text(doc, path):
    """the fixture as the native programs read it: lines of hex floats (see tests/native/camera_models_host.cpp)"""
    hx = lambda v: float(v).hex()
    with open(path, "w") as f:
        f.write("eps_d %s\n" % hx(doc["eps_d"]))
        for c in doc["cases"]:
            f.write("case %s %d %s %s %s %d\n" % (c["name"], c["model"], " ".join(hx(v) for v in c["proj"]), " ".join(hx(v) for v in c["dist"]), hx(c["xi"]), len(c["turning"])))
            for t, r in c["turning"]:
                f.write("turn %s %s %s %s\n" % (hx(t[0]), hx(t[1]), hx(r[0]), hx(r[1])))
            for p in c["points"]:
                un = p.get("un", [[0.0, 0.0], [0.0, 0.0]])
                f.write("pt %s %s %d %d %d %s %s\n" % (hx(p["uv"][0]), hx(p["uv"][1]), int(p["double_only"]), int(p["pair_ok"]), p["n_roots"],
                                                   " ".join(hx(v) for hl in p["ray"] for v in hl), " ".join(hx(v) for hl in un for v in hl)))


def test_fixture_is_what_the_issue_describes():
    doc = load_fixture()
    assert os.path.getsize(GOLDEN) < 128 * 1024
    assert doc["eps_d"] == 4 * doc["ref_route_max_err"] and 1e-16 < doc["eps_d"] < 1e-13   # "a few 1e-14" at the most: the reference's own route, times four
    names = [c["name"] for c in doc["cases"]]
    assert names == ["mei_xi1", "mei_xi199_dist", "mei_xi07_nodist", "mei_xi0_dist", "kb_zero", "kb_k2", "kb_k2k3", "kb_k2k3k4", "kb_mono9", "kb_neglead", "kb_wiggle"]
    by = {c["name"]: c for c in doc["cases"]}
    assert by["mei_xi1"]["xi"] == 1.0 and by["mei_xi199_dist"]["xi"] == 1.99 and by["mei_xi07_nodist"]["dist"] == [0, 0, 0, 0] and by["mei_xi0_dist"]["xi"] == 0.0
    assert by["kb_mono9"]["dist"] == [-0.012, 0.006, -0.003, 0.0006] and by["kb_neglead"]["dist"] == [0.02, -0.01, 0.004, -0.05] and by["kb_wiggle"]["dist"] == [-0.9, 0.35, -0.05, 0.0025]
    assert [round(t[0][0], 3) for t in by["kb_neglead"]["turning"]] == [1.112] and [round(t[0][0], 3) for t in by["kb_wiggle"]["turning"]] == [0.734, 1.339]
    for c in doc["cases"]:
        pts = c["points"]
        assert len(pts) == 66 and pts[0]["uv"] == c["proj"][2:] and pts[1]["double_only"] and not any(p["double_only"] for p in pts[2:])
        assert [p["uv"] for p in pts[2:6]] == [[0, 0], [639, 0], [0, 479], [639, 479]]
        assert all(np.float32(v) == v for p in pts[2:] for v in p["uv"])          # float pixels, as the tracker has them
        assert sum(1 for p in pts if not p["pair_ok"]) <= 0.05 * len(pts)
        if c["model"] == 2:
            assert abs(pts[1]["rho"] - 1e-12) < 1e-15                                # the phi = 0 branch
            assert all(min([abs(d) for d in p["switch"]["rho_minus_turning"]] + [1.0]) >= 1e-6 for p in pts[6:])
    assert {p["n_roots"] for p in by["kb_neglead"]["points"]} == {0, 2} and {p["n_roots"] for p in by["kb_wiggle"]["points"]} == {1, 3}


def test_header_meets_the_fixture_under_the_sanitizers(tmp_path):
    exe, txt = tmp_path / "camera_models_host", tmp_path / "camera_models.txt"
    write_fixture_text(load_fixture(), txt)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", str(exe), os.path.join(ROOT, "tests", "native", "camera_models_host.cpp")])
    out = subprocess.run([str(exe), str(txt)], capture_output=True, text=True)
    print(out.stdout[-6000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-3000:]
    assert "all: ok" in out.stdout


def test_struct_layout_in_c99(tmp_path):
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "include/groundfusion_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %d %d %d\\n", sizeof(gf_camera_model), '
                   'offsetof(gf_camera_model, model), offsetof(gf_camera_model, reserved), offsetof(gf_camera_model, proj), offsetof(gf_camera_model, dist), offsetof(gf_camera_model, xi), '
                   'GF_CAMERA_PINHOLE, GF_CAMERA_MEI, GF_CAMERA_KANNALA_BRANDT); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", ROOT, "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["80", "0", "4", "8", "40", "72", "0", "1", "2"]


def test_python_mirror_and_exports():
    import gfamd
    m = gfamd.CameraModel
    assert C.sizeof(m) == 80 and [(n, getattr(m, n).offset) for n, _ in m._fields_] == [("model", 0), ("reserved", 4), ("proj", 8), ("dist", 40), ("xi", 72)]
    assert (gfamd.CAMERA_PINHOLE, gfamd.CAMERA_MEI, gfamd.CAMERA_KANNALA_BRANDT) == (0, 1, 2)
    header = open(os.path.join(ROOT, "include", "groundfusion_hip.h")).read()
    lib = gfamd.lib()
    for fn in ("gf_tracker_set_seq_camera", "gf_tracker_get_seq_camera", "gf_camera_lift_batch", "gf_camera_lift_batch_device", "gf_camera_project_batch", "gf_camera_from_yaml",
               "gf_estimator_cfg_from_yaml_camera", "gf_estimator_set_camera"):
        assert re.search(r"^int %s\(" % fn, header, re.M) and hasattr(lib, fn) and fn in gfamd.EXPORTS, fn
    assert callable(gfamd.FeatureTracker.set_seq_camera) and callable(gfamd.FeatureTracker.get_seq_camera) and callable(gfamd.SlidingWindowEstimator.set_camera)
    # spaceToPlane runs on the host: the fixture's rays project back onto their pixels where the root is unique
    doc = load_fixture()
    for c in doc["cases"]:
        cam = m.make(c["model"], c["proj"], c["dist"], c["xi"])
        pts = [p for p in c["points"] if p["n_roots"] == 1]
        if not pts:
            continue
        uv = gfamd.camera_project([cam], [[[hl[0] for hl in p["ray"]] for p in pts]])[0]
        assert np.abs(uv - np.array([p["uv"] for p in pts])).max() <= 1e-9, c["name"]
    with pytest.raises(gfamd.GfError, match="k3"):
        gfamd.camera_project([m.make("KANNALA_BRANDT", [285, 285, 320, 240], [-0.01, 0.0, 0.0, 1e-4])], [[[0, 0, 1]]])
    with pytest.raises(gfamd.GfError, match="first"):
        bad = np.array([0, 2, 1], np.int32)
        gfamd._chk(lib.gf_camera_project_batch((m * 2)(m.make(0, [1, 1, 0, 0]), m.make(0, [1, 1, 0, 0])), 2, bad.ctypes.data_as(C.POINTER(C.c_int)), None, None))


PINHOLE_YAML = """%YAML:1.0
---
model_type: PINHOLE
camera_name: camera
image_width: 640
image_height: 480
distortion_parameters:
   k1: 0.1
   k2: -0.2
   p1: 0.001
   p2: -0.002
projection_parameters:
   fx: 600.5
   fy: 601.5
   cx: 320.25
   cy: 240.75
"""
MEI_YAML = """%YAML:1.0
---
model_type: MEI
camera_name: camera
image_width: 640
image_height: 480
mirror_parameters:
   xi: 1.25
distortion_parameters:
   k1: -0.1
   k2: 0.02
   p1: 0.0003
   p2: -0.0004
projection_parameters:
   gamma1: 700.5
   gamma2: 701.5
   u0: 321.0
   v0: 239.0
"""
KB_YAML = """%YAML:1.0
---
model_type: KANNALA_BRANDT
camera_name: camera
image_width: 640
image_height: 480
projection_parameters:
   k2: -0.012
   k3: 0.006
   k4: -0.003
   k5: 0.0006
   mu: 285.5
   mv: 286.25
   u0: 320.5
   v0: 240.25
"""
CONFIG_YAML = """%YAML:1.0
imu: 0
wheel: 0
depth: 1
num_of_cam: 1
cam0_calib: "cam.yaml"
image_width: 640
image_height: 480
max_cnt: 150
min_dist: 30
flow_back: 1
max_num_iterations: 8
max_solver_time: 0.04
keyframe_parallax: 10.0
estimate_extrinsic: 0
body_T_cam0: !!opencv-matrix
   rows: 4
   cols: 4
   dt: d
   data: [1, 0, 0, 0,
          0, 1, 0, 0,
          0, 0, 1, 0,
          0, 0, 0, 1]
"""


def test_yaml_readers(tmp_path):
    import gfamd
    files = {}
    for name, text in (("pinhole", PINHOLE_YAML), ("mei", MEI_YAML), ("kb", KB_YAML), ("full", PINHOLE_YAML.replace("PINHOLE", "PINHOLE_FULL")),
                       ("scaramuzza", MEI_YAML.replace("MEI", "SCARAMUZZA")), ("no_mu", KB_YAML.replace("   mu: 285.5\n", "")), ("no_type", PINHOLE_YAML.replace("model_type: PINHOLE\n", "")),
                       ("k3_zero", KB_YAML.replace("k3: 0.006", "k3: 0.0"))):
        files[name] = tmp_path / (name + ".yaml")
        files[name].write_text(text)
    assert gfamd.camera_from_yaml(files["pinhole"]).as_dict() == {"model": 0, "proj": [600.5, 601.5, 320.25, 240.75], "dist": [0.1, -0.2, 0.001, -0.002], "xi": 0.0}
    assert gfamd.camera_from_yaml(files["no_type"]).as_dict() == gfamd.camera_from_yaml(files["pinhole"]).as_dict()
    assert gfamd.camera_from_yaml(files["mei"]).as_dict() == {"model": 1, "proj": [700.5, 701.5, 321.0, 239.0], "dist": [-0.1, 0.02, 0.0003, -0.0004], "xi": 1.25}
    assert gfamd.camera_from_yaml(files["kb"]).as_dict() == {"model": 2, "proj": [285.5, 286.25, 320.5, 240.25], "dist": [-0.012, 0.006, -0.003, 0.0006], "xi": 0.0}
    for name, word in (("full", "PINHOLE_FULL"), ("scaramuzza", "SCARAMUZZA"), ("no_mu", "mu"), ("k3_zero", "k3")):
        with pytest.raises(gfamd.GfError, match=word):
            gfamd.camera_from_yaml(files[name])
    with pytest.raises(gfamd.GfError, match="cannot open"):
        gfamd.camera_from_yaml(tmp_path / "absent.yaml")

    # the estimator's reader: the old entry point keeps its refusal, the new one takes the three models and hands the model back
    (tmp_path / "config.yaml").write_text(CONFIG_YAML)
    for text, model in ((MEI_YAML, 1), (KB_YAML, 2), (PINHOLE_YAML, 0)):
        (tmp_path / "cam.yaml").write_text(text)
        if model:
            with pytest.raises(gfamd.GfError, match="only PINHOLE is built"):
                gfamd.estimator_cfg_from_yaml(tmp_path / "config.yaml")
        old = None if model else gfamd.estimator_cfg_from_yaml(tmp_path / "config.yaml")
        cfg, cam = gfamd.estimator_cfg_from_yaml_camera(tmp_path / "config.yaml")
        assert cam.as_dict() == gfamd.camera_from_yaml(tmp_path / "cam.yaml").as_dict() and cam.model == model
        t = cfg.tracker
        if model:
            assert [t.fx, t.fy, t.cx, t.cy, t.k1, t.k2, t.p1, t.p2] == list(cam.proj) + [0.0] * 4
        else:
            assert bytes(old) == bytes(cfg) and [t.fx, t.fy, t.cx, t.cy, t.k1, t.k2, t.p1, t.p2] == list(cam.proj) + list(cam.dist)
        assert (t.width, t.height, t.max_cnt, t.min_dist, cfg.with_tracker) == (640, 480, 150, 30, 1)
    (tmp_path / "cam.yaml").write_text(PINHOLE_YAML.replace("PINHOLE", "SCARAMUZZA"))
    with pytest.raises(gfamd.GfError, match="SCARAMUZZA"):
        gfamd.estimator_cfg_from_yaml_camera(tmp_path / "config.yaml")
