"""PINHOLE_FULL and SCARAMUZZA cameras without a GPU: csrc/gf_camera_models.hpp and the PINHOLE_FULL projection of csrc/gf_depth_reg.hpp in
tests/native/camera_wide_host.cpp, a stand-alone program built plain and under the address and undefined-behaviour sanitizers, against
tests/golden/camera_models_wide.json.gz; gf_camera_model_ex through a C99 compile; gfamd's mirror of it; the YAML readers, accepted and refused; the refusals of
the wide checker through the C ABI; and the old entry points, which keep refusing what they refused."""
import ctypes as C
import gzip
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "camera_models_wide.json.gz")
FX = float.fromhex


def load_fixture():
    return json.loads(gzip.open(GOLDEN).read())


def value60(hl):
    import mpmath as mp
    return mp.mpf(FX(hl[0])) + mp.mpf(FX(hl[1]))


def sca_bar(doc):
    """four times the largest deviation of the numpy double route from the 60-digit value over the fixture's SCARAMUZZA projections, computed here from the
    stored values as eps_d is for Kannala-Brandt; checked against the figure the generator stored"""
    import mpmath as mp
    mp.mp.dps = 60
    worst = mp.mpf(0)
    for c in doc["cases"]:
        if c["model"] != 4:
            continue
        for p in c["points"]:
            if p["px60"]:
                for got, want in zip(p["px_d"], p["px60"]):
                    w = value60(want)
                    worst = max(worst, abs(mp.mpf(FX(got)) - w) / max(1, abs(w)))
    assert float(worst) == doc["sca_proj_route_max_err"]
    return 4 * float(worst)


def write_fixture_text(doc, path):
    """the fixture as the native program reads it: lines of hex floats (see tests/native/camera_wide_host.cpp)"""
    hx = lambda v: float(v).hex()
    zeros = lambda n: ["0x0p+0"] * n
    with open(path, "w") as f:
        f.write("bar %s\n" % hx(sca_bar(doc)))
        for c in doc["cases"]:
            nums = c.get("proj", [0] * 4) + c.get("dist", [0] * 8) + [0.0] + c.get("poly", [0] * 5) + c.get("inv_poly", [0] * 20) + c.get("affine", [0] * 5)
            f.write("case %s %d %s\n" % (c["name"], c["model"], " ".join(hx(v) for v in nums)))
            for p in c["points"]:
                r60 = [v for hl in p["ray60"] for v in hl] if p["ray60"] else zeros(6)
                p60 = [v for hl in p["px60"] for v in hl] if p["px60"] else zeros(4)
                f.write("pt %s %d %s %d %s\n" % (" ".join(p["uv"] + p["ray_d"] + p["un_d"] + p["px_d"]), int(bool(p["ray60"])), " ".join(r60), int(bool(p["px60"])), " ".join(p60)))


def test_fixture_is_what_the_issue_describes():
    doc = load_fixture()
    assert os.path.getsize(GOLDEN) < 128 * 1024
    assert [c["name"] for c in doc["cases"]] == ["full_zero", "full_opencv5", "full_kinect8", "full_barrel", "full_pole", "sca_190_identity", "sca_affine", "sca_horizon_inside"]
    assert doc["full_passes"] == 9 and doc["image"] == [640, 480]
    assert 1e-16 < doc["sca_proj_route_max_err"] < 1e-12   # a few ulps of a pixel coordinate of some hundreds, through atan2 and 20 terms
    by = {c["name"]: c for c in doc["cases"]}
    ray = lambda p: [FX(t) for t in p["ray_d"]]
    finite = lambda v: all(math.isfinite(t) for t in v)
    for c in doc["cases"]:
        pts = c["points"]
        uv = [[FX(t) for t in p["uv"]] for p in pts]
        assert uv[:5] == [[320, 240], [0, 0], [639, 0], [0, 479], [639, 479]]                              # the centre pixel and the four corners
        assert all(not (0 <= u <= 639 and 0 <= v <= 479) for u, v in uv[5:8]) and finite(sum(uv[5:8], []))   # well outside the image
        assert any(math.isnan(u) for u, v in uv) and any(u == math.inf for u, v in uv) and any(v == -math.inf for u, v in uv) and any(u == -math.inf for u, v in uv)
        assert len(uv) == doc["n_fixed"] + doc["n_seeded"] + (2 if c["name"] == "full_pole" else 0)
        assert all(np.float32(t) == t for u, v in uv for t in (u, v) if math.isfinite(t))                   # float pixels, as the tracker has them
        for p, (u, v) in zip(pts, uv):
            if not (math.isfinite(u) and math.isfinite(v)):
                assert not finite(ray(p)) and p["ray60"] is None                                            # NaN and the infinities come out non-finite
            if 0 <= u <= 639 and 0 <= v <= 479 and c["name"] != "full_pole":
                assert finite(ray(p)) and p["ray60"] is not None
    assert by["full_zero"]["dist"] == [0] * 8
    d = by["full_opencv5"]["dist"]
    assert all(d[:5]) and d[5:] == [0, 0, 0]                                                                # k1 k2 p1 p2 k3, k4..k6 zero
    d = by["full_kinect8"]["dist"]
    assert all(d) and 0.1 < abs(d[0]) < 2 and 1 < abs(d[1]) < 5 and 0.5 < abs(d[4]) < 3 and 0.1 < abs(d[5]) < 2 and 1 < abs(d[6]) < 5 and 0.5 < abs(d[7]) < 3
    assert by["full_kinect8"]["points"][4]["inv_dist"] < 1e-12                                              # a mild lens: nine passes converge
    assert by["full_barrel"]["points"][4]["inv_dist"] > 1e-6                                                # the ninth iterate at the corner is NOT the inverse
    pole = by["full_pole"]
    assert 1 + pole["dist"][0] * ((576 - pole["proj"][2]) / pole["proj"][0]) ** 2 == 0                      # the denominator crosses zero inside the image
    assert [[FX(t) for t in p["uv"]] for p in pole["points"][13:15]] == [[576, 240], [320, 496 - 0]] and not any(finite(ray(p)) for p in pole["points"][13:15])
    assert by["sca_190_identity"]["affine"][:3] == [1, 0, 0]
    for name in ("sca_190_identity", "sca_affine"):   # 190 degrees: the corner ray is at least 95 degrees from the axis
        x, y, z = ray(by[name]["points"][4])
        assert math.degrees(math.atan2(math.hypot(x, y), z)) >= 94.9
    a = by["sca_affine"]["affine"]
    assert a[0] != 1 and a[1] != 0 and a[2] != 0
    for p in by["sca_affine"]["points"][1:5]:         # the ray is built from the uncorrected xc = p - centre, exactly; xc_a differs from it
        u, v = [FX(t) for t in p["uv"]]
        assert ray(p)[:2] == [u - a[3], v - a[4]]
        inv = 1.0 / (a[0] - a[1] * a[2])
        assert inv * (ray(p)[0] - a[1] * ray(p)[1]) != ray(p)[0]
    signs = {ray(p)[2] > 0 for p, (u, v) in zip(by["sca_horizon_inside"]["points"], [[FX(t) for t in p["uv"]] for p in by["sca_horizon_inside"]["points"]]) if 0 <= u <= 639 and 0 <= v <= 479}
    assert signs == {True, False}                                                                          # points beyond the horizon, inside the image: P.z changes sign


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "sanitizers"])
def test_header_meets_the_fixture(tmp_path, flags):
    exe, txt = tmp_path / "camera_wide_host", tmp_path / "camera_models_wide.txt"
    write_fixture_text(load_fixture(), txt)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-ffp-contract=off"] + flags +
                          ["-o", str(exe), os.path.join(ROOT, "tests", "native", "camera_wide_host.cpp")])
    out = subprocess.run([str(exe), str(txt)], capture_output=True, text=True)
    print(out.stdout[-6000:])
    assert out.returncode == 0, out.stdout[-6000:] + out.stderr[-3000:]
    assert "all: ok" in out.stdout and out.stdout.count("the brute force agrees") == 2


def test_struct_layout_in_c99(tmp_path):
    src, exe = tmp_path / "t.c", tmp_path / "t"
    fields = ["model", "reserved", "proj", "dist", "xi", "poly", "inv_poly", "affine"]
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "include/groundfusion_hip.h"\nint main(void) { printf("%zu %zu ' + "%zu " * len(fields) + '%d %d\\n", '
                   'sizeof(gf_camera_model_ex), sizeof(gf_camera_model), ' + ", ".join("offsetof(gf_camera_model_ex, %s)" % f for f in fields) +
                   ', GF_CAMERA_PINHOLE_FULL, GF_CAMERA_SCARAMUZZA); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", ROOT, "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["352", "80", "0", "4", "8", "40", "104", "112", "152", "312", "3", "4"]


def test_python_mirror_and_exports():
    import gfamd
    m = gfamd.CameraModelEx
    assert C.sizeof(m) == 352 and [(n, getattr(m, n).offset) for n, _ in m._fields_] == [
        ("model", 0), ("reserved", 4), ("proj", 8), ("dist", 40), ("xi", 104), ("poly", 112), ("inv_poly", 152), ("affine", 312)]
    assert (gfamd.CAMERA_PINHOLE_FULL, gfamd.CAMERA_SCARAMUZZA) == (3, 4) and C.sizeof(gfamd.CameraModel) == 80
    header = open(os.path.join(ROOT, "include", "groundfusion_hip.h")).read()
    lib = gfamd.lib()
    for fn in ("gf_tracker_set_seq_camera_ex", "gf_tracker_get_seq_camera_ex", "gf_camera_lift_batch_ex", "gf_camera_lift_batch_device_ex", "gf_camera_project_batch_ex",
               "gf_camera_from_yaml_ex", "gf_estimator_cfg_from_yaml_camera_ex", "gf_estimator_set_camera_ex", "gf_depth_register_batch_ex", "gf_depth_register_batch_device_ex", "gf_tracker_get_camera_lift_stats"):
        assert re.search(r"^int %s\(" % fn, header, re.M) and hasattr(lib, fn) and fn in gfamd.EXPORTS, fn
    assert callable(gfamd.estimator_cfg_from_yaml_camera_ex) and callable(gfamd.FeatureTracker.camera_lift_stats)
    full = m.make("PINHOLE_FULL", [500, 501, 320, 240], [0.1, -0.2, 1e-3, -1e-3, 0.05])
    assert full.as_dict()["dist"] == [0.1, -0.2, 1e-3, -1e-3, 0.05, 0, 0, 0] and full.model == 3
    old = gfamd.CameraModel.make("MEI", [500, 501, 320, 240], [-0.1, 0.01, 0, 0], 1.2)
    wide = m.of(old)
    assert (wide.model, list(wide.proj), list(wide.dist), wide.xi) == (1, list(old.proj), list(old.dist) + [0] * 4, 1.2) and m.of(wide) is wide


def test_projection_on_the_host_and_the_wide_checker_through_the_abi():
    """gf_camera_project_batch_ex runs on the host: the fixture through the C ABI (PINHOLE_FULL: the bits; SCARAMUZZA: the bar), models 0-2 as the old call gives
    them, and the refusals of the wide checker by the name of the field"""
    import gfamd
    doc = load_fixture()
    bar = sca_bar(doc)
    m = gfamd.CameraModelEx
    cams, rays = [], []
    for c in doc["cases"]:
        cams.append(m.make(c["model"], c.get("proj", [0] * 4), c.get("dist", ()), 0.0, c.get("poly", ()), c.get("inv_poly", ()), c.get("affine", ())))
        rays.append(np.array([[FX(t) for t in p["ray_d"]] for p in c["points"]]))
    uv = gfamd.camera_project(cams, rays)
    for c, got in zip(doc["cases"], uv):
        for p, g in zip(c["points"], got):
            want = np.array([FX(t) for t in p["px_d"]])
            if c["model"] == 3:
                ok = np.isfinite(want)
                assert np.array_equal(g[ok].view(np.uint64), want[ok].view(np.uint64)) and not np.isfinite(g[~ok]).any(), (c["name"], p["uv"])
            elif p["px60"]:
                for gi, hl in zip(g, p["px60"]):
                    w = value60(hl)
                    assert abs(gi - w) <= bar * max(1, abs(w)), (c["name"], p["uv"])
    # models 0-2 in the wide struct: the old call's bits; a mixed list is widened as a whole
    old = [gfamd.CameraModel.make("PINHOLE", [600.5, 601.5, 320.25, 240.75], [0.1, -0.2, 1e-3, -2e-3]), gfamd.CameraModel.make("MEI", [700.5, 701.5, 321, 239], [-0.1, 0.02, 3e-4, -4e-4], 1.25),
           gfamd.CameraModel.make("KANNALA_BRANDT", [285.5, 286.25, 320.5, 240.25], [-0.012, 0.006, -0.003, 0.0006])]
    xyz = [np.array([[0.1, -0.2, 1.0], [-0.7, 0.4, 0.9], [0.0, 0.0, 2.0]])] * 3
    a, b = gfamd.camera_project(old, xyz), gfamd.camera_project([m.of(c) for c in old], xyz)
    mixed = gfamd.camera_project(old + [cams[2]], xyz + [xyz[0]])
    for i in range(3):
        assert np.array_equal(a[i].view(np.uint64), b[i].view(np.uint64)) and np.array_equal(a[i].view(np.uint64), mixed[i].view(np.uint64))
    # refusals, by field
    kin, sca = doc["cases"][2], doc["cases"][6]

    def refused(word, **change):
        base = dict(model=change.pop("model", 3), proj=list(kin["proj"]), dist=list(kin["dist"]), xi=0.0, poly=list(sca["poly"]), inv_poly=list(sca["inv_poly"]), affine=list(sca["affine"]))
        reserved = change.pop("reserved", 0)
        for k, (i, v) in change.items():
            base[k][i] = v
        cam = m.make(**base)
        cam.reserved = reserved
        with pytest.raises(gfamd.GfError, match=word):
            gfamd.camera_project([cam], [[[0.1, 0.2, 1.0]]])
    refused("model", model=5)
    refused("model", model=-1)
    refused("reserved", reserved=2)
    refused("fx", proj=(0, 0.0))
    refused("fy", proj=(1, -1.0))
    refused("cx", proj=(2, math.nan))
    refused("k6", dist=(7, math.inf))
    refused("k3", dist=(4, math.nan))
    refused(r"poly\[4\]", model=4, poly=(4, math.nan))
    refused(r"inv_poly\[19\]", model=4, inv_poly=(19, math.inf))
    refused("ae", model=4, affine=(2, math.nan))
    refused(r"ac - ad \* ae", model=4, affine=(0, sca["affine"][1] * sca["affine"][2]))
    # the 80-byte struct still refuses models 3 and 4 wherever it is taken
    for model in (3, 4):
        with pytest.raises(gfamd.GfError, match="model"):
            gfamd.camera_project([gfamd.CameraModel.make(model, [500, 500, 320, 240])], [[[0, 0, 1]]])


FULL_YAML = """%YAML:1.0
---
model_type: PINHOLE_FULL
camera_name: camera
image_width: 640
image_height: 480
distortion_parameters:
   k1: 0.52
   k2: -2.7
   k3: 1.5
   k4: 0.4
   k5: -2.5
   k6: 1.4
   p1: 0.0004
   p2: -0.00015
projection_parameters:
   fx: 504.5
   fy: 504.75
   cx: 322.5
   cy: 241.25
"""
SCA_YAML = """%YAML:1.0
---
model_type: scaramuzza
camera_name: camera
image_width: 640
image_height: 480
poly_parameters:
   p0: -241.5
   p1: 0.0
   p2: 0.0014
   p3: -1.5e-07
   p4: 2.5e-09
inv_poly_parameters:
{inv}
affine_parameters:
   ac: 1.0005
   ad: 0.0002
   ae: -0.0003
   cx: 318.5
   cy: 241.25
""".format(inv="\n".join("   p%d: %r" % (i, 380.0 / (i + 1) ** 3 * (-1) ** i) for i in range(20)))
PINHOLE_YAML = FULL_YAML.replace("PINHOLE_FULL", "PINHOLE")
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
    ex = gfamd.CameraModelEx
    texts = {"full": FULL_YAML, "full_lower": FULL_YAML.replace("PINHOLE_FULL", "pinhole_full"), "sca": SCA_YAML, "sca_upper": SCA_YAML.replace("scaramuzza", "SCARAMUZZA"),
             "sca_mixed": SCA_YAML.replace("scaramuzza", "Scaramuzza"), "pinhole": PINHOLE_YAML, "no_fx": FULL_YAML.replace("   fx: 504.5\n", ""), "no_fy": FULL_YAML.replace("   fy: 504.75\n", ""),
             "no_k5": FULL_YAML.replace("   k5: -2.5\n", ""), "sca_singular": SCA_YAML.replace("ac: 1.0005", "ac: 0.5").replace("ad: 0.0002", "ad: 2.0").replace("ae: -0.0003", "ae: 0.25"), "sca_no_ac": SCA_YAML.replace("   ac: 1.0005\n", "").replace("ad: 0.0002", "ad: 0.0"),
             "unknown": FULL_YAML.replace("PINHOLE_FULL", "PINHOLE_HALF")}
    files = {}
    for name, text in texts.items():
        files[name] = tmp_path / (name + ".yaml")
        files[name].write_text(text)
    want_full = {"model": 3, "proj": [504.5, 504.75, 322.5, 241.25], "dist": [0.52, -2.7, 0.0004, -0.00015, 1.5, 0.4, -2.5, 1.4], "xi": 0.0, "poly": [0.0] * 5, "inv_poly": [0.0] * 20, "affine": [0.0] * 5}
    assert gfamd.camera_from_yaml(files["full"], ex).as_dict() == want_full and gfamd.camera_from_yaml(files["full_lower"], ex).as_dict() == want_full
    want_sca = {"model": 4, "proj": [0.0] * 4, "dist": [0.0] * 8, "xi": 0.0, "poly": [-241.5, 0.0, 0.0014, -1.5e-07, 2.5e-09], "inv_poly": [380.0 / (i + 1) ** 3 * (-1) ** i for i in range(20)],
                "affine": [1.0005, 0.0002, -0.0003, 318.5, 241.25]}
    for name in ("sca", "sca_upper", "sca_mixed"):
        assert gfamd.camera_from_yaml(files[name], ex).as_dict() == want_sca, name
    no_k5 = dict(want_full, dist=[0.52, -2.7, 0.0004, -0.00015, 1.5, 0.4, 0.0, 1.4])     # a missing numeric key reads as 0, as everywhere
    assert gfamd.camera_from_yaml(files["no_k5"], ex).as_dict() == no_k5
    narrow, wide = gfamd.camera_from_yaml(files["pinhole"]), gfamd.camera_from_yaml(files["pinhole"], ex)   # models 0-2: the old reader's numbers in the wide struct
    assert bytes(ex.of(narrow)) == bytes(wide) and wide.model == 0 and list(wide.dist) == [0.52, -2.7, 0.0004, -0.00015, 0, 0, 0, 0]
    for name, word in (("no_fx", "fx"), ("no_fy", "fy"), ("sca_singular", r"ac - ad \* ae"), ("sca_no_ac", r"ac - ad \* ae"), ("unknown", "PINHOLE_HALF")):
        with pytest.raises(gfamd.GfError, match=word):
            gfamd.camera_from_yaml(files[name], ex)
    with pytest.raises(gfamd.GfError, match="cannot open"):
        gfamd.camera_from_yaml(tmp_path / "absent.yaml", ex)
    # the old reader keeps refusing the two models by the name the file gives, and now points at the wide one
    for name, word in (("full", "PINHOLE_FULL"), ("full_lower", "pinhole_full"), ("sca", "scaramuzza"), ("sca_upper", "SCARAMUZZA")):
        with pytest.raises(gfamd.GfError, match=word + ".*gf_camera_from_yaml_ex"):
            gfamd.camera_from_yaml(files[name])

    # the estimator's readers
    (tmp_path / "config.yaml").write_text(CONFIG_YAML)
    for text, model in ((FULL_YAML, 3), (SCA_YAML, 4), (PINHOLE_YAML, 0)):
        (tmp_path / "cam.yaml").write_text(text)
        cfg, cam = gfamd.estimator_cfg_from_yaml_camera_ex(tmp_path / "config.yaml")
        assert cam.as_dict() == gfamd.camera_from_yaml(tmp_path / "cam.yaml", ex).as_dict() and cam.model == model
        t = cfg.tracker
        got = [t.fx, t.fy, t.cx, t.cy, t.k1, t.k2, t.p1, t.p2]
        if model == 3:
            assert got == list(cam.proj) + [0.0] * 4
        elif model == 4:
            assert got == [1.0, 1.0, 318.5, 241.25] + [0.0] * 4
        else:
            old_cfg, old_cam = gfamd.estimator_cfg_from_yaml_camera(tmp_path / "config.yaml")
            assert bytes(old_cfg) == bytes(cfg) and bytes(ex.of(old_cam)) == bytes(cam) and bytes(gfamd.estimator_cfg_from_yaml(tmp_path / "config.yaml")) == bytes(cfg)
        assert (t.width, t.height, t.max_cnt, t.min_dist, cfg.with_tracker) == (640, 480, 150, 30, 1)
        if model:   # the old readers' unchanged refusals
            with pytest.raises(gfamd.GfError, match="only PINHOLE is built"):
                gfamd.estimator_cfg_from_yaml(tmp_path / "config.yaml")
            with pytest.raises(gfamd.GfError, match="PINHOLE_FULL" if model == 3 else "scaramuzza"):
                gfamd.estimator_cfg_from_yaml_camera(tmp_path / "config.yaml")
