"""Stereo depth without a GPU: csrc/gf_stereo_depth.hpp -- the header the kernel, the tracker's host stage and the building blocks compile -- in
tests/native/stereo_depth_host.cpp, a stand-alone program built twice (plain, and under the address and undefined-behaviour sanitizers), held bit for bit against
the numpy restatement of tests/stereo_depth_ref.py, through files; the census of the restatement, which has to show that the cases reach every reason code and
both sides of every gate; planted points, which hold the closed form to a projection it does not contain; the refusals of the check, in the program and through
gf_stereo_depth_batch_host; gf_stereo_depth_cfg through a C99 compile and gfamd's mirror of it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import stereo_depth_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "stereo_depth_host.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-ffp-contract=off"]   # the flags of test_depth_reg_host.py
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
hx = lambda v: float(v).hex()


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("stereo_depth_host")
    out = {}
    for name, extra in (("plain", []), ("sanitized", SANITIZE)):
        exe = d / ("stereo_depth_host_" + name)
        subprocess.check_call([os.environ.get("CXX", "g++")] + FLAGS + extra + ["-o", str(exe), SRC])
        out[name] = str(exe)
    return out


@pytest.fixture(scope="module")
def expected():
    """the restatement on every case, once: name -> (depth_mm, why)"""
    return {c["name"]: ref.depth(c["left"], c["right"], c["cfg"], c["lu"], c["ru"], c["st"]) for c in ref.cases() + [ref.kb_case()]}


def camera_fields(cam):
    return "%d %s" % (ref.MODEL_ID[cam["model"]], " ".join(hx(v) for v in tuple(cam["proj"]) + tuple(cam["dist"]) + (cam["xi"],) + tuple(cam["poly"]) + (0.0,) * 20 + tuple(cam["affine"])))


def cfg_fields(c):
    return "%d %d %s" % (c["enable"], c["right_obs"], " ".join(hx(v) for v in tuple(c["R"]) + tuple(c["t"]) + (c["min_parallax"], c["max_epipolar"], c["min_depth"], c["max_depth"])))


def run_case(exe, c, d):
    case, out = d / (c["name"] + ".txt"), d / (c["name"] + ".out")
    rows = "".join("%s %s %s %s %d\n" % (hx(l[0]), hx(l[1]), hx(r[0]), hx(r[1]), s) for l, r, s in zip(c["lu"], c["ru"], c["st"]))
    case.write_text("%s\n%s\n%s\n%d\n%s" % (camera_fields(c["left"]), camera_fields(c["right"]), cfg_fields(c["cfg"]), len(c["lu"]), rows))
    r = subprocess.run([exe, "run", str(case), str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    census = [int(v) for v in re.search(r"^census (.*)$", r.stdout, re.M).group(1).split()]
    got = np.array([[int(v) for v in line.split()] for line in out.read_text().splitlines()], np.int64).reshape(-1, 2)
    return got[:, 0].astype(np.uint16), got[:, 1].astype(np.uint8), census


def hold_kb(c, mm, why, want_mm, want_why):
    """KANNALA_BRANDT: sin / cos / atan2 differ by library, so within one count, and the same reason wherever the restatement is not within 1e-9 of a gate"""
    far = ~ref.near_a_gate(c)
    assert far.sum() >= 0.9 * len(far)
    assert np.array_equal(why[far], want_why[far])
    both = (why == ref.WHY["ok"]) & (want_why == ref.WHY["ok"])
    assert both.sum() >= 20 and np.abs(mm[both].astype(np.int64) - want_mm[both].astype(np.int64)).max() <= 1


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_header_equals_restatement(programs, expected, tmp_path, build):
    for c in ref.cases():
        mm, why, census = run_case(programs[build], c, tmp_path)
        want_mm, want_why = expected[c["name"]]
        assert np.array_equal(why, want_why), "%s (%s build): reasons differ at %s" % (c["name"], build, np.nonzero(why != want_why)[0][:8])
        assert np.array_equal(mm, want_mm), "%s (%s build): depths differ at %s" % (c["name"], build, np.nonzero(mm != want_mm)[0][:8])
        assert census[1:] == [ref.census(want_why)[k] for k in ("no_match", "lift", "parallax", "behind", "epipolar", "range", "ok")] and census[0] == 0
    c = ref.kb_case()
    mm, why, _ = run_case(programs[build], c, tmp_path)
    hold_kb(c, mm, why, *expected["kb"])


def test_cases_reach_every_reason_and_both_sides_of_every_gate(programs, expected, tmp_path):
    """the census and every gate-boundary expectation below are asserted on what the HEADER returns (the plain build of the stand-alone program), which first has
    to equal the restatement"""
    cases = {c["name"]: c for c in ref.cases()}
    got = {}
    for c in ref.cases():
        mm, why, _ = run_case(programs["plain"], c, tmp_path)
        assert np.array_equal(mm, expected[c["name"]][0]) and np.array_equal(why, expected[c["name"]][1]), c["name"]
        got[c["name"]] = (mm, why)
    expected = dict(got, kb=expected["kb"])
    cen = {n: ref.census(e[1]) for n, e in expected.items()}
    print(cen)
    total = {k: sum(c[k] for n, c in cen.items() if n != "kb") for k in ref.WHY}
    for k in ref.WHY:                                               # every reason code, at least two points each
        assert total[k] >= 2, (k, total)
    ok, W = ref.WHY["ok"], ref.WHY
    only = lambda name: (int(expected[name][0][0]), int(expected[name][1][0]))
    # a rectified rig and one with a rotated, vertically offset right eye; every model without transcendentals on either eye
    assert cases["rect"]["cfg"]["R"] == ref.IDENTITY and cases["rect"]["cfg"]["t"][1] == 0 and cases["tilt_full_mei"]["cfg"]["t"][1] != 0 and cases["tilt_full_mei"]["cfg"]["R"][1] != 0
    eyes = lambda side: {c[side]["model"] for n, c in cases.items() if cen[n]["ok"] >= 20}
    assert eyes("left") >= {"PINHOLE", "PINHOLE_FULL", "MEI", "SCARAMUZZA"} and eyes("right") >= {"PINHOLE", "PINHOLE_FULL", "MEI", "SCARAMUZZA"}
    assert any(v != 0 for v in cases["rect"]["left"]["dist"])       # the pinhole is a distorted one
    # the parallax and epipolar bounds: neighbouring doubles of the gate, one match, the comparison flips between them
    for lo, hi, field, reason in (("parallax_below", "parallax_above", "min_parallax", "parallax"), ("epipolar_above", "epipolar_below", "max_epipolar", "epipolar")):
        a, b = cases[lo]["cfg"][field], cases[hi]["cfg"][field]
        assert b in (np.nextafter(a, np.inf), np.nextafter(a, -np.inf)), (a, b)
        assert only(lo)[1] == ok and only(lo)[0] > 0 and only(hi) == (0, W[reason])
    # half to even: 1000 s == k + 0.5 exactly (the search asserts it), k even stays, k odd goes up; the double below the tie stays at k
    ties = {c["name"]: want for c, want in ref.tie_cases()}
    for name, want in ties.items():
        assert only(name) == (want, ok), (name, only(name), want)
    assert ties["tie_even"] % 2 == 0 and ties["tie_even"] == ties["tie_even_below"] and ties["tie_odd"] % 2 == 0 and ties["tie_odd"] == ties["tie_odd_below"] + 1
    # min_depth / max_depth in counts, and the last count
    assert [int(v) for v in expected["min_2000"][0]] == [0, 2000, 2001] and [int(v) for v in expected["min_2000"][1]] == [W["range"], ok, ok]
    assert [int(v) for v in expected["max_2000"][0]] == [1999, 2000, 0] and [int(v) for v in expected["max_2000"][1]] == [ok, ok, W["range"]]
    assert [int(v) for v in expected["last_count"][0]] == [65535, 0] and [int(v) for v in expected["last_count"][1]] == [ok, W["range"]]
    # P.z <= 0 through MEI and SCARAMUZZA, NaN pixels in either eye, s > 0 with u < 0
    p = ref.parts(cases["lift_mei"]["left"], cases["lift_mei"]["right"], cases["lift_mei"]["cfg"], cases["lift_mei"]["lu"], cases["lift_mei"]["ru"])
    assert p["Pl"][0, 2] <= 0 and np.isfinite(p["Pl"][0]).all() and expected["lift_mei"][1][0] == W["lift"]
    c = cases["lift_sca"]
    p = ref.parts(c["left"], c["right"], c["cfg"], c["lu"], c["ru"])
    assert p["Pr"][0, 2] <= 0 and np.isfinite(p["Pr"][0]).all() and expected["lift_sca"][1][0] == W["lift"]
    assert [int(v) for v in expected["nan"][1]] == [W["lift"], W["lift"], W["lift"], ok]
    c = cases["behind_u"]
    p = ref.parts(c["left"], c["right"], c["cfg"], c["lu"], c["ru"])
    assert (p["s"] > 0).all() and (p["u"] < 0).all() and (expected["behind_u"][1] == W["behind"]).all()
    c = cases["behind_both"]
    p = ref.parts(c["left"], c["right"], c["cfg"], c["lu"], c["ru"])
    assert (p["s"] < 0).all() and (expected["behind_both"][1] == W["behind"]).all()
    assert cen["tilt_mei_full"]["epipolar"] >= 5 and cen["rect"]["no_match"] >= 10 and cen["rect"]["range"] >= 10
    assert [len(cases[n]["lu"]) for n in ("edge_64", "edge_0", "edge_130", "edge_1", "edge_63", "edge_65")] == [64, 0, 130, 1, 63, 65]


# The points of the planted test: seeds and spreads per pair of models.  Nothing had to be moved: with |x / z|, |y / z| <= 0.25 every point of every pair met the
# bar in the restatement as first drawn (PINHOLE's eight passes and PINHOLE_FULL's ninth iterate are converged there to well under a quarter of a millimetre).
PLANTED = [("PINHOLE", ref.PIN, ref.PIN, ref.RECT), ("PINHOLE_FULL / MEI", ref.FULL, ref.MEI, ref.TILT), ("MEI / PINHOLE", ref.MEI, ref.PIN, ref.TILT),
           ("PINHOLE / PINHOLE_FULL", ref.PIN_PLAIN, ref.FULL, ref.RECT)]


def test_planted_points_come_back_to_the_millimetre():
    """independent of the closed form: 3-D points projected into both eyes by the library's host projection; z at millimetre centres plus 0.25 mm, so the depth
    is rint(1000 z) exactly, in the restatement and in the library's host form"""
    import gfamd
    for i, (name, left, right, rig) in enumerate(PLANTED):
        xyz, lu, ru = ref.planted(left, right, rig, 60, 100 + i)
        c = ref.cfg(rig["R"], rig["t"], 10.0)
        want = np.rint(1000.0 * xyz[:, 2]).astype(np.int64)
        assert np.array_equal(want, np.floor(1000.0 * xyz[:, 2]).astype(np.int64)) and want.min() >= 500 and want.max() <= 8000
        mm, why = ref.depth(left, right, c, lu, ru, np.ones(len(lu), np.uint8))
        assert (why == ref.WHY["ok"]).all(), (name, ref.census(why))
        assert np.array_equal(mm.astype(np.int64), want), (name, np.nonzero(mm != want)[0])
        got_mm, got_why = gfamd.stereo_depth_host([ref.gf(left)], [ref.gf(right)], [ref.gf_cfg(c)], [lu], [ru], [np.ones(len(lu), np.uint8)])
        assert np.array_equal(got_mm[0], mm) and np.array_equal(got_why[0], why), name


def test_batch_host_equals_restatement_as_one_batch(expected):
    import gfamd
    cs = ref.cases()
    mm, why = gfamd.stereo_depth_host([ref.gf(c["left"]) for c in cs], [ref.gf(c["right"]) for c in cs], [ref.gf_cfg(c["cfg"]) for c in cs], [c["lu"] for c in cs],
                                      [c["ru"] for c in cs], [c["st"] for c in cs])
    for c, m, w in zip(cs, mm, why):
        assert np.array_equal(m, expected[c["name"]][0]) and np.array_equal(w, expected[c["name"]][1]), c["name"]


def refusals():
    good = ref.cfg(ref.TILT["R"], ref.TILT["t"], 10.0)
    rows = [("ok", good), ("ok", dict(good, right_obs=0)), ("ok", dict(good, max_depth=65.535))]
    rows += [("enable", dict(good, enable=2)), ("enable", dict(good, enable=-1)), ("right_obs", dict(good, right_obs=2)), ("right_obs", dict(good, right_obs=-1))]
    for i in range(9):
        R = list(good["R"]); R[i] = float("nan")
        rows.append(("R[%d]" % i, dict(good, R=R)))
    for i in range(3):
        t = list(good["t"]); t[i] = float("inf")
        rows.append(("t[%d]" % i, dict(good, t=t)))
    for k in ("min_parallax", "max_epipolar", "min_depth", "max_depth"):
        rows += [(k, dict(good, **{k: float("nan")})), (k, dict(good, **{k: float("inf")})), (k, dict(good, **{k: 0.0})), (k, dict(good, **{k: -1.0}))]
    rows.append(("no rotation", dict(good, R=[(1 + 1e-8) * v for v in good["R"]])))        # 2e-8 from orthonormal: refused at 1e-9
    rows.append(("ok", dict(good, R=[(1 + 1e-10) * v for v in good["R"]])))                # 2e-10: accepted
    rows.append(("determinant", dict(good, R=[-v for v in good["R"]])))                    # orthonormal with determinant -1
    rows.append(("t is 0", dict(good, t=(0.0, 0.0, 0.0))))
    rows.append(("min_depth", dict(good, min_depth=10.0)))                                 # min_depth >= max_depth
    rows.append(("min_depth", dict(good, min_depth=11.0)))
    rows.append(("65.535", dict(good, max_depth=65.536)))
    return rows


def test_check_refuses_each_field_by_name(programs):
    rows = refusals()
    text = "".join(cfg_fields(r) + "\n" for _, r in rows)
    for build in ("plain", "sanitized"):
        r = subprocess.run([programs[build], "check"], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(rows)
        for (word, _), line in zip(rows, lines):
            if word == "ok":
                assert line == "ok", line
            else:
                assert line != "ok" and word in line and "gf_stereo_depth_cfg" in line, (word, line)


def test_batch_host_refuses_what_the_setter_refuses():
    """the setter's checks through gf_stereo_depth_batch_host: by name, and nothing written"""
    import gfamd
    lu, ru, st = np.array([[200.0, 130.0]], np.float32), np.array([[190.0, 130.0]], np.float32), np.ones(1, np.uint8)
    for word, c in refusals():
        call = lambda: gfamd.stereo_depth_host([ref.gf(ref.PIN)], [ref.gf(ref.PIN)], [ref.gf_cfg(c)], [lu], [ru], [st])
        if word == "ok":
            mm, why = call()
            assert why[0][0] == ref.WHY["ok"] and mm[0][0] > 0
        else:
            with pytest.raises(gfamd.GfError) as e:
                call()
            assert word in str(e.value) and "set 0" in str(e.value) and "gf_stereo_depth_cfg" in str(e.value), (word, str(e.value))
    bad = gfamd.CameraModelEx.make("PINHOLE", (0.0, 400.0, 160.0, 120.0))
    for left, right, word in ((bad, ref.gf(ref.PIN), "left camera"), (ref.gf(ref.PIN), bad, "right camera")):
        with pytest.raises(gfamd.GfError) as e:
            gfamd.stereo_depth_host([left], [right], [ref.gf_cfg(refusals()[0][1])], [lu], [ru], [st])
        assert word in str(e.value) and "proj[0]" in str(e.value)
    lib = gfamd.lib()
    cam, cf = (gfamd.CameraModelEx * 1)(ref.gf(ref.PIN)), (gfamd.StereoDepthCfg * 1)(ref.gf_cfg(refusals()[0][1]))
    mm, why = np.full(1, 777, np.uint16), np.full(1, 99, np.uint8)
    args = lambda first: (1, first.ctypes.data_as(C.POINTER(C.c_int)), cam, cam, cf, lu.ctypes.data_as(C.POINTER(C.c_float)), ru.ctypes.data_as(C.POINTER(C.c_float)),
                          st.ctypes.data_as(C.POINTER(C.c_uint8)), mm.ctypes.data_as(C.POINTER(C.c_uint16)), why.ctypes.data_as(C.POINTER(C.c_uint8)))
    assert lib.gf_stereo_depth_batch_host(*args(np.array([1, 1], np.int32))) == -1 and b"first[0]" in lib.gf_last_error()
    assert lib.gf_stereo_depth_batch_host(*args(np.array([0, -1], np.int32))) == -1 and b"below" in lib.gf_last_error()
    assert lib.gf_stereo_depth_batch_host(0, *args(np.array([0, 1], np.int32))[1:]) == -1 and b"0 sets" in lib.gf_last_error()
    assert mm[0] == 777 and why[0] == 99                                                   # a refused call writes nothing
    assert lib.gf_stereo_depth_batch_host(*args(np.array([0, 1], np.int32))) == 0 and why[0] == ref.WHY["ok"]


def test_struct_layout_in_c99(tmp_path):
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "include/groundfusion_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n", '
                   'sizeof(gf_stereo_depth_cfg), offsetof(gf_stereo_depth_cfg, enable), offsetof(gf_stereo_depth_cfg, right_obs), offsetof(gf_stereo_depth_cfg, R), '
                   'offsetof(gf_stereo_depth_cfg, t), offsetof(gf_stereo_depth_cfg, min_parallax), offsetof(gf_stereo_depth_cfg, max_epipolar), '
                   'offsetof(gf_stereo_depth_cfg, min_depth), offsetof(gf_stereo_depth_cfg, max_depth), sizeof(gf_stereo_depth_stats), GF_STEREO_DEPTH_NO_MATCH, GF_STEREO_DEPTH_OK); '
                   'return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", ROOT, "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["136", "0", "4", "8", "80", "104", "112", "120", "128", "80", "1", "7"]


def test_python_mirror_and_exports():
    import gfamd
    S = gfamd.StereoDepthCfg
    assert C.sizeof(S) == 136 and (S.enable.offset, S.right_obs.offset, S.R.offset, S.t.offset, S.min_parallax.offset, S.max_epipolar.offset, S.min_depth.offset,
                                   S.max_depth.offset) == (0, 4, 8, 80, 104, 112, 120, 128)
    assert C.sizeof(gfamd.StereoDepthStats) == 80 and [k for k, _ in gfamd.StereoDepthStats._fields_] == ["calls", "launches", "points", "with_depth", "no_match", "lift",
                                                                                                       "parallax", "behind", "epipolar", "range"]
    assert gfamd.STEREO_DEPTH_WHY == ref.WHY
    header = open(os.path.join(ROOT, "include", "groundfusion_hip.h")).read()
    lib = gfamd.lib()
    for fn in ("gf_tracker_set_seq_stereo_depth", "gf_tracker_get_seq_stereo_depth", "gf_tracker_get_stereo_depth_stats", "gf_stereo_depth_batch", "gf_stereo_depth_batch_device",
               "gf_stereo_depth_batch_host"):
        assert re.search(r"^int %s\(" % fn, header, re.M) and hasattr(lib, fn) and fn in gfamd.EXPORTS, fn
    c = ref.gf_cfg(ref.cfg(ref.TILT["R"], ref.TILT["t"], 3.0, right_obs=0))
    assert c.as_dict()["R"] == list(ref.TILT["R"]) and c.as_dict()["t"] == list(ref.TILT["t"]) and c.max_depth == 3.0 and c.right_obs == 0 and c.enable == 1
    assert (c.min_parallax, c.max_epipolar, c.min_depth) == (gfamd.STEREO_DEPTH_MIN_PARALLAX, gfamd.STEREO_DEPTH_MAX_EPIPOLAR, gfamd.STEREO_DEPTH_MIN_DEPTH)
    for name in ("set_seq_stereo_depth", "get_seq_stereo_depth", "stereo_depth_stats"):
        assert hasattr(gfamd.FeatureTracker, name)
    assert callable(gfamd.stereo_depth) and callable(gfamd.stereo_depth_device) and callable(gfamd.stereo_depth_host)
