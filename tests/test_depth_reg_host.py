"""Depth registration without a GPU: csrc/gf_depth_reg.hpp -- the header the scatter kernel, the tracker's setter and the building blocks compile -- in
tests/native/depth_reg_host.cpp, a stand-alone program built twice (plain, and under the address and undefined-behaviour sanitizers), held byte for byte against
the brute force inside that program and against the numpy restatement of tests/depth_reg_ref.py, through files; the census of the restatement, which has to show
that the cases reach every rule of the definition; the refusals of the check; gf_depth_reg through a C99 compile and gfamd's mirror of it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import depth_reg_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "depth_reg_host.cpp")
FLAGS = ["-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-ffp-contract=off"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
OUTCOMES = ["zero", "behind", "not_finite", "out_of_range", "over_bound", "empty", "writes"]   # gfdreg::Outcome


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("depth_reg_host")
    out = {}
    for name, extra in (("plain", []), ("sanitized", SANITIZE)):
        exe = d / ("depth_reg_host_" + name)
        subprocess.check_call([os.environ.get("CXX", "g++")] + FLAGS + extra + ["-o", str(exe), SRC])
        out[name] = str(exe)
    return out


@pytest.fixture(scope="module")
def expected():
    """the restatement on every case, once: name -> (frame, census)"""
    return {c["name"]: ref.register(c["depth"], c["reg"], c["colour"], c["wc"], c["hc"]) for c in ref.cases()}


def reg_fields(reg):
    hx = lambda v: float(v).hex()
    return "%d %d %s %s %s" % (reg["width"], reg["height"], " ".join(hx(reg[k]) for k in ("fx", "fy", "cx", "cy", "scale")), " ".join(hx(v) for v in reg["R"]), " ".join(hx(v) for v in reg["T"]))


def run_case(exe, c, d):
    case, depth, out = d / (c["name"] + ".txt"), d / (c["name"] + ".depth"), d / (c["name"] + ".out")
    case.write_text("%s %s %d %d\n" % (reg_fields(c["reg"]), " ".join(float(v).hex() for v in c["colour"]), c["wc"], c["hc"]))
    np.ascontiguousarray(c["depth"], "<u2").tofile(str(depth))
    r = subprocess.run([exe, "run", str(case), str(depth), str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and "brute: ok" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    census = [int(v) for v in re.search(r"^census (.*)$", r.stdout, re.M).group(1).split()]
    return np.fromfile(str(out), "<u2").reshape(c["hc"], c["wc"]), dict(zip(OUTCOMES, census))


@pytest.mark.parametrize("build", ["plain", "sanitized"])
def test_header_equals_brute_force_and_restatement(programs, expected, tmp_path, build):
    for c in ref.cases():
        got, census = run_case(programs[build], c, tmp_path)
        want, want_census = expected[c["name"]]
        assert np.array_equal(got, want), "%s (%s build): %d pixels differ from the restatement" % (c["name"], build, int((got != want).sum()))
        assert census == {k: want_census[k] for k in OUTCOMES}, c["name"]


def test_cases_reach_every_rule(expected):
    cen = {n: e[1] for n, e in expected.items()}
    print(cen)
    names = [c["name"] for c in ref.cases()]
    assert names == ["identity", "d435", "down", "behind", "one_count", "torture", "overflow"]
    for c in ref.cases():
        assert 32 <= c["reg"]["width"] <= 64 and 32 <= c["reg"]["height"] <= 48
    ident = ref.cases()[0]
    assert np.array_equal(expected["identity"][0], ident["depth"])                       # the identity returns its input
    assert {1, 40000, 65535} <= set(ident["depth"].reshape(-1).tolist()) and cen["identity"]["zero"] > 0.03 * ident["depth"].size
    assert cen["identity"]["multi_pixel"] == 0 and cen["identity"]["holes"] == cen["identity"]["zero"]
    for k in OUTCOMES + ["clipped", "multi_pixel", "decided", "holes"]:                  # every rule is taken somewhere
        assert any(c[k] > 0 for c in cen.values()), k
    for n in ("d435", "down", "behind"):                                                 # the three cases with a baseline
        assert cen[n]["decided"] >= 10, (n, cen[n])
    assert cen["d435"]["multi_pixel"] > 500                                              # depth is the coarser image there
    assert cen["down"]["multi_pixel"] == 0 and cen["down"]["empty"] > 1000               # ... and the finer one here: most depth pixels cover no colour centre
    assert cen["behind"]["behind"] >= 50
    assert cen["one_count"]["over_bound"] >= 1 and cen["torture"]["over_bound"] >= 1
    assert cen["overflow"]["not_finite"] > 0 and cen["overflow"]["writes"] == 0
    assert cen["d435"]["out_of_range"] >= 1
    tort = ref.cases()[5]
    assert {0, 1, 65535} <= set(tort["depth"].reshape(-1).tolist()) and tort["colour"][4] == -0.3 and cen["torture"]["writes"] > 100


def refusals():
    good = ref.make_reg(48, 40, 42.0, 42.0, 23.7, 19.6, 0.001, ref.rot(0.3, -0.2, 0.1), (0.015, 0.0, 0.0))
    rows = [("ok", good)]
    for k, v, word in (("width", 7, "width"), ("width", 4097, "width"), ("height", 7, "height"), ("height", 4097, "height"), ("fx", 0.0, "fx"), ("fy", -1.0, "fy"),
                       ("scale", 0.0, "scale"), ("fx", float("nan"), "fx"), ("fy", float("inf"), "fy"), ("cx", float("nan"), "cx"), ("cy", float("-inf"), "cy"),
                       ("scale", float("inf"), "scale")):
        rows.append((word, dict(good, **{k: v})))
    for i in range(9):
        R = list(good["R"]); R[i] = float("nan")
        rows.append(("R[%d]" % i, dict(good, R=R)))
    for i in range(3):
        T = list(good["T"]); T[i] = float("inf")
        rows.append(("T[%d]" % i, dict(good, T=T)))
    rows.append(("reflection", dict(good, R=[-v for v in good["R"]])))                    # determinant -1
    rows.append(("no rotation", dict(good, R=[1.001 * v for v in good["R"]])))            # scaled by 1.001
    rows.append(("ok", dict(good, R=[(1 + 1e-8) * v for v in good["R"]])))                # within 1e-6: accepted
    return rows


def test_check_refuses_each_field_by_name(programs):
    rows = refusals()
    text = "".join(reg_fields(r) + "\n" for _, r in rows)
    for build in ("plain", "sanitized"):
        r = subprocess.run([programs[build], "check"], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = r.stdout.splitlines()
        assert len(lines) == len(rows)
        for (word, _), line in zip(rows, lines):
            if word == "ok":
                assert line == "ok", line
            else:
                assert line != "ok" and word in line and "gf_depth_reg" in line, (word, line)


def test_struct_layout_in_c99(tmp_path):
    src, exe = tmp_path / "t.c", tmp_path / "t"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "include/groundfusion_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(gf_depth_reg), '
                   'offsetof(gf_depth_reg, width), offsetof(gf_depth_reg, height), offsetof(gf_depth_reg, fx), offsetof(gf_depth_reg, scale), offsetof(gf_depth_reg, R), '
                   'offsetof(gf_depth_reg, T)); return 0; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", ROOT, "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["144", "0", "4", "8", "40", "48", "120"]


def test_python_mirror_and_exports():
    import gfamd
    assert C.sizeof(gfamd.DepthReg) == 144 and gfamd.DepthReg.R.offset == 48 and gfamd.DepthReg.T.offset == 120 and gfamd.DepthReg.scale.offset == 40
    header = open(os.path.join(ROOT, "include", "groundfusion_hip.h")).read()
    lib = gfamd.lib()
    for fn in ("gf_tracker_set_seq_depth_reg", "gf_tracker_get_seq_depth_reg", "gf_tracker_get_depth_reg_stats", "gf_depth_register_batch", "gf_depth_register_batch_device"):
        assert re.search(r"^int %s\(" % fn, header, re.M) and hasattr(lib, fn) and fn in gfamd.EXPORTS, fn
    r = gfamd.DepthReg.make(48, 40, 42.0, 41.0, 23.0, 19.0, 0.00025, ref.rot(0.1, 0.2, 0.3), (0.015, 0.0, -0.001))
    assert r.as_dict()["R"] == ref.rot(0.1, 0.2, 0.3) and r.scale == 0.00025 and (r.width, r.height) == (48, 40)
    for name in ("set_seq_depth_reg", "get_seq_depth_reg", "depth_reg_stats"):
        assert hasattr(gfamd.FeatureTracker, name)
    assert callable(gfamd.depth_register) and callable(gfamd.depth_register_device)
