"""A pixel format and an equalise switch per sequence without a GPU: the header's declarations, gfamd's ctypes mirror of gf_tracker_seq_format, the exported
names, and tests/native/seq_format_host.cpp -- the limits of gf_tracker_set_seq_format and the plan of a mixed call (gf_seq_format.hpp) in a stand-alone host
program under the address and undefined-behaviour sanitizers."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "groundfusion_hip.h")
NAMES = ("gf_tracker_set_seq_format", "gf_tracker_get_seq_format", "gf_cvt_gray_mixed_device", "gf_cvt_gray_mixed")


def test_header_declares_the_entry_points_behind_their_citation():
    header = open(HEADER).read()
    for fn in NAMES:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*^int %s\(" % fn, header, re.S | re.M)
        assert m, "%s is not declared behind a comment" % fn
        assert "rosNodeTest.cpp:238" in m.group(1), "%s: the comment in front of it does not cite rosNodeTest.cpp:238" % fn
    assert "one handle per encoding" not in re.sub(r"\s+", " ", header)


def test_ctypes_mirror_of_the_header():
    import gfamd
    header = open(HEADER).read()
    body = re.search(r"typedef struct gf_tracker_seq_format \{(.*?)\} gf_tracker_seq_format;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            ctype, names = decl.split(None, 1)
            fields += [(n.strip(), {"int": C.c_int}[ctype]) for n in names.split(",")]
    assert [n for n, _ in fields] == ["pixel_format", "equalize", "host_stride"]
    assert fields == list(gfamd.TrackerSeqFormat._fields_) and C.sizeof(gfamd.TrackerSeqFormat) == 12
    # the handle's structs stay byte for byte as they were
    assert C.sizeof(gfamd.TrackerCfg) == 7 * 4 + 4 + 8 * 8 + 2 * 4 and gfamd.TrackerStats._fields_[-1][0] == "sequence_frames"


def test_names_are_exported_and_in_the_library():
    import gfamd
    lib = gfamd.lib()
    for name in NAMES:
        assert name in gfamd.EXPORTS and hasattr(lib, name), name
    for name in ("TrackerSeqFormat", "cvt_gray_mixed", "cvt_gray_mixed_device"):
        assert hasattr(gfamd, name), name
    for name in ("set_seq_format", "get_seq_format", "device_frame_offsets"):
        assert hasattr(gfamd.FeatureTracker, name), name


def test_header_compiles_as_c99(tmp_path):
    src = tmp_path / "c99.c"
    src.write_text('#include "groundfusion_hip.h"\nint main(void) { gf_tracker_seq_format f = {GF_PIX_BGR8, 1, 0}; return f.host_stride + (int)sizeof(gf_frame_ref) - 16; }\n')
    subprocess.check_call(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), "-o", str(tmp_path / "c99"), str(src)])
    assert subprocess.run([str(tmp_path / "c99")]).returncode == 0


def test_limits_and_plans_under_the_sanitizers(tmp_path):
    exe = tmp_path / "seq_format_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-o", str(exe), os.path.join(ROOT, "tests", "native", "seq_format_host.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "all: ok" in out.stdout and out.stdout.count(": ok") == 4 and "180 calls" in out.stdout
