"""Frames by reference (gf_frame_ref; gf_tracker_track_some_device_refs / _track_batch_device_refs / gf_tracker_set_roi_some_device_refs) on the surfaces a
caller sees -- the header, the ctypes binding, the C++ class -- and the rules host and device share (csrc/gf_frame_ref.hpp: what an entry must satisfy, which
load form a frame gets), run on the CPU by tests/native/frame_ref_host.cpp.  No GPU needed."""
import ctypes as C
import inspect
import itertools
import os
import re
import subprocess

import gfamd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "groundfusion_hip.h")
ENTRY_POINTS = ("gf_tracker_track_some_device_refs", "gf_tracker_track_batch_device_refs", "gf_tracker_set_roi_some_device_refs")


def test_header_declares_the_entry_points_and_cites_the_reference():
    text = open(HEADER).read()
    assert re.search(r"typedef struct gf_frame_ref \{ const void\* data; size_t pitch; \} gf_frame_ref;", text)
    for name in ENTRY_POINTS:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(gf_tracker\* h, " % name, text, re.S)
        assert m, "%s(gf_tracker*, ...) is not declared behind a comment" % name
        assert "feature_tracker.h:47" in m.group(1), "%s does not cite the reference's trackImage" % name
    stats = re.search(r"typedef struct gf_tracker_stats \{(.*?)\} gf_tracker_stats;", text, re.S).group(1)
    members = re.sub(r"/\*.*?\*/", "", stats, flags=re.S)
    assert re.search(r"long long frames_unaligned;", members) and re.search(r"long long sequence_frames;\s*$", members)
    assert "tight height x width x bytes per pixel, back to back in list order." not in text, "the header still says device frames must be tight and back to back"


def test_binding_mirrors_the_structures(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "include/groundfusion_hip.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(gf_frame_ref), '
                   'offsetof(gf_frame_ref, pitch), sizeof(gf_tracker_stats), offsetof(gf_tracker_stats, frames_unaligned)); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", ROOT, str(src), "-o", str(exe)])
    ref_size, pitch_at, stats_size, counter_at = map(int, subprocess.check_output([str(exe)]).split())
    assert C.sizeof(gfamd.FrameRef) == ref_size == 16 and gfamd.FrameRef.pitch.offset == pitch_at == 8
    assert C.sizeof(gfamd.TrackerStats) == stats_size and gfamd.TrackerStats.frames_unaligned.offset == counter_at
    assert gfamd.TrackerStats._fields_[-1] == ("sequence_frames", C.c_longlong)
    t = gfamd.frame_refs([(4096, 640), None, (0, 7)])
    assert (t[0].data, t[0].pitch, t[1].data, t[1].pitch, t[2].data, t[2].pitch) == (4096, 640, None, 0, None, 7)


def test_binding_and_library_export_them():
    lib = gfamd.lib()
    for name in ENTRY_POINTS:
        assert name in gfamd.EXPORTS and hasattr(lib, name), name
    ft = gfamd.FeatureTracker
    assert list(inspect.signature(ft.trackImageSomeDeviceRefs).parameters)[1:5] == ["seqs", "ts", "gray_refs", "depth_refs"]
    assert inspect.signature(ft.trackImageSomeDeviceRefs).parameters["depth_refs"].default is None
    assert list(inspect.signature(ft.trackImageBatchDeviceRefs).parameters)[1:4] == ["ts", "gray_refs", "depth_refs"]
    assert list(inspect.signature(ft.set_roi_device_refs).parameters)[1:3] == ["seqs", "mask_refs"]
    for opt in ("unpack", "out", "n_out"):
        assert opt in inspect.signature(ft.trackImageSomeDeviceRefs).parameters and opt in inspect.signature(ft.trackImageBatchDeviceRefs).parameters


def test_null_handle_is_refused_without_a_device():
    lib = gfamd.lib()
    table = gfamd.frame_refs([(4096, 640)])
    seq, t, n = (C.c_int * 1)(0), (C.c_double * 1)(0.0), (C.c_int * 1)(0)
    out = (gfamd.FeatureObs * 4)()
    assert lib.gf_tracker_track_some_device_refs(None, 1, seq, t, table, None, out, 4, n) == -1 and b"null handle" in lib.gf_last_error()
    assert lib.gf_tracker_track_batch_device_refs(None, t, table, None, out, 4, n) == -1 and b"null handle" in lib.gf_last_error()
    assert lib.gf_tracker_set_roi_some_device_refs(None, 1, seq, table) == -1 and b"null handle" in lib.gf_last_error()
    assert lib.gf_tracker_set_roi_some_device_refs(None, 1, seq, None) == -1


def _model(data, pitch, row, u16, may_null):
    """the rules as the issue states them, written down a second time"""
    if data == 0:
        verdict = 0 if may_null else 1
    elif pitch < row:
        verdict = 2
    elif u16 and (data % 2 or pitch % 2):
        verdict = 3
    else:
        verdict = 0
    form = 16 if data % 16 == 0 and pitch % 16 == 0 else 4 if data % 4 == 0 and pitch % 4 == 0 else 1
    return verdict, form, int(form < 16), int(form < 4)


def test_checks_and_form_selection_on_the_cpu(tmp_path):
    exe = tmp_path / "frame_ref_host"
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "native", "frame_ref_host.cpp"), "-o", str(exe)])
    base = 1 << 33      # addresses beyond 32 bits, as device pointers are
    cases = [(d, p, r, u, m) for d, p, r, u, m in itertools.product(
        [0, base, base + 1, base + 2, base + 4, base + 8, base + 16, base + 20, base + 257], [0, 1, 639, 640, 641, 642, 644, 656, 677, 768, 1280, 1281, 1282, (1 << 32) + 16],
        [640, 1280], [0, 1], [0, 1])]
    text = "".join("%d %d %d %d %d\n" % c for c in cases)
    got = subprocess.run([str(exe)], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    assert len(got) == len(cases) + 1
    for c, line in zip(cases, got):
        assert tuple(map(int, line.split())) == _model(*c), c
    seen = {_model(*c)[0] for c in cases}, {_model(*c)[1] for c in cases}
    assert seen == ({0, 1, 2, 3}, {1, 4, 16})


def test_cpp_host_mirror_takes_a_frame_reference(tmp_path):
    """host/feature_tracker.h: the trackImage overload on gf_frame_ref compiles against the C-ABI with plain g++, next to the overload on host images, and refuses
    a frame while the size is unknown (a device pointer carries none)"""
    src = tmp_path / "t.cpp"
    src.write_text('#include <cmath>\n#include "ground-fusion_amd/host/feature_tracker.h"\n'
                   'int main() { gf::FeatureTracker t; bool threw = false; gf_frame_ref img{reinterpret_cast<const void*>(4096), 640}, none{nullptr, 0};\n'
                   '  try { t.trackImage(0.0, img, none); } catch (const std::runtime_error&) { threw = true; }   /* size unknown */\n'
                   '  gf::FeatureFrame (gf::FeatureTracker::*a)(double, const gf_frame_ref&, const gf_frame_ref&, int) = &gf::FeatureTracker::trackImage; (void)a;\n'
                   '  gf::FeatureFrame (gf::FeatureTracker::*b)(double, const gf::GrayImage&, const gf::DepthImage&) = &gf::FeatureTracker::trackImage; (void)b;\n'
                   '  return threw ? 0 : 1; }\n')
    exe = tmp_path / "t"
    lib = os.path.join(ROOT, "ground-fusion_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", ROOT, str(src), "-L", lib, "-lgroundfusion_hip", "-Wl,-rpath," + lib, "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0
