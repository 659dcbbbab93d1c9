"""The list entry points of the tracker (gf_tracker_track_some / _track_some_device / _prefetch_some) on the surfaces a caller sees: the header, the ctypes
binding and the stats structure.  No GPU needed."""
import ctypes as C
import inspect
import os
import re
import subprocess

import gfamd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "groundfusion_hip.h")
ENTRY_POINTS = ("gf_tracker_track_some", "gf_tracker_track_some_device", "gf_tracker_prefetch_some")


def test_header_declares_the_list_entry_points_and_cites_the_reference():
    text = open(HEADER).read()
    for name in ENTRY_POINTS:
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(gf_tracker\* h, int count, const int\* seq," % name, text, re.S)
        assert m, "%s(gf_tracker*, int count, const int* seq, ...) is not declared behind a comment" % name
        assert "feature_tracker.h:47" in m.group(1), "%s does not cite the reference's trackImage" % name
    stats = re.search(r"typedef struct gf_tracker_stats \{(.*?)\} gf_tracker_stats;", text, re.S).group(1)
    members = re.sub(r"/\*.*?\*/", "", stats, flags=re.S)
    assert re.search(r"long long sequence_frames;\s*$", members), "sequence_frames is not the last member of gf_tracker_stats"


def test_binding_exports_them_and_mirrors_the_stats():
    for name in ENTRY_POINTS:
        assert name in gfamd.EXPORTS
    assert gfamd.TrackerStats._fields_[-1] == ("sequence_frames", C.c_longlong)
    ft = gfamd.FeatureTracker
    assert list(inspect.signature(ft.trackImageSome).parameters)[1:4] == ["seqs", "ts", "imgs"]
    assert list(inspect.signature(ft.trackImageSomeDevice).parameters)[1:4] == ["seqs", "ts", "d_gray_ptr"]
    for opt in ("unpack", "out", "n_out"):     # the options of trackImageBatchDevice
        assert opt in inspect.signature(ft.trackImageSomeDevice).parameters and opt in inspect.signature(ft.trackImageBatchDevice).parameters
    assert inspect.signature(ft.prefetchHost).parameters["seqs"].default is None
    assert inspect.signature(ft.trackImage).parameters["seq"].default == 0


def test_library_exports_them():
    lib = C.CDLL(gfamd.LIB_PATH) if os.path.exists(gfamd.LIB_PATH) else None
    assert lib is not None, "build the library first (python __graft_entry__.py)"
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name


def test_stats_structure_has_the_size_the_header_gives_it(tmp_path):
    src = tmp_path / "s.c"
    src.write_text('#include <stdio.h>\n#include "include/groundfusion_hip.h"\nint main(void) { printf("%zu %zu\\n", sizeof(gf_tracker_stats), sizeof(long long)); return 0; }\n')
    exe = tmp_path / "s"
    subprocess.check_call(["gcc", "-I", ROOT, str(src), "-o", str(exe)])
    size, ll = map(int, subprocess.check_output([str(exe)]).split())
    assert C.sizeof(gfamd.TrackerStats) == size
    assert gfamd.TrackerStats.sequence_frames.offset == size - ll
