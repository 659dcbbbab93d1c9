"""The track image's outer layers without a GPU: the YAML key, the C-ABI's declarations, the C++ host mirrors, and gf_replay's refusal of --track-images with
--ranks.  (The shared code itself: tests/test_track_draw_host.py; the recording stage: tests/test_track_host_draw.py; the device: tests/test_track_draw_gpu.py.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gf_tracker_set_show_track", "gf_tracker_track_image_some_device", "gf_tracker_track_image", "gf_draw_track_batch", "gf_estimator_set_show_track",
         "gf_estimator_get_track_image", "gf_show_track_from_yaml")


def test_capi_declares_the_track_image_calls():
    import gfamd
    header = open(os.path.join(ROOT, "include", "groundfusion_hip.h")).read()
    for name in NAMES:
        assert name in gfamd.EXPORTS and hasattr(gfamd.lib(), name), name
        at = header.index("int " + name + "(")
        comment = header[header.rindex("/*", 0, at):at]
        assert "feature_tracker.cpp:849-905" in comment or ":1047" in comment, "%s does not cite drawTrack / getTrackImage" % name


@pytest.mark.parametrize("text,want", [("show_track: 1\n", 1), ("show_track: 0           # publish tracking image as topic\n", 0), ("", 0), ("show_track: 1.0\n", 1)])
def test_show_track_from_yaml(tmp_path, text, want):
    import gfamd
    path = tmp_path / "c.yaml"
    path.write_text("%YAML:1.0\n\nimu: 1\nnum_of_cam: 1\n" + text + "max_cnt: 150\n")
    assert gfamd.show_track_from_yaml(str(path)) == want


def test_show_track_from_yaml_refuses_a_missing_file(tmp_path):
    import gfamd
    with pytest.raises(gfamd.GfError, match="cannot open"):
        gfamd.show_track_from_yaml(str(tmp_path / "none.yaml"))


def test_estimator_cfg_is_unchanged_by_the_key(tmp_path):
    """gf_estimator_cfg stays as it is: the same bytes with `show_track: 1` and `show_track: 0` in the exported configuration"""
    import ctypes as C
    import gfamd
    import synth_stream as SS
    st = SS.Stream(1, t_still=0.2, t_move=0.2)
    cfgs = []
    for v in (0, 1):
        d = tmp_path / ("d%d" % v)
        d.mkdir()
        st.export(str(d), n_frames=1, show_track=v, output_path="x")
        assert gfamd.show_track_from_yaml(str(d / "config.yaml")) == v
        cfgs.append(bytes(memoryview(gfamd.estimator_cfg_from_yaml(str(d / "config.yaml"))).cast("B")))
    assert cfgs[0] == cfgs[1] and len(cfgs[0]) == C.sizeof(gfamd.EstimatorCfg)


def test_replay_refuses_track_images_with_ranks(tmp_path):
    exe = os.path.join(ROOT, "bin", "gf_replay")
    assert os.path.exists(exe), "bin/gf_replay is missing: run `python __graft_entry__.py` (build)"
    for line in (["--track-images", str(tmp_path / "out"), "--ranks", "2", "c.yaml", "a", "b"], ["--ranks", "2", "c.yaml", "a", "b", "--track-images", str(tmp_path / "out")]):
        r = subprocess.run([exe] + line, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2 and "--track-images goes with the single-process forms" in r.stderr, r.stderr
    r = subprocess.run([exe, "c.yaml", "a", "--track-images"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--track-images needs a directory" in r.stderr
    assert not (tmp_path / "out").exists()


def test_cpp_host_mirrors_have_the_track_image(tmp_path):
    """host/feature_tracker.h, host/estimator.h and host/replay_node.h compile against the C-ABI with plain g++; before the first frame there is no picture"""
    src = tmp_path / "t.cpp"
    src.write_text('#include <cmath>\n#include "ground-fusion_amd/host/replay_node.h"\n'
                   'int main() { gf::FeatureTracker t; t.setShowTrack(true); std::vector<uint8_t> store; gf::ImageView<uint8_t> v; bool threw = false;\n'
                   '  try { t.getTrackImage(store, v); } catch (const std::runtime_error&) { threw = true; }   /* no frame yet */\n'
                   '  void (gf::Estimator::*f)(bool) = &gf::Estimator::setShowTrack; (void)f;\n'
                   '  void (gf::Estimator::*g)(std::vector<uint8_t>&, gf::ImageView<uint8_t>&) = &gf::Estimator::getTrackImage; (void)g;\n'
                   '  return threw ? 0 : 1; }\n')
    exe = tmp_path / "t"
    lib = os.path.join(ROOT, "ground-fusion_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", ROOT, str(src), "-L", lib, "-lgroundfusion_hip", "-Wl,-rpath," + lib, "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0
