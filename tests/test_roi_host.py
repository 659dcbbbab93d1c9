"""The target of the region-of-interest tests, pinned on the CPU: tests/roi_tracker_ref.cpp is the oracle's tracker with setMask starting from a region of
interest R.  It is the yardstick of tests/test_roi_gpu.py, so it is held first to what it must be: the oracle itself, bit for bit, without a region and with an
all-255 one -- with and without prediction / outlier feedback -- and something else with a real one, which never reports a point on an excluded pixel.
No GPU needed."""
import numpy as np
import pytest

import roi_ref as RR


@pytest.fixture(scope="module")
def ref(oracle, tmp_path_factory):
    return RR.build(tmp_path_factory.mktemp("roi_ref"))


def _cfg(oracle, c, **kw):
    return oracle.default_cfg(max_cnt=c[2], min_dist=c[3], **kw)


def _state_same(a, b, what):
    assert all(np.array_equal(x, y) for x, y in zip(a.state(), b.state())), "%s: state differs" % what


@pytest.mark.parametrize("case", RR.SIZES, ids=RR.size_id)
@pytest.mark.parametrize("roi", ["none", "all255"])
def test_helper_without_a_region_is_the_oracle(oracle, ref, case, roi):
    w, h = case[:2]
    otr, rtr = oracle.Tracker(_cfg(oracle, case)), RR.Tracker(ref, _cfg(oracle, case))
    if roi == "all255":
        rtr.set_roi(np.full((h, w), 255, np.uint8))
    for k, f in enumerate(RR.frames(w, h)):
        d = RR.depth(k, w, h)
        RR.same(otr.track(0.0666 * k, f, d), rtr.track(0.0666 * k, f, d), "frame %d" % k)
        _state_same(otr, rtr, "frame %d" % k)
    assert rtr.dropped_outside() == 0


@pytest.mark.parametrize("case", RR.SIZES, ids=RR.size_id)
@pytest.mark.parametrize("name", ["A", "B"])
def test_helper_with_a_region_differs_and_reports_nothing_outside(oracle, ref, case, name):
    w, h, max_cnt = case[:3]
    R = RR.region(name, w, h)
    otr, rtr = oracle.Tracker(_cfg(oracle, case)), RR.Tracker(ref, _cfg(oracle, case))
    rtr.set_roi(R)
    differs, prev, carried = False, None, []
    for k, f in enumerate(RR.frames(w, h)):
        d = RR.depth(k, w, h)
        (oi, oo), (ri, ro) = otr.track(0.0666 * k, f, d), rtr.track(0.0666 * k, f, d)
        differs = differs or not (np.array_equal(oi, ri) and np.array_equal(oo.view(np.uint64), ro.view(np.uint64)))
        assert RR.on_excluded(ro, R) == 0, "frame %d: a point on an excluded pixel" % k
        assert len(set(ri.tolist())) == len(ri)
        if prev is not None:
            carried.append(len(np.intersect1d(ri, prev)))
        prev = ri
    assert differs, "a real region of interest changed nothing"
    # what the GPU tests rely on: the feature is exercised (tracks leave the region) and the sequences are alive (ids carried over)
    print("%dx%d %s: %d tracks dropped outside, fewest ids carried over %d of %d" % (w, h, name, rtr.dropped_outside(), min(carried), max_cnt))
    assert rtr.dropped_outside() >= 1
    assert 3 * min(carried) >= max_cnt


def _feedback(rng, k, cfg, trackers, ids_out):
    """set_prediction / remove_outliers as tests/test_tracker_gpu.py drives them, on every tracker of the list alike (they hold the same state)"""
    rm = ids_out[rng.random(len(ids_out)) < 0.05]
    for tr in trackers:
        tr.remove_outliers(rm)
    ids, _, pts = trackers[0].state()
    sel = rng.random(len(ids)) < 0.7
    noise = 200.0 if k == 3 else 1.0     # frame 3: garbage predictions, most fail and the fallback runs
    uv = pts[sel] + rng.normal(0, noise, (sel.sum(), 2))
    xyz = np.stack([(uv[:, 0] - cfg.cx) / cfg.fx * 2.0, (uv[:, 1] - cfg.cy) / cfg.fy * 2.0, np.full(len(uv), 2.0)], 1)
    for tr in trackers:
        tr.set_prediction(ids[sel], xyz)


@pytest.mark.parametrize("case", [RR.SIZES[0], RR.SIZES[3]], ids=RR.size_id)
@pytest.mark.parametrize("roi", ["none", "all255"])
def test_helper_with_feedback_is_the_oracle(oracle, ref, case, roi):
    """the restated prediction branch and the `< 10` fallback, against the oracle's"""
    w, h = case[:2]
    cfg = _cfg(oracle, case, depth_cam=0)
    otr, rtr = oracle.Tracker(cfg), RR.Tracker(ref, cfg)
    if roi == "all255":
        rtr.set_roi(np.full((h, w), 255, np.uint8))
    rng = np.random.default_rng(9)
    for k, f in enumerate(RR.frames(w, h, seed=3)):
        o, r = otr.track(0.0666 * k, f, None), rtr.track(0.0666 * k, f, None)
        RR.same(o, r, "frame %d" % k)
        _state_same(otr, rtr, "frame %d" % k)
        _feedback(rng, k, cfg, [otr, rtr], o[0])


def test_helper_with_feedback_and_a_region_reports_nothing_outside(oracle, ref):
    case = RR.SIZES[0]
    w, h = case[:2]
    cfg = _cfg(oracle, case, depth_cam=0)
    R = RR.region("A", w, h)
    otr, rtr = oracle.Tracker(cfg), RR.Tracker(ref, cfg)
    rtr.set_roi(R)
    differs = False
    for k, f in enumerate(RR.frames(w, h)):
        o, r = otr.track(0.0666 * k, f, None), rtr.track(0.0666 * k, f, None)
        differs = differs or not np.array_equal(o[0], r[0])
        assert RR.on_excluded(r[1], R) == 0
        for tr, out in ((otr, o), (rtr, r)):   # each tracker is fed back from its own state
            _feedback(np.random.default_rng(100 + k), k, cfg, [tr], out[0])
    assert differs and rtr.dropped_outside() >= 1


def test_capi_declares_the_region_of_interest_calls():
    import gfamd
    for name in ("gf_tracker_set_roi", "gf_tracker_set_roi_some_device", "gf_tracker_get_roi"):
        assert name in gfamd.EXPORTS and hasattr(gfamd.lib(), name)


def test_cpp_host_mirror_takes_a_region_of_interest(tmp_path):
    """host/feature_tracker.h and host/estimator.h: setRegionOfInterest(pointer, stride) compiles against the C-ABI with plain g++; before the first frame the
    tracker class keeps the mask for the handle it creates then, and refuses one while the frame size is unknown"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "t.cpp"
    src.write_text('#include <cmath>\n#include "ground-fusion_amd/host/feature_tracker.h"\n#include "ground-fusion_amd/host/estimator.h"\n'
                   'int main() { std::vector<uint8_t> m(480 * 650, 255); gf::FeatureTracker t; bool threw = false;\n'
                   '  try { t.setRegionOfInterest(m.data(), 650); } catch (const std::runtime_error&) { threw = true; }   /* size unknown */\n'
                   '  t.setIntrinsics(640, 480, 600, 600, 320, 240); t.setRegionOfInterest(m.data(), 650); t.setRegionOfInterest(nullptr, 0);\n'
                   '  bool short_row = false; try { t.setRegionOfInterest(m.data(), 639); } catch (const std::runtime_error&) { short_row = true; }\n'
                   '  void (gf::Estimator::*f)(const uint8_t*, int) = &gf::Estimator::setRegionOfInterest; (void)f;\n'
                   '  return threw && short_row ? 0 : 1; }\n')
    exe = tmp_path / "t"
    lib = os.path.join(root, "ground-fusion_amd", "lib")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", root, str(src), "-L", lib, "-lgroundfusion_hip", "-Wl,-rpath," + lib, "-o", str(exe)])
    assert subprocess.call([str(exe)]) == 0
