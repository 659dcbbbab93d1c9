"""rejectWithF on the device (csrc/gf_reject_f_kernels.hpp) against the restatement of tests/reject_f_ref.py, byte for byte, and the tracker with the stage
on against the same tracker fed by the host form.  No tolerance anywhere."""
import os

import numpy as np
import pytest

import reject_f_ref as RF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(name, st, res, ref):
    want_st, want_res, _ = ref
    assert st.tobytes() == want_st.tobytes(), "%s: %d status bytes differ from the restatement" % (name, int((st != want_st).sum()))
    assert (res["m"], res["rejected"], res["winner"], res["inliers"]) == want_res, (name, res, want_res)


def test_building_block_one_batch_of_different_m():
    import gfamd
    ref, cases = RF.reference(), RF.cases()
    names = list(cases)
    st, res = gfamd.reject_f([cases[n][0] for n in names], [cases[n][1] for n in names], [cases[n][2] for n in names])
    for k, n in enumerate(names):
        _same(n, st[k], res[k], ref[n])


@pytest.mark.parametrize("name", list(RF.cases()))
def test_building_block_each_case_alone(name):
    import gfamd
    pairs, thr, seed = RF.cases()[name]
    st, res = gfamd.reject_f([pairs], thr, seed)
    _same(name, st[0], res[0], RF.reference()[name])


def test_building_block_behind_a_longer_case_and_twice():
    """short cases behind the capacity case in one batch, and cases run twice in it for the same bytes"""
    import gfamd
    ref, cases = RF.reference(), RF.cases()
    order = ["capacity", "m9", "capacity", "duplicate", "m9"]
    st, res = gfamd.reject_f([cases[n][0] for n in order], [cases[n][1] for n in order], [cases[n][2] for n in order])
    for k, n in enumerate(order):
        _same("%s at %d" % (n, k), st[k], res[k], ref[n])
    assert st[1].tobytes() == st[4].tobytes() and st[0].tobytes() == st[2].tobytes()


def test_building_block_on_device_memory():
    import gfamd
    import torch
    ref, cases = RF.reference(), RF.cases()
    names = ["m65", "nonfinite", "m7"]
    pairs = np.concatenate([cases[n][0] for n in names])
    d_pairs = torch.from_numpy(pairs).cuda()
    d_status = torch.full((len(pairs) + 64,), 7, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    res = gfamd.reject_f_device([len(cases[n][0]) for n in names], d_pairs.data_ptr(), d_status.data_ptr(), [cases[n][1] for n in names], [cases[n][2] for n in names])
    got = d_status.cpu().numpy()
    assert (got[len(pairs):] == 7).all(), "a byte beyond the last pair was written"
    at = 0
    for k, n in enumerate(names):
        _same(n, got[at:at + len(cases[n][0])], res[k], ref[n])
        at += len(cases[n][0])


# ---- the tracker.  Three sequences on 160 x 120 frames of a stream in which a patch moves against the scene (tests/reject_f_ref.py): 0 with the switch on, 1 with
# it off, 2 a PINHOLE_FULL camera with the switch on.  The yardstick of the device form is the same handle under GF_REJECT_F_HOST=1, whose stage
# tests/test_reject_f_track_host.py holds to the CPU tracker and to the restatement; the yardstick of an off sequence is a handle that never calls the setter.
W, H = 160, 120
LISTS = [[0, 1, 2], [2, 0, 1], [1, 2], [0, 2, 1], [2, 1, 0], [1, 0], [0, 1, 2]]      # skip and reorder
FULL = dict(proj=[150.5, 151.25, 80.5, 60.25], dist=[0.52, -2.7, 4e-4, -1.5e-4, 1.5, 0.4, -2.5, 1.4])
DT = 0.0666
OWN_SIZE = (144, 104)      # of sequence 0 in the run with a frame size per sequence
_G = {}


def _frames(size0):
    if size0 not in _G:
        _G[size0] = [RF.stream(*(size0 if b == 0 else (W, H)), n=len(LISTS), seed=3 + 5 * b) for b in range(3)]
    return _G[size0]


def _handle(gf, on, size0=(W, H), show=False):
    t = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=3, max_cnt=60, min_dist=8, depth_cam=0))
    t.set_seq_camera(2, gf.CameraModelEx.make("PINHOLE_FULL", **FULL))
    if size0 != (W, H):
        t.set_seq_size(0, *size0)
    if on:
        t.set_seq_reject_f(0, f_threshold=1.0, seed=5)
        t.set_seq_reject_f(2, gf.RejectFCfg(1, 9, 1.0, 0.0))
    if show:
        t.set_show_track(True, [0])
    return t


def _far_prediction(t, seq):
    ids, _, pts = t.state(seq)
    c = t.cfg
    xyz = np.stack([(pts[:, 0] + 400.0 - c.cx) / c.fx * 2.0, (pts[:, 1] + 400.0 - c.cy) / c.fy * 2.0, np.full(len(ids), 2.0)], 1)
    t.setPrediction(ids, xyz, seq=seq)


def _run(gf, route, on=True, size0=(W, H), fail_at=None, show=False):
    """every call's (ids, observations) and every sequence's state after it, the stage's counters, the tracker's, and the pictures of sequence 0 if asked"""
    import torch
    frames = _frames(size0)
    t = _handle(gf, on, size0, show)
    out, pictures, keep = [], [], []

    def stage(k):
        g = [torch.from_numpy(frames[b][k]).pin_memory() for b in LISTS[k]]
        keep.append(g)
        t.prefetchHost([x.data_ptr() for x in g], seqs=LISTS[k])      # one address per frame

    if route == "prefetch":
        stage(0)
    for k, L in enumerate(LISTS):
        if fail_at == k:
            _far_prediction(t, 0)
        before = t.state(0)
        before = tuple(np.array(x, copy=True) for x in before)
        ts = [DT * k] * len(L)
        if route == "host":
            res = t.trackImageSome(L, ts, [frames[b][k] for b in L])
        elif route == "device":
            dg = torch.from_numpy(np.stack([frames[b][k] for b in L])).cuda()
            torch.cuda.synchronize()
            res = t.trackImageSomeDevice(L, ts, dg.data_ptr())
        elif route == "refs":
            dg = [torch.from_numpy(np.pad(frames[b][k], ((0, 0), (0, 5 + b)))).cuda() for b in L]      # a pitch of its own per frame
            torch.cuda.synchronize()
            res = t.trackImageSomeDeviceRefs(L, ts, [(x.data_ptr(), x.shape[1]) for x in dg])
        else:
            if k + 1 < len(LISTS):
                stage(k + 1)
            res = t.trackPrefetched(ts)
        out.append([(np.array(i, copy=True), np.array(o, copy=True)) for i, o in res] + [tuple(np.array(x, copy=True) for x in t.state(b)) for b in range(3)])
        if show and 0 in L:
            pictures.append((frames[0][k], before, out[-1][len(L)], t.track_image(0)))
    rf, st = t.reject_f_stats(), t.stats()
    t.close()
    return out, rf, st, pictures


def _same_run(a, b, what, seqs=(0, 1, 2)):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        L = LISTS[k]
        for i, q in enumerate(L):
            if q in seqs:
                assert np.array_equal(x[i][0], y[i][0]), "%s: call %d, sequence %d: ids differ" % (what, k, q)
                assert x[i][1].tobytes() == y[i][1].tobytes(), "%s: call %d, sequence %d: observations differ" % (what, k, q)      # all eight fields, as bytes
        for q in seqs:
            sx, sy = x[len(L) + q], y[len(L) + q]
            assert all(u.tobytes() == v.tobytes() for u, v in zip(sx, sy)), "%s: call %d, sequence %d: state differs" % (what, k, q)


def _yardstick(gf, monkeypatch, **kw):
    """the host form: the same handle created under GF_REJECT_F_HOST=1"""
    key = ("host form", os.environ.get("GF_LK_POINTS"), os.environ.get("GF_CAMERA_LIFT_HOST")) + tuple(sorted(kw.items()))
    if key not in _G:
        with monkeypatch.context() as m:
            m.setenv("GF_REJECT_F_HOST", "1")
            _G[key] = _run(gf, "host", **kw)
    return _G[key]


def _expected_jobs(fail_at=None):
    """calls and (sequence, call) pairs the stage runs on: a sequence with the switch on that has taken a frame before (60 points; its first frame has none)"""
    seen, calls, pairs = set(), 0, 0
    for k, L in enumerate(LISTS):
        n = sum(1 for q in L if q in (0, 2) and q in seen)
        calls += (1 if n else 0) + (1 if fail_at == k else 0)
        pairs += n
        seen |= set(L)
    return calls, pairs


@pytest.mark.parametrize("route", ["host", "device", "refs", "prefetch"])
def test_tracker_device_form_equals_host_form(gf, monkeypatch, route):
    monkeypatch.delenv("GF_REJECT_F_HOST", raising=False)
    want, want_rf, _, _ = _yardstick(gf, monkeypatch)
    got, rf, st, _ = _run(gf, route)
    _same_run(got, want, route)
    calls, pairs = _expected_jobs()
    print(route, rf, want_rf)
    assert rf["rejected"] > 0 and rf["launches"] == calls and rf["sequences"] == pairs and rf["kernel_ms"] > 0
    assert want_rf["launches"] == 0 and want_rf["kernel_ms"] == 0
    assert {k: rf[k] for k in ("sequences", "candidates", "rejected", "no_model")} == {k: want_rf[k] for k in ("sequences", "candidates", "rejected", "no_model")}


def test_off_sequence_and_untouched_handle_are_the_parents(gf, monkeypatch):
    monkeypatch.delenv("GF_REJECT_F_HOST", raising=False)
    on, rf_on, st_on, _ = _run(gf, "device")
    off, rf_off, st_off, _ = _run(gf, "device", on=False)
    _same_run(on, off, "the sequence with the switch off", seqs=(1,))
    assert all(v == 0 for v in rf_off.values()), rf_off
    for key in ("lk_launches", "frames", "sequence_frames", "pyr_head", "pyr_down_tail"):
        assert st_on[key] == st_off[key], key
    differs = any(x[i][1].tobytes() != y[i][1].tobytes() or not np.array_equal(x[i][0], y[i][0]) for k, (x, y) in enumerate(zip(on, off)) for i, q in enumerate(LISTS[k]) if q == 0)
    assert differs, "the stage changed nothing on sequence 0: the test would pass without the feature"


@pytest.mark.parametrize("env", ["GF_LK_POINTS=4", "GF_CAMERA_LIFT_HOST=1"])
def test_tracker_under_the_other_switches(gf, monkeypatch, env):
    monkeypatch.delenv("GF_REJECT_F_HOST", raising=False)
    monkeypatch.setenv(*env.split("="))
    want, want_rf, _, _ = _yardstick(gf, monkeypatch)
    got, rf, _, _ = _run(gf, "device")
    _same_run(got, want, env)
    assert rf["rejected"] == want_rf["rejected"] > 0


def test_tracker_with_a_frame_size_per_sequence(gf, monkeypatch):
    monkeypatch.delenv("GF_REJECT_F_HOST", raising=False)
    want, want_rf, _, _ = _yardstick(gf, monkeypatch, size0=OWN_SIZE)
    got, rf, _, _ = _run(gf, "host", size0=OWN_SIZE)
    _same_run(got, want, "sizes")
    assert rf["rejected"] == want_rf["rejected"] > 0
    plain, _, _, _ = _yardstick(gf, monkeypatch)
    _same_run(got, plain, "the sequences of the handle's own size beside a smaller neighbour", seqs=(1, 2))


def test_failed_prediction_takes_the_second_launch(gf, monkeypatch):
    monkeypatch.delenv("GF_REJECT_F_HOST", raising=False)
    want, want_rf, want_st, _ = _yardstick(gf, monkeypatch, fail_at=3)
    got, rf, st, _ = _run(gf, "device", fail_at=3)
    _same_run(got, want, "fallback")
    calls, pairs = _expected_jobs(fail_at=3)
    assert rf["launches"] == calls == _expected_jobs()[0] + 1 and rf["sequences"] == pairs == want_rf["sequences"]
    assert st["lk_launches"] == want_st["lk_launches"] and rf["rejected"] == want_rf["rejected"]


def test_track_image_shows_the_kept_features(gf, monkeypatch):
    import track_draw_ref as TD
    monkeypatch.delenv("GF_REJECT_F_HOST", raising=False)
    _, rf, _, pictures = _run(gf, "device", show=True)
    assert rf["rejected"] > 0 and len(pictures) >= 4
    arrows = 0
    for bg, (ids0, _, pts0), (ids1, cnt1, pts1), img in pictures:
        at = {int(i): k for k, i in enumerate(ids0)}
        has = np.array([int(i) in at for i in ids1], bool)
        prev = np.array([pts0[at[int(i)]] if int(i) in at else (0, 0) for i in ids1], np.float32).reshape(-1, 2)
        assert np.array_equal(img, TD.render(bg, pts1, cnt1, prev, has)), "the picture is not the one the kept features imply"
        arrows += int(has.sum())
    assert arrows > 0


def test_setter_getter_and_refusals(gf):
    import torch
    t = _handle(gf, on=False)
    assert t.get_seq_reject_f(0).enable == 0
    for bad, word in ((0.0, "f_threshold"), (-1.0, "f_threshold"), (float("nan"), "f_threshold"), (float("inf"), "f_threshold")):
        with pytest.raises(gf.GfError, match=word):
            t.set_seq_reject_f(0, f_threshold=bad)
    with pytest.raises(gf.GfError, match="focal_length"):
        t.set_seq_reject_f(0, f_threshold=1.0, focal_length=-2.0)
    assert t.get_seq_reject_f(0).enable == 0 and all(v == 0 for v in t.reject_f_stats().values())      # refused: nothing changed
    t.set_seq_reject_f(1, f_threshold=1.5, seed=3, focal_length=300.0)
    assert t.get_seq_reject_f(1).as_dict() == {"enable": 1, "seed": 3, "f_threshold": 1.5, "focal_length": 300.0}
    frames = _frames((W, H))
    g = torch.from_numpy(np.stack([frames[1][0]])).pin_memory()
    t.prefetchHost(g.data_ptr(), seqs=[1])
    with pytest.raises(gf.GfError, match="staged frame"):
        t.set_seq_reject_f(1, None)
    with pytest.raises(gf.GfError, match="staged frame"):
        t.set_seq_reject_f(1, f_threshold=2.0)
    assert t.get_seq_reject_f(1).f_threshold == 1.5
    t.set_seq_reject_f(0, f_threshold=1.0)      # a sequence the staged frame does not list: allowed
    t.trackPrefetched([0.0])
    t.set_seq_reject_f(1, None)                 # between frames, at any time
    assert t.get_seq_reject_f(1).enable == 0
    t.close()


# ---- pixel rows with a camera each: the tracker's launch (lift = 1) as a building block
KB_SCENES = [(60, 24, 9000), (150, 45, 9001), (150, 60, 9002), (60, 24, 9003)]


def test_kannala_brandt_planted_scenes_through_the_kernels_lift(gf):
    """KANNALA_BRANDT lifts through transcendentals, so host and device bits may differ: planted scenes projected through that camera into pixel rows, lifted
    inside reject_f_kernel as the tracker's launch lifts them, one batch, held to the planted mask only -- no planted outlier kept, no planted inlier lost at
    less than 0.05 px noise"""
    cam = gf.CameraModel.make(*RF.KB)
    scenes = [RF.camera_scene(gf, cam, n, n_out, seed) for n, n_out, seed in KB_SCENES]
    st, res = gf.reject_f_pixels([cam] * len(scenes), [RF.KB_SIZE] * len(scenes), [s[0] for s in scenes], [s[1] for s in scenes], 1.0, 0.0, [s[2] for s in KB_SCENES])
    for k, (prev, cur, planted) in enumerate(scenes):
        kept_out, lost_in = int((st[k][planted] != 0).sum()), int((st[k][~planted] == 0).sum())
        print("scene %d: kept outliers %d, lost inliers %d, %s" % (KB_SCENES[k][2], kept_out, lost_in, res[k]))
        assert kept_out == 0, "a planted outlier was kept"
        assert lost_in == 0, "a planted inlier was lost"
        assert res[k]["m"] == len(planted) and res[k]["rejected"] == int(planted.sum())


def test_pixel_rows_kernel_equals_host_form_where_the_lift_has_no_transcendental(gf):
    """PINHOLE with distortion and PINHOLE_FULL, two frame sizes, a focal length of the caller's: byte for byte"""
    cams = [gf.CameraModel.make("PINHOLE", [500.0, 498.5, 300.25, 250.5], [0.05, -0.02, 0.001, -0.002]),
            gf.CameraModelEx.make("PINHOLE_FULL", proj=[480.0, 481.0, 322.0, 238.0], dist=[0.12, -0.3, 4e-4, -1.5e-4, 0.2, 0.1, -0.2, 0.1])]
    sizes, focal = [(640, 480), (600, 500)], [0.0, 300.0]
    scenes = [RF.camera_scene(gf, c, 90, 27, 9100 + k) for k, c in enumerate(cams)]
    args = (cams, sizes, [s[0] for s in scenes], [s[1] for s in scenes], 1.0, focal, [3, 4])
    st, res = gf.reject_f_pixels(*args)
    hst, hres = gf.reject_f_pixels(*args, host=True)
    for k in range(2):
        assert st[k].tobytes() == hst[k].tobytes() and res[k] == hres[k], (k, res[k], hres[k])
        assert res[k]["rejected"] >= 27


def test_tracker_with_a_kannala_brandt_sequence(gf, monkeypatch):
    """a KANNALA_BRANDT sequence with the switch on, on the stream whose patch turns against the scene: the stage runs on it inside the tracker and rejects;
    its two forms are not held to each other (their lifts may differ in the last bits)"""
    monkeypatch.delenv("GF_REJECT_F_HOST", raising=False)
    frames = _frames((W, H))[0]
    t = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=1, max_cnt=60, min_dist=8, depth_cam=0))
    t.set_seq_camera(0, gf.CameraModel.make("KANNALA_BRANDT", [80.5, 81.25, 80.5, 60.25], [-0.012, 0.006, -0.003, 0.0006]))
    t.set_seq_reject_f(0, f_threshold=1.0, seed=2)
    for k, f in enumerate(frames):
        ids, obs = t.trackImage(DT * k, f)
        assert len(ids) == 60
    rf = t.reject_f_stats()
    t.close()
    assert rf["launches"] == rf["sequences"] == len(frames) - 1 and rf["rejected"] > 0 and rf["candidates"] > rf["rejected"], rf
