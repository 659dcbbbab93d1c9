"""The region of interest of a tracker sequence (gf_tracker_set_roi / _set_roi_some_device / _get_roi) against tests/roi_tracker_ref.cpp, the oracle's tracker
with setMask starting from the region (pinned by tests/test_roi_host.py).  Every comparison is feature ids, the eight observation doubles as bit patterns and
ids / track_cnt / prev_pts, on every frame.

The frame sizes are the smallest at which the new code can go wrong -- a partial last strip (60 columns) and a partial last band (30 rows) -- and the shipped
configuration once:
    132 x 97    3 strips across, the last 12 columns wide; 4 bands, the last 7 rows
    188 x 122   width 8 mod 60, height 2 mod 30
    64 x 61     height 1 mod 30: the last band is one row, its halo row is image row h - 1
    640 x 480   max_cnt 150, min_dist 30
Region A excludes the bottom third, region B the left two fifths and a disc of radius h // 5 about (3w // 4, h // 2): edges that cut through strips and bands at
no multiple of anything.  A case counts only if the helper drops at least one track for lying outside and, on every frame after the first, at least a third of
max_cnt ids are carried over from the frame before; both are asserted on the helper's side.  Run with -m gpu."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import roi_ref as RR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.0666


@pytest.fixture(scope="module")
def ref(oracle, tmp_path_factory):
    return RR.build(tmp_path_factory.mktemp("roi_ref"))


def _ocfg(oracle, case, **kw):
    return oracle.default_cfg(max_cnt=case[2], min_dist=case[3], **kw)


def _gcfg(gf, case, **kw):
    return gf.default_cfg(width=case[0], height=case[1], max_cnt=case[2], min_dist=case[3], **kw)


_RUNS = {}


def _helper_run(oracle, ref, case, name, seed=0):
    """the helper over the K shared frames with region `name` ("A", "B", None) set before the first: [(ids, obs, state)] per frame, computed once"""
    key = (case, name, seed)
    if key not in _RUNS:
        w, h, max_cnt = case[:3]
        tr = RR.Tracker(ref, _ocfg(oracle, case))
        if name:
            tr.set_roi(RR.region(name, w, h))
        out, prev = [], None
        for k, f in enumerate(RR.frames(w, h, seed=seed)):
            ids, obs = tr.track(DT * k, f, RR.depth(k, w, h))
            if name and seed == 0:   # the conditions of a case
                assert RR.on_excluded(obs, RR.region(name, w, h)) == 0
                assert prev is None or 3 * len(np.intersect1d(ids, prev)) >= max_cnt, "frame %d: too few ids carried over" % k
            prev = ids
            out.append((ids, obs, tr.state()))
        if name and seed == 0:
            assert tr.dropped_outside() >= 1, "the helper dropped no track for lying outside the region"
        _RUNS[key] = out
    return _RUNS[key]


def _same_frame(expect, got, state, what):
    RR.same(expect[:2], got, what)
    assert all(np.array_equal(a, b) for a, b in zip(expect[2], state)), "%s: state differs" % what


# ---- 1
@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("case", RR.SIZES, ids=RR.size_id)
def test_six_frames_against_the_helper(gf, oracle, ref, case, name):
    w, h = case[:2]
    R = RR.region(name, w, h)
    expect = _helper_run(oracle, ref, case, name)
    gtr = gf.FeatureTracker(_gcfg(gf, case))
    gtr.set_roi(R)
    for k, f in enumerate(RR.frames(w, h)):
        g = gtr.trackImage(DT * k, f, RR.depth(k, w, h))
        assert RR.on_excluded(g[1], R) == 0, "frame %d: a reported point on an excluded pixel" % k
        _same_frame(expect[k], g, gtr.state(), "%s frame %d" % (name, k))
    st = gtr.stats()
    assert st["output_features"] == sum(len(e[0]) for e in expect)   # counts what is returned
    gtr.close()


# ---- 2
@pytest.mark.parametrize("case", RR.SIZES, ids=RR.size_id)
def test_nothing_changes_without_a_region(gf, oracle, case):
    """a handle with an all-255 region, one whose region was set and cleared before the first frame (both have allocated the table) and one that never had one:
    the same bits, which are the oracle's"""
    w, h = case[:2]
    otr = oracle.Tracker(_ocfg(oracle, case))
    white, cleared, never = (gf.FeatureTracker(_gcfg(gf, case)) for _ in range(3))
    white.set_roi(np.full((h, w), 255, np.uint8))
    cleared.set_roi(RR.region("B", w, h))
    cleared.set_roi(None)
    assert white.get_roi() is not None and cleared.get_roi() is None and never.get_roi() is None
    for k, f in enumerate(RR.frames(w, h)):
        d = RR.depth(k, w, h)
        o = otr.track(DT * k, f, d)
        for tag, g in (("all-255", white), ("cleared", cleared), ("never", never)):
            RR.same(o, g.trackImage(DT * k, f, d), "%s frame %d" % (tag, k))
            assert all(np.array_equal(a, b) for a, b in zip(otr.state(), g.state())), "%s frame %d: state differs" % (tag, k)
    for g in (white, cleared, never):
        g.close()


# ---- 3
def test_region_belongs_to_the_sequence_not_the_list_position(gf, oracle, ref):
    """three sequences of one handle -- regions A, none, B -- driven by track_some lists that change order and in which a sequence sits calls out: each equals its
    own single-sequence helper"""
    case = RR.SIZES[0]
    w, h = case[:2]
    names, seeds = ("A", None, "B"), (0, 1, 0)
    expect = [_helper_run(oracle, ref, case, names[b], seeds[b]) for b in range(3)]
    video = [RR.frames(w, h, seed=s) for s in seeds]
    gtr = gf.FeatureTracker(_gcfg(gf, case, batch=3))
    gtr.set_roi(RR.region("B", w, h), seq=2)
    gtr.set_roi(RR.region("A", w, h), seq=0)
    lists = [[0, 1, 2], [2, 0], [1, 2, 0], [0], [2, 1], [1, 0, 2], [2, 1, 0], [0, 1], [1, 2], [0, 2, 1]]
    done = [0, 0, 0]
    for call, seqs in enumerate(lists):
        seqs = [s for s in seqs if done[s] < RR.K]
        if not seqs:
            continue
        res = gtr.trackImageSome(seqs, [DT * done[s] for s in seqs], [video[s][done[s]] for s in seqs], [RR.depth(done[s], w, h) for s in seqs])
        for i, s in enumerate(seqs):
            _same_frame(expect[s][done[s]], res[i], gtr.state(s), "call %d, sequence %d frame %d" % (call, s, done[s]))
            done[s] += 1
    assert min(done) >= 4, done
    gtr.close()


# ---- 4
@pytest.mark.parametrize("case", RR.SIZES[:2], ids=RR.size_id)
def test_region_replaced_between_frames(gf, oracle, ref, case):
    """A before frame 0, B before frame 2, cleared before frame 4: the helper doing the same"""
    w, h = case[:2]
    plan = {0: RR.region("A", w, h), 2: RR.region("B", w, h), 4: None}
    rtr = RR.Tracker(ref, _ocfg(oracle, case))
    gtr = gf.FeatureTracker(_gcfg(gf, case))
    for k, f in enumerate(RR.frames(w, h)):
        if k in plan:
            rtr.set_roi(plan[k]); gtr.set_roi(plan[k])
        d = RR.depth(k, w, h)
        r = rtr.track(DT * k, f, d)
        _same_frame(r + (rtr.state(),), gtr.trackImage(DT * k, f, d), gtr.state(), "frame %d" % k)
    assert rtr.dropped_outside() >= 1
    gtr.close()


# ---- 5
@pytest.mark.parametrize("case", [RR.SIZES[0], RR.SIZES[2]], ids=RR.size_id)
def test_device_setter_leaves_the_bits_of_the_host_setter(gf, oracle, ref, case):
    import torch
    w, h = case[:2]
    A, B = RR.region("A", w, h), RR.region("B", w, h)
    # any non-zero byte means allowed
    rng = np.random.default_rng(5)
    A2, B2 = (np.where(R != 0, rng.integers(1, 256, R.shape), 0).astype(np.uint8) for R in (A, B))
    host = gf.FeatureTracker(_gcfg(gf, case, batch=2))
    dev = gf.FeatureTracker(_gcfg(gf, case, batch=2))
    host.set_roi(A2, seq=1); host.set_roi(B2, seq=0)
    d_masks = torch.from_numpy(np.stack([A2, B2])).cuda()
    torch.cuda.synchronize()
    dev.set_roi_device([1, 0], d_masks.data_ptr())     # mask 0 (A) for sequence 1, mask 1 (B) for sequence 0
    for seq, R in ((1, A), (0, B)):
        assert np.array_equal(host.get_roi(seq), R), "host setter, sequence %d" % seq
        assert np.array_equal(dev.get_roi(seq), host.get_roi(seq)), "device setter, sequence %d" % seq
    # a pitched host mask gives the same bits
    wide = np.full((h, w + 9), 255, np.uint8)
    wide[:, :w] = A2
    host.set_roi(wide[:, :w], seq=0)
    assert np.array_equal(host.get_roi(0), A)
    expect = {1: _helper_run(oracle, ref, case, "A"), 0: _helper_run(oracle, ref, case, "B")}
    for k, f in enumerate(RR.frames(w, h)):
        d = RR.depth(k, w, h)
        res = dev.trackImageBatch([DT * k] * 2, [f, f], [d, d])
        for seq in (0, 1):
            _same_frame(expect[seq][k], res[seq], dev.state(seq), "after the device setter, sequence %d frame %d" % (seq, k))
    dev.set_roi_device([0], None)
    assert dev.get_roi(0) is None and np.array_equal(dev.get_roi(1), A)
    host.close(); dev.close()


# ---- 6
@pytest.mark.parametrize("entry", ["prefetched", "device", "equalize"])
def test_every_entry_point(gf, oracle, ref, entry):
    """(host frames: test_six_frames_against_the_helper)"""
    import torch
    case = RR.SIZES[0]
    w, h = case[:2]
    R = RR.region("B", w, h)
    video = RR.frames(w, h)
    if entry == "equalize":
        import clahe_ref
        rtr = RR.Tracker(ref, _ocfg(oracle, case))
        rtr.set_roi(R)
        expect = []
        for k, f in enumerate(video):
            r = rtr.track(DT * k, clahe_ref.clahe(f), RR.depth(k, w, h))
            expect.append(r + (rtr.state(),))
        assert rtr.dropped_outside() >= 1
    else:
        expect = _helper_run(oracle, ref, case, "B")
    gtr = gf.FeatureTracker(_gcfg(gf, case, equalize=int(entry == "equalize")))
    gtr.set_roi(R)
    if entry == "prefetched":
        pg = [torch.from_numpy(f[None].copy()).pin_memory() for f in video]
        pd = [torch.from_numpy(RR.depth(k, w, h)[None].view(np.int16).copy()).pin_memory() for k in range(RR.K)]
        gtr.prefetchHost(pg[0].data_ptr(), pd[0].data_ptr())
    for k, f in enumerate(video):
        d = RR.depth(k, w, h)
        if entry == "prefetched":
            if k + 1 < RR.K:
                gtr.prefetchHost(pg[k + 1].data_ptr(), pd[k + 1].data_ptr())
            g = gtr.trackPrefetched([DT * k])[0]
        elif entry == "device":
            dg, dd = torch.from_numpy(f[None].copy()).cuda(), torch.from_numpy(d[None].view(np.int16).copy()).cuda()
            torch.cuda.synchronize()
            g = gtr.trackImageBatchDevice([DT * k], dg.data_ptr(), dd.data_ptr())[0]
        else:
            g = gtr.trackImage(DT * k, f, d)
        _same_frame(expect[k], g, gtr.state(), "%s frame %d" % (entry, k))
    gtr.close()


# ---- 7
def test_with_prediction_and_outlier_feedback(gf, oracle, ref):
    """set_prediction / remove_outliers between frames as tests/test_tracker_sizes_gpu.py drives them (frame 3: garbage predictions, the < 10 fallback), region A"""
    case = RR.SIZES[0]
    w, h = case[:2]
    ocfg = _ocfg(oracle, case, depth_cam=0)
    rtr = RR.Tracker(ref, ocfg)
    gtr = gf.FeatureTracker(_gcfg(gf, case, depth_cam=0))
    R = RR.region("A", w, h)
    rtr.set_roi(R); gtr.set_roi(R)
    cfg = gtr.cfg
    rng = np.random.default_rng(9)
    for k, f in enumerate(RR.frames(w, h)):
        r = rtr.track(DT * k, f, None)
        _same_frame(r + (rtr.state(),), gtr.trackImage(DT * k, f, None), gtr.state(), "frame %d" % k)
        rm = r[0][rng.random(len(r[0])) < 0.05]
        rtr.remove_outliers(rm); gtr.removeOutliers(rm)
        ids, _, pts = rtr.state()
        sel = rng.random(len(ids)) < 0.7
        noise = 200.0 if k == 3 else 1.0
        uv = pts[sel] + rng.normal(0, noise, (sel.sum(), 2))
        xyz = np.stack([(uv[:, 0] - cfg.cx) / cfg.fx * 2.0, (uv[:, 1] - cfg.cy) / cfg.fy * 2.0, np.full(len(uv), 2.0)], 1)
        rtr.set_prediction(ids[sel], xyz); gtr.setPrediction(ids[sel], xyz)
    assert rtr.dropped_outside() >= 1
    gtr.close()


# ---- 8
@pytest.mark.parametrize("edge", ["nothing", "block5x5", "row0_col0"])
def test_edge_regions(gf, oracle, ref, edge):
    case = RR.SIZES[0]
    w, h = case[:2]
    R = np.zeros((h, w), np.uint8)
    if edge == "block5x5":
        R[40:45, 70:75] = 255      # inside the second strip of the second band
    elif edge == "row0_col0":
        R[0, :] = 255; R[:, 0] = 255   # candidates need x >= 1 and y >= 1
    rtr = RR.Tracker(ref, _ocfg(oracle, case))
    gtr = gf.FeatureTracker(_gcfg(gf, case))
    rtr.set_roi(R); gtr.set_roi(R)
    for k, f in enumerate(RR.frames(w, h)):
        d = RR.depth(k, w, h)
        r = rtr.track(DT * k, f, d)
        g = gtr.trackImage(DT * k, f, d)    # GF_OK: a failing call raises
        _same_frame(r + (rtr.state(),), g, gtr.state(), "%s frame %d" % (edge, k))
        if edge != "block5x5":
            assert len(g[0]) == 0, "frame %d: %d features" % (k, len(g[0]))
        else:
            assert len(g[0]) <= 25 and RR.on_excluded(g[1], R) == 0
    gtr.close()


# ---- 9
def test_refused_calls_change_nothing(gf, oracle, ref):
    import torch
    case = RR.SIZES[0]
    w, h = case[:2]
    L, INVALID = gf.lib(), -1
    A, B = RR.region("A", w, h), RR.region("B", w, h)
    expect = _helper_run(oracle, ref, case, "A")
    gtr = gf.FeatureTracker(_gcfg(gf, case, batch=2))
    video = RR.frames(w, h)
    has = C.c_int(0)
    buf = np.zeros((h, w), np.uint8)
    d_masks = torch.from_numpy(np.stack([B, B, B])).cuda()
    torch.cuda.synchronize()
    dp = C.c_void_p(d_masks.data_ptr())
    pB = B.ctypes.data_as(C.POINTER(C.c_uint8))
    pbuf = buf.ctypes.data_as(C.POINTER(C.c_uint8))

    def ints(*v):
        return (C.c_int * len(v))(*v)

    def refusals():
        return [L.gf_tracker_set_roi(None, 0, pB, w), L.gf_tracker_set_roi(gtr.h, -1, pB, w), L.gf_tracker_set_roi(gtr.h, 2, pB, w),
                L.gf_tracker_set_roi(gtr.h, 0, pB, w - 1),
                L.gf_tracker_set_roi_some_device(None, 1, ints(0), dp), L.gf_tracker_set_roi_some_device(gtr.h, 2, ints(0, 0), dp),
                L.gf_tracker_set_roi_some_device(gtr.h, 2, ints(0, 2), dp), L.gf_tracker_set_roi_some_device(gtr.h, 1, ints(-1), dp),
                L.gf_tracker_set_roi_some_device(gtr.h, -1, ints(0), dp), L.gf_tracker_set_roi_some_device(gtr.h, 3, ints(0, 1, 0), dp),
                L.gf_tracker_set_roi_some_device(gtr.h, 2, ints(1, 1), None),
                L.gf_tracker_get_roi(None, 0, pbuf, w, C.byref(has)), L.gf_tracker_get_roi(gtr.h, 2, pbuf, w, C.byref(has)),
                L.gf_tracker_get_roi(gtr.h, 0, pbuf, w - 1, C.byref(has))]

    # on a handle that has no region yet: still none afterwards
    assert refusals() == [INVALID] * 14
    assert gtr.get_roi(0) is None and gtr.get_roi(1) is None
    gtr.set_roi(A, seq=0)
    for k in range(2):
        _same_frame(expect[k], gtr.trackImage(DT * k, video[k], RR.depth(k, w, h)), gtr.state(), "frame %d" % k)
    before = gtr.state()
    assert refusals() == [INVALID] * 14
    assert b"" != L.gf_last_error()
    assert np.array_equal(gtr.get_roi(0), A) and gtr.get_roi(1) is None
    assert all(np.array_equal(a, b) for a, b in zip(before, gtr.state()))
    for k in range(2, RR.K):
        _same_frame(expect[k], gtr.trackImage(DT * k, video[k], RR.depth(k, w, h)), gtr.state(), "frame %d, after the refused calls" % k)
    gtr.close()


# ---- 10
def test_estimator_with_its_own_tracker_takes_the_region(gf):
    """gf_estimator_set_roi(A) on an estimator that owns its tracker ends every frame in the bits of an estimator fed through gf_estimator_input_feature by a
    stand-alone tracker with A (multiple_thread: every second image reaches the back end, no feedback into the tracker)"""
    import synth_stream as SS
    st = SS.Stream(1, t_still=1.0, t_move=1.0, v_max=0.4, yaw0=0.0, yaw_turn=-0.6, split_x=1.8, turn_delay=0.8)
    cfg = gf.default_estimator_cfg(tio=SS.TIO, rio=SS.RIO, multiple_thread=1, with_tracker=1)
    cfg.tracker = gf.default_cfg()
    own = gf.SlidingWindowEstimator(cfg)
    cfg2 = gf.default_estimator_cfg(tio=SS.TIO, rio=SS.RIO, multiple_thread=1)
    cfg2.tracker = gf.default_cfg()
    fed = gf.SlidingWindowEstimator(cfg2)
    tracker = gf.FeatureTracker(gf.default_cfg())
    A = RR.region("A", 640, 480)
    own.set_roi(A); tracker.set_roi(A)
    tp, n_img = -1.0, 0
    for k in range(len(st.cam_t)):
        for e in (own, fed):
            t1 = st.feed(e, k, tp)
        tp = t1
        img, dep = st.image(k)
        t = float(st.cam_t[k])
        fo = own.inputImage(t, img, dep)
        ids, obs = tracker.trackImage(t, img, dep)
        assert sorted(fo) == sorted(int(i) for i in ids) and RR.on_excluded(obs, A) == 0, "image %d" % k
        n_img += 1
        if n_img % 2 != 0:
            continue
        fed.inputFeature(t, {int(i): o for i, o in zip(ids, obs)})
        so, sf = own.state(), fed.state()
        for key in so:
            assert np.array_equal(np.asarray(so[key]), np.asarray(sf[key])), "image %d: %s differs" % (k, key)
        fa, fb = own.features(), fed.features()
        for key in fa:
            assert np.array_equal(fa[key], fb[key]), "image %d: feature list %s differs" % (k, key)
    assert own.state()["frame_count"] >= 5
    own.close(); fed.close(); tracker.close()


def test_estimator_without_a_tracker_refuses_the_region(gf):
    est = gf.SlidingWindowEstimator(gf.default_estimator_cfg())
    with pytest.raises(gf.GfError, match="without a tracker"):
        est.set_roi(np.full((480, 640), 255, np.uint8))
    est.close()


def test_replay_tool_roi_option(gf, tmp_path):
    """an all-white mask writes the vio.txt of a run without the option, byte for byte; a mask of the wrong size is refused with a message"""
    import synth_stream as SS
    st = SS.Stream(1, t_still=1.0, t_move=1.0, v_max=0.4, yaw0=0.0, yaw_turn=-0.6, split_x=1.8, turn_delay=0.8)
    d = str(tmp_path)
    st.export(d)
    exe = os.path.join(ROOT, "bin", "gf_replay")
    assert os.path.exists(exe), "bin/gf_replay is missing: run `python __graft_entry__.py` (build)"
    white, small = os.path.join(d, "white.pgm"), os.path.join(d, "small.pgm")
    gf.write_pgm(white, np.full((480, 640), 255, np.uint8))
    gf.write_pgm(small, np.full((240, 320), 255, np.uint8))
    cfg = os.path.join(d, "config.yaml")
    plain = subprocess.run([exe, cfg, d, os.path.join(d, "vio_plain.txt")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0, plain.stderr
    roi = subprocess.run([exe, "--roi", white, cfg, d, os.path.join(d, "vio_roi.txt")], capture_output=True, text=True, timeout=300)
    assert roi.returncode == 0, roi.stderr
    a, b = open(os.path.join(d, "vio_plain.txt"), "rb").read(), open(os.path.join(d, "vio_roi.txt"), "rb").read()
    assert len(a) > 0 and a == b
    bad = subprocess.run([exe, cfg, d, os.path.join(d, "vio_bad.txt"), "--roi", small], capture_output=True, text=True, timeout=300)
    assert bad.returncode != 0 and "--roi" in bad.stderr and "320 x 240" in bad.stderr and "640 x 480" in bad.stderr, bad.stderr
