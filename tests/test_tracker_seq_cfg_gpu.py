"""Parameters per sequence of a tracker handle (gf_tracker_set_seq_cfg / _get_seq_cfg / gf_tracker_reset_seq): max_cnt, min_dist, flow_back, depth_cam and the
camera calibration, in the launches the sequences share.

The reference for a sequence is one oracle.Tracker built with that sequence's twelve values and fed only that sequence's frames, as in
tests/test_tracker_subset_gpu.py; every comparison is bit for bit (ids, observations as uint64, state()) on every frame.

Frames: 320 x 240 (6 x 8 detector strips; a disc of radius 30 crosses three strips), 8 per sequence, a constant depth image.  The mixed handle is created with
the largest count and the tightest spacing of its fleet, 500 / 12:
    sequence 0   untouched
    sequence 1   150 / 30, the calibration of a second camera with all four distortion coefficients non-zero
    sequence 2   300 / 20, flow_back 0
    sequence 3   200 / 15, depth_cam 0 (no depth image on the host route, and none on every other frame of the prefetched route)
So that the cases can fail, the oracle alone has to tell the configurations apart on these frames (_reference asserts it, on the CPU): the handle's own
parameters give sequences 1-3 something else on at least one frame, flow_back 1 gives sequence 2 something else, and among the set sequences there are frames
that want more than 16 corners (select_corners_kernel) and frames that want 1 .. 16 (select_topk_kernel).  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import roi_ref as RR
import synth

pytestmark = pytest.mark.gpu

DT = 0.0666
W, H, K, B = 320, 240, 8, 4
HANDLE = dict(max_cnt=500, min_dist=12, flow_back=1, depth_cam=1)
CAM1 = dict(fx=605.687407, fy=607.16452123, cx=323.35155412, cy=236.66167004, k1=0.15860811, k2=-0.34018021, p1=-0.00180768, p2=0.00032313)
SEQ = {0: {}, 1: dict(max_cnt=150, min_dist=30, **CAM1), 2: dict(max_cnt=300, min_dist=20, flow_back=0), 3: dict(max_cnt=200, min_dist=15, depth_cam=0)}
SEEDS = (1100, 1101, 1102, 1103)
ROUTES = ("host", "device", "prefetch")
FIELDS = ("max_cnt", "min_dist", "flow_back", "depth_cam", "fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")
_REF = {}


def _same(o, g, what):
    assert np.array_equal(o[0], g[0]), "%s: feature id lists differ" % what
    assert np.array_equal(o[1].view(np.uint64), g[1].view(np.uint64)), "%s: observations differ" % what


def _same_state(a, b, what):
    assert len(a) == len(b) == 3 and all(np.array_equal(x, y) for x, y in zip(a, b)), "%s: state differs" % what


def _equal(a, b):
    return np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))


def _rotated(listed, k):
    r = k % len(listed)
    return listed[r:] + listed[:r]


def _ocfg(oracle, **fields):
    """the oracle's configuration: the handle's values, then the sequence's own"""
    c = oracle.default_cfg(**HANDLE)
    for k, v in fields.items():
        setattr(c, k, v)
    return c


def _oracle_run(oracle, frames, depth, first=0, **fields):
    """[(result, state)] of one oracle tracker built with `fields` over frames[first:], the frame k at DT * k"""
    otr = oracle.Tracker(_ocfg(oracle, **fields))
    out = []
    for k in range(first, len(frames)):
        res = otr.track(DT * k, frames[k], depth if otr.cfg.depth_cam else None)
        out.append((res, tuple(np.array(x, copy=True) for x in otr.state())))
    return out


def _reference(oracle):
    """frames[b][k], the depth image, ref[b][k] = (result, state) of sequence b's own oracle; computed once, with the conditions of the module's docstring"""
    if not _REF:
        frames = [synth.tracker_sequence(s, K, W, H) for s in SEEDS]
        depth = np.full((H, W), 1500, np.uint16)
        ref = [_oracle_run(oracle, frames[b], depth, **SEQ[b]) for b in range(B)]
        for b in (1, 2, 3):
            other = _oracle_run(oracle, frames[b], depth)
            assert any(not _equal(ref[b][k][0], other[k][0]) for k in range(K)), "sequence %d: the handle's parameters give the same result on every frame" % b
        other = _oracle_run(oracle, frames[2], depth, **dict(SEQ[2], flow_back=1))
        assert any(not _equal(ref[2][k][0], other[k][0]) for k in range(K)), "sequence 2: flow_back 1 gives the same result on every frame"
        # want = max_cnt - the tracks kept by setMask = max_cnt - the ids that come from the frame before
        wants = [SEQ[b]["max_cnt"] - len(np.intersect1d(ref[b][k][0][0], ref[b][k - 1][0][0])) for b in (1, 2, 3) for k in range(1, K)]
        assert any(w > 16 for w in wants) and any(0 < w <= 16 for w in wants), wants
        _REF["x"] = (frames, depth, ref)
    return _REF["x"]


def _mixed_handle(gf):
    gtr = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=B, **HANDLE))
    for b in (1, 2, 3):
        gtr.set_seq_cfg(b, **SEQ[b])
    return gtr


def _step(gf, gtr, route, L, k, frames, depth, keep, last=None):
    """frame k for the listed sequences through `route`; prefetch: the frame was staged before, the next one (list `last`) is staged under this one"""
    import torch
    ts = [DT * k] * len(L)
    if route == "host":
        return gtr.trackImageSome(L, ts, [frames[b][k] for b in L], [None if b == 3 else depth for b in L])
    if route == "device":
        dg = torch.from_numpy(np.stack([frames[b][k] for b in L])).cuda()
        dd = torch.from_numpy(np.stack([depth] * len(L)).view(np.int16)).cuda()
        torch.cuda.synchronize()
        return gtr.trackImageSomeDevice(L, ts, dg.data_ptr(), dd.data_ptr())
    if last is not None:
        _stage(gtr, last, k + 1, frames, depth, keep)
    return gtr.trackPrefetched(ts)


def _stage(gtr, L, k, frames, depth, keep):
    import torch
    g = torch.from_numpy(np.stack([frames[b][k] for b in L])).pin_memory()
    d = torch.from_numpy(np.stack([depth] * len(L)).view(np.int16)).pin_memory()
    keep.append((g, d))
    # sequence 3 (depth_cam 0) comes with a NULL depth entry on the odd frames, beside neighbours whose depth images are read
    da = [None if b == 3 and k % 2 else d.data_ptr() + 2 * i * H * W for i, b in enumerate(L)]
    gtr.prefetchHost(g.data_ptr(), da, seqs=L)


def _run_mixed(gf, oracle, route):
    frames, depth, ref = _reference(oracle)
    gtr = _mixed_handle(gf)
    lists = [_rotated(list(range(B)), k) for k in range(K)]
    keep = []
    if route == "prefetch":
        _stage(gtr, lists[0], 0, frames, depth, keep)
    for k in range(K):
        res = _step(gf, gtr, route, lists[k], k, frames, depth, keep, lists[k + 1] if k + 1 < K else None)
        for i, b in enumerate(lists[k]):
            _same(ref[b][k][0], res[i], "%s route, frame %d, sequence %d (list position %d)" % (route, k, b, i))
            _same_state(ref[b][k][1], gtr.state(b), "%s route, frame %d, sequence %d" % (route, k, b))
    for b in range(B):
        assert gtr.get_seq_cfg(b) == {**_handle_fields(gf), **SEQ[b]}
    gtr.close()


def _handle_fields(gf):
    c = gf.default_cfg(width=W, height=H, batch=B, **HANDLE)
    return {k: getattr(c, k) for k in FIELDS}


# ---- 1
@pytest.mark.parametrize("route", ROUTES)
def test_mixed_handle(gf, oracle, route):
    """four sequences with four configurations share every launch; each equals its own oracle at every frame, the list in another order on every call"""
    _run_mixed(gf, oracle, route)


# ---- 2
def _predict(rng, cam, ids, pts, garbage):
    """predictions for 70 % of the tracks, a pixel of noise around where they are, through the sequence's own camera (its distortion left out: a prediction need
    not be right); garbage: every track predicted far outside the image, so that the forward pass from there fails for all of them"""
    sel = np.ones(len(ids), bool) if garbage else rng.random(len(ids)) < 0.7
    uv = pts[sel] + (5000.0 if garbage else rng.normal(0, 1.0, (sel.sum(), 2)))
    xyz = np.stack([(uv[:, 0] - cam["cx"]) / cam["fx"] * 2.0, (uv[:, 1] - cam["cy"]) / cam["fy"] * 2.0, np.full(len(uv), 2.0)], 1)
    return ids[sel], xyz


def test_prediction_and_outlier_feedback(gf, oracle):
    """setPrediction / removeOutliers on sequences 1 (its own camera in spaceToPlane) and 2 (no reverse check) of the mixed handle.  In one call sequence 1 gets
    garbage predictions and falls under ten forward successes, so the three-level re-launch runs for it alone beside sequences that keep their pass."""
    frames, depth, _ = _reference(oracle)
    otrs = [oracle.Tracker(_ocfg(oracle, **SEQ[b])) for b in range(B)]
    gtr = _mixed_handle(gf)
    cams = [gtr.get_seq_cfg(b) for b in range(B)]
    rng = np.random.default_rng(11)
    step_no = [0]

    def step(launches):
        k = step_no[0]
        L = _rotated(list(range(B)), k)
        before = gtr.stats()["lk_launches"]
        res = _step(gf, gtr, "host", L, k, frames, depth, None)
        for i, b in enumerate(L):
            _same(otrs[b].track(DT * k, frames[b][k], None if b == 3 else depth), res[i], "frame %d, sequence %d" % (k, b))
        for b in range(B):
            _same_state(otrs[b].state(), gtr.state(b), "frame %d, sequence %d" % (k, b))
        assert gtr.stats()["lk_launches"] - before == launches
        step_no[0] += 1
        return dict(zip(L, res))

    def feedback(b, garbage=False):
        ids = otrs[b].state()[0]
        rm = ids[rng.random(len(ids)) < 0.05]
        otrs[b].remove_outliers(rm); gtr.removeOutliers(rm, seq=b)
        ids, _, pts = otrs[b].state()
        pid, xyz = _predict(rng, cams[b], ids, pts, garbage)
        otrs[b].set_prediction(pid, xyz); gtr.setPrediction(pid, xyz, seq=b)

    step(0)                  # first frames: nothing to track
    step(1)
    feedback(1); feedback(2)
    step(2)                  # the plain launch for 0 and 3, the predicted one for 1 and 2
    feedback(1, garbage=True)
    feedback(2)
    prev2 = otrs[2].state()[0]
    res = step(3)            # plain (0, 3), predicted (1, 2), and the re-launch for 1 alone
    assert len(np.intersect1d(res[2][0], prev2)) >= 10      # sequence 2 kept its predicted pass
    step(1)
    gtr.close()


# ---- 3
def test_setter_equal_to_the_default(gf, oracle):
    """a handle whose sequences are all set to the handle's own values returns the bits of an untouched handle"""
    frames, depth, _ = _reference(oracle)
    plain = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=B, **HANDLE))
    same = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=B, **HANDLE))
    for b in range(B):
        same.set_seq_cfg(b, **plain.get_seq_cfg(b))
        assert same.get_seq_cfg(b) == plain.get_seq_cfg(b) == _handle_fields(gf)
    L = list(range(B))
    for k in range(K):
        a = plain.trackImageSome(L, [DT * k] * B, [frames[b][k] for b in L], [depth] * B)
        c = same.trackImageSome(L, [DT * k] * B, [frames[b][k] for b in L], [depth] * B)
        for b in L:
            _same(a[b], c[b], "frame %d, sequence %d" % (k, b))
            _same_state(plain.state(b), same.state(b), "frame %d, sequence %d" % (k, b))
    assert min(len(x[0]) for x in a) > 16
    plain.close(); same.close()


# ---- 4
def test_reset(gf, oracle):
    """sequence 1 is reset after frame 3 and given new parameters: from frame 4 it is a fresh oracle built with them; sequences 0, 2 and 3 go on as they were.
    A setter without a reset, after frame 0, is refused and changes nothing."""
    frames, depth, ref = _reference(oracle)
    new = {**_handle_fields(gf), **dict(max_cnt=100, min_dist=25, flow_back=0, depth_cam=1)}
    fresh = _oracle_run(oracle, frames[1], depth, first=4, **new)
    gtr = _mixed_handle(gf)
    for k in range(K):
        if k == 4:
            gtr.reset_seq(1)
            assert all(len(x) == 0 for x in gtr.state(1)) and gtr.get_seq_cfg(1) == {**_handle_fields(gf), **SEQ[1]}     # the parameters are settings: they stay
            gtr.set_seq_cfg(1, **new)
            assert gtr.get_seq_cfg(1) == new
        L = _rotated(list(range(B)), k)
        res = _step(gf, gtr, "host", L, k, frames, depth, None)
        for i, b in enumerate(L):
            o = fresh[k - 4] if b == 1 and k >= 4 else ref[b][k]
            _same(o[0], res[i], "frame %d, sequence %d" % (k, b))
            _same_state(o[1], gtr.state(b), "frame %d, sequence %d" % (k, b))
        if k == 0:
            before = gtr.get_seq_cfg(2)
            with pytest.raises(gf.GfError, match="gf status -1.*sequence 2 has taken a frame"):
                gtr.set_seq_cfg(2, max_cnt=10)
            with pytest.raises(gf.GfError, match="gf status -1.*sequence 2 has taken a frame"):
                gtr.set_seq_cfg(2)
            assert gtr.get_seq_cfg(2) == before
    assert fresh[0][0][0].min() == 0 and not _equal(fresh[0][0], ref[1][4][0])      # ids start again at 0
    gtr.close()


# ---- 5
def test_refusals(gf, oracle):
    """every refusal of the setter: GF_ERR_INVALID, a message that names the field, and get_seq_cfg unchanged afterwards"""
    frames, depth, _ = _reference(oracle)
    lib = gf.lib()
    gtr = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=2, **HANDLE))
    gtr.set_seq_cfg(1, **SEQ[1])
    before = [gtr.get_seq_cfg(b) for b in range(2)]
    assert before[0] == _handle_fields(gf) and before[1] == {**_handle_fields(gf), **SEQ[1]}
    c = gf.TrackerSeqCfg(**before[1])
    assert lib.gf_tracker_set_seq_cfg(None, 0, C.byref(c)) == -1 and b"null handle" in lib.gf_last_error()
    assert lib.gf_tracker_get_seq_cfg(None, 0, C.byref(c)) == -1
    assert lib.gf_tracker_reset_seq(None, 0) == -1 and b"null handle" in lib.gf_last_error()
    for seq in (-1, 2):
        with pytest.raises(gf.GfError, match="gf status -1.*sequence %d of a handle of 2" % seq):
            gtr.set_seq_cfg(seq, max_cnt=100)
        with pytest.raises(gf.GfError, match="gf status -1.*sequence %d of a handle of 2" % seq):
            gtr.get_seq_cfg(seq)
        with pytest.raises(gf.GfError, match="gf status -1.*sequence %d of a handle of 2" % seq):
            gtr.reset_seq(seq)
    bad = [("max_cnt", 0), ("max_cnt", 501), ("min_dist", 11), ("min_dist", 129), ("flow_back", 2), ("flow_back", -1), ("depth_cam", 2), ("depth_cam", -1),
           ("fx", 0.0), ("fx", -600.0), ("fy", 0.0), ("fy", float("nan"))]
    for b in range(2):
        for field, value in bad:
            with pytest.raises(gf.GfError, match=r"gf status -1.*gf_tracker_seq_cfg\.%s " % field):
                gtr.set_seq_cfg(b, **{field: value})
        with pytest.raises(TypeError):
            gtr.set_seq_cfg(b, width=640)
        assert gtr.get_seq_cfg(b) == before[b]
    gtr.trackImageSome([1], [0.0], [frames[1][0]], [depth])
    with pytest.raises(gf.GfError, match="gf status -1.*sequence 1 has taken a frame"):
        gtr.set_seq_cfg(1, max_cnt=100)
    assert [gtr.get_seq_cfg(b) for b in range(2)] == before
    gtr.set_seq_cfg(0, max_cnt=100)      # sequence 0 has taken none: still allowed, and the limits are inclusive
    gtr.set_seq_cfg(0, max_cnt=500, min_dist=128)
    gtr.set_seq_cfg(0, max_cnt=1, min_dist=12)
    gtr.set_seq_cfg(0)
    assert gtr.get_seq_cfg(0) == before[0]
    gtr.close()


def test_refused_while_a_staged_frame_lists_the_sequence(gf, oracle):
    """gf_tracker_prefetch_some judged the depth pointers of a staged frame with the parameters then in force (sequence 1: depth_cam 0, a NULL depth entry): until
    gf_tracker_track_prefetched has consumed the frame, setter and reset are refused for the listed sequence, nothing changed, and allowed for its neighbour"""
    import torch
    frames, depth, _ = _reference(oracle)
    own = dict(max_cnt=200, min_dist=15, depth_cam=0)
    gtr = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=2, **HANDLE))
    gtr.set_seq_cfg(1, **own)
    g = torch.from_numpy(np.ascontiguousarray(frames[3][0])).pin_memory()
    gtr.prefetchHost([g.data_ptr()], [None], seqs=[1])
    before = gtr.get_seq_cfg(1)
    for call in (lambda: gtr.set_seq_cfg(1, depth_cam=1), lambda: gtr.set_seq_cfg(1), lambda: gtr.reset_seq(1)):
        with pytest.raises(gf.GfError, match="gf status -1.*sequence 1 is listed by a staged frame"):
            call()
    assert gtr.get_seq_cfg(1) == before == {**_handle_fields(gf), **own}
    gtr.set_seq_cfg(0, max_cnt=100)      # not listed
    gtr.reset_seq(0)
    res = gtr.trackPrefetched([0.0])
    o = oracle.Tracker(_ocfg(oracle, **own)).track(0.0, frames[3][0], None)
    _same(o, res[0], "the staged frame")
    gtr.reset_seq(1)                     # consumed: allowed again
    gtr.set_seq_cfg(1, depth_cam=1)
    gtr.close()


# ---- 6
@pytest.mark.parametrize("env", ["GF_LK_POINTS=4", "GF_SELECT_TOPK=0"])
def test_mixed_handle_under_the_switches(gf, oracle, monkeypatch, env):
    """the mixed handle on lk_track_mp_kernel<4>, and with every frame's corners through the sort"""
    monkeypatch.setenv(*env.split("="))
    _run_mixed(gf, oracle, "host")


# ---- 7
def test_with_a_region_of_interest(gf, oracle, tmp_path):
    """a sequence with its own min_dist and max_cnt AND a region of interest, against the region-of-interest helper built with that sequence's parameters
    (132 x 97: a partial last strip and a partial last band); its untouched neighbour, without a region, against the plain helper"""
    ref = RR.build(tmp_path)
    w, h, max_cnt, min_dist = RR.SIZES[0]
    own = dict(max_cnt=30, min_dist=9)
    R = RR.region("B", w, h)
    ocfg = [oracle.default_cfg(max_cnt=max_cnt, min_dist=min_dist), oracle.default_cfg(**own)]
    helpers = [RR.Tracker(ref, c) for c in ocfg]
    helpers[1].set_roi(R)
    gtr = gf.FeatureTracker(gf.default_cfg(width=w, height=h, batch=2, max_cnt=max_cnt, min_dist=min_dist))
    gtr.set_seq_cfg(1, **own)
    gtr.set_roi(R, seq=1)
    fr = [RR.frames(w, h), RR.frames(w, h, seed=1)]
    differs = False
    plain = RR.Tracker(ref, ocfg[0])
    plain.set_roi(R)
    for k in range(RR.K):
        L = [1, 0] if k % 2 else [0, 1]
        d = RR.depth(k, w, h)
        res = gtr.trackImageSome(L, [DT * k] * 2, [fr[b][k] for b in L], [d, d])
        for i, b in enumerate(L):
            e = helpers[b].track(DT * k, fr[b][k], d)
            RR.same(e, res[i], "frame %d, sequence %d" % (k, b))
            _same_state(helpers[b].state(), gtr.state(b), "frame %d, sequence %d" % (k, b))
            if b == 1:
                assert RR.on_excluded(res[i][1], R) == 0
                differs = differs or not _equal(e, plain.track(DT * k, fr[1][k], d))
    assert differs, "the handle's parameters give sequence 1 the same result on every frame"
    gtr.close()
