"""The sequences of one tracker handle advancing independently (gf_tracker_track_some / _track_some_device / _prefetch_some, gf_tracker_track on a batch handle).

The reference is one oracle.Tracker per sequence, fed only the frames that sequence takes; every comparison is bit for bit (ids, observations as uint64,
state()) on every call, and the state of every sequence that sits a call out is held to what it was.  Run with -m gpu."""
import numpy as np
import pytest

import clahe_ref as R
import synth

pytestmark = pytest.mark.gpu

DT = 0.0666
STEPS = 12
# which steps each of the six sequences takes a frame at: two at full rate, two at half rate, two dropping frames irregularly (gaps of up to three frames)
SCHEDULE = {0: set(range(STEPS)), 3: set(range(STEPS)), 1: set(range(0, STEPS, 2)), 4: set(range(0, STEPS, 2)),
            2: {0, 2, 3, 6, 7, 8, 9, 10, 11}, 5: {0, 1, 3, 4, 7, 8, 9, 11}}
ROUTES = ("host", "device", "prefetch")
_REF = {}


def _same(o, g, what):
    assert np.array_equal(o[0], g[0]), "%s: feature id lists differ" % what
    assert np.array_equal(o[1].view(np.uint64), g[1].view(np.uint64)), "%s: observations differ" % what


def _same_state(a, b, what):
    assert len(a) == len(b) == 3 and all(np.array_equal(x, y) for x, y in zip(a, b)), "%s: state differs" % what


def _state_copy(st):
    return tuple(np.array(x, copy=True) for x in st)


def _rotated(listed, k):
    """the list in another order on every call: the order of a list carries no meaning"""
    r = k % len(listed)
    return listed[r:] + listed[:r]


def _reference(oracle, w, h, max_cnt, min_dist, equalize=False, depth_cam=1):
    """frames, the constant depth image and, per (sequence, step taken), what that sequence's own oracle returned and its state afterwards"""
    key = (w, h, max_cnt, min_dist, equalize, depth_cam)
    if key not in _REF:
        frames = [synth.tracker_sequence(1000 + b, STEPS, w, h) for b in range(6)]
        depth = np.full((h, w), 1500, np.uint16)
        ref = {}
        for b in range(6):
            otr = oracle.Tracker(oracle.default_cfg(max_cnt=max_cnt, min_dist=min_dist, depth_cam=depth_cam))
            for k in sorted(SCHEDULE[b]):
                f = frames[b][k]
                res = otr.track(DT * k, R.clahe(f) if equalize else f, depth)
                ref[b, k] = (res, _state_copy(otr.state()))
        _REF[key] = (frames, depth, ref)
    return _REF[key]


def _run_schedule(gf, oracle, route, w, h, max_cnt, min_dist, floor, equalize=False):
    import torch
    frames, depth, ref = _reference(oracle, w, h, max_cnt, min_dist, equalize)
    gtr = gf.FeatureTracker(gf.default_cfg(width=w, height=h, batch=6, max_cnt=max_cnt, min_dist=min_dist, equalize=int(equalize)))
    lists = [_rotated([b for b in range(6) if k in SCHEDULE[b]], k) for k in range(STEPS)]
    assert min(len(l) for l in lists) == 2 and max(len(l) for l in lists) == 6 and len({tuple(sorted(l)) for l in lists}) >= 5
    last = {}      # sequence -> its state after its latest frame
    keep = []      # page-locked frames stay alive until they are consumed

    def stage(k):
        g = torch.from_numpy(np.stack([frames[b][k] for b in lists[k]])).pin_memory()
        d = torch.from_numpy(np.stack([depth] * len(lists[k])).view(np.int16)).pin_memory()
        keep.append((g, d))
        gtr.prefetchHost(g.data_ptr(), d.data_ptr(), seqs=lists[k])

    if route == "prefetch":
        stage(0)
    listed_total = 0
    for k in range(STEPS):
        L = lists[k]
        ts = [DT * k] * len(L)
        if route == "host":
            res = gtr.trackImageSome(L, ts, [frames[b][k] for b in L], [depth] * len(L))
        elif route == "device":
            dg = torch.from_numpy(np.stack([frames[b][k] for b in L])).cuda()
            dd = torch.from_numpy(np.stack([depth] * len(L)).view(np.int16)).cuda()
            torch.cuda.synchronize()
            res = gtr.trackImageSomeDevice(L, ts, dg.data_ptr(), dd.data_ptr())
        else:
            if k + 1 < STEPS:
                stage(k + 1)      # the next frame, for another set of sequences, travels while this one is tracked
            res = gtr.trackPrefetched(ts)
        assert len(res) == len(L)
        listed_total += len(L)
        for i, b in enumerate(L):
            o, ostate = ref[b, k]
            _same(o, res[i], "step %d, sequence %d (list position %d)" % (k, b, i))
            if b in last:       # not the sequence's first frame: the tracks must have come through, however long it sat out
                carried = int((gtr.state(b)[1] > 1).sum())
                if floor is not None:
                    assert carried >= floor, "step %d, sequence %d: %d carried tracks" % (k, b, carried)
                    assert len(res[i][0]) == max_cnt
            last[b] = ostate
        for b in range(6):      # listed or not: every sequence's state is that of its own oracle after its latest frame
            _same_state(last[b], gtr.state(b), "step %d, sequence %d%s" % (k, b, "" if b in L else " (not listed)"))
    st = gtr.stats()
    assert st["frames"] == STEPS and st["sequence_frames"] == listed_total == sum(len(v) for v in SCHEDULE.values())
    gtr.close()


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("max_cnt,min_dist,floor", [(150, 30, 120), (500, 12, 450)])
def test_schedules_bit_exact(gf, oracle, max_cnt, min_dist, floor, route):
    """cameras at full rate, at half rate and dropping frames share one handle, through each of the three entry points.  A slot that is one number per handle
    fails here: a sequence that sat out an odd number of calls would read its previous frame from the wrong pyramid.  The floors (carried tracks, track_cnt > 1,
    of 150 / 500 on every frame after a sequence's first) sit below what the oracle alone carries on these seeds and schedules (136 of 150, 471 of 500)."""
    _run_schedule(gf, oracle, route, 640, 480, max_cnt, min_dist, floor)


@pytest.mark.parametrize("w,h,equalize,env,route", [
    (752, 480, False, None, "host"), (644, 481, False, None, "device"), (752, 480, True, None, "device"),
    (752, 480, False, "GF_LK_POINTS=4", "host"), (752, 480, False, "GF_PYR_HEAD=0", "prefetch"), (752, 480, False, "GF_SELECT_TOPK=0", "host")],
    ids=["752x480", "644x481", "752x480-equalize", "752x480-GF_LK_POINTS=4", "752x480-GF_PYR_HEAD=0", "752x480-GF_SELECT_TOPK=0"])
def test_schedules_in_the_other_forms(gf, oracle, monkeypatch, w, h, equalize, env, route):
    """the same schedule on the byte-wise pyramid kernels (752 x 480), the dword level 0 (644 x 481), behind the equalisation (the oracle gets frames equalised by
    clahe_ref) and under each kept kernel variant.  Oracle alone: 139 / 137 of 150 carried at 752 x 480 / 644 x 481."""
    if env:
        monkeypatch.setenv(*env.split("="))
    _run_schedule(gf, oracle, route, w, h, 150, 30, None if equalize else 120, equalize)


def test_late_start_and_early_stop(gf, oracle):
    """sequence 1 gets its first frame at step 4 (no previous frame: detector only), sequence 2 stops after step 7 while the others go on"""
    K = 10
    takes = {0: range(K), 1: range(4, K), 2: range(0, 8)}
    frames = [synth.tracker_sequence(1010 + b, K) for b in range(3)]
    depth = np.full(frames[0][0].shape, 1200, np.uint16)
    otrs = [oracle.Tracker(oracle.default_cfg()) for _ in range(3)]
    gtr = gf.FeatureTracker(gf.default_cfg(batch=3))
    stopped = None
    for k in range(K):
        L = [b for b in (2, 0, 1) if k in takes[b]]
        res = gtr.trackImageSome(L, [DT * k] * len(L), [frames[b][k] for b in L], [depth] * len(L))
        for i, b in enumerate(L):
            _same(otrs[b].track(DT * k, frames[b][k], depth), res[i], "step %d, sequence %d" % (k, b))
        for b in range(3):
            _same_state(otrs[b].state(), gtr.state(b), "step %d, sequence %d" % (k, b))
        if k < 4:
            assert len(gtr.state(1)[0]) == 0
        if k == 4:
            assert len(res[L.index(1)][0]) == 150 and gtr.state(1)[1].max() == 1
        if k == 7:
            stopped = _state_copy(gtr.state(2))
            assert len(stopped[0]) == 150 and stopped[1].max() == 8
        if k > 7:
            _same_state(stopped, gtr.state(2), "step %d: the stopped sequence" % k)
    gtr.close()


def test_the_list_form_is_the_lock_step_form(gf, oracle):
    B, K = 4, 5
    frames = [synth.tracker_sequence(1020 + b, K) for b in range(B)]
    depth = [np.full(frames[0][0].shape, 900 + 100 * b, np.uint16) for b in range(B)]
    lock, inorder, permuted = (gf.FeatureTracker(gf.default_cfg(batch=B)) for _ in range(3))
    perm = [2, 0, 3, 1]
    for k in range(K):
        ts = [DT * k + 0.001 * b for b in range(B)]
        a = lock.trackImageBatch(ts, [frames[b][k] for b in range(B)], depth)
        b_ = inorder.trackImageSome(list(range(B)), ts, [frames[b][k] for b in range(B)], depth)
        c = permuted.trackImageSome(perm, [ts[b] for b in perm], [frames[b][k] for b in perm], [depth[b] for b in perm])
        for b in range(B):
            _same(a[b], b_[b], "step %d, sequence %d, listed in order" % (k, b))
            _same(a[b], c[perm.index(b)], "step %d, sequence %d, permuted list" % (k, b))
            _same_state(lock.state(b), inorder.state(b), "in order")
            _same_state(lock.state(b), permuted.state(b), "permuted")
        assert min(len(x[0]) for x in a) == 150
    assert lock.stats()["sequence_frames"] == inorder.stats()["sequence_frames"] == permuted.stats()["sequence_frames"] == B * K
    for t in (lock, inorder, permuted):
        t.close()


def _predict(rng, cfg, ids, pts, garbage):
    """predictions for 70 % of the tracks, a pixel of noise around where they are; garbage: every track predicted far outside the image, so that the forward pass
    from there fails for all of them"""
    sel = np.ones(len(ids), bool) if garbage else rng.random(len(ids)) < 0.7
    uv = pts[sel] + (5000.0 if garbage else rng.normal(0, 1.0, (sel.sum(), 2)))
    xyz = np.stack([(uv[:, 0] - cfg.cx) / cfg.fx * 2.0, (uv[:, 1] - cfg.cy) / cfg.fy * 2.0, np.full(len(uv), 2.0)], 1)
    return ids[sel], xyz


def test_pending_prediction_survives_sitting_out(gf, oracle):
    """setPrediction / removeOutliers on a sequence that then sits out two calls: the prediction is used at its next frame (hasPrediction is cleared only inside
    trackImage, feature_tracker.cpp:312).  Later one listed sequence gets garbage predictions, so that it alone takes the three-level fallback
    (feature_tracker.cpp:124-132) while a neighbour with good predictions and one without any share the call.  Every sequence consumes its own frames in order."""
    B = 3
    frames = [synth.tracker_sequence(1030 + b, 8) for b in range(B)]
    otrs = [oracle.Tracker(oracle.default_cfg(depth_cam=0)) for _ in range(B)]
    gtr = gf.FeatureTracker(gf.default_cfg(batch=B, depth_cam=0))
    cfg = gtr.cfg
    rng = np.random.default_rng(11)
    nxt = [0] * B

    def step(L, launches):
        before = gtr.stats()["lk_launches"]
        ts = [DT * nxt[b] for b in L]
        res = gtr.trackImageSome(L, ts, [frames[b][nxt[b]] for b in L])
        for i, b in enumerate(L):
            _same(otrs[b].track(ts[i], frames[b][nxt[b]], None), res[i], "sequence %d, its frame %d" % (b, nxt[b]))
            assert len(res[i][0]) == 150
            nxt[b] += 1
        for b in range(B):
            _same_state(otrs[b].state(), gtr.state(b), "sequence %d" % b)
        assert gtr.stats()["lk_launches"] - before == launches

    def feedback(b, garbage=False):
        ids = otrs[b].state()[0]
        rm = ids[rng.random(len(ids)) < 0.05]
        otrs[b].remove_outliers(rm); gtr.removeOutliers(rm, seq=b)
        ids, _, pts = otrs[b].state()
        pid, xyz = _predict(rng, cfg, ids, pts, garbage)
        otrs[b].set_prediction(pid, xyz); gtr.setPrediction(pid, xyz, seq=b)

    step([0, 1, 2], 0)       # first frames: nothing to track
    step([0, 1, 2], 1)
    feedback(1)
    step([2, 0], 1)          # sequence 1 sits out twice with its prediction pending
    step([0, 2], 1)
    step([2, 1, 0], 2)       # ... and starts from it here: the plain launch for 0 and 2, the predicted one for 1
    feedback(0, garbage=True)   # fewer than 10 forward successes
    feedback(1)
    step([1, 2, 0], 3)       # plain (2), predicted (0, 1), and the fallback relaunch for 0 alone
    step([0, 1, 2], 1)
    gtr.close()


def test_refused_calls_change_nothing(gf, oracle):
    import torch
    B = 3
    frames = [synth.tracker_sequence(1040 + b, 4) for b in range(B)]
    depth = np.full(frames[0][0].shape, 1000, np.uint16)
    otrs = [oracle.Tracker(oracle.default_cfg()) for _ in range(B)]
    gtr = gf.FeatureTracker(gf.default_cfg(batch=B))

    def valid(k, L):
        res = gtr.trackImageSome(L, [DT * k] * len(L), [frames[b][k] for b in L], [depth] * len(L))
        for i, b in enumerate(L):
            _same(otrs[b].track(DT * k, frames[b][k], depth), res[i], "step %d, sequence %d" % (k, b))

    valid(0, [0, 1, 2])
    valid(1, [1, 0])
    before = [_state_copy(gtr.state(b)) for b in range(B)]
    stats = gtr.stats()
    img = frames[0][2]
    dev = torch.from_numpy(np.stack([img] * 4)).cuda()
    pin = torch.from_numpy(np.stack([img] * 4)).pin_memory()
    torch.cuda.synchronize()
    bad = [([0, 3], "names sequence 3"), ([-1], "names sequence -1"), ([1, 2, 1], "listed twice"), ([0, 1, 2, 0], "4 sequences listed")]
    for L, msg in bad:
        with pytest.raises(gf.GfError, match="gf status -1.*" + msg):
            gtr.trackImageSome(L, [1.0] * len(L), [img] * len(L), [depth] * len(L))
        with pytest.raises(gf.GfError, match="gf status -1.*" + msg):
            gtr.trackImageSomeDevice(L, [1.0] * len(L), dev.data_ptr())
        with pytest.raises(gf.GfError, match="gf status -1.*" + msg):
            gtr.prefetchHost(pin.data_ptr(), seqs=L)
    with pytest.raises(gf.GfError, match="gf status -1.*null image"):
        gtr.trackImageSome([2, 0], [1.0, 1.0], [img, None], [depth, depth])
    with pytest.raises(gf.GfError, match="gf status -1"):       # nothing was staged by the refused prefetches
        gtr.trackPrefetched([1.0] * B)
    assert gtr.trackImageSome([], [], []) == [] and len(gtr.trackImageSomeDevice([], [], dev.data_ptr())) == 0     # count == 0: accepted, nothing happens
    for b in range(B):
        _same_state(before[b], gtr.state(b), "sequence %d after the refused calls" % b)
    assert gtr.stats()["frames"] == stats["frames"] and gtr.stats()["sequence_frames"] == stats["sequence_frames"] == 5
    valid(2, [2, 0, 1])      # sequence 2 after sitting out, the others as usual: still the oracle's bits
    valid(3, [1, 2])
    for b in range(B):
        _same_state(otrs[b].state(), gtr.state(b), "sequence %d at the end" % b)
    gtr.close()


def test_a_full_machine_with_a_quarter_listed(gf, oracle):
    """batch 256 at VGA through the device entry point: sequences 0..7 take every frame, 64 of the other 248 are listed per call in rotation (each of them every
    third or fourth call).  Sequence b sees the frames of seed 1000 + b % 16, at its own steps; a fixed sample of 16 sequences is held to its oracle."""
    import torch
    B, K, NSEED = 256, 8, 16
    frames = [synth.tracker_sequence(1000 + s, K) for s in range(NSEED)]
    h, w = frames[0][0].shape
    depth = np.full((h, w), 1500, np.uint16)
    sample = [0, 3, 7, 8, 9, 40, 71, 72, 100, 135, 136, 199, 200, 231, 254, 255]
    otrs = {b: oracle.Tracker(oracle.default_cfg()) for b in sample}
    gtr = gf.FeatureTracker(gf.default_cfg(batch=B))
    dd = torch.from_numpy(np.stack([depth] * 72).view(np.int16)).cuda()
    taken = dict.fromkeys(sample, 0)
    total = 0
    for k in range(K):
        L = list(range(8)) + [8 + (64 * k + j) % 248 for j in range(64)]
        assert len(set(L)) == 72
        L = _rotated(L, 5 * k)
        dg = torch.from_numpy(np.stack([frames[b % NSEED][k] for b in L])).cuda()
        torch.cuda.synchronize()
        res = gtr.trackImageSomeDevice(L, [DT * k] * len(L), dg.data_ptr(), dd.data_ptr())
        total += len(L)
        assert all(len(r[0]) == 150 for r in res)
        for i, b in enumerate(L):
            if b in otrs:
                _same(otrs[b].track(DT * k, frames[b % NSEED][k], depth), res[i], "step %d, sequence %d" % (k, b))
                taken[b] += 1
        for b in sample:
            _same_state(otrs[b].state(), gtr.state(b), "step %d, sequence %d" % (k, b))
    assert all(taken[b] == K for b in sample if b < 8) and all(2 <= taken[b] <= 3 for b in sample if b >= 8), taken
    st = gtr.stats()
    assert st["sequence_frames"] == total == 72 * K and st["frames"] == K
    gtr.close()


def test_track_image_of_one_sequence_on_a_batch_handle(gf, oracle):
    """gf_tracker_track on a batch-4 handle is the list of one; the four sequences interleaved irregularly, each consuming its own frames in order"""
    B = 4
    order = [0, 1, 0, 2, 3, 3, 1, 0, 2, 2, 1, 3, 0, 0, 2, 1, 3, 3, 2, 1]
    frames = [synth.tracker_sequence(1050 + b, order.count(b)) for b in range(B)]
    depth = [np.full(frames[0][0].shape, 700 + 50 * b, np.uint16) for b in range(B)]
    otrs = [oracle.Tracker(oracle.default_cfg()) for _ in range(B)]
    gtr = gf.FeatureTracker(gf.default_cfg(batch=B))
    nxt = [0] * B
    for n, b in enumerate(order):
        f, t = frames[b][nxt[b]], DT * nxt[b]
        _same(otrs[b].track(t, f, depth[b]), gtr.trackImage(t, f, depth[b], seq=b), "call %d, sequence %d" % (n, b))
        nxt[b] += 1
        for c in range(B):
            _same_state(otrs[c].state(), gtr.state(c), "call %d, sequence %d" % (n, c))
    assert gtr.stats()["sequence_frames"] == gtr.stats()["frames"] == len(order) and gtr.state(0)[1].max() == order.count(0)
    gtr.close()
