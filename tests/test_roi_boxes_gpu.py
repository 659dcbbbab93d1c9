"""Exclusion boxes per sequence and frame (gf_tracker_set_boxes_some / _get_boxes, gf_roi_boxes_batch, gf_estimator_set_boxes, gf_replay --boxes): the region in
force is R_eff = R_base AND NOT union(boxes), composed on the device.  Every comparison is byte for byte or bit for bit:
    1  gf_roi_boxes_batch (the composing kernel's bits) against the Python raster of tests/roi_boxes_ref.py, on the hard lists
    2  the tracker with set_boxes before every frame against tests/roi_tracker_ref.cpp's tracker given set_roi(raster of that frame's boxes AND base)
    3  the same bits through every entry point
    4  the order of the setters, 5 refusals, 7 estimator and gf_replay
A tracker case counts only if the helper drops at least one track for lying in a box and, on every frame after the first, at least a third of max_cnt ids carry
over from the frame before; both are asserted on the helper's side.  Run with -m gpu."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import roi_boxes_ref as BR
import roi_ref as RR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.0666
SMALL = RR.SIZES[0]   # 132 x 97


@pytest.fixture(scope="module")
def ref(oracle, tmp_path_factory):
    return RR.build(tmp_path_factory.mktemp("roi_boxes_ref"))


def _ocfg(oracle, case, **kw):
    return oracle.default_cfg(max_cnt=case[2], min_dist=case[3], **kw)


def _gcfg(gf, case, **kw):
    return gf.default_cfg(width=case[0], height=case[1], max_cnt=case[2], min_dist=case[3], **kw)


def _base(name, w, h):
    return RR.region(name, w, h) if name else None


def _drops_in_a_box(oracle, ref, case, name, video, boxes_of, k):
    """How many tracks the helper drops at frame k for lying in a box and nowhere else: two helpers take frames 0 .. k - 1 with the same regions, then one takes
    frame k with the boxes and the other with the base alone; both start that frame from one state and LK gives them the same points, so the difference of
    their drop counts is the points on pixels that the base allows and a box excludes"""
    w, h = case[:2]
    base = _base(name, w, h)
    counts = []
    for with_boxes in (True, False):
        tr = RR.Tracker(ref, _ocfg(oracle, case))
        for j in range(k + 1):
            tr.set_roi(BR.raster(boxes_of(j), w, h, base) if j < k or with_boxes else base)
            before = tr.dropped_outside()
            tr.track(DT * j, video[j], RR.depth(j, w, h))
        counts.append(tr.dropped_outside() - before)
    return counts[0] - counts[1]


_RUNS = {}


def _helper_run(oracle, ref, case, name, seed=0, boxes_of=None, check=True, gray_of=None):
    """the helper over the K shared frames with set_roi(raster of frame k's boxes AND base `name`) before frame k: [(ids, obs, state)], computed once.
    boxes_of(k): the frame's boxes (default: BR.moving_boxes); check: assert the conditions of a case"""
    key = (case, name, seed, boxes_of, gray_of)
    if key not in _RUNS:
        w, h, max_cnt = case[:3]
        base = _base(name, w, h)
        of = boxes_of or (lambda k: BR.moving_boxes(w, h, k))
        video = RR.frames(w, h, seed=seed)
        if gray_of:
            video = [gray_of(f) for f in video]
        tr = RR.Tracker(ref, _ocfg(oracle, case))
        out, prev = [], None
        for k, f in enumerate(video):
            R = BR.raster(of(k), w, h, base)
            tr.set_roi(R)
            ids, obs = tr.track(DT * k, f, RR.depth(k, w, h))
            if check:
                assert RR.on_excluded(obs, R) == 0
                assert prev is None or 3 * len(np.intersect1d(ids, prev)) >= max_cnt, "frame %d: too few ids carried over" % k
            prev = ids
            out.append((ids, obs, tr.state()))
        if check:
            assert tr.dropped_outside() >= 1
            assert any(_drops_in_a_box(oracle, ref, case, name, video, of, k) >= 1 for k in range(1, RR.K)), "the helper dropped no track for lying in a box"
        _RUNS[key] = out
    return _RUNS[key]


def _same_frame(expect, got, state, what):
    RR.same(expect[:2], got, what)
    assert all(np.array_equal(a, b) for a, b in zip(expect[2], state)), "%s: state differs" % what


# ---- 1
@pytest.mark.parametrize("size", BR.GPU_SIZES, ids=lambda s: "%dx%d" % s)
def test_composing_kernel_against_the_raster(gf, size):
    """every hard list with no base and with regions A and B, in one batch of mixed list lengths (zero and the cap among them)"""
    w, h = size
    lists, bases, names = [], [], []
    for bname, base in BR.bases(w, h).items():
        for lname, l in BR.hard_lists(w, h).items():
            lists.append(l); bases.append(base); names.append("%s / %s" % (lname, bname))
    assert {len(l) for l in lists} >= {0, 1, BR.CAP}
    white = np.full((h, w), 255, np.uint8)
    got = gf.roi_boxes_batch(lists, w, h, np.stack([white if b is None else b for b in bases]))
    plain = gf.roi_boxes_batch(lists[:len(BR.hard_lists(w, h))], w, h)   # no base masks at all
    for i, name in enumerate(names):
        expect = BR.raster(lists[i], w, h, bases[i])
        assert np.array_equal(got[i], expect), "%s: %d pixels differ" % (name, int((got[i] != expect).sum()))
        if bases[i] is None:
            assert np.array_equal(plain[i], expect), "%s without base masks" % name
    assert any((BR.raster(l, w, h) == 0).any() for l in lists)


def test_composing_kernel_at_widths_that_are_no_multiple_of_four(gf):
    """gf_roi_boxes_batch takes any width >= 1 and height >= 1: the lanes' words start at every phase of a 16-byte piece"""
    for w, h in [(33, 1), (1, 31), (7, 95), (1030, 31), (61, 64)]:
        hl = BR.hard_lists(w, h)
        lists = list(hl.values())
        base = np.random.default_rng(w).integers(0, 2, (len(lists), h, w)).astype(np.uint8)
        got = gf.roi_boxes_batch(lists, w, h, base)
        for i, name in enumerate(hl):
            assert np.array_equal(got[i], BR.raster(lists[i], w, h, base[i])), "%d x %d, %s" % (w, h, name)


# ---- 2
@pytest.mark.parametrize("name", ["A", None], ids=["base_A", "no_base"])
@pytest.mark.parametrize("case", RR.SIZES, ids=RR.size_id)
def test_six_frames_of_moving_boxes_against_the_helper(gf, oracle, ref, case, name):
    w, h = case[:2]
    base = _base(name, w, h)
    expect = _helper_run(oracle, ref, case, name)
    gtr = gf.FeatureTracker(_gcfg(gf, case))
    if name:
        gtr.set_roi(base)
    for k, f in enumerate(RR.frames(w, h)):
        boxes = BR.moving_boxes(w, h, k)
        assert 1 <= len(boxes) <= 3
        gtr.set_boxes(boxes)
        assert np.array_equal(gtr.get_boxes(), np.array(boxes, np.int32))
        g = gtr.trackImage(DT * k, f, RR.depth(k, w, h))
        R = BR.raster(boxes, w, h, base)
        assert RR.on_excluded(g[1], R) == 0, "frame %d: a reported point on an excluded pixel" % k
        assert np.array_equal(gtr.get_roi(), R)
        _same_frame(expect[k], g, gtr.state(), "frame %d" % k)
    gtr.close()


# ---- 3
@pytest.mark.parametrize("entry", ["prefetched", "device", "device_refs", "some", "colour", "equalize"])
def test_every_entry_point(gf, oracle, ref, entry):
    """(host frames: test_six_frames_of_moving_boxes_against_the_helper)"""
    import torch
    case = SMALL
    w, h = case[:2]
    video = RR.frames(w, h)
    gray_of = None
    if entry == "equalize":
        import clahe_ref
        gray_of = clahe_ref.clahe
    expect = _helper_run(oracle, ref, case, "A", gray_of=gray_of, check=gray_of is None)
    gtr = gf.FeatureTracker(_gcfg(gf, case, equalize=int(entry == "equalize"), pixel_format=gf.PIX_BGR8 if entry == "colour" else 0))
    gtr.set_roi(RR.region("A", w, h))
    if entry == "prefetched":
        pg = [torch.from_numpy(f[None].copy()).pin_memory() for f in video]
        pd = [torch.from_numpy(RR.depth(k, w, h)[None].view(np.int16).copy()).pin_memory() for k in range(RR.K)]
        gtr.prefetchHost(pg[0].data_ptr(), pd[0].data_ptr())
    for k, f in enumerate(video):
        d = RR.depth(k, w, h)
        gtr.set_boxes_some([0], [BR.moving_boxes(w, h, k)])
        if entry == "prefetched":
            if k + 1 < RR.K:
                gtr.prefetchHost(pg[k + 1].data_ptr(), pd[k + 1].data_ptr())
            g = gtr.trackPrefetched([DT * k])[0]
        elif entry in ("device", "device_refs"):
            dg, dd = torch.from_numpy(f[None].copy()).cuda(), torch.from_numpy(d[None].view(np.int16).copy()).cuda()
            torch.cuda.synchronize()
            if entry == "device":
                g = gtr.trackImageBatchDevice([DT * k], dg.data_ptr(), dd.data_ptr())[0]
            else:
                g = gtr.trackImageSomeDeviceRefs([0], [DT * k], [(dg.data_ptr(), w)], [(dd.data_ptr(), 2 * w)])[0]
        elif entry == "some":
            g = gtr.trackImageSome([0], [DT * k], [f], [d])[0]
        elif entry == "colour":
            g = gtr.trackImage(DT * k, np.repeat(f[:, :, None], 3, 2), d)   # equal channels convert to the gray value itself
        else:
            g = gtr.trackImage(DT * k, f, d)
        _same_frame(expect[k], g, gtr.state(), "%s frame %d" % (entry, k))
    gtr.close()


def _static_boxes(w, h, b):
    """a list of its own for sequence b of the batch-5 handle; that of sequence 3 is empty"""
    return [[(w // 5, h // 6, w // 2, h // 3)], [(w // 2, h // 4, w - 10, h // 2), (3, 3, 20, 20)], [(-5, h // 2, w // 3, h + 5)], [],
            [(w // 3, 10, w // 3 + 30, 50), (10, h // 2, 40, h // 2 + 20), (w - 30, 5, w + 9, 30)]][b]


def test_batch_of_five_with_a_list_per_sequence_and_a_sequence_that_sits_out(gf, oracle, ref):
    """five sequences, each with its own boxes (one with none) that stay; sequence 1 sits out two calls and its boxes hold for its next frame; every sequence
    equals its own single-sequence helper"""
    case = SMALL
    w, h = case[:2]
    of = [(lambda b: (lambda k: _static_boxes(w, h, b)))(b) for b in range(5)]
    seeds = (0, 1, 0, 1, 2)
    expect = []
    for b in range(5):
        tr = RR.Tracker(ref, _ocfg(oracle, case))
        tr.set_roi(BR.raster(of[b](0), w, h))
        run = []
        for k, f in enumerate(RR.frames(w, h, seed=seeds[b])):
            r = tr.track(DT * k, f, RR.depth(k, w, h))
            run.append(r + (tr.state(),))
        expect.append(run)
    video = [RR.frames(w, h, seed=s) for s in seeds]
    gtr = gf.FeatureTracker(_gcfg(gf, case, batch=5))
    gtr.set_boxes_some([4, 0, 3, 1, 2], [of[b](0) for b in (4, 0, 3, 1, 2)])
    for b in range(5):
        assert np.array_equal(gtr.get_boxes(b), np.array(of[b](0), np.int32).reshape(-1, 4))
    assert gtr.get_roi(3) is None and gtr.get_roi(0) is not None
    lists = [[0, 1, 2, 3, 4], [4, 2, 0, 3], [3, 0, 2, 4], [1, 0, 2, 3, 4], [0, 1, 2, 3, 4], [1, 4, 3, 2, 0], [1, 2, 3, 4, 0], [1]]
    done = [0] * 5
    for call, seqs in enumerate(lists):
        seqs = [s for s in seqs if done[s] < RR.K]
        res = gtr.trackImageSome(seqs, [DT * done[s] for s in seqs], [video[s][done[s]] for s in seqs], [RR.depth(done[s], w, h) for s in seqs])
        for i, s in enumerate(seqs):
            _same_frame(expect[s][done[s]], res[i], gtr.state(s), "call %d, sequence %d frame %d" % (call, s, done[s]))
            done[s] += 1
    assert done == [RR.K] * 5, done
    gtr.close()


# ---- 4
def test_order_of_the_setters(gf, oracle, ref):
    """base after boxes, boxes after base, boxes cleared (the base bits are back), base cleared (the boxes stay), reset_seq (the boxes stay), and a sequence that
    is not listed keeps what it had -- each through get_roi and through a tracked frame against the helper given the raster"""
    case = SMALL
    w, h = case[:2]
    A, B = RR.region("A", w, h), RR.region("B", w, h)
    b1, b2 = BR.moving_boxes(w, h, 1), BR.moving_boxes(w, h, 4)
    # (what the library is told before frame k, the region in force then)
    plan = [(lambda g: (g.set_boxes(b1), g.set_roi(A)), BR.raster(b1, w, h, A)),            # base after boxes
            (lambda g: (g.set_roi(B), g.set_boxes(b2)), BR.raster(b2, w, h, B)),            # boxes after base
            (lambda g: g.set_boxes([]), B),                                                  # cleared: the base bits are back
            (lambda g: (g.set_boxes(b1), g.set_roi(None)), BR.raster(b1, w, h)),            # the base cleared: the boxes stay
            (lambda g: g.set_boxes_some([1], [b2]), BR.raster(b1, w, h)),                   # sequence 0 is not listed
            (lambda g: g.set_boxes_some([0, 1], None), None)]                               # all listed cleared
    rtr = RR.Tracker(ref, _ocfg(oracle, case))
    gtr = gf.FeatureTracker(_gcfg(gf, case, batch=2))
    for k, f in enumerate(RR.frames(w, h)):
        act, R = plan[k]
        act(gtr)
        rtr.set_roi(R)
        got = gtr.get_roi(0)
        assert (got is None and R is None) or np.array_equal(got, R), "frame %d: get_roi" % k
        d = RR.depth(k, w, h)
        r = rtr.track(DT * k, f, d)
        _same_frame(r + (rtr.state(),), gtr.trackImage(DT * k, f, d), gtr.state(), "frame %d" % k)
    assert rtr.dropped_outside() >= 1
    assert len(gtr.get_boxes(0)) == 0 and len(gtr.get_boxes(1)) == 0 and gtr.get_roi(1) is None
    # reset_seq keeps the boxes: the sequence starts over under them
    gtr.set_boxes(b2)
    gtr.reset_seq(0)
    assert np.array_equal(gtr.get_boxes(0), np.array(b2, np.int32)) and np.array_equal(gtr.get_roi(0), BR.raster(b2, w, h))
    rtr = RR.Tracker(ref, _ocfg(oracle, case))
    rtr.set_roi(BR.raster(b2, w, h))
    for k, f in enumerate(RR.frames(w, h)[:3]):
        d = RR.depth(k, w, h)
        r = rtr.track(DT * k, f, d)
        _same_frame(r + (rtr.state(),), gtr.trackImage(DT * k, f, d), gtr.state(), "after reset_seq, frame %d" % k)
    gtr.close()


def test_device_setters_of_the_base_recompose_under_the_boxes(gf, oracle, ref):
    """gf_tracker_set_roi_some_device and _refs on sequences that have boxes: the masks are packed into the base table and the boxes stay in force over them;
    clearing the base through the device setter leaves the boxes"""
    import torch
    case = SMALL
    w, h = case[:2]
    A, B = RR.region("A", w, h), RR.region("B", w, h)
    b0, b1 = BR.moving_boxes(w, h, 2), BR.moving_boxes(w, h, 3)
    gtr = gf.FeatureTracker(_gcfg(gf, case, batch=2))
    gtr.set_boxes_some([0, 1], [b0, b1])
    d_masks = torch.from_numpy(np.stack([A, B])).cuda()
    torch.cuda.synchronize()
    gtr.set_roi_device([1, 0], d_masks.data_ptr())     # A for sequence 1, B for sequence 0
    assert np.array_equal(gtr.get_roi(0), BR.raster(b0, w, h, B)) and np.array_equal(gtr.get_roi(1), BR.raster(b1, w, h, A))
    rtr = [RR.Tracker(ref, _ocfg(oracle, case)) for _ in range(2)]
    rtr[0].set_roi(BR.raster(b0, w, h, B)); rtr[1].set_roi(BR.raster(b1, w, h, A))
    video = RR.frames(w, h)

    def frame(k):
        d = RR.depth(k, w, h)
        res = gtr.trackImageBatch([DT * k] * 2, [video[k]] * 2, [d, d])
        for s in range(2):
            r = rtr[s].track(DT * k, video[k], d)
            _same_frame(r + (rtr[s].state(),), res[s], gtr.state(s), "sequence %d frame %d" % (s, k))

    frame(0); frame(1)
    gtr.set_roi_device_refs([0, 1], [(d_masks[0].data_ptr(), w), (d_masks[1].data_ptr(), w)])   # now A for sequence 0, B for sequence 1
    rtr[0].set_roi(BR.raster(b0, w, h, A)); rtr[1].set_roi(BR.raster(b1, w, h, B))
    assert np.array_equal(gtr.get_roi(0), BR.raster(b0, w, h, A)) and np.array_equal(gtr.get_roi(1), BR.raster(b1, w, h, B))
    frame(2); frame(3)
    gtr.set_roi_device([0], None)                      # the base of sequence 0 cleared: its boxes stay
    rtr[0].set_roi(BR.raster(b0, w, h))
    assert np.array_equal(gtr.get_roi(0), BR.raster(b0, w, h)) and np.array_equal(gtr.get_roi(1), BR.raster(b1, w, h, B))
    frame(4); frame(5)
    assert rtr[0].dropped_outside() >= 1 and rtr[1].dropped_outside() >= 1
    gtr.close()


# ---- 5
def test_refused_calls_change_nothing(gf, oracle, ref):
    case = SMALL
    w, h = case[:2]
    L, INVALID = gf.lib(), -1
    expect = _helper_run(oracle, ref, case, "A")
    gtr = gf.FeatureTracker(_gcfg(gf, case, batch=2))
    video = RR.frames(w, h)

    def ints(*v):
        return (C.c_int * len(v))(*v)

    many = (gf.Box * (BR.CAP + 1))()
    one = (gf.Box * 4)(*[gf.Box(1, 1, 50, 50)] * 4)
    out, n = (gf.Box * 4)(), C.c_int(0)

    def refusals():
        S = L.gf_tracker_set_boxes_some
        return [S(None, 1, ints(0), ints(0, 1), one), S(gtr.h, -1, ints(0), ints(0, 1), one), S(gtr.h, 3, ints(0, 1, 0), ints(0, 1, 2, 3), one),
                S(gtr.h, 1, ints(2), ints(0, 1), one), S(gtr.h, 1, ints(-1), ints(0, 1), one), S(gtr.h, 2, ints(1, 1), ints(0, 1, 2), one),
                S(gtr.h, 1, ints(0), ints(1, 2), one), S(gtr.h, 2, ints(0, 1), ints(0, 2, 1), one), S(gtr.h, 1, ints(0), ints(0, BR.CAP + 1), many),
                S(gtr.h, 2, ints(0, 1), ints(0, 0, 1), None), S(gtr.h, 1, ints(0), None, one),
                L.gf_tracker_get_boxes(None, 0, out, 4, C.byref(n)), L.gf_tracker_get_boxes(gtr.h, 2, out, 4, C.byref(n)), L.gf_tracker_get_boxes(gtr.h, 0, out, 4, None)]

    # on a handle that has no boxes yet: still none afterwards
    assert refusals() == [INVALID] * 14
    assert len(gtr.get_boxes(0)) == 0 and gtr.get_roi(0) is None
    L.gf_tracker_set_boxes_some(gtr.h, 2, ints(0, 1), ints(0, 2, 1), one)
    assert b"list position 1" in L.gf_last_error()
    gtr.set_roi(RR.region("A", w, h))
    for k in range(RR.K):
        boxes = BR.moving_boxes(w, h, k)
        gtr.set_boxes(boxes)
        before = gtr.state()
        assert refusals() == [INVALID] * 14
        assert np.array_equal(gtr.get_boxes(0), np.array(boxes, np.int32)) and len(gtr.get_boxes(1)) == 0
        assert np.array_equal(gtr.get_roi(0), BR.raster(boxes, w, h, RR.region("A", w, h))) and gtr.get_roi(1) is None
        assert all(np.array_equal(a, b) for a, b in zip(before, gtr.state()))
        _same_frame(expect[k], gtr.trackImage(DT * k, video[k], RR.depth(k, w, h)), gtr.state(), "frame %d, after the refused calls" % k)
    gtr.close()


# ---- 6
def _odd_boxes(w, h):
    """lists a tracker would never produce: boxes over dots and strokes, box over box, degenerate, thin and off-frame boxes, extreme corners"""
    return [(10, 8, 40, 30), (25, 20, 60, 50), (25, 20, 60, 50), (5, 5, 5, 30), (7, 7, 8, 8), (9, 40, 12, 44), (50, 10, 56, 14), (30, 5, 20, 9), (-20, -20, 6, 6),
            (w - 9, h - 7, w + 30, h + 30), (w + 5, 0, w + 9, 9), (BR.I32_MIN, h // 2, BR.I32_MAX, h // 2 + 9), (w // 2, BR.I32_MIN, w // 2 + 7, BR.I32_MAX),
            (BR.I32_MIN, BR.I32_MIN, BR.I32_MIN + 1, BR.I32_MIN + 1), (BR.I32_MAX - 1, 3, BR.I32_MAX, 9), (0, 0, w - 1, h - 1), (0, 0, w, h)]


@pytest.mark.parametrize("size", [(64, 61), (132, 97), (70, 33)], ids=lambda s: "%dx%d" % s)
def test_picture_building_block_with_boxes_equals_the_restatement(gf, size):
    import track_draw_ref as TD
    w, h = size
    rng = np.random.default_rng(w)
    gray = rng.integers(0, 256, (3, h, w)).astype(np.uint8)
    lists = [TD.random_lists(rng, n, w, h) for n in (40, 0, 12)]
    odd = _odd_boxes(w, h)
    boxes = [odd, odd[:3], []]
    got = gf.draw_track(gray, lists, boxes=boxes)
    plain = gf.draw_track(gray, lists)
    for b in range(3):
        want = BR.render(gray[b], *lists[b], boxes=boxes[b])
        assert np.array_equal(got[b], want), "frame %d: %d pixels differ" % (b, int((got[b] != want).any(2).sum()))
    assert np.array_equal(got[2], plain[2]), "no boxes: today's picture"
    covered = (got[0] != plain[0]).any(2)
    assert covered.sum() > 100 and ((plain[0][covered] != gray[0][covered][:, None]).any(1)).sum() > 10, "no frame lies over a dot or a stroke"


def test_tracker_pictures_show_each_frame_s_own_boxes(gf):
    """show_track with moving boxes: every frame's picture is the restatement's for the states before and after the call and that frame's boxes; a second
    sequence without boxes gives today's picture; boxes set after the frame do not change its picture"""
    import track_draw_ref as TD
    case = SMALL
    w, h = case[:2]
    video = RR.frames(w, h)
    gtr = gf.FeatureTracker(_gcfg(gf, case, batch=2, depth_cam=0))
    gtr.set_show_track(True)     # before the first box setter: the rows of primitives grow with it
    for k, f in enumerate(video):
        boxes = BR.moving_boxes(w, h, k)
        gtr.set_boxes(boxes, seq=0)
        before = [gtr.state(b) for b in range(2)]
        gtr.trackImageBatch([DT * k] * 2, [f, f])
        for b in range(2):
            pts1, cnt1, prev, has = _lists_of(before[b], gtr.state(b))
            want = BR.render(f, pts1, cnt1, prev, has, boxes if b == 0 else ())
            assert np.array_equal(gtr.track_image(b), want), "frame %d, sequence %d" % (k, b)
            if b == 1:
                assert np.array_equal(want, TD.render(f, pts1, cnt1, prev, has))
        gtr.set_boxes([(0, 0, 20, 20)], seq=0)   # for the next frame: the recorded picture stays
        assert np.array_equal(gtr.track_image(0), BR.render(f, *_lists_of(before[0], gtr.state(0)), boxes=boxes)), "frame %d: a later setter changed the picture" % k
    gtr.close()


def _lists_of(before, after):
    ids0, _, pts0 = before
    ids1, cnt1, pts1 = after
    at = {int(i): j for j, i in enumerate(ids0)}
    has = np.array([int(i) in at for i in ids1], bool)
    prev = np.array([pts0[at[int(i)]] if int(i) in at else (0, 0) for i in ids1], np.float32).reshape(-1, 2)
    return pts1, cnt1, prev, has


# ---- 7
def test_replay_tool_boxes_option(gf, tmp_path):
    """the same box on every frame writes the vio.txt of --roi with that box's raster; a boxes file without lines writes the vio.txt of a run without the option"""
    import synth_stream as SS
    st = SS.Stream(1, t_still=1.0, t_move=1.0, v_max=0.4, yaw0=0.0, yaw_turn=-0.6, split_x=1.8, turn_delay=0.8)
    d = str(tmp_path)
    st.export(d)
    exe = os.path.join(ROOT, "bin", "gf_replay")
    assert os.path.exists(exe), "bin/gf_replay is missing: run `python __graft_entry__.py` (build)"
    box = (200, 150, 420, 330)
    pgm, every, none = os.path.join(d, "box.pgm"), os.path.join(d, "every.txt"), os.path.join(d, "none.txt")
    gf.write_pgm(pgm, BR.raster([box], 640, 480))
    with open(every, "w") as f:
        for t in st.cam_t:
            f.write("%r %d %d %d %d\n" % ((float(t),) + box))
    open(none, "w").close()
    cfg = os.path.join(d, "config.yaml")
    runs = {"plain": [], "roi": ["--roi", pgm], "boxes": ["--boxes", every], "none": ["--boxes", none]}
    vio = {}
    for name, opt in runs.items():
        out = os.path.join(d, "vio_%s.txt" % name)
        r = subprocess.run([exe] + opt + [cfg, d, out], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        vio[name] = open(out, "rb").read()
    assert len(vio["roi"]) > 0 and vio["boxes"] == vio["roi"], "--boxes with one box on every frame against --roi with its raster"
    assert vio["none"] == vio["plain"]
    assert vio["roi"] != vio["plain"], "the box changes nothing: the comparison shows nothing"


def test_estimator_without_a_tracker_refuses_the_boxes(gf):
    est = gf.SlidingWindowEstimator(gf.default_estimator_cfg())
    with pytest.raises(gf.GfError, match="without a tracker"):
        est.set_boxes([(1, 2, 30, 40)])
    est.close()
