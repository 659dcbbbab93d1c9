"""A frame size per sequence (gf_tracker_set_seq_size): sequences of different sizes in one handle, in shared launches.

The reference is twofold and bit for bit throughout (ids, observations viewed as uint64, state): the oracle's tracker at each sequence's size, and one
homogeneous handle per size, which is the code of a handle without sizes.  One handle of 644 x 481 holds six sequences of 644 x 481, 640 x 480, 640 x 160,
320 x 240, 64 x 48 and 40 x 36 with the max_cnt / min_dist of the matching rows of test_tracker_sizes_gpu.SIZES: every pyramid route, 1 to 4 levels, LK asking for
level 3 of a 2-level pyramid, a partial last strip and band of the detector, a frame of a single strip.  Run with -m gpu."""

import ctypes as C

import numpy as np
import pytest

import cvt_gray_ref as CR
import raw_gray_ref as RAW
from test_tracker_sizes_gpu import ROUTE, SIZES, _depth, _frames, route

pytestmark = pytest.mark.gpu

W, H = 644, 481
SIX = [(644, 481), (640, 480), (640, 160), (320, 240), (64, 48), (40, 36)]
PAR = {(c[0], c[1]): (c[4], c[5]) for c in SIZES}      # max_cnt, min_dist of the size's row
K = 6
DT = 0.0666
KB = ("KANNALA_BRANDT", [142.5, 143.25, 160.5, 120.25], [-0.9, 0.35, -0.05, 0.0025], 0.0)   # tests/test_camera_models_gpu.py


def _seed(size):
    return SIX.index(size) if size in SIX else 0


def _same(a, b, what):
    (ai, ao), (bi, bo) = a, b
    assert np.array_equal(ai, bi), "%s: feature id lists differ" % what
    assert np.array_equal(ao.view(np.uint64), bo.view(np.uint64)), "%s: observations differ" % what


def _same_state(a, b, what):
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), "%s: state differs" % what


def _homogeneous(gf, size, **kw):
    mc, md = PAR[size]
    return gf.FeatureTracker(gf.default_cfg(width=size[0], height=size[1], max_cnt=mc, min_dist=md, **kw))


def _mixed(gf, sizes=SIX, **kw):
    """one handle of 644 x 481, min_dist 2 (the capacity: the smallest listed), sequence q with sizes[q] and its row's max_cnt / min_dist"""
    tr = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=len(sizes), max_cnt=150, min_dist=2, **kw))
    for q, s in enumerate(sizes):
        if s != (W, H):
            tr.set_seq_size(q, *s)
        assert tr.get_seq_size(q) == s
        tr.set_seq_cfg(q, max_cnt=PAR[s][0], min_dist=PAR[s][1])
    return tr


class Ref:
    """per size: the frames, the depth images, and per frame the oracle's (ids, obs) and state -- which one homogeneous handle of that size reproduces"""

    def __init__(self, gf, oracle):
        self.frames, self.depth, self.res, self.state, self.stats = {}, {}, {}, {}, {}
        for s in SIX:
            w, h = s
            self.frames[s] = _frames(w, h, K, seed=_seed(s))
            self.depth[s] = [_depth(10 * _seed(s) + k, w, h) for k in range(K)]
            otr = oracle.Tracker(oracle.default_cfg(max_cnt=PAR[s][0], min_dist=PAR[s][1]))
            gtr = _homogeneous(gf, s)
            self.res[s], self.state[s] = [], []
            for k in range(K):
                o = otr.track(DT * k, self.frames[s][k], self.depth[s][k])
                g = gtr.trackImage(DT * k, self.frames[s][k], self.depth[s][k])
                _same(o, g, "homogeneous handle of %dx%d against the oracle, frame %d" % (w, h, k))
                _same_state(otr.state(), gtr.state(0), "homogeneous %dx%d frame %d" % (w, h, k))
                assert len(g[0]) > 0
                self.res[s].append(o)
                self.state[s].append(otr.state())
            self.stats[s] = gtr.stats()
            gtr.close()


@pytest.fixture(scope="module")
def ref(gf, oracle):
    return Ref(gf, oracle)


def _routes(sizes, calls=1):
    r = dict.fromkeys(ROUTE, 0)
    for s in set(sizes):
        for k, v in route(*s).items():
            r[k] += int(v) * calls
    return r


def _check(ref, tr, sizes, seqs, ks, res, what):
    for i, q in enumerate(seqs):
        s = sizes[q]
        _same(ref.res[s][ks[i]], res[i], "%s: sequence %d (%dx%d) frame %d" % (what, q, s[0], s[1], ks[i]))
        _same_state(ref.state[s][ks[i]], tr.state(q), "%s: sequence %d (%dx%d) frame %d" % (what, q, s[0], s[1], ks[i]))


def _device_block(torch, arrays, dtype):
    flat = np.concatenate([np.ascontiguousarray(a).view(dtype).ravel() for a in arrays])
    return torch.from_numpy(flat).cuda()


def _call(gf, tr, entry, sizes, seqs, ks, ref, keep):
    """one call for the listed sequences, sequence seqs[i] taking its frame ks[i], through the named entry point; keep: what must outlive the call"""
    import torch
    ts = [DT * k for k in ks]
    imgs = [ref.frames[sizes[q]][k] for q, k in zip(seqs, ks)]
    deps = [ref.depth[sizes[q]][k] for q, k in zip(seqs, ks)]
    if entry == "host":
        return tr.trackImageSome(seqs, ts, imgs, deps)
    if entry == "device":
        dg, dd = _device_block(torch, imgs, np.uint8), _device_block(torch, deps, np.int16)
        offs, total = tr.device_size_offsets(seqs)
        assert total == dg.numel() and tr.device_size_offsets(seqs, 2)[1] == 2 * dd.numel()
        torch.cuda.synchronize()
        return tr.trackImageSomeDevice(seqs, ts, dg.data_ptr(), dd.data_ptr())
    if entry == "refs":   # every frame in an allocation of its own, the gray rows 36 bytes and the depth rows 20 pixels longer than the frame is wide, the padding 255 / 0xFFFF
        gt, dt = [], []
        for a, d in zip(imgs, deps):
            g = torch.full((a.shape[0], a.shape[1] + 36), 255, dtype=torch.uint8)
            g[:, :a.shape[1]] = torch.from_numpy(a)
            e = torch.full((d.shape[0], d.shape[1] + 20), -1, dtype=torch.int16)
            e[:, :d.shape[1]] = torch.from_numpy(d.view(np.int16))
            gt.append(g.cuda()); dt.append(e.cuda())
        torch.cuda.synchronize()
        return tr.trackImageSomeDeviceRefs(seqs, ts, [(t.data_ptr(), t.stride(0)) for t in gt], [(t.data_ptr(), 2 * t.stride(0)) for t in dt])
    assert entry == "prefetched"
    raise AssertionError("staged by the caller")


def _stage(tr, sizes, seqs, ks, ref, keep):
    """gf_tracker_prefetch_some: page-locked frames of each sequence's own height, rows 644 elements apart, the padding 255 / 0xFFFF"""
    import torch
    gt, dt = [], []
    for q, k in zip(seqs, ks):
        a, d = ref.frames[sizes[q]][k], ref.depth[sizes[q]][k]
        g = torch.full((a.shape[0], W), 255, dtype=torch.uint8).pin_memory()
        g[:, :a.shape[1]] = torch.from_numpy(a)
        e = torch.full((d.shape[0], W), -1, dtype=torch.int16).pin_memory()
        e[:, :d.shape[1]] = torch.from_numpy(d.view(np.int16))
        gt.append(g); dt.append(e)
    keep.append((gt, dt))
    tr.prefetchHost([t.data_ptr() for t in gt], [t.data_ptr() for t in dt], stride=W, dstride=W, seqs=seqs)


@pytest.mark.parametrize("entry", ["host", "device", "refs", "prefetched"])
def test_six_sizes_in_one_handle(gf, ref, entry):
    tr = _mixed(gf)
    seqs, keep = list(range(6)), []
    if entry == "prefetched":
        _stage(tr, SIX, seqs, [0] * 6, ref, keep)
    for k in range(K):
        if entry == "prefetched":
            if k + 1 < K:
                _stage(tr, SIX, seqs, [k + 1] * 6, ref, keep)
            res = tr.trackPrefetched([DT * k] * 6)
        else:
            res = _call(gf, tr, entry, SIX, seqs, [k] * 6, ref, keep)
        _check(ref, tr, SIX, seqs, [k] * 6, res, "%s frame %d" % (entry, k))
    st = tr.stats()
    assert {k: st[k] for k in ROUTE} == _routes(SIX, K), st      # each size on the route a handle of that size takes, once per call
    for s in SIX:
        assert {k: ref.stats[s][k] for k in ROUTE} == _routes([s], K)
        assert st["lk_launches"] == ref.stats[s]["lk_launches"] == K - 1    # that of a homogeneous call: one launch for all six sizes
    assert st["frames"] == K and st["sequence_frames"] == 6 * K
    # rows w + 36 bytes apart: a frame whose level 0 goes through the dword kernel is read in dwords as ever, the others miss their reader's 16 bytes
    narrow = sum(1 for w, h in SIX if not route(w, h)["pyr_level0_dword"] and (w + 36) % 16)
    assert st["frames_unaligned"] == (K * narrow if entry == "refs" else 0), st
    tr.close()


def test_lists_of_some_sequences(gf, ref):
    """a list that names two of the six, a list in reverse order, a sequence that sits out three frames: every sequence takes its own next frame whenever it is listed"""
    tr = _mixed(gf)
    nxt = [0] * 6
    plan = [[0, 1, 2, 3, 4, 5], [3, 1], [5, 4, 3, 2, 1, 0], [4, 0], [1, 3, 5], [0, 1, 2, 3, 4, 5], [5, 2], [2, 4, 0, 3]]   # sequence 2 sits out calls 3, 4 (and 1), 5 sits out 3
    want = dict.fromkeys(ROUTE, 0)
    for c, seqs in enumerate(plan):
        ks = [nxt[q] for q in seqs]
        res = _call(gf, tr, "host" if c % 2 else "device", SIX, seqs, ks, ref, [])
        _check(ref, tr, SIX, seqs, ks, res, "call %d" % c)
        for q in seqs:
            nxt[q] += 1
        for k, v in _routes([SIX[q] for q in seqs]).items():
            want[k] += v
        for q in range(6):   # the sequences that were not listed keep their state
            if q not in seqs and nxt[q] > 0:
                _same_state(ref.state[SIX[q]][nxt[q] - 1], tr.state(q), "call %d: unlisted sequence %d" % (c, q))
    st = tr.stats()
    assert {k: st[k] for k in ROUTE} == want, st
    assert max(nxt) <= K and st["sequence_frames"] == sum(len(p) for p in plan)
    tr.close()


def test_two_small_sequences_beside_a_large_one(gf, ref):
    sizes = [(64, 48), (644, 481), (64, 48)]
    tr = _mixed(gf, sizes)
    for k in range(K):
        seqs = [0, 1, 2] if k % 2 == 0 else [2, 1, 0]
        ks = [k, k, max(k - 1, 0)] if k % 2 == 0 else [max(k - 1, 0), k, k]   # the second small sequence is a frame behind the first: same size, states of their own
        if k == 0:
            seqs, ks = [0, 1], [0, 0]
        res = _call(gf, tr, "device" if k % 2 else "refs", sizes, seqs, ks, ref, [])
        _check(ref, tr, sizes, seqs, ks, res, "frame %d" % k)
    st = tr.stats()
    assert {k: st[k] for k in ROUTE} == _routes(sizes, K), st     # two distinct sizes per call, whatever the number of sequences
    tr.close()


@pytest.mark.parametrize("switch", ["GF_LK_POINTS=2", "GF_LK_POINTS=4", "GF_PYR_HEAD=0", "GF_SELECT_TOPK=0", "GF_TRACKER_COPIES=1", "GF_CAMERA_LIFT_HOST=1"])
def test_six_sizes_under_each_switch(gf, ref, monkeypatch, switch):
    key, val = switch.split("=")
    monkeypatch.setenv(key, val)   # read by gf_tracker_create
    tr = _mixed(gf)
    seqs = list(range(6))
    for k in range(K):
        res = _call(gf, tr, "device" if k % 2 else "host", SIX, seqs, [k] * 6, ref, [])
        _check(ref, tr, SIX, seqs, [k] * 6, res, "%s frame %d" % (switch, k))
    st = tr.stats()
    want = dict.fromkeys(ROUTE, 0)
    for s in SIX:
        for name, v in route(*s, head_enabled=key != "GF_PYR_HEAD").items():
            want[name] += int(v) * K
    assert {k: st[k] for k in ROUTE} == want and st["lk_launches"] == K - 1, st
    tr.close()


def test_settings_of_their_own_on_a_small_and_a_large_size(gf):
    """gf_tracker_set_seq_cfg (own max_cnt, min_dist, flow_back = 0, depth_cam = 0), a Kannala-Brandt camera, setPrediction / removeOutliers between frames with the
    `< 10` fallback on the small one: a 64 x 48 and a 640 x 480 sequence of one handle against one homogeneous handle each with the same settings"""
    sizes = [(64, 48), (640, 480)]
    own = [dict(max_cnt=24, min_dist=4, flow_back=0, depth_cam=0), dict(max_cnt=120, min_dist=25, flow_back=0, depth_cam=0)]
    cam = gf.CameraModel.make(*KB)
    mix = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=2, max_cnt=150, min_dist=2))
    homo = []
    for q, s in enumerate(sizes):
        mix.set_seq_size(q, *s)
        mix.set_seq_cfg(q, **own[q])
        mix.set_seq_camera(q, cam)
        hm = gf.FeatureTracker(gf.default_cfg(width=s[0], height=s[1], max_cnt=150, min_dist=2))
        hm.set_seq_cfg(0, **own[q])
        hm.set_seq_camera(0, cam)
        homo.append(hm)
    frames = [_frames(s[0], s[1], K, seed=7) for s in sizes]
    rng = np.random.default_rng(11)
    fallbacks = []   # per frame and sequence: the homogeneous handle took the `< 10` branch (a second LK launch)
    for k in range(K):
        before = mix.stats()["lk_launches"]
        res = mix.trackImageSome([0, 1], [DT * k] * 2, [frames[0][k], frames[1][k]], None)
        took = mix.stats()["lk_launches"] - before
        fb = []
        for q in range(2):
            was = homo[q].stats()["lk_launches"]
            g = homo[q].trackImage(DT * k, frames[q][k], None)
            fb.append(homo[q].stats()["lk_launches"] - was - (1 if k else 0))
            _same(g, res[q], "sequence %d frame %d" % (q, k))
            _same_state(homo[q].state(0), mix.state(q), "sequence %d frame %d" % (q, k))
            assert len(g[0]) == own[q]["max_cnt"]
            ids, _, pts = mix.state(q)
            rm = ids[rng.random(len(ids)) < 0.05]
            mix.removeOutliers(rm, seq=q); homo[q].removeOutliers(rm)
            ids, _, pts = mix.state(q)
            sel = rng.random(len(ids)) < 0.7
            noise = 200.0 if (k == 3 and q == 0) else 1.0   # frame 3, the small sequence: garbage predictions, fewer than 10 succeed and the fallback runs for it alone
            uv = pts[sel] + rng.normal(0, noise, (int(sel.sum()), 2))
            xyz = 2.0 * gf.camera_lift([cam], [uv])[1][0]   # the camera's own rays: its projection brings a prediction back to uv
            mix.setPrediction(ids[sel], xyz, seq=q); homo[q].setPrediction(ids[sel], xyz)
        # one launch from the predictions for both sizes, and one more for the fallback if either sequence takes it: the launches of a homogeneous call
        assert took == (1 + max(fb) if k else 0), (k, took, fb)
        fallbacks.append(fb)
    assert fallbacks[4][0] == 1, fallbacks                                 # the garbage set after frame 3 sent the small sequence through the fallback
    assert any(max(fb) == 0 for fb in fallbacks[1:]), fallbacks           # ... and other frames went without
    mix.close()
    for h in homo:
        h.close()


def test_refusals_leave_the_next_frames_bits_unchanged(gf, ref):
    import torch
    L = gf.lib()
    tr = _mixed(gf)
    seqs = list(range(6))

    def refused(fn, *words):
        with pytest.raises(gf.GfError, match="gf status -1") as e:
            fn()
        for wd in words:
            assert wd in str(e.value), (wd, str(e.value))

    # ---- the setter, before any frame
    assert L.gf_tracker_set_seq_size(None, 0, 64, 48) == -1 and L.gf_tracker_get_seq_size(None, 0, None, None) == -1
    refused(lambda: tr.set_seq_size(6, 64, 48), "sequence 6")
    refused(lambda: tr.set_seq_size(-1, 64, 48), "sequence -1")
    for w, h, word in ((28, 48, "width"), (648, 480, "width"), (642, 480, "width"), (64, 31, "height"), (64, 482, "height"), (0, 48, "width"), (64, 0, "height")):
        refused(lambda: tr.set_seq_size(4, w, h), word)
        assert tr.get_seq_size(4) == (64, 48)
    big = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=10, max_cnt=30, min_dist=5))
    for q in range(7):
        big.set_seq_size(q, 64 + 4 * q, 48 + q)
    refused(lambda: big.set_seq_size(7, 400, 300), "GF_MAX_SEQ_SIZES")           # the ninth distinct size, the handle's own included
    assert big.get_seq_size(7) == (W, H)
    big.set_seq_size(7, 64, 48)                                                    # a size in force is shared
    big.set_seq_size(6, 0, 0)                                                      # (0, 0): back to the handle's, and its row is free again
    assert big.get_seq_size(6) == (W, H)
    big.set_seq_size(8, 400, 300)
    assert big.get_seq_size(8) == (400, 300)
    big.close()
    # a base region of interest is an image of the old size
    roi = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=2))
    roi.set_roi(np.full((H, W), 255, np.uint8), seq=1)
    refused(lambda: roi.set_seq_size(1, 64, 48), "region of interest", "clear")
    roi.set_roi(None, seq=1)
    roi.set_seq_size(1, 64, 48)
    assert roi.get_seq_size(1) == (64, 48)
    roi.close()

    for k in range(K):
        # ---- between frames: every refusal below leaves the run that follows on the reference
        if k == 1:
            refused(lambda: tr.set_seq_size(4, 40, 36), "has taken a frame", "width")      # fixed while the sequence holds tracking state
            refused(lambda: tr.set_seq_size(1, 0, 0), "has taken a frame")
            assert tr.get_seq_size(4) == (64, 48) and tr.get_seq_size(1) == (640, 480)
        if k == 2:   # a stride or pitch shorter than the own row, naming the list position
            imgs = [ref.frames[s][k] for s in SIX]
            deps = [ref.depth[s][k] for s in SIX]
            refused(lambda: tr.trackImageSome(seqs, [DT * k] * 6, imgs, deps, stride=640), "list position 0", "stride")
            refused(lambda: tr.trackImageSome([5, 1], [DT * k] * 2, [imgs[5], imgs[1]], [deps[5], deps[1]], stride=644, dstride=600), "list position 1", "depth")
            g = [torch.from_numpy(a).cuda() for a in imgs]
            refs = [(t.data_ptr(), t.stride(0)) for t in g]
            short = list(refs)
            short[2] = (refs[2][0], 636)
            refused(lambda: tr.trackImageSomeDeviceRefs(seqs, [DT * k] * 6, short), "list position 2", "pitch")
            refused(lambda: tr.trackImageSomeDeviceRefs([4, 3], [DT * k] * 2, [refs[4], (refs[3][0], 64)]), "list position 1", "pitch")
            refused(lambda: tr.prefetchHost([a.ctypes.data for a in imgs], None, stride=320, seqs=seqs), "list position 0")
        if k == 3:   # masks: a pitch shorter than the own row, a host mask of the handle's size, a tight list taken at the handle's size
            m = [torch.full((s[1], s[0]), 255, dtype=torch.uint8).cuda() for s in SIX]
            refused(lambda: tr.set_roi_device_refs([4, 1], [(m[4].data_ptr(), 64), (m[1].data_ptr(), 636)]), "list position 1", "pitch")
            with pytest.raises(AssertionError):
                tr.set_roi(np.full((H, W), 255, np.uint8), seq=4)
            assert gf.lib().gf_tracker_set_roi(tr.h, 4, np.full((48, 64), 255, np.uint8).ctypes.data_as(C.POINTER(C.c_uint8)), 60) == -1 and "64 pixels" in gf.lib().gf_last_error().decode()
            block = torch.full((2, H, W), 255, dtype=torch.uint8).cuda()
            # a tight list taken at the handle's size: the library sees a pointer and cannot know; the caller's layout helper gives the sum of the own sizes, and
            # the wrapper holds the block's bytes against it when it is told them
            assert tr.device_size_offsets([4, 1]) == ([0, 64 * 48], 64 * 48 + 640 * 480) != ([0, W * H], block.numel())
            with pytest.raises(ValueError, match="each of its own size"):
                tr.set_roi_device([4, 1], block.data_ptr(), nbytes=block.numel())
            assert tr.get_roi(4) is None and tr.get_roi(1) is None
        res = _call(gf, tr, "host" if k % 2 else "device", SIX, seqs, [k] * 6, ref, [])
        _check(ref, tr, SIX, seqs, [k] * 6, res, "frame %d" % k)
    # a staged frame that lists the sequence
    tr.reset_seq(4)
    keep = []
    _stage(tr, SIX, [4, 0], [0, 0], ref, keep)
    refused(lambda: tr.set_seq_size(4, 40, 36), "staged frame")
    tr.trackPrefetched([0.0, DT * K])
    tr.close()


def test_a_slot_that_held_larger_pyramids(gf, ref):
    """4 frames at 644 x 481 fill both pyramid slots of the sequence; after gf_tracker_reset_seq the same sequence tracks 64 x 48 frames with the bits of a fresh handle"""
    tr = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=2, max_cnt=150, min_dist=2))
    for q in range(2):
        tr.set_seq_cfg(q, max_cnt=PAR[(W, H)][0], min_dist=PAR[(W, H)][1])
    for k in range(4):
        res = tr.trackImageSome([0, 1], [DT * k] * 2, [ref.frames[(W, H)][k]] * 2, [ref.depth[(W, H)][k]] * 2)
        for q in range(2):
            _same(ref.res[(W, H)][k], res[q], "large frame %d" % k)
    small = (64, 48)
    with pytest.raises(gf.GfError, match="has taken a frame"):
        tr.set_seq_size(1, *small)
    tr.reset_seq(1)
    tr.set_seq_size(1, *small)
    tr.set_seq_cfg(1, max_cnt=PAR[small][0], min_dist=PAR[small][1])
    for k in range(K):
        seqs, ks = ([1, 0], [k, 4 + k]) if k < 2 else ([1], [k])   # the large neighbour goes on beside it for two frames
        res = tr.trackImageSome(seqs, [DT * x for x in ks], [ref.frames[small][k]] + ([ref.frames[(W, H)][ks[1]]] if k < 2 else []),
                                [ref.depth[small][k]] + ([ref.depth[(W, H)][ks[1]]] if k < 2 else []))
        _same(ref.res[small][k], res[0], "small frame %d in the slot of a large sequence" % k)
        _same_state(ref.state[small][k], tr.state(1), "small frame %d" % k)
        if k < 2:
            _same(ref.res[(W, H)][ks[1]], res[1], "the large neighbour, frame %d" % ks[1])
    tr.reset_seq(1)   # the size is a setting: it stays
    assert tr.get_seq_size(1) == small
    tr.close()


def test_a_handle_that_never_calls_the_setter(gf, oracle):
    """4 frames at 640 x 480: the counters of a handle on which the setter was never called, of one on which it only ever took nothing back or named the handle's own
    size, and of one whose other sequence has a size but is not listed, are the same -- the launches of the code as it was"""
    frames = _frames(640, 480, 4)
    names = ROUTE + ("lk_launches", "select_global_sort", "select_streamed", "frames_unaligned", "frames", "sequence_frames")
    recorded = None
    for kind in ("never", "nothing to take back", "unlisted neighbour"):
        otr = oracle.Tracker(oracle.default_cfg())
        tr = gf.FeatureTracker(gf.default_cfg(batch=2))
        if kind == "nothing to take back":
            tr.set_seq_size(0, 0, 0); tr.set_seq_size(1, 640, 480)
            assert tr.get_seq_size(0) == tr.get_seq_size(1) == (640, 480)
        if kind == "unlisted neighbour":
            tr.set_seq_size(1, 64, 48)
        for k, f in enumerate(frames):
            d = _depth(k, 640, 480)
            _same(otr.track(DT * k, f, d), tr.trackImage(DT * k, f, d, seq=0), "%s, frame %d" % (kind, k))
        st = {n: tr.stats()[n] for n in names}
        if recorded is None:
            recorded = st
            assert {n: st[n] for n in ROUTE} == {n: 4 * v for n, v in route(640, 480).items()} and st["lk_launches"] == 3 and st["frames_unaligned"] == 0
        assert st == recorded, (kind, st, recorded)
        tr.close()


def _pitched_cuda(torch, a, extra, fill):
    """the array's rows `extra` elements further apart on the device, the padding `fill`: (tensor, (address, pitch in bytes))"""
    t = torch.full((a.shape[0], a.shape[1] + extra), fill, dtype=torch.uint8)
    t[:, :a.shape[1]] = torch.from_numpy(a)
    t = t.cuda()
    return t, (t.data_ptr(), t.stride(0))


def test_region_boxes_and_track_image_on_a_small_and_a_large_size(gf):
    """a region of interest through the host, the tight device and the _refs setters and back through get_roi, exclusion boxes that cross the small frame's edge, and
    the track image of both: a 64 x 48 and a 640 x 480 sequence of one 644 x 481 handle against one homogeneous handle each with the same settings"""
    import torch
    sizes = [(64, 48), (640, 480)]
    par = [dict(max_cnt=30, min_dist=3), dict(max_cnt=150, min_dist=30)]
    mix = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=2, max_cnt=150, min_dist=2))
    homo = []
    for q, s in enumerate(sizes):
        mix.set_seq_size(q, *s)
        mix.set_seq_cfg(q, **par[q])
        homo.append(gf.FeatureTracker(gf.default_cfg(width=s[0], height=s[1], **par[q])))
        homo[q].set_show_track(True)
    mix.set_show_track(True)
    frames = [_frames(s[0], s[1], K, seed=3) for s in sizes]
    depth = [[_depth(30 + 10 * q + k, s[0], s[1]) for k in range(K)] for q, s in enumerate(sizes)]

    def region(kind, w, h):
        r = np.full((h, w), 255, np.uint8)
        if kind == "host":
            r[:, : w // 3] = 0                       # the left third excluded
        elif kind == "device":
            r[2 * h // 3:, :] = 0                    # the bottom third: the small frame's last band is a partial one
        else:
            r[h // 4: h // 2, w // 4: 3 * w // 4] = 0
            r[:, w - 5:] = 0
        return r

    boxes = [np.array([[50, 30, 100, 70], [-10, -5, 6, 9]], np.int32), np.array([[600, 400, 700, 500], [100, 100, 180, 200]], np.int32)]   # over the right / bottom edge, over the top left corner
    for k in range(K):
        if k in (0, 2, 4):
            kind = {0: "host", 2: "device", 4: "refs"}[k]
            masks = [region(kind, *s) for s in sizes]
            if kind == "host":
                for q in range(2):
                    mix.set_roi(masks[q], seq=q)
            elif kind == "device":   # the larger mask first: the small one starts 640 x 480 bytes into the block
                block = torch.from_numpy(np.concatenate([masks[1].ravel(), masks[0].ravel()])).cuda()
                offs, total = mix.device_size_offsets([1, 0])
                assert offs == [0, 640 * 480] and total == block.numel()
                mix.set_roi_device([1, 0], block.data_ptr(), nbytes=block.numel())
            else:
                held = [_pitched_cuda(torch, m, 13, 0) for m in masks]   # rows w + 13 bytes apart, the padding excluded pixels: any read of it shows
                mix.set_roi_device_refs([0, 1], [r for _, r in held])
            for q in range(2):
                homo[q].set_roi(masks[q])
                assert mix.get_roi(q).shape == masks[q].shape and (k > 0 or np.array_equal(mix.get_roi(q), masks[q]))   # (from frame 1 on the boxes are taken out of it)
                assert np.array_equal(mix.get_roi(q), homo[q].get_roi(0)), "frame %d: get_roi of sequence %d" % (k, q)
        if k == 1:
            mix.set_boxes_some([1, 0], [boxes[1], boxes[0]])
            for q in range(2):
                homo[q].set_boxes(boxes[q])
                assert np.array_equal(mix.get_boxes(q), boxes[q])
                assert np.array_equal(mix.get_roi(q), homo[q].get_roi(0)), "get_roi of sequence %d under its boxes" % q
                assert (mix.get_roi(q) == 0).any() and (mix.get_roi(q) == 255).any()
        res = mix.trackImageSome([1, 0], [DT * k] * 2, [frames[1][k], frames[0][k]], [depth[1][k], depth[0][k]])
        for i, q in enumerate([1, 0]):
            g = homo[q].trackImage(DT * k, frames[q][k], depth[q][k])
            _same(g, res[i], "sequence %d frame %d" % (q, k))
            _same_state(homo[q].state(0), mix.state(q), "sequence %d frame %d" % (q, k))
            assert len(g[0]) >= (8 if q == 0 else 60), (q, k, len(g[0]))
            pic = mix.track_image(q)
            assert pic.shape == (sizes[q][1], sizes[q][0], 3) and np.array_equal(pic, homo[q].track_image(0)), "the track image of sequence %d, frame %d" % (q, k)
        # both pictures in one call, into device memory with a pitch: one launch per distinct size
        dst = [torch.zeros((s[1], 3 * s[0] + 7), dtype=torch.uint8).cuda() for s in sizes]
        mix.track_image_device([0, 1], [(t.data_ptr(), t.stride(0)) for t in dst])
        for q in range(2):
            got = dst[q].cpu().numpy()
            assert np.array_equal(got[:, : 3 * sizes[q][0]].reshape(sizes[q][1], sizes[q][0], 3), homo[q].track_image(0)) and not got[:, 3 * sizes[q][0]:].any()
    mix.close()
    for h in homo:
        h.close()


def test_formats_and_equalisation_on_a_small_and_a_large_size(gf):
    """gf_tracker_set_seq_format beside gf_tracker_set_seq_size: one Bayer, one BGR and one equalised sequence at 160 x 120 and at 640 x 480 (sizes tests/test_clahe_gpu.py
    covers) in one handle, through the host list, the tight device and the _refs entry points, against one homogeneous handle per sequence"""
    import torch
    import synth
    settings = [(RAW.BAYER_GRBG8, 0), (CR.BGR8, 0), (CR.MONO8, 1)]
    seqs = [(s, f, e) for s in ((160, 120), (640, 480)) for f, e in settings]
    B, KF = len(seqs), 4
    mix = gf.FeatureTracker(gf.default_cfg(width=640, height=480, batch=B, min_dist=10))
    homo, raw = [], []
    for q, ((w, h), f, e) in enumerate(seqs):
        mix.set_seq_size(q, w, h)
        mix.set_seq_format(q, f, e)
        homo.append(gf.FeatureTracker(gf.default_cfg(width=w, height=h, min_dist=10, pixel_format=f, equalize=e)))
        gray = synth.tracker_sequence(1000 + 31 * q, KF, w=w, h=h)
        raw.append([np.ascontiguousarray(g) if f == CR.MONO8 else CR.colourise(g, f, 97 * k + q) if f in CR.CHANNELS else RAW.encode(g, f, 97 * k + q) for k, g in enumerate(gray)])
    order = [3, 0, 5, 1, 4, 2]   # sizes and formats interleaved
    for k in range(KF):
        fr = [raw[q][k] for q in order]
        dep = [np.full((seqs[q][0][1], seqs[q][0][0]), 1000 + 37 * k, np.uint16) for q in order]
        ts = [DT * k] * B
        if k % 3 == 0:
            res = mix.trackImageSome(order, ts, fr, dep)
        elif k % 3 == 1:
            block = torch.from_numpy(np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in fr])).cuda()
            offs, total = mix.device_frame_offsets(order)
            assert total == block.numel() and offs == [int(o) for o in np.cumsum([0] + [a.size for a in fr])[:-1]]
            dd = torch.from_numpy(np.concatenate([d.view(np.int16).ravel() for d in dep])).cuda()
            torch.cuda.synchronize()
            res = mix.trackImageSomeDevice(order, ts, block.data_ptr(), dd.data_ptr())
        else:
            held = [_pitched_cuda(torch, np.ascontiguousarray(a).reshape(a.shape[0], -1), 9, 255) for a in fr]
            dts = [torch.from_numpy(d.view(np.int16)).cuda() for d in dep]
            torch.cuda.synchronize()
            res = mix.trackImageSomeDeviceRefs(order, ts, [r for _, r in held], [(t.data_ptr(), 2 * t.stride(0)) for t in dts])
        for i, q in enumerate(order):
            g = homo[q].trackImage(DT * k, raw[q][k], dep[i])
            _same(g, res[i], "sequence %d (%dx%d, format %d, equalize %d) frame %d" % (q, seqs[q][0][0], seqs[q][0][1], seqs[q][1], seqs[q][2], k))
            _same_state(homo[q].state(0), mix.state(q), "sequence %d frame %d" % (q, k))
            assert len(g[0]) >= 20
    st = mix.stats()
    assert {n: st[n] for n in ROUTE} == _routes([(160, 120), (640, 480)], KF), st     # two sizes: two passes of the pyramid per call, whatever the formats
    mix.close()
    for h in homo:
        h.close()


def test_region_rows_of_a_sequence_that_shrinks_and_grows_again(gf, ref):
    """boxes at the handle's size, then the slot shrinks to 64 x 48 with the boxes kept, the boxes are cleared there, and the slot grows back to the handle's size:
    no word of the region table that a compose in the small geometry did not reach may keep the zeros of the long-gone boxes.  Held against a fresh handle, and
    against the oracle through it, at every stage."""
    big, small = (W, H), (64, 48)
    boxes = np.array([[100, 60, 500, 400], [0, 420, 643, 480]], np.int32)     # most of the frame: a leak costs corners at once

    def fresh(size, with_boxes):
        t = gf.FeatureTracker(gf.default_cfg(width=size[0], height=size[1], max_cnt=PAR[size][0], min_dist=PAR[size][1]))
        if with_boxes:
            t.set_boxes(boxes)
        return t

    def run(tr, q, size, other, n, what):
        for k in range(n):
            a = tr.trackImage(DT * k, ref.frames[size][k], ref.depth[size][k], seq=q)
            b = other.trackImage(DT * k, ref.frames[size][k], ref.depth[size][k])
            _same(b, a, "%s, frame %d" % (what, k))
            _same_state(other.state(0), tr.state(q), "%s, frame %d" % (what, k))
        return a

    tr = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=2, max_cnt=150, min_dist=2))
    q = 1
    tr.set_seq_cfg(q, max_cnt=PAR[big][0], min_dist=PAR[big][1])
    tr.set_boxes(boxes, seq=q)                                   # (1) zeros in the geometry of the handle's width
    f = fresh(big, True)
    last = run(tr, q, big, f, 2, "boxes at the handle's size")
    assert len(last[0]) < PAR[big][0], "the boxes leave room for every corner: the case shows nothing"
    f.close()
    tr.reset_seq(q)
    tr.set_seq_size(q, *small)                                   # (2) the boxes stay, composed in the small frame
    tr.set_seq_cfg(q, max_cnt=PAR[small][0], min_dist=PAR[small][1])
    assert np.array_equal(tr.get_boxes(q), boxes)
    f = fresh(small, True)
    run(tr, q, small, f, 2, "the boxes kept at 64 x 48")
    f.close()
    tr.reset_seq(q)
    tr.set_boxes(None, seq=q)                                    # (3) cleared by a compose in the small geometry
    tr.set_seq_size(q, 0, 0)                                     # (4) back to the handle's size without boxes
    tr.set_seq_cfg(q, max_cnt=PAR[big][0], min_dist=PAR[big][1])
    assert tr.get_seq_size(q) == big and len(tr.get_boxes(q)) == 0 and tr.get_roi(q) is None
    for k in range(3):
        g = tr.trackImage(DT * k, ref.frames[big][k], ref.depth[big][k], seq=q)
        _same(ref.res[big][k], g, "grown again without boxes, frame %d" % k)     # the fresh handle of the module's reference, which is the oracle's
        _same_state(ref.state[big][k], tr.state(q), "grown again, frame %d" % k)
        assert len(g[0]) == PAR[big][0]
    # the other way round: boxes set while small, then grown with them
    tr.reset_seq(q)
    tr.set_seq_size(q, *small)
    tr.set_boxes(boxes, seq=q)
    tr.reset_seq(q)
    tr.set_seq_size(q, 640, 480)
    tr.set_seq_cfg(q, max_cnt=PAR[(640, 480)][0], min_dist=PAR[(640, 480)][1])
    f = fresh((640, 480), True)
    run(tr, q, (640, 480), f, 2, "boxes set at 64 x 48, grown to 640 x 480")
    f.close()
    tr.close()
