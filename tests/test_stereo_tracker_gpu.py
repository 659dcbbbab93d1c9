"""The stereo branch of the tracker (gf_tracker_set_seq_stereo; feature_tracker.cpp:259-303) against the restatement of tests/stereo_ref.py: every field of every
observation, ids, camera ids, n_out, state and the stage's counters, bit for bit.  Three sequences on one handle -- a stereo sequence with a distorted PINHOLE right
camera and FLOW_BACK, a stereo sequence with a PINHOLE_FULL right camera without FLOW_BACK, a plain mono sequence -- by reference, in lock step and through lists
that skip and reorder, with pitched and odd-aligned right frames between guard bytes, a null right entry in the middle of a run, a frame size per sequence,
equalisation of both eyes, and the right lifts on the device and on the host.  Run with -m gpu."""
import numpy as np
import pytest

import clahe_ref
import roi_ref as RR
import stereo_ref as SR
from stereo_ref import RIGHT_DIST, RIGHT_PROJ, stamp

pytestmark = pytest.mark.gpu

FULL_PROJ = (410.5, 409.25, 66.0, 48.5)
FULL_DIST = (0.21, -0.09, 0.0011, -0.0007, 0.012, 0.18, -0.05, 0.004)   # k1 k2 p1 p2 k3 k4 k5 k6
GUARD = 0xA7


def _cams(gf):
    return gf.CameraModelEx.make("PINHOLE", RIGHT_PROJ, RIGHT_DIST), gf.CameraModelEx.make("PINHOLE_FULL", FULL_PROJ, FULL_DIST)


def _frames(case, seed):
    """(left, right) frames of a sequence: the shared scene for seed 0, the same recipe on other textures otherwise"""
    w, h = case[:2]
    if seed == 0:
        return SR.scene(w, h)
    left = [np.ascontiguousarray(f, np.uint8) for f in RR.frames(w, h, n=SR.K, seed=seed)]
    return left, [SR.right_frame(f, k) for k, f in enumerate(left)]


class Surface:
    """frames on the device: tight, or each in its own pitched allocation at an odd address between guard bytes"""

    def __init__(self, frames, pitched):
        import torch
        self.keep, self.refs, self.pitched = [], [], pitched
        for f in frames:
            h, w = f.shape
            if not pitched:
                t = torch.from_numpy(np.array(f, np.uint8)).cuda()
                self.refs.append((t.data_ptr(), w))
            else:
                pitch, lead = w + 5, 33
                host = np.full(lead + h * pitch + 64, GUARD, np.uint8)
                host[lead:lead + h * pitch].reshape(h, pitch)[:, :w] = f
                t = torch.from_numpy(host).cuda()
                self.refs.append((t.data_ptr() + lead, pitch))
                self.shape = (h, w, pitch, lead)
            self.keep.append(t)

    def guards_intact(self, frames):
        if not self.pitched:
            return True
        h, w, pitch, lead = self.shape
        for t, f in zip(self.keep, frames):
            host = t.cpu().numpy()
            body = host[lead:lead + h * pitch].reshape(h, pitch)
            if not ((host[:lead] == GUARD).all() and (host[lead + h * pitch:] == GUARD).all() and (body[:, w:] == GUARD).all() and np.array_equal(body[:, :w], f)):
                return False
        return True


def _run(gf, oracle, handle_case, seq_cases, schedule, null_right=(), sizes=False, equalize=(), frame_index=None):
    """seq_cases[q] = (case, seed, right camera index or None, flow_back).  schedule[k]: the sequences call k lists, in that order; a sequence's frames advance with
    the calls that list it.  null_right: (sequence, its frame number) pairs handed a null right entry.  equalize: the sequences that equalise (the node equalises
    both eyes: the restatement runs tests/clahe_ref.py on the left and on the right frame); an even one gets the switch ahead of its right camera, an odd one behind.
    frame_index: which frame of its scene a sequence's k-th frame is (default: the k-th)."""
    W, H = handle_case[:2]
    max_cnt, min_dist = max(c[0][2] for c in seq_cases), min(c[0][3] for c in seq_cases)   # the handle's are the capacity of its sequences'
    cams = _cams(gf)
    B = len(seq_cases)
    g = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=B, max_cnt=max_cnt, min_dist=min_dist, flow_back=1, depth_cam=0))
    refs, left, right, surf_l, surf_r, eq_l, eq_r = [], [], [], [], [], [], []
    for q, (case, seed, cam, fb) in enumerate(seq_cases):
        w, h, mc, md = case
        if sizes and (w, h) != (W, H):
            g.set_seq_size(q, w, h)
        g.set_seq_cfg(q, max_cnt=mc, min_dist=md, flow_back=fb)
        if q in equalize and q % 2 == 0:
            g.set_seq_format(q, equalize=1)
        if cam is not None:
            g.set_seq_stereo(q, cams[cam])
            if q in equalize and q % 2 == 1:
                g.set_seq_format(q, equalize=1)
            assert g.get_seq_stereo(q).enable == 1 and g.get_seq_stereo(q).right.model == cams[cam].model
        else:
            assert g.get_seq_stereo(q).enable == 0
        lift = None
        if cam == 0:
            lift = lambda p: SR.pinhole_lift(RIGHT_PROJ, RIGHT_DIST, p)
        elif cam == 1:
            lift = lambda p, c=cams[1]: gf.camera_lift([c], [p], rays=False)[0][0]
        refs.append(SR.Tracker(oracle, mc, md, fb, lift))
        L, R = _frames(case, seed)
        left.append(L); right.append(R)
        eq_l.append([clahe_ref.clahe(f) for f in L] if q in equalize else L); eq_r.append([clahe_ref.clahe(f) for f in R] if q in equalize else R)
        surf_l.append(Surface(L, False)); surf_r.append(Surface(R, pitched=(q == 0)))
    out = np.zeros((B, g.cap), gf.OBS_DTYPE)
    n_out = np.zeros(B, np.int32)
    frame_of = [0] * B
    want_stats = dict(calls=0, launches=0, points=0, matched=0, right_pyramids=0)
    for listed in schedule:
        ts, gl, gr, expect = [], [], [], []
        ran = 0
        for q in listed:
            n_th = frame_of[q]
            frame_of[q] += 1
            k = frame_index[n_th] if frame_index else n_th
            stereo = seq_cases[q][2] is not None
            has_right = stereo and (q, n_th) not in null_right
            ts.append(stamp(n_th))
            gl.append(surf_l[q].refs[k])
            gr.append(surf_r[q].refs[k] if has_right else None)
            before = refs[q].census["points"], refs[q].census["kept"]
            expect.append(refs[q].track(stamp(n_th), eq_l[q][k], eq_r[q][k] if has_right else None))
            if has_right:
                ran += 1
                want_stats["points"] += refs[q].census["points"] - before[0]
                want_stats["matched"] += refs[q].census["kept"] - before[1]
        if ran:
            want_stats["calls"] += 1; want_stats["launches"] += 1; want_stats["right_pyramids"] += ran
        n = g.trackImageSomeDeviceRefs(listed, ts, gl, gr if any(r is not None for r in gr) else None, unpack=False, out=out, n_out=n_out)
        for i, q in enumerate(listed):
            ids, cam, obs = expect[i]
            what = "sequence %d, its frame %d" % (q, frame_of[q] - 1)
            assert n[i] == len(ids), "%s: n_out %d, the restatement's %d" % (what, n[i], len(ids))
            o = out[i, :n[i]]
            assert np.array_equal(o["id"], ids) and np.array_equal(o["camera_id"], cam), "%s: ids or camera ids differ" % what
            bad = np.nonzero((o["v"].view(np.uint64) != np.ascontiguousarray(obs).view(np.uint64)).any(axis=1))[0]
            assert len(bad) == 0, "%s: observations %s differ (camera ids %s)" % (what, bad[:8], cam[bad[:8]])
            sids, scnt, spts = refs[q].state()
            gids, gcnt, gpts = g.state(q)
            assert np.array_equal(gids, sids) and np.array_equal(gcnt, scnt) and np.array_equal(gpts.view(np.uint32), spts.view(np.uint32)), "%s: state differs" % what
    assert g.stereo_stats() == want_stats, (g.stereo_stats(), want_stats)
    for q in range(B):
        assert surf_r[q].guards_intact(right[q]), "sequence %d: a right frame or its guard bytes were written" % q
    st = dict(g.stats(), lift=g.camera_lift_stats())
    g.close()
    return refs, want_stats, st


A, T = SR.CASES
THREE = [(A, 0, 0, 1), (A, 1, 1, 0), (A, 2, None, 1)]
LOCK = [[0, 1, 2]] * SR.K
PYR_COUNTERS = ("pyr_head", "pyr_level0_vec16", "pyr_level0_dword", "pyr_down_tail", "pyr_down_pad4", "pyr_down_bytes")


def _pyramid_counters(passes):
    """what `passes` passes of launch_pyramid over 132 x 97 frames count: the width is no multiple of 16 and level 1 (66 x 49) none of 4, so level 0 goes through the
    dword kernel and each of the two further levels (66 x 49, 33 x 25; 17 x 13 is below the window) through the byte kernel"""
    return dict(pyr_head=0, pyr_level0_vec16=0, pyr_level0_dword=passes, pyr_down_tail=0, pyr_down_pad4=0, pyr_down_bytes=2 * passes)


@pytest.mark.parametrize("lift_host", [None, "1"])
def test_three_sequences_in_lock_step(gf, oracle, monkeypatch, lift_host):
    """lift_host None: the PINHOLE_FULL right camera of sequence 1 is lifted by one more list entry of the call's camera_lift_kernel launch (one launch per call; the
    PINHOLE right camera of sequence 0 on the host, as a pinhole ever is); GF_CAMERA_LIFT_HOST=1: every lift on the host, no launch.  The same bits both ways."""
    if lift_host is None:
        monkeypatch.delenv("GF_CAMERA_LIFT_HOST", raising=False)
    else:
        monkeypatch.setenv("GF_CAMERA_LIFT_HOST", lift_host)
    refs, stats, st = _run(gf, oracle, A, THREE, LOCK)
    assert stats["calls"] == SR.K and stats["right_pyramids"] == 2 * SR.K and 4 * stats["matched"] >= stats["points"] and stats["points"] == 2 * SR.K * A[2]
    assert refs[0].census["rev_fail"] + refs[0].census["border"] + refs[0].census["distance_alone"] > 0      # FLOW_BACK rejects on sequence 0 ...
    assert refs[1].census["kept"] == refs[1].census["points"] - refs[1].census["fwd_fail"]                   # ... and sequence 1 keeps every forward success
    assert st["lift"] == (dict(launches=SR.K, sequences=SR.K) if lift_host is None else dict(launches=0, sequences=0)), st["lift"]
    assert {k: st[k] for k in PYR_COUNTERS} == _pyramid_counters(2 * SR.K) and st["lk_launches"] == SR.K - 1   # a left and a right pass per call, the temporal launches of a mono handle


def test_lists_that_skip_and_reorder_and_a_null_right_entry(gf, oracle):
    schedule = [[2, 0], [1], [0, 1, 2], [1, 0], [0], [2, 1, 0], [1, 2], [0, 1], [2], [2]]
    assert [sum(q in s for s in schedule) for q in range(3)] == [SR.K] * 3
    refs, stats, _ = _run(gf, oracle, A, THREE, schedule, null_right={(0, 3), (1, 0)})
    assert stats["right_pyramids"] == 2 * SR.K - 2 and stats["calls"] < len(schedule)


def test_a_frame_size_per_sequence(gf, oracle):
    """132 x 97 and 64 x 61 inside a 188 x 122 handle: one stereo launch serves both sizes, the right pyramids are built size by size"""
    M = SR.MIXED
    seqs = [(A, 0, 0, 1), (T, 0, 1, 1), (M, 0, None, 1), (T, 1, 0, 0)]
    _, stats, _ = _run(gf, oracle, M, seqs, [[0, 1, 2, 3]] * SR.K, sizes=True)
    assert stats["launches"] == SR.K and stats["right_pyramids"] == 3 * SR.K


def test_both_eyes_equalised(gf, oracle):
    """equalize = 1 on both stereo sequences (one set ahead of its right camera, one behind) and on none of the mono one: CLAHE runs on the right frames too, the
    pitched odd-aligned ones of sequence 0 included, and the frames themselves stay as they are"""
    _, stats, _ = _run(gf, oracle, A, THREE, LOCK, equalize={0, 1}, null_right={(1, 2)})
    assert stats["right_pyramids"] == 2 * SR.K - 1


def test_both_eyes_equalised_at_two_sizes(gf, oracle):
    M = SR.MIXED
    seqs = [(A, 0, 0, 1), (T, 0, 1, 1), (M, 0, None, 1), (T, 1, 0, 0)]
    _run(gf, oracle, M, seqs, [[0, 1, 2, 3], [3, 1], [0, 2, 1, 3], [1, 0, 3], [0, 1, 2, 3], [2, 0], [1, 3, 0], [2], [2]], sizes=True, equalize={0, 1, 3})


def test_a_handle_without_stereo(gf, oracle):
    """no setter, no stage: the counters of the stage stay zero and the handle launches what a mono handle launches -- one temporal LK launch per frame behind the
    first, one pyramid pass per call (counted kernel by kernel), no camera lift -- and the observations are the oracle's"""
    mono = [(A, 0, None, 1), (A, 1, None, 0), (A, 2, None, 1)]
    _, stats, st = _run(gf, oracle, A, mono, LOCK)
    assert stats == dict(calls=0, launches=0, points=0, matched=0, right_pyramids=0)
    assert st["lk_launches"] == SR.K - 1 and st["frames"] == SR.K and st["sequence_frames"] == 3 * SR.K
    assert {k: st[k] for k in PYR_COUNTERS} == _pyramid_counters(SR.K), {k: st[k] for k in PYR_COUNTERS}
    assert st["lift"] == dict(launches=0, sequences=0)


def _snapshot(g, seqs):
    st = g.stats()
    return ([tuple(a.tobytes() for a in g.state(q)) for q in seqs], g.stereo_stats(), {k: v for k, v in st.items() if not k.startswith("ms_")}, g.camera_lift_stats())


def test_refusals(gf, oracle):
    """every refusal by name, with state and stats as they were; and a stereo sequence without a second image is a mono frame on every entry point"""
    import torch
    cams = _cams(gf)
    w, h, mc, md = A
    g = gf.FeatureTracker(gf.default_cfg(width=w, height=h, batch=3, max_cnt=mc, min_dist=md, flow_back=1, depth_cam=0))
    reg = gf.DepthReg.make(w, h, 100.0, 100.0, w / 2, h / 2)
    g.set_seq_cfg(1, depth_cam=1)
    g.set_seq_depth_reg(2, reg)
    left, right = SR.scene(w, h)
    o = oracle.Tracker(oracle.default_cfg(max_cnt=mc, min_dist=md, flow_back=1, depth_cam=0))
    want = [o.track(stamp(k), left[k], None) for k in range(4)]
    depth = RR.depth(0, w, h)
    d_left = [torch.from_numpy(np.array(f)).cuda() for f in left]
    d_depth = torch.from_numpy(depth.astype(np.int16)).cuda()

    def refused(match, call):
        before = _snapshot(g, range(3))
        with pytest.raises(gf.GfError, match=match):
            call()
        assert _snapshot(g, range(3)) == before, "a refused call changed state or stats (%s)" % match

    refused("depth_cam", lambda: g.set_seq_stereo(1, cams[0]))
    refused("depth registration", lambda: g.set_seq_stereo(2, cams[0]))
    refused("reserved", lambda: g.set_seq_stereo(0, gf.StereoCfg(1, 7, cams[0])))
    g.set_seq_format(0, pixel_format=gf.PIX_BGR8)
    refused("MONO8", lambda: g.set_seq_stereo(0, cams[0]))
    g.set_seq_format(0)
    g.set_seq_stereo(0, cams[0])
    refused("stereo", lambda: g.set_seq_cfg(0, depth_cam=1))
    refused("stereo", lambda: g.set_seq_depth_reg(0, reg))
    refused("MONO8", lambda: g.set_seq_format(0, pixel_format=gf.PIX_RGB8))
    # with a second image: refused on the host-image, tight and prefetch entry points; without one: a mono frame on each
    refused("stereo sequence", lambda: g.trackImageSome([0], [stamp(0)], [left[0]], [depth]))
    RR.same(want[0], g.trackImageSome([0], [stamp(0)], [left[0]])[0], "host image")
    refused("stereo sequence", lambda: g.trackImageSomeDevice([0], [stamp(1)], d_left[1].data_ptr(), d_depth.data_ptr()))
    RR.same(want[1], g.trackImageSomeDevice([0], [stamp(1)], d_left[1].data_ptr())[0], "tight device frames")
    refused("stereo sequence", lambda: g.prefetchHost([left[2].ctypes.data], [depth.ctypes.data], seqs=[0]))
    g.prefetchHost([left[2].ctypes.data], seqs=[0])
    RR.same(want[2], g.trackPrefetched([stamp(2)])[0], "prefetched")
    refused("stereo sequence", lambda: g.trackImage(stamp(3), left[3], depth, seq=0))
    RR.same(want[3], g.trackImage(stamp(3), left[3], None, seq=0), "one sequence")
    assert g.stereo_stats() == dict(calls=0, launches=0, points=0, matched=0, right_pyramids=0)
    refused("taken a frame", lambda: g.set_seq_stereo(0, cams[1]))
    # a reset clears the right-hand state: the first stereo frame behind it has no right velocity
    ref = SR.Tracker(oracle, mc, md, 1, lambda p: SR.pinhole_lift(RIGHT_PROJ, RIGHT_DIST, p))
    d_right = [torch.from_numpy(np.array(f)).cuda() for f in right]
    out, n_out = np.zeros((3, g.cap), gf.OBS_DTYPE), np.zeros(3, np.int32)
    for rounds in range(2):
        g.reset_seq(0)
        ref.reset()
        for k in range(2):
            ids, cam, obs = ref.track(stamp(k), left[k], right[k])
            n = g.trackImageSomeDeviceRefs([0], [stamp(k)], [(d_left[k].data_ptr(), w)], [(d_right[k].data_ptr(), w)], unpack=False, out=out, n_out=n_out)
            o_ = out[0, :n[0]]
            assert np.array_equal(o_["id"], ids) and np.array_equal(o_["camera_id"], cam) and np.array_equal(o_["v"].view(np.uint64), np.ascontiguousarray(obs).view(np.uint64)), (rounds, k)
            if k == 0:
                assert not o_["v"][cam == 1][:, 5:7].any()
    g.close()


@pytest.mark.parametrize("mono_beside", [False, True])
def test_a_call_in_which_no_sequence_wants_corners(gf, oracle, mono_beside):
    """a frame that repeats the one before it keeps every track (max_cnt of them), so no listed sequence wants corners and the call has no detection: the stereo tables
    go down in a hand-over of their own, the stereo kernel gathers tracked survivors alone, and the PINHOLE_FULL right camera is lifted by a launch that holds the
    right set alone.  With a mono sequence beside them or without."""
    seqs = [(A, 0, 0, 1), (A, 2, 1, 0)] + ([(A, 5, None, 1)] if mono_beside else [])   # textures on which a repeated frame keeps every track
    order = [0, 0, 0, 1, 1, 2]
    refs, stats, st = _run(gf, oracle, A, seqs, [list(range(len(seqs)))] * SR.K, frame_index=order)
    for case, seed, _, fb in seqs:      # the premise, on the oracle: frames 1, 2 and 4 repeat their predecessor, carry all max_cnt ids over and want nothing
        o, prev = oracle.Tracker(oracle.default_cfg(max_cnt=case[2], min_dist=case[3], flow_back=fb, depth_cam=0)), None
        for n_th, k in enumerate(order):
            ids = o.track(stamp(n_th), _frames(case, seed)[0][k], None)[0]
            if n_th in (1, 2, 4):
                same = np.array_equal(np.sort(ids), np.sort(prev))      # setMask's sort may reorder them
                assert len(ids) == case[2] and same, "frame %d of seed %d wants corners" % (n_th, seed)
            prev = ids
    assert stats["calls"] == SR.K and stats["points"] == 2 * SR.K * A[2]
    assert st["lift"] == dict(launches=SR.K, sequences=SR.K)
