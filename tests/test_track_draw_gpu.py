"""The track image on the device (csrc/gf_track_draw_kernels.hpp): the building block gf_draw_track_batch on lists a tracker would never produce, and
gf_tracker_track_image / _track_image_some_device through real tracker runs, the estimator and gf_replay -- every picture byte for byte against
tests/track_draw_ref.py, the definition of DESIGN.md section 4 restated in Python.  There is no tolerance anywhere.  Every list that has arrows is first
checked on the CPU to keep its tip coordinates 1e-9 away from the ties of lrint.  Run with -m gpu."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import synth
import track_draw_ref as TD

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.0666
GUARD, FILL = 96, 0xC3


# ---------------------------------------------------------------------------------------------------------------- the building block
def _empty(w, h):
    return np.zeros((0, 2), np.float32), np.zeros(0, np.int32), np.zeros((0, 2), np.float32), np.zeros(0, bool)


def _corners(w, h):
    cur = np.array([(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (-3, -3), (w + 2, h + 2), (-6, 5), (w / 2, h + 5)], np.float32)   # the last two cover nothing
    return cur, np.arange(1, len(cur) + 1, dtype=np.int32), cur.copy(), np.zeros(len(cur), bool)


def _zero_length(w, h):
    cur = np.array([(5, 5), (0, 0), (w - 1, h - 1), (w // 2 + 0.5, h // 2 + 1.5), (-1, 7)], np.float32)   # (.5, 1.5): half to even; the last one is clipped to one column
    return cur, np.full(len(cur), 3, np.int32), cur.copy(), np.ones(len(cur), bool)


def _diagonal(w, h):
    cur, prev = np.array([(0, 0), (w - 1, 0)], np.float32), np.array([(w - 1, h - 1), (0, h - 1)], np.float32)
    return cur, np.array([25, 1], np.int32), prev, np.ones(2, bool)


def _tips_outside(w, h):
    cur = np.array([(30, 20), (w - 30, 20), (30, h - 20), (20, 20), (w + 20, h // 2)], np.float32)
    prev = np.array([(1, 1), (w - 2, 0), (0, h - 1), (-25, -9), (w - 2, h // 2 + 3)], np.float32)   # heads at the border: their tips leave the image; one head, one tail outside
    return cur, np.array([2, 7, 12, 19, 40], np.int32), prev, np.ones(len(cur), bool)


def _patch500(w, h):
    rng = np.random.default_rng(500)
    cur = (20 + rng.uniform(0, 7.4, (500, 2))).astype(np.float32)
    prev = (20 + rng.uniform(0, 7.4, (500, 2))).astype(np.float32)
    return cur, rng.integers(1, 26, 500).astype(np.int32), prev, np.ones(500, bool)


def _overlapping(w, h):
    """dots of every track_cnt 1 .. 25, 6 pixels apart (radius 5: every neighbour pair overlaps), arrows from every second one across its neighbours"""
    cur = np.array([(8 + 6 * (k % 5), 6 + 6 * (k // 5)) for k in range(25)], np.float32)
    prev = cur + np.array([(13, 5)], np.float32)
    return cur, np.arange(1, 26, dtype=np.int32), prev, (np.arange(25) % 2 == 0)


def _far_arrows(w, h):
    """arrows whose far ends lie tens of thousands of pixels outside the image, and one near the edge of the builder's range: the products of the coverage
    test are far beyond 32 bits"""
    cur = np.array([(w // 2, h // 2), (5, h - 6), (w - 4, 3)], np.float32)
    prev = np.array([(20000, -15000), (-900001, 700003), (w - 4, 2 ** 20)], np.float32)
    return cur, np.array([4, 9, 21], np.int32), prev, np.ones(3, bool)


def _random(seed):
    return lambda w, h: TD.random_lists(np.random.default_rng(seed), 40, w, h, reach=20.0)


LISTS = {"empty": _empty, "corners_and_clipping": _corners, "zero_length_arrows": _zero_length, "diagonal_arrow": _diagonal, "tips_leave_the_image": _tips_outside,
         "500_features_in_one_patch": _patch500, "overlapping_dots_1_to_25": _overlapping, "arrows_from_far_outside": _far_arrows, "random": _random(11)}
# (w, h, pitch - 3 w, address & 15 of the destination): no multiple of any tile or of 4, at an odd address and pitch; and 16-byte-aligned everything
LAYOUTS = {"67x45_odd": (67, 45, 5, 1), "64x48_aligned": (64, 48, 0, 0)}
_WANT = {}


def _case(name, layout):
    """three frames (seeded noise backgrounds): the named list, a random one, the empty one; their expected pictures, computed once"""
    key = (name, layout)
    if key not in _WANT:
        w, h = LAYOUTS[layout][:2]
        gray = np.random.default_rng(5 + list(LAYOUTS).index(layout)).integers(0, 256, (3, h, w), dtype=np.uint8)
        lists = [LISTS[name](w, h), _random(23)(w, h), _empty(w, h)]
        want, rules = [], None
        for g, l in zip(gray, lists):
            img, by_index, by_green, margin = TD.render(g, *l, with_rules=True)
            assert margin > 1e-9, "an arrow tip within 1e-9 of a tie of lrint"
            rules = rules or (by_index, by_green)
            want.append(img)
        _WANT[key] = (gray, lists, np.stack(want), rules)
    return _WANT[key]


def _dst(w, h, extra, phase, batch=3):
    """a destination of `batch` frames inside a larger buffer of FILL bytes: (whole buffer, [batch, h, pitch] view at address & 15 == phase)"""
    pitch = 3 * w + extra
    buf = np.full(2 * GUARD + 16 + batch * h * pitch, FILL, np.uint8)
    off = GUARD + (phase - (buf.ctypes.data + GUARD)) % 16
    view = buf[off:off + batch * h * pitch].reshape(batch, h, pitch)
    assert (view.ctypes.data & 15) == phase
    return buf, view


def _check_dst(buf, view, want, w):
    assert np.array_equal(view[:, :, :3 * w].reshape(want.shape), want), "%d pixels differ" % (view[:, :, :3 * w].reshape(want.shape) != want).any(-1).sum()
    rest = buf.copy()
    off = view.ctypes.data - buf.ctypes.data
    rest[off:off + view.size].reshape(view.shape)[:, :, :3 * w] = FILL
    assert (rest == FILL).all(), "%d bytes outside the pixels were written" % (rest != FILL).sum()


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("name", list(LISTS))
def test_building_block_equals_the_definition(gf, name, layout):
    w, h, extra, phase = LAYOUTS[layout]
    gray, lists, want, rules = _case(name, layout)
    if name == "overlapping_dots_1_to_25":
        print("pixels decided by the largest index: %d, by green over dots: %d" % rules)
        assert rules[0] >= 100 and rules[1] >= 100
    if name == "500_features_in_one_patch":
        assert 4 * len(lists[0][1]) > 256   # more primitives on one tile than the kernel's LDS list holds
    buf, view = _dst(w, h, extra, phase)
    if phase == 0:
        assert (gray.ctypes.data & 15) == 0 and (view.shape[2] & 15) == 0
    gf.draw_track(gray, lists, dst=view)
    _check_dst(buf, view, want, w)
    first = view.copy()
    view[:] = FILL
    gf.draw_track(gray, lists, dst=view)   # two runs, the same bytes
    assert np.array_equal(view, first)


def test_building_block_reads_a_pitched_background_and_returns_new_pictures(gf):
    """the frames as a crop at the right edge of a wider array: the last pixel of the last row is the last byte of the allocation, and nothing behind it is read"""
    w, h = 67, 45
    gray, lists, want, _ = _case("random", "67x45_odd")
    wide = np.full((3 * h, w + 9), 200, np.uint8)
    wide[:, 9:] = gray.reshape(3 * h, w)
    crop = wide.reshape(3, h, w + 9)[:, :, 9:]   # a view: rows w + 9 bytes apart
    assert crop.ctypes.data + 3 * h * (w + 9) - 9 == wide.ctypes.data + wide.size and not crop.flags.c_contiguous
    got = gf.draw_track(crop, lists)
    assert got.shape == (3, h, w, 3) and np.array_equal(got, want)
    assert np.array_equal(gf.draw_track(gray[0], lists[0]), want[0])


def test_building_block_writes_a_crop_of_a_wider_destination(gf):
    """the destination likewise: three pictures side by side in one wide image, each written through its own view, whose last row ends before its pitch does"""
    w, h = 67, 45
    gray, lists, want, _ = _case("random", "67x45_odd")
    wide = np.full((h, 3 * 3 * w + 2), FILL, np.uint8)
    for b in range(3):
        view = wide[None, :, 2 + 3 * w * b:2 + 3 * w * (b + 1)]   # [1, h, 3 w], rows a whole wide row apart; the last picture's last pixel is the last byte of `wide`
        gf.draw_track(gray[b:b + 1], lists[b:b + 1], dst=view)
    assert (wide[:, :2] == FILL).all()
    assert np.array_equal(wide[:, 2:].reshape(h, 3, w, 3).transpose(1, 0, 2, 3), want)


@pytest.mark.parametrize("bad", ["nan", "beyond_2_20", "negative_track_cnt", "arrow_from_infinity"])
def test_building_block_refuses_what_the_builder_refuses(gf, bad):
    gray = np.zeros((45, 67), np.uint8)
    cur, cnt, prev, has = np.array([(5, 5), (9, 9)], np.float32), np.array([1, 2], np.int32), np.array([(6, 6), (7, 7)], np.float32), np.array([1, 1], bool)
    if bad == "nan":
        cur[1, 0] = np.nan
    elif bad == "beyond_2_20":
        cur[1, 1] = 2 ** 20 + 1
    elif bad == "negative_track_cnt":
        cnt[0] = -1
    else:
        prev[0, 0] = np.inf
    buf, view = _dst(67, 45, 5, 1, batch=1)
    with pytest.raises(gf.GfError):
        gf.draw_track(gray[None], [(cur, cnt, prev, has)], dst=view)
    assert (buf == FILL).all()


# ---------------------------------------------------------------------------------------------------------------- through the tracker
B, K, MAX_CNT, MIN_DIST = 3, 6, 60, 12
SIZES = [(176, 192), (320, 240)]
_FRAMES = {}


def frames_of(w, h, n_seq=B, k=K):
    key = (w, h, n_seq, k)
    if key not in _FRAMES:
        _FRAMES[key] = [synth.tracker_sequence(2100 + b, k, w, h) for b in range(n_seq)]
    return _FRAMES[key]


def colour_of(f):
    return np.ascontiguousarray(np.stack([f, f // 2 + 30, 255 - f], -1))


def expected(bg, before, after):
    """the picture the states before and after a call imply"""
    ids0, _, pts0 = before
    ids1, cnt1, pts1 = after
    at = {int(i): k for k, i in enumerate(ids0)}
    has = np.array([int(i) in at for i in ids1], bool)
    prev = np.array([pts0[at[int(i)]] if int(i) in at else (0, 0) for i in ids1], np.float32).reshape(-1, 2)
    img, _, _, margin = TD.render(bg, pts1, cnt1, prev, has, with_rules=True)
    assert margin > 1e-9, "an arrow tip within 1e-9 of a tie of lrint"
    return img, int(has.sum())


class DeviceImage:
    """a destination on the device at an odd address and pitch, inside a buffer of FILL bytes"""

    def __init__(self, w, h, extra=7, offset=1):
        import torch
        self.w, self.h, self.pitch, self.offset = w, h, 3 * w + extra, GUARD + offset
        self.buf = torch.full((2 * GUARD + 16 + h * self.pitch,), FILL, dtype=torch.uint8, device="cuda")
        self.ref = (self.buf.data_ptr() + self.offset, self.pitch)

    def host(self):
        return self.buf.cpu().numpy()

    def pixels(self):
        a = self.host()
        return a[self.offset:self.offset + self.h * self.pitch].reshape(self.h, self.pitch)[:, :3 * self.w].reshape(self.h, self.w, 3).copy()

    def untouched_outside(self):
        a = self.host()
        a[self.offset:self.offset + self.h * self.pitch].reshape(self.h, self.pitch)[:, :3 * self.w] = FILL
        return bool((a == FILL).all())


def host_image_into(gf, gtr, seq, dst, stride):
    """gf_tracker_track_image into the caller's own array (track_image makes a new one)"""
    return gf.lib().gf_tracker_track_image(gtr.h, seq, dst.ctypes.data_as(C.POINTER(C.c_uint8)), stride)


MODES = ["mono8", "equalize", "rgb8", "frame_refs"]


@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("mode", MODES)
def test_tracker_pictures_equal_the_definition(gf, mode, size):
    import torch
    w, h = size
    frames = frames_of(w, h)
    cfg = gf.default_cfg(width=w, height=h, batch=B, max_cnt=MAX_CNT, min_dist=MIN_DIST, depth_cam=0, equalize=int(mode == "equalize"),
                         pixel_format=gf.PIX_RGB8 if mode == "rgb8" else gf.PIX_MONO8)
    gtr = gf.FeatureTracker(cfg)
    gtr.set_show_track(True)
    background = {"mono8": lambda f: f, "frame_refs": lambda f: f, "equalize": lambda f: gf.clahe(f), "rgb8": lambda f: gf.cvt_gray(colour_of(f), gf.PIX_RGB8)}[mode]
    nxt, last, arrows = [0] * B, [None] * B, 0
    dev = [DeviceImage(w, h) for _ in range(B)]
    for k in range(K):
        L = [0, 1, 2] if k % 2 == 0 else [1, 0]          # sequence 2 sits out every other call; the list's order changes
        before = {b: gtr.state(b) for b in range(B)}
        fr = [frames[b][nxt[b]] for b in L]
        ts = [DT * nxt[b] for b in L]
        if mode == "frame_refs":
            surf = [torch.from_numpy(np.pad(f, ((0, 0), (0, 5)))).cuda() for f in fr]
            torch.cuda.synchronize()
            gtr.trackImageSomeDeviceRefs(L, ts, [(s.data_ptr(), w + 5) for s in surf])
            for s in surf:
                s.fill_(0)                                   # the caller's buffer is overwritten before the picture is fetched
            torch.cuda.synchronize()
        else:
            gtr.trackImageSome(L, ts, [colour_of(f) for f in fr] if mode == "rgb8" else fr)
        for b in L:
            nxt[b] += 1
        for i, b in enumerate(L):
            want, carried = expected(background(fr[i]), before[b], gtr.state(b))
            arrows += carried
            got = gtr.track_image(b)
            assert np.array_equal(got, want), "call %d, sequence %d: %d pixels differ" % (k, b, (got != want).any(2).sum())
            last[b] = want
        # the device form for all three at once, the one that sat out included: it returns its previous picture
        gtr.track_image_device([2, 0, 1], [dev[2].ref, dev[0].ref, dev[1].ref])
        for b in range(B):
            assert np.array_equal(dev[b].pixels(), last[b]), "call %d, sequence %d (device)" % (k, b)
            assert dev[b].untouched_outside()
        # feedback after the frame does not change the picture
        ids, _, pts = gtr.state(0)
        gtr.removeOutliers(ids[::5], seq=0)
        ids, _, pts = gtr.state(0)
        gtr.setPrediction(ids[::2], np.stack([(pts[::2, 0] - cfg.cx) / cfg.fx * 2, (pts[::2, 1] - cfg.cy) / cfg.fy * 2, np.full(len(ids[::2]), 2.0)], 1), seq=0)
        assert np.array_equal(gtr.track_image(0), last[0]), "call %d: removeOutliers / setPrediction changed the picture" % k
    assert arrows >= 100   # features were carried from frame to frame: the pictures had arrows
    gtr.close()


def test_picture_shows_exactly_the_reported_features(gf):
    """a per-sequence max_cnt and a region of interest: dots from the reported ids and pixel coordinates alone"""
    w, h = SIZES[0]
    frames = frames_of(w, h)
    gtr = gf.FeatureTracker(gf.default_cfg(width=w, height=h, batch=2, max_cnt=MAX_CNT, min_dist=MIN_DIST, depth_cam=0))
    gtr.set_seq_cfg(1, max_cnt=20)
    roi = np.zeros((h, w), np.uint8)
    roi[:, :w // 2] = 255
    gtr.set_roi(roi, seq=0)
    gtr.set_show_track(True)
    for k in range(4):
        before = [gtr.state(b) for b in range(2)]
        res = gtr.trackImageSome([0, 1], [DT * k] * 2, [frames[0][k], frames[1][k]])
        for b in range(2):
            ids, obs = res[b]
            _, cnt, _ = gtr.state(b)
            want, _ = expected(frames[b][k], before[b], (ids, cnt, obs[:, 3:5].astype(np.float32)))
            assert np.array_equal(gtr.track_image(b), want), "frame %d, sequence %d" % (k, b)
        assert len(res[1][0]) <= 20 and len(res[0][0]) >= 5
        assert (np.rint(res[0][1][:, 3]) < w // 2).all()
    gtr.close()


def test_refusals_leave_the_destination_untouched(gf):
    w, h = SIZES[0]
    frames = frames_of(w, h)
    gtr = gf.FeatureTracker(gf.default_cfg(width=w, height=h, batch=2, max_cnt=MAX_CNT, min_dist=MIN_DIST, depth_cam=0))
    dev = [DeviceImage(w, h), DeviceImage(w, h)]
    host = np.full((h, 3 * w + 4), FILL, np.uint8)

    def refused(seqs, refs, match, host_seq=0, stride=3 * w + 4):
        with pytest.raises(gf.GfError, match=match):
            gtr.track_image_device(seqs, refs)
        if host_seq is not None:
            assert host_image_into(gf, gtr, host_seq, host, stride) != 0
        assert (host == FILL).all() and all((d.host() == FILL).all() for d in dev)

    refused([0], [dev[0].ref], "list position 0.*show_track is off")
    gtr.trackImage(0.0, frames[0][0], seq=0)                  # a frame with the switch off records nothing
    gtr.set_show_track(True)
    refused([0], [dev[0].ref], "list position 0.*no frame recorded")
    gtr.trackImageSome([0, 1], [DT, DT], [frames[0][1], frames[1][1]])
    refused([0, 0], [dev[0].ref, dev[1].ref], "listed twice", host_seq=None)
    refused([0, 1], [dev[0].ref, (dev[1].ref[0], 3 * w - 1)], "list position 1.*pitch shorter than a row", host_seq=1, stride=3 * w - 1)
    refused([1, 0], [dev[1].ref, (0, 3 * w)], "list position 1.*null data", host_seq=None)
    refused([0, 2], [dev[0].ref, dev[1].ref], "names sequence 2", host_seq=2)
    refused([0, 1, 0], [dev[0].ref] * 3, "3 sequences listed", host_seq=-1)
    with pytest.raises(gf.GfError, match="null table"):
        gtr.track_image_device([0], None)
    gtr.reset_seq(1)                                          # keeps the switch, drops the picture
    refused([0, 1], [dev[0].ref, dev[1].ref], "list position 1.*no frame recorded", host_seq=1)
    gtr.track_image_device([0], [dev[0].ref])                 # sequence 0 still has its own
    assert not (dev[0].host() == FILL).all() and dev[0].untouched_outside()
    gtr.trackImage(0.0, frames[1][0], seq=1)                  # ... and sequence 1 has one again with its next frame, without setting the switch again
    assert gtr.track_image(1).shape == (h, w, 3)
    gtr.set_show_track(False, seqs=[0])
    with pytest.raises(gf.GfError, match="show_track is off"):
        gtr.track_image(0)
    gtr.close()


COUNTERS = ("frames", "lk_launches", "lk_points", "lk_level_passes", "lk_iterations", "tracked_features", "output_features", "select_streamed", "select_global_sort",
            "pyr_head", "pyr_level0_vec16", "pyr_level0_dword", "pyr_down_tail", "pyr_down_pad4", "pyr_down_bytes", "frames_unaligned", "sequence_frames")


def test_drawing_observes_and_never_steers(gf):
    w, h = SIZES[0]
    frames = frames_of(w, h)
    runs = []
    for show in (False, True):
        gtr = gf.FeatureTracker(gf.default_cfg(width=w, height=h, batch=B, max_cnt=MAX_CNT, min_dist=MIN_DIST, depth_cam=0))
        if show:
            gtr.set_show_track(True)
        out = []
        for k in range(K):
            res = gtr.trackImageSome([0, 1, 2], [DT * k] * 3, [frames[b][k] for b in range(B)])
            if show:
                for b in range(B):
                    gtr.track_image(b)
            out.append((res, [gtr.state(b) for b in range(B)]))
        runs.append((out, gtr.stats()))
        gtr.close()
    (a, sa), (b, sb) = runs
    for k in range(K):
        for i in range(B):
            assert np.array_equal(a[k][0][i][0], b[k][0][i][0]) and np.array_equal(a[k][0][i][1].view(np.uint64), b[k][0][i][1].view(np.uint64)), "frame %d, sequence %d" % (k, i)
            assert all(np.array_equal(x, y) for x, y in zip(a[k][1][i], b[k][1][i])), "frame %d, sequence %d: state" % (k, i)
    assert {n: sa[n] for n in COUNTERS} == {n: sb[n] for n in COUNTERS} and sa["frames"] == K


def test_estimator_and_replay_tool_give_the_tracker_s_picture(gf, tmp_path):
    """gf_estimator_get_track_image on 3 frames of a synthetic dataset, and `gf_replay --track-images` on the same dataset: the stand-alone tracker's pictures"""
    import synth_stream as SS
    st = SS.Stream(1, t_still=1.0, t_move=1.0, v_max=0.4, yaw0=0.0, yaw_turn=-0.6, split_x=1.8, turn_delay=0.8)
    d = str(tmp_path)
    n = st.export(d, n_frames=3, show_track=1)
    assert n == 3
    cfg = gf.estimator_cfg_from_yaml(os.path.join(d, "config.yaml"))
    assert gf.show_track_from_yaml(os.path.join(d, "config.yaml")) == 1
    own = gf.SlidingWindowEstimator(cfg)
    tracker = gf.FeatureTracker(cfg.tracker)
    own.set_show_track(True); tracker.set_show_track(True)
    want, tp = [], -1.0
    for k in range(n):
        tp = st.feed(own, k, tp)
        img, dep = st.image(k)
        before = tracker.state(0)
        own.inputImage(float(st.cam_t[k]), img, dep)
        tracker.trackImage(float(st.cam_t[k]), img, dep)
        pic = tracker.track_image(0)
        assert np.array_equal(pic, expected(img, before, tracker.state(0))[0]), "frame %d" % k
        assert np.array_equal(own.track_image(), pic), "frame %d: the estimator's picture" % k
        want.append(pic)
    own.close(); tracker.close()
    bare = gf.SlidingWindowEstimator(gf.default_estimator_cfg())
    with pytest.raises(gf.GfError, match="without a tracker"):
        bare.set_show_track(True)
    bare.close()
    exe = os.path.join(ROOT, "bin", "gf_replay")
    assert os.path.exists(exe), "bin/gf_replay is missing: run `python __graft_entry__.py` (build)"
    out_dir = os.path.join(d, "pictures")
    run = subprocess.run([exe, "--track-images", out_dir, os.path.join(d, "config.yaml"), d, os.path.join(d, "vio.txt")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr
    assert sorted(os.listdir(out_dir)) == ["%06d.ppm" % k for k in range(n)]
    h, w = want[0].shape[:2]
    head = b"P6\n%d %d\n255\n" % (w, h)
    for k in range(n):
        raw = open(os.path.join(out_dir, "%06d.ppm" % k), "rb").read()
        assert raw.startswith(head) and len(raw) == len(head) + 3 * w * h
        rgb = np.frombuffer(raw[len(head):], np.uint8).reshape(h, w, 3)
        assert np.array_equal(rgb[:, :, ::-1], want[k]), "picture %d" % k    # a PPM is R, G, B: the picture's bgr8 bytes reversed
    plain = subprocess.run([exe, os.path.join(d, "config.yaml"), d, os.path.join(d, "vio2.txt")], capture_output=True, text=True, timeout=300)
    assert plain.returncode == 0 and sorted(os.listdir(out_dir)) == ["%06d.ppm" % k for k in range(n)]   # `show_track: 1` alone writes nothing anywhere
