"""Device frames handed to the tracker by reference: one pointer and row pitch per listed sequence (gf_tracker_track_some_device_refs / _track_batch_device_refs /
gf_tracker_set_roi_some_device_refs).

The yardstick is the tight entry point of the same library on the same pixels (gf_tracker_track_some_device, itself held to the oracle by the other files): every
comparison is bit for bit -- ids, observations viewed as uint64 (the depths among them), state() of every sequence after every call -- and there is no tolerance
anywhere.  One case goes to oracle.Tracker directly.  Every surface a call was given is compared byte for byte with what it held before the call.

Sizes: small ones that take each pyramid route (asserted from the stats): 320 x 136 the head kernel (three levels; at 320 x 240 the fourth level, 40 x 30, is
within one reflection of its border and the pyramid takes the 16-byte level 0 with byte-wise levels above it, which is the second size), 644 x 481 the dword
level 0 with byte-wise levels, 40 x 36 a single level.  Device memory is torch uint8 tensors (allocations are at least 256-byte aligned); views at byte offsets give the alignments.
Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import synth

pytestmark = pytest.mark.gpu

DT = 0.0666
K = 6                       # frames per sequence
MAX_CNT, MIN_DIST = 60, 12
SIZES = [(320, 136), (320, 240), (644, 481), (40, 36)]
# (byte offset of row 0 inside its allocation, pitch - row bytes) of sequence b % 3: 16-byte aligned, dword aligned, not aligned at all
MIXED = [(0, 0), (4, 36), (1, 37)]
_FRAMES = {}


def frames_of(w, h, n_seq=4, k=K):
    """mono frames [sequence][step], rendered once per size"""
    key = (w, h, n_seq, k)
    if key not in _FRAMES:
        _FRAMES[key] = [synth.tracker_sequence(1100 + b, k, w, h) for b in range(n_seq)]
    return _FRAMES[key]


def same(a, b, what):
    assert np.array_equal(a[0], b[0]), "%s: feature id lists differ" % what
    assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64)), "%s: observations differ" % what


def same_state(a, b, what):
    assert len(a) == len(b) == 3 and all(np.array_equal(x, y) for x, y in zip(a, b)), "%s: state differs" % what


def same_run(base, run, what):
    assert len(base) == len(run)
    for k, ((res_a, st_a), (res_b, st_b)) in enumerate(zip(base, run)):
        assert len(res_a) == len(res_b)
        for i in range(len(res_a)):
            same(res_a[i], res_b[i], "%s: call %d, list position %d" % (what, k, i))
        for s in range(len(st_a)):
            same_state(st_a[s], st_b[s], "%s: call %d, sequence %d" % (what, k, s))


class Surface:
    """a frame inside a larger device allocation: `rows_total` rows of `pitch` bytes from byte `offset` on, the frame's h rows of `row` bytes at row y0 and byte
    x0 of them; everything else holds `fill` (one byte, or a seed for random bytes)"""

    def __init__(self, frame, offset=0, pad=0, fill=0x5A, rows_total=None, y0=0, x0=0, pitch=None):
        import torch
        a = np.ascontiguousarray(frame).view(np.uint8).reshape(frame.shape[0], -1)
        h, row = a.shape
        self.pitch = pitch or row + pad + x0
        rows = rows_total or h + y0
        n = offset + rows * self.pitch + 3
        if isinstance(fill, int):
            host = np.full(n, fill, np.uint8)
        else:
            host = np.random.default_rng(fill[0]).integers(0, 256, n, dtype=np.uint8)
        start = offset + y0 * self.pitch + x0
        np.lib.stride_tricks.as_strided(host[start:], (h, row), (self.pitch, 1))[:] = a
        self.buf = torch.from_numpy(host).cuda()
        self.before = self.buf.clone()
        self.ref = (self.buf.data_ptr() + start, self.pitch)

    def unwritten(self):
        import torch
        return torch.equal(self.buf, self.before)


def drive(gf, cfg, frames, lists, place=None, depth=None, depth_place=None, hook=None, setup=None, tracker=None, start=0):
    """one handle through the calls of `lists` (the sequences of each call; every sequence consumes its own frames in order).  place = None: the tight entry point
    on the listed frames stacked into one tensor; else place(b, i, frame) -> Surface and the _refs entry point, each surface held to its bytes after the call.
    depth: [sequence] u16 images or None; depth_place(b, i, image) -> Surface or None (a null entry).  tracker / start: go on with a handle whose sequences have taken `start` frames.  Returns ([(results, states of all sequences)], stats)."""
    import torch
    gtr = tracker or gf.FeatureTracker(cfg)
    B = gtr.cfg.batch
    if setup:
        setup(gtr)
    nxt = [start] * B
    run = []
    for k, L in enumerate(lists):
        ts = [DT * nxt[b] for b in L]
        fr = [frames[b][nxt[b]] for b in L]
        if place is None:
            dg = torch.from_numpy(np.stack(fr)).cuda()
            dd = torch.from_numpy(np.stack([depth[b] for b in L]).view(np.int16)).cuda() if depth is not None else None
            torch.cuda.synchronize()
            res = gtr.trackImageSomeDevice(L, ts, dg.data_ptr(), dd.data_ptr() if dd is not None else None)
        else:
            surf = [place(b, i, f) for i, (b, f) in enumerate(zip(L, fr))]
            dsurf = [depth_place(b, i, depth[b]) for i, b in enumerate(L)] if depth is not None else None
            torch.cuda.synchronize()
            res = gtr.trackImageSomeDeviceRefs(L, ts, [s.ref for s in surf], None if dsurf is None else [None if s is None else s.ref for s in dsurf])
            assert all(s.unwritten() for s in surf + [s for s in dsurf or [] if s is not None]), "call %d wrote into a caller's surface" % k
        for b in L:
            nxt[b] += 1
        run.append((res, [gtr.state(b) for b in range(B)]))
        if hook:
            hook(gtr, k)
    st = gtr.stats()
    if tracker is None:
        gtr.close()
    return run, st


def mixed_place(b, i, f):
    off, pad = MIXED[b % 3]
    return Surface(f, offset=off, pad=pad)


def lock_step(B, k=K):
    return [list(range(B))] * k


def route_of(st):
    return {n: st[n] for n in ("pyr_head", "pyr_level0_vec16", "pyr_level0_dword", "pyr_down_tail", "pyr_down_pad4", "pyr_down_bytes")}


def check_route(st, w, h, calls):
    if (w, h) == (320, 136):
        assert st["pyr_head"] == calls == st["pyr_down_tail"] and st["pyr_level0_dword"] == st["pyr_level0_vec16"] == 0
    elif (w, h) == (320, 240):
        assert st["pyr_level0_vec16"] == calls and st["pyr_down_bytes"] == 3 * calls and st["pyr_head"] == st["pyr_level0_dword"] == 0
    elif (w, h) == (644, 481):
        assert st["pyr_level0_dword"] == calls and st["pyr_down_bytes"] >= calls and st["pyr_head"] == 0
    else:
        assert st["pyr_level0_dword"] == calls and st["pyr_head"] == st["pyr_down_bytes"] == st["pyr_down_pad4"] == st["pyr_down_tail"] == 0


def cfg_of(gf, w, h, batch=3, **kw):
    kw.setdefault("depth_cam", 0)
    return gf.default_cfg(width=w, height=h, batch=batch, max_cnt=MAX_CNT, min_dist=MIN_DIST, **kw)


_BASE = {}


def baseline(gf, w, h):
    """the tight entry point, lock step, three sequences, no depth: shared by the cases that scatter the same frames"""
    if (w, h) not in _BASE:
        _BASE[w, h] = drive(gf, cfg_of(gf, w, h), frames_of(w, h), lock_step(3))
    return _BASE[w, h]


@pytest.mark.parametrize("w,h", SIZES)
def test_own_allocations_are_the_aligned_form(gf, w, h):
    """cases 1 and 13: every frame in an allocation of its own, pitch = width.  The route and every counter are those of the handle that only knows the old entry
    points, whose new counter stays 0"""
    base, st0 = baseline(gf, w, h)
    run, st = drive(gf, cfg_of(gf, w, h), frames_of(w, h), lock_step(3), place=lambda b, i, f: Surface(f))
    same_run(base, run, "own allocations %dx%d" % (w, h))
    check_route(st, w, h, K)
    check_route(st0, w, h, K)
    assert st["frames_unaligned"] == 0 == st0["frames_unaligned"]
    for n in ("frames", "sequence_frames", "lk_launches", "lk_points", "lk_level_passes", "lk_iterations", "tracked_features", "output_features"):
        assert st[n] == st0[n], n
    assert route_of(st) == route_of(st0)
    print("tracked features", w, h, st["tracked_features"], "of", 3 * (K - 1) * MAX_CNT)
    if w >= 320:
        assert st["tracked_features"] > 3 * (K - 1) * MAX_CNT // 2, "the scene does not carry its tracks: the case shows nothing"


@pytest.mark.parametrize("w,h,unaligned", [(320, 136, 2), (320, 240, 2), (644, 481, 1), (40, 36, 1)])
def test_one_call_mixes_the_load_forms(gf, w, h, unaligned):
    """case 2: base offsets 0 / 4 / 1 and pitches w, w + 36, w + 37 in one call.  The counter: frames that miss the widest piece of the kernel that reads them --
    16 bytes in the head kernel and the 16-byte level 0 (the offset-4 and the offset-1 frame), a dword in the dword level 0 (the offset-1 frame alone)"""
    base, _ = baseline(gf, w, h)
    run, st = drive(gf, cfg_of(gf, w, h), frames_of(w, h), lock_step(3), place=mixed_place)
    same_run(base, run, "mixed alignments %dx%d" % (w, h))
    check_route(st, w, h, K)
    assert st["frames_unaligned"] == unaligned * K


@pytest.mark.parametrize("fill", [0xFF, (7,)], ids=["0xFF", "random"])
def test_luma_plane_and_crop(gf, fill):
    """cases 3 and 4: sequence 0 is the luma plane of an NV12-shaped surface (pitch rounded up to 256, 3 h / 2 rows, chroma and padding filled), sequence 1 a crop
    window of a wider and taller image, sequence 2 a crop at an odd column.  Two fillings of everything around the frames, the same bits"""
    w, h = 320, 136

    def place(b, i, f):
        if b == 0:
            return Surface(f, pitch=(w + 255) // 256 * 256, rows_total=3 * h // 2, fill=fill)
        return Surface(f, pad=64, rows_total=h + 20, y0=7, x0=16 if b == 1 else 13, fill=fill)

    base, _ = baseline(gf, w, h)
    run, st = drive(gf, cfg_of(gf, w, h), frames_of(w, h), lock_step(3), place=place)
    same_run(base, run, "luma plane and crops")
    assert st["frames_unaligned"] == K and st["pyr_head"] == K     # the crop at column 13; pitches 512 and 400 and column 16 keep the 16-byte form


def _in_format(gf, fmt, f):
    """a frame of the format whose gray image is close to f"""
    if fmt == gf.PIX_RGB8:
        return np.stack([f, np.roll(f, 1, 1), 255 - f // 2], -1)
    if fmt == gf.PIX_BAYER_RGGB8:
        return f
    if fmt == gf.PIX_YUV422_UYVY:
        return np.stack([np.roll(f, 3, 0), f], -1)
    v = f.astype(np.uint16) * 257 ^ (np.roll(f, 2, 1) & 63)
    return v.astype("<u2").view(np.uint8).reshape(f.shape[0], f.shape[1], 2)


@pytest.mark.parametrize("fmt", ["PIX_RGB8", "PIX_BAYER_RGGB8", "PIX_YUV422_UYVY", "PIX_MONO16"])
def test_pixel_formats_scattered(gf, fmt):
    """case 6: the conversion kernels are the first readers.  Sequence 0 takes the dword form at 16 pixels a lane, sequence 1 (offset 4, pitch + 36) the same, sequence
    2 (offset 1: MONO16 at an odd address; pitch + 37: RGB8 rows 997 bytes apart) the byte form -- two launches in one call"""
    w, h = 320, 240
    fmt = getattr(gf, fmt)
    frames = [[_in_format(gf, fmt, f) for f in seq] for seq in frames_of(w, h)]
    base, _ = drive(gf, cfg_of(gf, w, h, pixel_format=fmt), frames, lock_step(3))
    run, st = drive(gf, cfg_of(gf, w, h, pixel_format=fmt), frames, lock_step(3), place=mixed_place)
    same_run(base, run, "pixel format %d" % fmt)
    print("tracked features", fmt, st["tracked_features"], "of", 3 * (K - 1) * MAX_CNT)
    assert st["frames_unaligned"] == K and st["pyr_level0_vec16"] == K
    assert st["tracked_features"] > 3 * (K - 1) * MAX_CNT // 3, "the converted frames do not carry their tracks: the case shows nothing"


def test_equalize_scattered(gf):
    """case 7: CLAHE is the first reader of MONO8 frames"""
    w, h = 320, 240
    base, _ = drive(gf, cfg_of(gf, w, h, equalize=1), frames_of(w, h), lock_step(3))
    run, st = drive(gf, cfg_of(gf, w, h, equalize=1), frames_of(w, h), lock_step(3), place=mixed_place)
    same_run(base, run, "equalize")
    assert st["frames_unaligned"] == 2 * K and st["pyr_level0_vec16"] == K


def _depths(w, h, n=4):
    rng = np.random.default_rng(5)
    return [rng.integers(300, 9000, (h, w), dtype=np.uint16) for _ in range(n)]


def _depth_case(gf, w, h):
    depth = _depths(w, h)
    setup = lambda t: t.set_seq_cfg(1, depth_cam=0)
    base, _ = drive(gf, cfg_of(gf, w, h, depth_cam=1), frames_of(w, h), lock_step(3), depth=depth, setup=setup)
    run, st = drive(gf, cfg_of(gf, w, h, depth_cam=1), frames_of(w, h), lock_step(3), place=mixed_place, depth=depth, setup=setup,
                    depth_place=lambda b, i, d: None if b == 1 else Surface(d, pad=40, offset=2 * b))
    same_run(base, run, "depth by reference")
    d0, d1 = run[-1][0][0][1][:, 7], run[-1][0][1][1][:, 7]
    assert len(set(d0)) > 10 and d0.min() >= 0.3 and set(d1) == {-2.4}, "the depths of the case are not the images' samples"
    return st


def test_depth_by_reference(gf):
    """case 8: u16 depth frames with a pitch of (w + 20) x 2 bytes in allocations of their own; sequence 1 has depth_cam = 0 and a null entry.  The samples of
    tracked points come from the LK kernel, those of new corners from the selection kernels: both read the table"""
    _depth_case(gf, 320, 240)


@pytest.mark.parametrize("env", ["GF_LK_POINTS=4", "GF_LK_POINTS=2", "GF_SELECT_TOPK=0"])
def test_kernel_variants_read_the_table(gf, monkeypatch, env):
    """case 9: the switches are read when a tracker is created, as in the other files' switch tests"""
    monkeypatch.setenv(*env.split("="))
    _depth_case(gf, 320, 240)


def _predict(rng, cfg, ids, pts):
    sel = rng.random(len(ids)) < 0.7
    uv = pts[sel] + rng.normal(0, 1.0, (sel.sum(), 2))
    xyz = np.stack([(uv[:, 0] - cfg.cx) / cfg.fx * 2.0, (uv[:, 1] - cfg.cy) / cfg.fy * 2.0, np.full(len(uv), 2.0)], 1)
    return ids[sel], xyz


def test_changing_lists_aliases_and_feedback(gf):
    """case 10: the list changes from call to call and is rotated, sequence 2 sits calls out, sequences 0 and 3 read the same frame memory (one surface, two
    entries), and setPrediction / removeOutliers go in between calls"""
    w, h = 320, 240
    fr = frames_of(w, h)
    frames = [fr[0], fr[1], fr[2], fr[0]]
    lists = [[0, 1, 2, 3], [1, 3, 0], [3, 0, 1, 2], [0, 3], [2, 1, 0, 3], [3, 1, 0]]

    def hook_of():
        rng = np.random.default_rng(3)

        def hook(gtr, k):
            if k in (1, 3):
                for b in (1, 3):
                    ids = gtr.state(b)[0]
                    gtr.removeOutliers(ids[rng.random(len(ids)) < 0.1], seq=b)
                    ids, _, pts = gtr.state(b)
                    gtr.setPrediction(*_predict(rng, gtr.cfg, ids, pts), seq=b)
        return hook

    shared = {}

    def place(b, i, f):
        if b in (0, 3):      # both are listed in every call and take the same frame: one surface, two entries of the table
            if id(f) not in shared:
                shared[id(f)] = Surface(f, offset=1, pad=37)
            return shared[id(f)]
        return mixed_place(b, i, f)

    base, st0 = drive(gf, cfg_of(gf, w, h, batch=4), frames, lists, hook=hook_of())
    run, st = drive(gf, cfg_of(gf, w, h, batch=4), frames, lists, place=place, hook=hook_of())
    same_run(base, run, "changing lists")
    assert st["lk_launches"] == st0["lk_launches"] > len(lists) - 1, "no call took the predicted launch"
    assert st["sequence_frames"] == sum(len(l) for l in lists)
    same(run[0][0][0], run[0][0][3], "sequences 0 and 3 of the first call, the same memory")
    assert len(shared) == len(lists)


def test_refs_route_against_the_oracle(gf, oracle):
    """the _refs route held to oracle.Tracker directly, scattered frames and depth, 320 x 240"""
    w, h = 320, 240
    frames, depth = frames_of(w, h), _depths(w, h)
    otrs = [oracle.Tracker(oracle.default_cfg(max_cnt=MAX_CNT, min_dist=MIN_DIST)) for _ in range(3)]
    lists = [[0, 1, 2], [2, 0], [1, 2, 0], [0, 1], [2, 1, 0], [1, 0, 2]]
    run, _ = drive(gf, cfg_of(gf, w, h, depth_cam=1), frames, lists, place=mixed_place, depth=depth, depth_place=lambda b, i, d: Surface(d, pad=40))
    nxt = [0, 0, 0]
    for k, L in enumerate(lists):
        for i, b in enumerate(L):
            same(otrs[b].track(DT * nxt[b], frames[b][nxt[b]], depth[b]), run[k][0][i], "call %d, sequence %d" % (k, b))
            nxt[b] += 1
        for b in range(3):
            same_state(otrs[b].state(), run[k][1][b], "call %d, sequence %d" % (k, b))


def test_batch_entry_is_the_full_list(gf):
    w, h = 320, 240
    base, _ = baseline(gf, w, h)
    frames = frames_of(w, h)
    gtr = gf.FeatureTracker(cfg_of(gf, w, h))
    for k in range(2):
        surf = [mixed_place(b, b, frames[b][k]) for b in range(3)]
        res = gtr.trackImageBatchDeviceRefs([DT * k] * 3, [s.ref for s in surf])
        for b in range(3):
            same(base[k][0][b], res[b], "batch entry, call %d, sequence %d" % (k, b))
    gtr.close()


def test_roi_masks_by_reference(gf):
    """case 11: masks as crops of a larger tensor give the bits of the tight setter, in gf_tracker_get_roi and in the tracking results"""
    import torch
    w, h = 320, 240
    rng = np.random.default_rng(9)
    masks = []
    for b in range(3):
        m = np.zeros((h, w), np.uint8)
        m[20 + 10 * b:h - 30, 30:w - 20 - 15 * b] = rng.integers(1, 256, (h - 50 - 10 * b, w - 50 - 15 * b), dtype=np.uint8)
        m[100:130, 100 + 20 * b:160] = 0
        masks.append(m)
    big = np.random.default_rng(10).integers(0, 256, (3, h + 11, w + 45), dtype=np.uint8)
    for b in range(3):
        big[b, 5:5 + h, 13:13 + w] = masks[b]
    dbig = torch.from_numpy(big).cuda()
    before = dbig.clone()
    pitch = w + 45
    refs = [(dbig.data_ptr() + b * (h + 11) * pitch + 5 * pitch + 13, pitch) for b in range(3)]
    order = [2, 0, 1]
    tight = torch.from_numpy(np.stack([masks[b] for b in order])).cuda()
    torch.cuda.synchronize()
    a, _ = drive(gf, cfg_of(gf, w, h), frames_of(w, h), lock_step(3), setup=lambda t: t.set_roi_device(order, tight.data_ptr()))
    got = {}

    def setup(t):
        t.set_roi_device_refs(order, [refs[b] for b in order])
        for b in range(3):
            got[b] = t.get_roi(b)

    r, _ = drive(gf, cfg_of(gf, w, h), frames_of(w, h), lock_step(3), setup=setup)
    same_run(a, r, "region of interest by reference")
    for b in range(3):
        assert np.array_equal(got[b], np.where(masks[b] != 0, 255, 0).astype(np.uint8)), "sequence %d: stored region" % b
    assert torch.equal(dbig, before)
    base, _ = baseline(gf, w, h)
    assert any(not np.array_equal(x[0][1], y[0][1]) for (x, _), (y, _) in zip(base, r)), "the regions change nothing: the case shows nothing"
    # clearing through the table form's NULL, and its refusals
    gtr = gf.FeatureTracker(cfg_of(gf, w, h))
    gtr.set_roi_device_refs([0, 1], [refs[0], refs[1]])
    gtr.set_roi_device_refs([1], None)
    assert gtr.get_roi(0) is not None and gtr.get_roi(1) is None
    for bad, msg in (([refs[0], None], "list position 1.*null data"), ([refs[0], (refs[1][0], w - 1)], "list position 1.*pitch shorter")):
        with pytest.raises(gf.GfError, match="gf status -1.*" + msg):
            gtr.set_roi_device_refs([0, 1], bad)
    with pytest.raises(gf.GfError, match="gf status -1.*listed twice"):
        gtr.set_roi_device_refs([1, 1], [refs[0], refs[1]])
    assert gtr.get_roi(1) is None and np.array_equal(gtr.get_roi(0), got[0])
    gtr.close()


def test_refusals_change_nothing(gf):
    """case 12: every refusal is GF_ERR_INVALID with the list position in its message, leaves state() of every sequence and the stats as they were, and the next
    valid call gives the baseline's bits"""
    w, h = 320, 240
    frames, depth = frames_of(w, h), _depths(w, h)
    setup = lambda t: t.set_seq_cfg(1, depth_cam=0)
    base, _ = drive(gf, cfg_of(gf, w, h, depth_cam=1), frames, lock_step(3), depth=depth, setup=setup)
    gtr = gf.FeatureTracker(cfg_of(gf, w, h, depth_cam=1))
    setup(gtr)
    dplace = lambda b, i, d: None if b == 1 else Surface(d, pad=40)
    run, _ = drive(gf, None, frames, lock_step(3, 2), place=mixed_place, depth=depth, depth_place=dplace, tracker=gtr)
    same_run(base[:2], run, "before the refusals")
    before, stats = [gtr.state(b) for b in range(3)], gtr.stats()
    g = [mixed_place(b, b, frames[b][2]).ref for b in range(3)]
    d = [Surface(depth[b], pad=40).ref for b in range(3)]
    L, ts = [0, 1, 2], [DT * 2] * 3
    bad = [
        (L, None, d, "null table"),
        (L, [g[0], None, g[2]], d, "gray frame at list position 1.*null data"),
        (L, [g[0], g[1], (g[2][0], w - 1)], d, "gray frame at list position 2.*pitch shorter"),
        (L, g, [None, d[1], d[2]], "depth frame at list position 0.*null data"),             # sequence 0 has a depth camera
        (L, g, [d[0], None, (d[2][0] + 1, d[2][1])], "depth frame at list position 2.*odd"),
        (L, g, [(d[0][0], d[0][1] + 1), None, d[2]], "depth frame at list position 0.*odd"),
        (L, g, [(d[0][0], 2 * w - 2), None, d[2]], "depth frame at list position 0.*pitch shorter"),
        ([0, 3], g[:2], None, "names sequence 3"), ([1, 2, 1], g, None, "listed twice"), ([0, 1, 2, 0], g + g[:1], None, "4 sequences listed"),
    ]
    for lst, gr, dr, msg in bad:
        with pytest.raises(gf.GfError, match="gf status -1.*" + msg):
            gtr.trackImageSomeDeviceRefs(lst, [1.0] * len(lst), gr, dr)
    out = np.zeros((3, gtr.cap), gf.OBS_DTYPE)
    n = np.zeros(3, np.int32)
    args = (gtr.h, 3, gf._p(np.array(L, np.int32), C.c_int), gf._p(np.array(ts), C.c_double), gf.frame_refs(g), None)
    assert gf.lib().gf_tracker_track_some_device_refs(*args, None, gtr.cap, gf._p(n, C.c_int)) == -1
    assert gf.lib().gf_tracker_track_some_device_refs(None, *args[1:], out.ctypes.data_as(C.POINTER(gf.FeatureObs)), gtr.cap, gf._p(n, C.c_int)) == -1
    assert gf.lib().gf_tracker_track_batch_device_refs(None, args[3], args[4], None, out.ctypes.data_as(C.POINTER(gf.FeatureObs)), gtr.cap, gf._p(n, C.c_int)) == -1
    assert len(gtr.trackImageSomeDeviceRefs([], [], None)) == 0 and len(gtr.trackImageSomeDeviceRefs([], [], [])) == 0     # count == 0: accepted, nothing happens
    for b in range(3):
        same_state(before[b], gtr.state(b), "sequence %d after the refused calls" % b)
    assert gtr.stats() == stats
    run, _ = drive(gf, None, frames, lock_step(3, K - 2), place=mixed_place, depth=depth, depth_place=dplace, tracker=gtr, start=2)
    for (res_a, st_a), (res_b, st_b) in zip(base[2:], run):
        for i in range(3):
            same(res_a[i], res_b[i], "after the refusals, list position %d" % i)
            same_state(st_a[i], st_b[i], "after the refusals, sequence %d" % i)
    gtr.close()
