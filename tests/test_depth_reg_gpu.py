"""Depth registration on the device (csrc/gf_depth_reg_kernels.hpp): the building blocks gf_depth_register_batch_device / gf_depth_register_batch held byte for byte
to the numpy restatement of tests/depth_reg_ref.py on its seven small cases (depth frames of 32 x 32 to 64 x 48: identity, a D435-like pair, down-sampling, a
colour camera in front of the depth camera, single counts, the torture case, an overflowing translation -- the census that shows they reach every rule is asserted
on the CPU, tests/test_depth_reg_host.py), and the tracker with a registration per sequence held bit for bit to a handle without any that is fed frames registered
beforehand.  There is no tolerance anywhere.  Device memory is torch uint8 tensors (allocations are at least 256-byte aligned); views at byte offsets and pitches
give the alignments: tight frames take the dword loads and the 16-byte stores, pitches that are odd multiples of 2 the u16 forms.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import depth_reg_ref as ref
import synth

pytestmark = pytest.mark.gpu

_EXPECTED = {}


def expected(c):
    """the restatement on a case, computed once and never changed"""
    if c["name"] not in _EXPECTED:
        out, _ = ref.register(c["depth"], c["reg"], c["colour"], c["wc"], c["hc"])
        out.setflags(write=False)
        _EXPECTED[c["name"]] = out
    return _EXPECTED[c["name"]]


def reg_of(gf, r):
    return gf.DepthReg.make(r["width"], r["height"], r["fx"], r["fy"], r["cx"], r["cy"], r["scale"], r["R"], r["T"])


def cam_of(gf, col):
    return gf.CameraModel.make(gf.CAMERA_PINHOLE, col[:4], col[4:])


class Plane:
    """a u16 frame [h, w] inside a device allocation: rows `pitch` bytes apart from byte `offset` on, a guard frame of the same size behind it; every byte that
    is not the frame's holds `fill`"""

    def __init__(self, w, h, pitch=None, offset=0, frame=None, fill=0x5A):
        import torch
        self.w, self.h, self.pitch, self.offset = w, h, pitch or 2 * w, offset
        host = np.full(offset + 2 * h * self.pitch, fill, np.uint8)
        if frame is not None:
            self.rows(host)[:] = np.ascontiguousarray(frame, "<u2").view(np.uint8).reshape(h, 2 * w)
        self.host = host
        self.buf = torch.from_numpy(host.copy()).cuda()
        self.ref = (self.buf.data_ptr() + offset, self.pitch)

    def rows(self, host):
        return np.lib.stride_tricks.as_strided(host[self.offset:], (self.h, 2 * self.w), (self.pitch, 1))

    def read(self):
        """(the frame, whether every byte outside its h rows of 2 w bytes -- the rest of each row, the guard frame -- is what it was)"""
        got = self.buf.cpu().numpy()
        frame = self.rows(got).copy().view("<u2")
        rest, was = got.copy(), self.host.copy()
        self.rows(rest)[:] = 0
        self.rows(was)[:] = 0
        return frame, np.array_equal(rest, was)


def run_block(gf, cases, src_pitch_extra=0, dst_pitch_extra=0, offset=0, one_at_a_time=False):
    import torch
    src = [Plane(c["reg"]["width"], c["reg"]["height"], 2 * c["reg"]["width"] + src_pitch_extra, offset, c["depth"]) for c in cases]
    dst = [Plane(c["wc"], c["hc"], 2 * c["wc"] + dst_pitch_extra, offset, None, 0xC3) for c in cases]
    torch.cuda.synchronize()
    regs, cams, sizes = [reg_of(gf, c["reg"]) for c in cases], [cam_of(gf, c["colour"]) for c in cases], [(c["wc"], c["hc"]) for c in cases]
    if one_at_a_time:
        for i in range(len(cases)):
            gf.depth_register_device([src[i].ref], [regs[i]], [cams[i]], [sizes[i]], [dst[i].ref])
    else:
        gf.depth_register_device([s.ref for s in src], regs, cams, sizes, [d.ref for d in dst])
    out = []
    for c, s, d in zip(cases, src, dst):
        frame, rest_ok = d.read()
        assert rest_ok, "%s: a byte outside the registered frame's rows was written" % c["name"]
        sf, s_ok = s.read()
        assert s_ok and np.array_equal(sf, c["depth"]), "%s: the source was written" % c["name"]
        out.append(frame)
    return out


def held(cases, frames, what):
    for c, f in zip(cases, frames):
        want = expected(c)
        assert np.array_equal(f, want), "%s, %s: %d of %d pixels differ from the restatement" % (what, c["name"], int((f != want).sum()), want.size)


def test_block_equals_restatement_as_one_batch_and_one_at_a_time(gf):
    cases = ref.cases()
    assert len({(c["reg"]["width"], c["reg"]["height"], c["wc"], c["hc"]) for c in cases}) >= 6   # one batch of different sizes
    a = run_block(gf, cases)
    held(cases, a, "one batch, tight frames")
    b = run_block(gf, cases)
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), "two runs differ"
    held(cases, run_block(gf, cases, one_at_a_time=True), "one at a time")
    held(cases[::-1], run_block(gf, cases[::-1]), "one batch, reversed")


@pytest.mark.parametrize("src_extra,dst_extra,offset", [(6, 10, 2), (4, 8, 4), (2, 2, 0), (16, 6, 16)])
def test_block_on_pitched_frames_writes_nothing_beyond_a_row(gf, src_extra, dst_extra, offset):
    """(6, 10, 2) and (2, 2, 0): pitches that are odd multiples of 2 (every case's 2 x width is a multiple of 4), so u16 loads and u16 stores; (4, 8, 4): dword
    loads, u16 stores; (16, 6, 16): dword loads from 16-byte rows, u16 stores.  Rows beyond 2 x wc bytes and the guard frame behind keep their bytes."""
    cases = ref.cases()
    held(cases, run_block(gf, cases, src_extra, dst_extra, offset), "pitches +%d / +%d at byte %d" % (src_extra, dst_extra, offset))


def test_block_odd_sizes(gf):
    """a depth frame of odd width (the last lane of a row of dword loads takes one count) into colour frames whose width is no multiple of 8 (the last lane of a
    row of the finish kernel writes u16s): crops of the D435-like case, against the restatement on the same crops"""
    c = ref.cases()[1]
    crops = []
    for k, (wd, hd, wc, hc) in enumerate([(47, 39, 61, 45), (33, 40, 64, 47), (48, 37, 59, 48)]):
        crops.append({"name": "d435_crop%d" % k, "depth": np.ascontiguousarray(c["depth"][:hd, :wd]), "reg": dict(c["reg"], width=wd, height=hd), "colour": c["colour"], "wc": wc, "hc": hc})
    held(crops, run_block(gf, crops, 2, 0, 0), "odd sizes, dword rows")      # 2 x 47 + 2 = 96: dword rows of an odd width
    held(crops, run_block(gf, crops, 0, 0, 0), "odd sizes, tight")


def test_z_buffer_is_primed_again(gf):
    """a batch with larger frames and nearer depths first: whatever it left in the z-buffer would win every minimum of the batch behind it.  The restatement is
    what a fresh process's first run gives (the tests above), so equality with it is equality with that run."""
    big = []
    for k, (w, h) in enumerate([(96, 80), (80, 64), (64, 64)]):
        d = np.full((h, w), 200 + k, np.uint16)   # 0.2 m: nearer than everything in the cases but the single counts
        big.append({"name": "near%d" % k, "depth": d, "reg": ref.make_reg(w, h, 0.9 * w, 0.9 * w, w / 2 - 0.5, h / 2 - 0.5), "colour": (0.9 * w, 0.9 * w, w / 2 - 0.5, h / 2 - 0.5, 0, 0, 0, 0), "wc": w, "hc": h})
    held(big, run_block(gf, big), "large near frames")
    cases = ref.cases()
    held(cases, run_block(gf, cases), "behind a batch of larger, nearer frames")
    held(cases[2:5], run_block(gf, cases[2:5]), "a shorter batch behind it")


def test_host_staged_form_equals_device_form(gf):
    cases = ref.cases()
    regs, cams, sizes = [reg_of(gf, c["reg"]) for c in cases], [cam_of(gf, c["colour"]) for c in cases], [(c["wc"], c["hc"]) for c in cases]
    out = gf.depth_register([c["depth"] for c in cases], regs, cams, sizes)
    held(cases, out, "gf_depth_register_batch")
    padded = []
    for c in cases:   # host frames with a row pitch
        a = np.full((c["reg"]["height"], c["reg"]["width"] + 3), 0x1234, np.uint16)
        a[:, :c["reg"]["width"]] = c["depth"]
        padded.append(a[:, :c["reg"]["width"]])
    held(cases, gf.depth_register(padded, regs, cams, sizes), "gf_depth_register_batch, pitched host frames")


def test_block_refusals(gf):
    c = ref.cases()[1]
    src, dst = Plane(48, 40, None, 0, c["depth"]), Plane(64, 48)
    reg, cam = reg_of(gf, c["reg"]), cam_of(gf, c["colour"])
    call = lambda s=src.ref, r=reg, m=cam, wh=(64, 48), d=dst.ref: gf.depth_register_device([s], [r], [m], [wh], [d])
    with pytest.raises(gf.GfError, match="pitch shorter than a row"):
        call(s=(src.ref[0], 94))
    with pytest.raises(gf.GfError, match="odd"):
        call(s=(src.ref[0] + 1, 96))
    with pytest.raises(gf.GfError, match="registered frame of entry 0.*pitch shorter"):
        call(d=(dst.ref[0], 126))
    with pytest.raises(gf.GfError, match="MEI"):
        call(m=gf.CameraModel.make(gf.CAMERA_MEI, c["colour"][:4], c["colour"][4:], 1.1))
    with pytest.raises(gf.GfError, match="colour size"):
        call(wh=(64, 5000))
    with pytest.raises(gf.GfError, match="scale"):
        call(r=reg_of(gf, dict(c["reg"], scale=0.0)))
    frame, rest_ok = dst.read()
    assert rest_ok and (frame == 0x5A5A).all(), "a refused call wrote"


# ---------------------------------------------------------------------------------------------------------------- the tracker
W, H = 160, 120
K = 8
DT = 0.0666
COLOUR = (150.0, 149.0, 79.5, 59.5)
DIST0 = (0.06, -0.09, 0.0005, -0.0003)            # sequence 0: colour distortion
LISTS = [[0, 1, 2], [2, 0], [1], [1, 2, 0], [0, 2], [2, 1, 0], [0, 1], [1, 0, 2], [2, 1], [1, 2, 0]]   # skip and reorder; every sequence takes its K frames
_TRACK = {}


def tracker_cfg(gf):
    cfg = gf.default_cfg(W, H, batch=3, max_cnt=40, min_dist=10, depth_cam=1)
    cfg.fx, cfg.fy, cfg.cx, cfg.cy = COLOUR
    return cfg


def tracker_inputs(w0=W, h0=H):
    """gray frames [sequence][step] and raw depth frames: sequence 0 from a 128 x 96 depth camera in 0.25 mm counts, 1 and 2 at the colour size in millimetres;
    w0 x h0: the colour size of sequence 0"""
    key = (w0, h0)
    if key not in _TRACK:
        gray = [synth.tracker_sequence(2100, K, w0, h0)] + [synth.tracker_sequence(2100 + b, K, W, H) for b in (1, 2)]
        raw = [[ref.scene(128, 96, 0.00025, 50 + k) for k in range(K)]] + [[ref.scene(W, H, 0.001, 60 + 10 * b + k) for k in range(K)] for b in (1, 2)]
        _TRACK[key] = (gray, raw)
    return _TRACK[key]


def regs_of_tracker(w0, h0):
    """sequence 0: a baseline, a small rotation, 0.25 mm counts; sequence 1: the identity registration"""
    r0 = ref.make_reg(128, 96, 118.0 * w0 / W, 118.0 * w0 / W, 63.5, 47.5, 0.00025, ref.rot(0.003, -0.002, 0.001), (0.02, 0.0005, -0.0004))
    r1 = ref.make_reg(W, H, *COLOUR)
    return r0, r1


def drive(gf, raw_planes, setup, lists=LISTS, w0=W, h0=H):
    """a handle of three sequences through `lists` on the _refs entry point; raw_planes[b][k]: the device depth frame of sequence b, step k.  Returns the results
    of every call, the states of all sequences behind it, and depth_reg_stats."""
    import torch
    gray, _ = tracker_inputs(w0, h0)
    t = gf.FeatureTracker(tracker_cfg(gf))
    setup(t)
    gplanes = [[torch.from_numpy(f).cuda() for f in gray[b]] for b in range(3)]
    torch.cuda.synchronize()
    nxt, run = [0, 0, 0], []
    for L in lists:
        ts = [DT * nxt[b] for b in L]
        g = [(gplanes[b][nxt[b]].data_ptr(), gplanes[b][nxt[b]].shape[1]) for b in L]
        d = [raw_planes[b][nxt[b]].ref for b in L]
        res = t.trackImageSomeDeviceRefs(L, ts, g, d)
        for b in L:
            nxt[b] += 1
        run.append((res, [t.state(b) for b in range(3)]))
    assert nxt == [K, K, K]
    st = t.depth_reg_stats()
    t.close()
    return run, st


def same_run(a, b, what, only=None):
    for k, ((ra, sa), (rb, sb)) in enumerate(zip(a, b)):
        for i, s in enumerate(LISTS[k]):
            if only is not None and s != only:
                continue
            assert np.array_equal(ra[i][0], rb[i][0]), "%s: call %d, sequence %d: ids differ" % (what, k, s)
            assert np.array_equal(ra[i][1].view(np.uint64), rb[i][1].view(np.uint64)), "%s: call %d, sequence %d: observations differ" % (what, k, s)
        for s in range(3):
            if only is None or s == only:
                assert all(np.array_equal(x, y) for x, y in zip(sa[s], sb[s])), "%s: call %d, sequence %d: state differs" % (what, k, s)


@pytest.mark.parametrize("w0,h0", [(W, H), (128, 96)])
def test_tracker_registers_on_the_device(gf, w0, h0):
    """(160, 120): every sequence at the handle's size.  (128, 96): sequence 0 has a frame size of its own, so the call takes the _sized forms of LK and the
    selection, and its depth is registered to 128 x 96."""
    _, raw = tracker_inputs(w0, h0)
    r0, r1 = regs_of_tracker(w0, h0)
    sized = (w0, h0) != (W, H)
    raw_planes = [[Plane(r["width"], r["height"], None, 0, raw[b][k]) for k in range(K)] for b, r in ((0, r0), (1, r1))] + [[Plane(W, H, None, 0, raw[2][k]) for k in range(K)]]
    # the frames of sequences 0 and 1 registered beforehand by the building block
    col0, col1 = cam_of(gf, COLOUR + DIST0), cam_of(gf, COLOUR + (0.0, 0.0, 0.0, 0.0))
    pre0 = [Plane(w0, h0) for _ in range(K)]
    pre1 = [Plane(W, H) for _ in range(K)]
    gf.depth_register_device([p.ref for p in raw_planes[0]], [reg_of(gf, r0)] * K, [col0] * K, [(w0, h0)] * K, [p.ref for p in pre0])
    gf.depth_register_device([p.ref for p in raw_planes[1]], [reg_of(gf, r1)] * K, [col1] * K, [(W, H)] * K, [p.ref for p in pre1])
    assert all(np.array_equal(pre1[k].read()[0], raw[1][k]) for k in range(K))          # the identity returns its input
    f0 = pre0[0].read()[0]
    assert (f0 != 0).mean() > 0.7 and f0.shape == (h0, w0)

    def common(t):
        k1, k2, p1, p2 = DIST0
        t.set_seq_cfg(0, k1=k1, k2=k2, p1=p1, p2=p2)
        if sized:
            t.set_seq_size(0, w0, h0)

    def with_reg(t):
        common(t)
        assert t.depth_reg_stats() == {"launches": 0, "frames": 0, "kernel_ms": 0.0} and t.get_seq_depth_reg(0) is None
        t.set_seq_depth_reg(0, reg_of(gf, r0))
        t.set_seq_depth_reg(1, reg_of(gf, r1))
        assert t.get_seq_depth_reg(0).as_dict() == reg_of(gf, r0).as_dict() and t.get_seq_depth_reg(2) is None

    a, st_a = drive(gf, raw_planes, with_reg, LISTS, w0, h0)
    b, st_b = drive(gf, [pre0, pre1, raw_planes[2]], common, LISTS, w0, h0)
    same_run(a, b, "registered in the call against registered beforehand")
    c, _ = drive(gf, [pre0, raw_planes[1], raw_planes[2]], common, LISTS, w0, h0)
    same_run(a, c, "identity registration against the raw frames", only=1)
    calls = sum(1 for L in LISTS if 0 in L or 1 in L)
    assert st_a["launches"] == 2 * calls and st_a["frames"] == sum((0 in L) + (1 in L) for L in LISTS) and st_a["kernel_ms"] > 0.0
    assert st_b == {"launches": 0, "frames": 0, "kernel_ms": 0.0}                        # a handle that never called the setter
    depths = np.concatenate([res[i][1][:, 7] for (res, _), L in zip(a, LISTS) for i, s in enumerate(L) if s == 0])
    assert len(depths) > 50 and (depths > 0).mean() > 0.5, "sequence 0 reports no depths: the test would show nothing"
    for p in raw_planes[0] + raw_planes[1]:
        f, ok = p.read()
        assert ok, "a raw depth frame's surroundings were written"


def fresh(gf, started=()):
    """a handle with a registration on sequence 0, none on 1 and 2; `started`: sequences that have taken one frame (without depth)"""
    gray, _ = tracker_inputs()
    t = gf.FeatureTracker(tracker_cfg(gf))
    t.set_seq_depth_reg(0, reg_of(gf, regs_of_tracker(W, H)[0]))
    for b in started:
        t.trackImageSome([b], [0.0], [gray[b][0]])
    return t, gray


def snapshot(t):
    return [t.state(b) for b in range(3)], t.stats()["sequence_frames"], t.depth_reg_stats()


def unchanged(a, b):
    return all(np.array_equal(x, y) for sa, sb in zip(a[0], b[0]) for x, y in zip(sa, sb)) and a[1:] == b[1:]


def test_other_entry_points_refuse_a_registered_sequence_with_depth(gf):
    import torch
    t, gray = fresh(gf, started=(0, 1))
    depth = np.full((H, W), 1500, np.uint16)
    before = snapshot(t)
    dg = torch.from_numpy(np.stack([gray[0][1], gray[1][1]])).cuda()
    dd = torch.from_numpy(np.stack([depth, depth]).view(np.int16)).cuda()
    dg3 = torch.from_numpy(np.stack([gray[b][1] for b in range(3)])).cuda()
    dd3 = torch.from_numpy(np.stack([depth] * 3).view(np.int16)).cuda()
    pin = np.ascontiguousarray(np.stack([gray[b][1] for b in range(3)]))
    pind = np.ascontiguousarray(np.stack([depth] * 3))
    torch.cuda.synchronize()

    def track_one():   # gf_tracker_track itself (FeatureTracker.trackImage goes through gf_tracker_track_some)
        out, n = np.zeros(t.cap, gf.OBS_DTYPE), C.c_int(0)
        f, d = np.ascontiguousarray(gray[0][1]), np.ascontiguousarray(depth)
        gf._chk(gf.lib().gf_tracker_track(t.h, 0, C.c_double(DT), f.ctypes.data_as(C.POINTER(C.c_uint8)), W, d.ctypes.data_as(C.POINTER(C.c_uint16)), W,
                                          out.ctypes.data_as(C.POINTER(gf.FeatureObs)), t.cap, C.byref(n)))

    for who, call in (("gf_tracker_track_some", lambda: t.trackImageSome([1, 0], [DT, DT], [gray[1][1], gray[0][1]], [depth, depth])),
                      ("gf_tracker_track", track_one),
                      ("gf_tracker_track_batch", lambda: t.trackImageBatch([DT] * 3, [gray[b][1] for b in range(3)], [depth] * 3)),
                      ("gf_tracker_track_some_device", lambda: t.trackImageSomeDevice([0, 1], [DT, DT], dg.data_ptr(), dd.data_ptr())),
                      ("gf_tracker_track_batch_device", lambda: t.trackImageBatchDevice([DT] * 3, dg3.data_ptr(), dd3.data_ptr())),
                      ("gf_tracker_prefetch_some", lambda: t.prefetchHost(pin.ctypes.data, pind.ctypes.data, seqs=[0, 2])),
                      ("gf_tracker_prefetch_batch", lambda: t.prefetchHost(pin.ctypes.data, pind.ctypes.data))):
        with pytest.raises(gf.GfError, match=r"%s: sequence 0 .*depth registration" % who):
            call()
        assert unchanged(before, snapshot(t)), who + " changed the handle"
    # without depth, and for lists without the sequence, they behave as before
    t.trackImageSome([0], [DT], [gray[0][1]])
    t.trackImageSome([1, 2], [DT, DT], [gray[1][1], gray[2][1]], [depth, depth])
    assert t.stats()["sequence_frames"] == before[1] + 3
    t.close()


def test_setter_state_rules_and_camera_interlock(gf):
    t, gray = fresh(gf, started=(0,))
    reg = reg_of(gf, regs_of_tracker(W, H)[0])
    with pytest.raises(gf.GfError, match="sequence 0 has taken a frame.*depth registration"):
        t.set_seq_depth_reg(0, None)
    with pytest.raises(gf.GfError, match="sequence 0 has taken a frame"):
        t.set_seq_depth_reg(0, reg)
    t.reset_seq(0)
    assert t.get_seq_depth_reg(0).as_dict() == reg.as_dict()                             # reset_seq keeps it
    t.set_seq_depth_reg(0, None)
    assert t.get_seq_depth_reg(0) is None
    t.set_seq_depth_reg(0, reg)
    pin = np.ascontiguousarray(np.stack([gray[1][0], gray[2][0]]))
    t.prefetchHost(pin.ctypes.data, seqs=[1, 2])                                         # staged without depth
    with pytest.raises(gf.GfError, match="sequence 1 is listed by a staged frame"):
        t.set_seq_depth_reg(1, reg)
    t.set_seq_depth_reg(0, reg)                                                          # a sequence the staged frame does not list
    t.trackPrefetched([0.0, 0.0])
    with pytest.raises(gf.GfError, match="gf_depth_reg.fx"):
        t.set_seq_depth_reg(0, reg_of(gf, dict(regs_of_tracker(W, H)[0], fx=-1.0)))
    assert t.get_seq_depth_reg(0).as_dict() == reg.as_dict()
    t.close()
    # the interlock with the camera model, both ways
    t = gf.FeatureTracker(tracker_cfg(gf))
    mei = gf.CameraModel.make(gf.CAMERA_MEI, COLOUR, (0.0, 0.0, 0.0, 0.0), 1.2)
    t.set_seq_camera(1, mei)
    with pytest.raises(gf.GfError, match="gf_tracker_set_seq_camera"):
        t.set_seq_depth_reg(1, reg)
    assert t.get_seq_depth_reg(1) is None
    t.set_seq_depth_reg(2, reg)
    with pytest.raises(gf.GfError, match="gf_tracker_set_seq_depth_reg"):
        t.set_seq_camera(2, mei)
    assert t.get_seq_camera(2).model == gf.CAMERA_PINHOLE
    t.set_seq_camera(2, gf.CameraModel.make(gf.CAMERA_PINHOLE, COLOUR, DIST0))           # a pinhole is no conflict
    t.set_seq_camera(1, gf.CameraModel.make(gf.CAMERA_PINHOLE, COLOUR))
    t.set_seq_depth_reg(1, reg)
    t.close()


def test_raw_depth_ref_with_a_short_or_odd_pitch_is_refused(gf):
    import torch
    t, gray = fresh(gf)
    g = [torch.from_numpy(gray[b][0]).cuda() for b in (1, 0)]
    raw = Plane(128, 96, None, 0, ref.scene(128, 96, 0.00025, 50))
    full = Plane(W, H, None, 0, np.full((H, W), 1500, np.uint16))
    torch.cuda.synchronize()
    grefs = [(x.data_ptr(), W) for x in g]
    before = snapshot(t)
    with pytest.raises(gf.GfError, match=r"raw depth frame at list position 1 \(sequence 0\): pitch shorter than a row"):
        t.trackImageSomeDeviceRefs([1, 0], [0.0, 0.0], grefs, [full.ref, (raw.ref[0], 254)])
    with pytest.raises(gf.GfError, match=r"raw depth frame at list position 1 \(sequence 0\): depth pointer or pitch is odd"):
        t.trackImageSomeDeviceRefs([1, 0], [0.0, 0.0], grefs, [full.ref, (raw.ref[0], 257)])
    with pytest.raises(gf.GfError, match=r"depth frame at list position 0 \(sequence 1\): pitch shorter than a row"):
        t.trackImageSomeDeviceRefs([1, 0], [0.0, 0.0], grefs, [(full.ref[0], 256), raw.ref])   # a row of the raw frame is too short for a sequence without one
    assert unchanged(before, snapshot(t))
    t.trackImageSomeDeviceRefs([1, 0], [0.0, 0.0], grefs, [full.ref, raw.ref])                  # 256-byte rows: what the registration asks for
    assert t.depth_reg_stats()["frames"] == 1
    t.close()


def test_a_sequence_without_a_depth_camera_carries_a_registration_that_never_runs(gf):
    """depth_cam == 0 on sequence 0: its raw frame (smaller than the colour frame) is neither registered nor sampled, and the call equals that of a handle
    without the registration that is given no frame for the sequence"""
    import torch
    gray, raw = tracker_inputs()
    reg = reg_of(gf, regs_of_tracker(W, H)[0])
    small, full = Plane(128, 96, None, 0, raw[0][0]), Plane(W, H, None, 0, raw[1][0])
    g = [[torch.from_numpy(gray[b][k]).cuda() for k in range(3)] for b in (0, 1)]
    torch.cuda.synchronize()
    runs = []
    for with_reg in (True, False):
        t = gf.FeatureTracker(tracker_cfg(gf))
        t.set_seq_cfg(0, depth_cam=0)
        if with_reg:
            t.set_seq_depth_reg(0, reg)
        out = [t.trackImageSomeDeviceRefs([0, 1], [DT * k] * 2, [(g[0][k].data_ptr(), W), (g[1][k].data_ptr(), W)], [small.ref if with_reg else None, full.ref]) for k in range(3)]
        assert t.depth_reg_stats()["frames"] == 0 and t.depth_reg_stats()["launches"] == 0
        runs.append((out, [t.state(b) for b in range(2)]))
        t.close()
    for k in range(3):
        for i in range(2):
            assert np.array_equal(runs[0][0][k][i][0], runs[1][0][k][i][0]) and np.array_equal(runs[0][0][k][i][1].view(np.uint64), runs[1][0][k][i][1].view(np.uint64)), (k, i)
    assert all(np.array_equal(x, y) for b in range(2) for x, y in zip(runs[0][1][b], runs[1][1][b]))
    assert len(runs[0][0][2][0][0]) > 10 and small.read()[1]
