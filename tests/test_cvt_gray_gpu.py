"""Colour -> MONO8 on the device (gf_cvt_gray_batch*, the tracker's `pixel_format`, the estimator and gf_replay on top of it) against the numpy restatement of
cv_bridge::toCvCopy(msg, MONO8) (cvt_gray_ref.py; getImageFromMsg, rosNodeTest.cpp:238-254), bit for bit: nothing here has a tolerance.  A handle that takes
colour frames must give what a MONO8 handle gives on the restatement's gray frames.  Run with -m gpu."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ground-fusion_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvt_gray_ref as R  # noqa: E402
import synth  # noqa: E402
import synth_stream as SS  # noqa: E402

pytestmark = pytest.mark.gpu

DT = 0.0666
NAMES = {R.MONO8: "mono8", R.RGB8: "rgb8", R.BGR8: "bgr8", R.RGBA8: "rgba8", R.BGRA8: "bgra8"}
_cache = {}


def _dev(a):
    """a host u8 array on the device (flat), synchronised"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return t


# ---------------------------------------------------------------------------------------------------------------- 1. every colour once
def _all_colours():
    """the three planes of a 4096 x 4096 frame that holds each of the 2^24 (r, g, b) values once, a random alpha plane, and the restatement's gray: computed once"""
    if "all" not in _cache:
        v = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
        r, g, b = (v & 255).astype(np.uint8), ((v >> 8) & 255).astype(np.uint8), (v >> 16).astype(np.uint8)
        a = np.random.default_rng(11).integers(0, 256, r.shape).astype(np.uint8)
        _cache["all"] = (r, g, b, a, R.gray_of(r, g, b))
    return _cache["all"]


@pytest.mark.parametrize("fmt", R.COLOUR, ids=[NAMES[f] for f in R.COLOUR])
def test_every_colour_once(gf, fmt):
    """weights, rounding and channel order for every input value, through the host entry and the device entry"""
    import torch
    r, g, b, a, want = _all_colours()
    frame = R.pack(r, g, b, fmt, a)
    assert np.array_equal(R.to_gray(frame, fmt), want)          # the packing puts the channels where the format says
    got = gf.cvt_gray(frame, fmt)
    assert got.shape == want.shape and np.array_equal(got, want), "%d pixels differ (host entry)" % int(np.sum(got != want))
    src = _dev(frame)
    dst = torch.zeros(4096 * 4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gf.cvt_gray_device(src.data_ptr(), 4096 * R.CHANNELS[fmt], fmt, dst.data_ptr(), 1, 4096, 4096)
    torch.cuda.synchronize()
    got = dst.cpu().numpy().reshape(4096, 4096)
    assert np.array_equal(got, want), "%d pixels differ (device entry)" % int(np.sum(got != want))


# ---------------------------------------------------------------------------------------------------------------- 2. shapes and alignments
# (width, height): one pixel, rows shorter than a piece, odd widths, exactly one / one more than a 64-pixel span, more than one workgroup, the tracker's small frame,
# VGA plus one minus one; (20, 3) and (36, 5) are multiples of 4 but not of 16 (the four-pixel pieces), which the list above does not contain
SIZES = [(1, 1), (3, 2), (5, 7), (17, 3), (64, 1), (65, 2), (257, 3), (160, 120), (641, 479), (20, 3), (36, 5)]
PADS = [0, 1, 2, 3, 5]
GUARD = 64


@pytest.mark.parametrize("fmt", [R.MONO8] + list(R.COLOUR), ids=[NAMES[f] for f in [R.MONO8] + list(R.COLOUR)])
def test_shapes_and_alignments(gf, fmt):
    """batch 3, every size, row padding 0 / 1 / 2 / 3 / 5 bytes of random content, on the device the source base at byte offsets 0 .. 3 (and once the destination
    off its dword too); the destination lies between guard bands that must come back untouched, the source must come back unchanged"""
    import torch
    ch, batch = R.CHANNELS[fmt], 3
    rng = np.random.default_rng(700 + fmt)
    for w, h in SIZES:
        shape = (batch, h, w) if fmt == R.MONO8 else (batch, h, w, ch)
        frames = rng.integers(0, 256, shape).astype(np.uint8)
        want = R.to_gray(frames, fmt)
        for pad in PADS:
            view, pitch = R.padded(frames, pad, seed=w + pad)
            base = view.base if view.base is not None else view
            while base.base is not None:
                base = base.base
            flat = np.ascontiguousarray(base).reshape(-1)                     # the rows with their padding, as they lie in memory
            assert flat.size == batch * h * pitch
            assert np.array_equal(R.to_gray(view, fmt), want)                # the padding does not matter to the reference
            got = gf.cvt_gray(view, fmt)
            assert np.array_equal(got, want), ("host entry", NAMES[fmt], w, h, pad)
            n_in = (batch * h - 1) * pitch + w * ch                          # the last row ends with its pixels
            for off in range(4):
                doff = 1 if off == 3 else 0
                src = torch.zeros(off + n_in, dtype=torch.uint8, device="cuda")
                src[off:] = torch.from_numpy(flat[:n_in]).cuda()
                dst = torch.full((GUARD + doff + batch * h * w + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                gf.cvt_gray_device(src.data_ptr() + off, pitch, fmt, dst.data_ptr() + GUARD + doff, batch, w, h)
                torch.cuda.synchronize()
                out = dst.cpu().numpy()
                tag = (NAMES[fmt], w, h, pad, off)
                assert np.array_equal(out[GUARD + doff:GUARD + doff + batch * h * w].reshape(batch, h, w), want), tag
                assert np.all(out[:GUARD + doff] == 0xA5) and np.all(out[GUARD + doff + batch * h * w:] == 0xA5), ("guard band written", tag)
                assert np.array_equal(src.cpu().numpy()[off:], flat[:n_in]), ("source modified", tag)


def test_stream_argument_and_mono8_in_place(gf):
    """asynchronous on the caller's stream; MONO8 may name the same tight frames as source and destination (every lane writes back what it read)"""
    import torch
    f = np.random.default_rng(3).integers(0, 256, (2, 33, 48, 3)).astype(np.uint8)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        src = torch.from_numpy(f).cuda()
        dst = torch.zeros(2 * 33 * 48, dtype=torch.uint8, device="cuda")
        gf.cvt_gray_device(src.data_ptr(), 48 * 3, R.BGR8, dst.data_ptr(), 2, 48, 33, stream=s.cuda_stream)
    s.synchronize()
    assert np.array_equal(dst.cpu().numpy().reshape(2, 33, 48), R.to_gray(f, R.BGR8))
    m = _dev(f[..., 0])
    gf.cvt_gray_device(m.data_ptr(), 48, R.MONO8, m.data_ptr(), 2, 48, 33)
    torch.cuda.synchronize()
    assert np.array_equal(m.cpu().numpy().reshape(2, 33, 48), f[..., 0])


# ---------------------------------------------------------------------------------------------------------------- 3. refusals
def _frames_small(fmt, n_frames=6, batch=3, w=160, h=120):
    """the colour stream of the tracker tests and the restatement's gray frames of it: [frame][sequence], computed once per format and size"""
    key = ("stream", fmt, n_frames, batch, w, h)
    if key not in _cache:
        seqs = [synth.tracker_sequence(1000 + 31 * b, n_frames, w=w, h=h) for b in range(batch)]
        colour = [np.stack([R.colourise(seqs[b][k], fmt, 97 * k + b) for b in range(batch)]) for k in range(n_frames)]
        gray = [R.to_gray(c, fmt) for c in colour]
        depth = [np.full((h, w), 1000 + 37 * k, np.uint16) for k in range(n_frames)]
        for c, g in zip(colour, gray):
            c.setflags(write=False)
            g.setflags(write=False)
        _cache[key] = (colour, gray, depth)
    return _cache[key]


def test_refusals_change_nothing(gf):
    import torch
    lib = gf.lib()
    w, h = 48, 16
    f = np.random.default_rng(9).integers(0, 256, (1, h, w, 3)).astype(np.uint8)
    buf = _dev(np.concatenate([f.reshape(-1), np.full(w * h, 0x5A, np.uint8)]))
    before = buf.cpu().numpy().copy()

    def refused(src, pitch, fmt, dst, what):
        rc = lib.gf_cvt_gray_batch_device(C.c_void_p(src), C.c_size_t(pitch), fmt, C.c_void_p(dst), 1, w, h, None)
        torch.cuda.synchronize()
        assert rc == -1 and what in lib.gf_last_error(), (rc, lib.gf_last_error())
        assert np.array_equal(buf.cpu().numpy(), before)

    p = buf.data_ptr()
    refused(p, 3 * w, R.RGB8, p, b"overlap")                         # in place
    refused(p, 3 * w, R.RGB8, p + 3 * w * h - 1, b"overlap")         # the destination begins on the source's last byte
    refused(p + 8, 3 * w, R.BGR8, p, b"overlap")                     # the destination's end reaches into the source
    refused(p, 3 * w - 1, R.RGB8, p + 3 * w * h, b"pitch")
    refused(p, 4 * w - 1, R.RGBA8, p + 3 * w * h, b"pitch")
    refused(p, 3 * w, 5, p + 3 * w * h, b"pixel format")
    refused(p, 3 * w, -1, p + 3 * w * h, b"pixel format")
    assert lib.gf_cvt_gray_batch_device(C.c_void_p(p), C.c_size_t(3 * w), R.RGB8, C.c_void_p(p + 3 * w * h), 1, w, h, None) == 0     # next to each other is fine
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy()[3 * w * h:].reshape(h, w), R.to_gray(f[0], R.RGB8))
    with pytest.raises(gf.GfError, match="overlap"):
        flat = np.zeros(3 * w * h + w * h, np.uint8)
        lib_src = flat[:3 * w * h].reshape(1, h, w, 3)
        gf._chk(lib.gf_cvt_gray_batch(C.c_void_p(lib_src.ctypes.data), C.c_size_t(3 * w), R.RGB8, gf._p(flat[2 * w * h:], C.c_uint8), 1, w, h))
    # a tracker handle: pixel_format out of range at create
    for bad in (-1, 5, 1 << 20):
        hnd = C.c_void_p()
        cfg = gf.default_cfg(width=160, height=120, pixel_format=bad)
        assert lib.gf_tracker_create(C.byref(cfg), C.byref(hnd)) == -1 and not hnd.value and b"pixel_format" in lib.gf_last_error()
    # a host stride below width x channels on a colour handle, on every host entry point; then the handle still does what a fresh one does
    colour, gray, depth = _frames_small(R.RGBA8)
    B, W, H = 3, 160, 120
    g = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=B, pixel_format=R.RGBA8))
    g.trackImageBatch([0.0] * B, list(colour[0]), [depth[0]] * B)
    state = [g.state(b) for b in range(B)]
    frames = g.stats()["frames"]
    ptrs = (C.POINTER(C.c_uint8) * B)(*[gf._p(colour[1][b], C.c_uint8) for b in range(B)])
    ts = np.full(B, DT)
    out, n = np.zeros((B, g.cap), gf.OBS_DTYPE), np.full(B, -3, np.int32)
    seq = np.arange(B, dtype=np.int32)
    for stride in (4 * W - 1, W, 0):
        calls = [lib.gf_tracker_track_batch(g.h, gf._p(ts, C.c_double), ptrs, stride, None, 0, out.ctypes.data_as(C.POINTER(gf.FeatureObs)), g.cap, gf._p(n, C.c_int)),
                 lib.gf_tracker_track_some(g.h, B, gf._p(seq, C.c_int), gf._p(ts, C.c_double), ptrs, stride, None, 0, out.ctypes.data_as(C.POINTER(gf.FeatureObs)), g.cap, gf._p(n, C.c_int)),
                 lib.gf_tracker_track(g.h, 1, C.c_double(DT), ptrs[1], stride, None, 0, out.ctypes.data_as(C.POINTER(gf.FeatureObs)), g.cap, gf._p(n, C.c_int)),
                 lib.gf_tracker_prefetch_batch(g.h, ptrs, stride, None, 0),
                 lib.gf_tracker_prefetch_some(g.h, B, gf._p(seq, C.c_int), ptrs, stride, None, 0)]
        assert calls == [-1] * 5 and b"stride" in lib.gf_last_error(), (stride, calls)
    assert lib.gf_tracker_track_prefetched(g.h, gf._p(ts, C.c_double), out.ctypes.data_as(C.POINTER(gf.FeatureObs)), g.cap, gf._p(n, C.c_int)) == -1     # nothing was staged
    assert np.all(n == -3) and not out["id"].any() and g.stats()["frames"] == frames
    for b in range(B):
        assert all(np.array_equal(x, y) for x, y in zip(state[b], g.state(b)))
    res = g.trackImageBatch([DT] * B, list(colour[1]), [depth[1]] * B)
    fresh = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=B))
    fresh.trackImageBatch([0.0] * B, list(gray[0]), [depth[0]] * B)
    ref = fresh.trackImageBatch([DT] * B, list(gray[1]), [depth[1]] * B)
    for b in range(B):
        assert np.array_equal(res[b][0], ref[b][0]) and np.array_equal(res[b][1].view(np.uint64), ref[b][1].view(np.uint64))
    g.close(); fresh.close()


# ---------------------------------------------------------------------------------------------------------------- 4. a colour handle equals a gray handle
LISTS = [[2, 0, 1], [1], [0, 2], [2, 1, 0], [1, 2], [0]]     # the `some` entries: lists that skip and reorder sequences


def _same(res_a, res_b, ga, gb, seqs, tag):
    assert len(res_a) == len(res_b) == len(seqs)
    for i in range(len(seqs)):
        assert np.array_equal(res_a[i][0], res_b[i][0]), ("feature ids differ", tag, i)
        assert np.array_equal(res_a[i][1].view(np.uint64), res_b[i][1].view(np.uint64)), ("observations differ", tag, i)
    for b in range(ga.cfg.batch):
        assert all(np.array_equal(x, y) for x, y in zip(ga.state(b), gb.state(b))), ("state differs", tag, b)


def _colour_equals_gray(gf, fmt, equalize, entry, W, H, B, K, pad=5):
    import torch
    colour, gray, depth = _frames_small(fmt, K, B, W, H)
    min_dist = 30 if W >= 640 else 10     # a 160 x 120 frame holds some twenty corners 30 pixels apart: closer ones, so that the comparison has something to compare
    ga = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=B, min_dist=min_dist, equalize=equalize, pixel_format=fmt))
    gb = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=B, min_dist=min_dist, equalize=equalize))
    every = list(range(B))
    if entry == "staged":
        pinned = [torch.from_numpy(np.array(c)).pin_memory() for c in colour]
        dpin = [torch.from_numpy(np.stack([d] * B).view(np.int16)).pin_memory() for d in depth]
        ga.prefetchHost(pinned[0].data_ptr(), dpin[0].data_ptr())
    n_out = 0
    for k in range(K):
        seqs = LISTS[k % len(LISTS)] if entry.startswith("some") else every
        ts = [DT * k] * len(seqs)
        dep = [depth[k]] * len(seqs)
        if entry == "host":             # 5 bytes of random row padding
            view, pitch = R.padded(colour[k], pad, seed=k)
            ra = ga.trackImageBatch(ts, list(view), dep, stride=pitch)
        elif entry == "some":
            ra = ga.trackImageSome(seqs, ts, [colour[k][s] for s in seqs], dep)
        elif entry == "staged":
            if k + 1 < K:
                ga.prefetchHost(pinned[k + 1].data_ptr(), dpin[k + 1].data_ptr())
            ra = ga.trackPrefetched(ts)
        else:
            raw = np.stack([colour[k][s] for s in seqs])
            dc = torch.from_numpy(raw).cuda()
            dd = torch.from_numpy(np.stack(dep).view(np.int16)).cuda()
            torch.cuda.synchronize()
            ra = ga.trackImageBatchDevice(ts, dc.data_ptr(), dd.data_ptr()) if entry == "device" else ga.trackImageSomeDevice(seqs, ts, dc.data_ptr(), dd.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(dc.cpu().numpy(), raw), "frame %d: the caller's device frames were modified" % k
        rb = gb.trackImageSome(seqs, ts, [gray[k][s] for s in seqs], dep)
        _same(ra, rb, ga, gb, seqs, (NAMES[fmt], equalize, entry, k))
        n_out = max(n_out, max(len(r[0]) for r in ra))
    assert n_out > 20, "the stream carries too few features to show anything"
    ga.close(); gb.close()


@pytest.mark.parametrize("entry", ["host", "device", "staged", "some", "some_device"])
@pytest.mark.parametrize("equalize", [0, 1])
@pytest.mark.parametrize("fmt", R.COLOUR, ids=[NAMES[f] for f in R.COLOUR])
def test_colour_handle_equals_gray_handle(gf, fmt, equalize, entry):
    """160 x 120, batch 3, 6 frames: observations (every bit), get_state and feature ids at every frame, for every format, with and without CLAHE behind the
    conversion, through every entry point that takes frames"""
    _colour_equals_gray(gf, fmt, equalize, entry, 160, 120, 3, 6)


@pytest.mark.parametrize("entry,fmt,equalize", [("device", R.BGRA8, 1), ("staged", R.RGB8, 0)], ids=["device-bgra8-equalize", "staged-rgb8"])
def test_colour_handle_equals_gray_handle_vga(gf, entry, fmt, equalize):
    """the same at the reference's frame size (the sixteen-pixel pieces, the fused pyramid head behind them): 640 x 480, batch 2, 3 frames"""
    _colour_equals_gray(gf, fmt, equalize, entry, 640, 480, 2, 3)


# ---------------------------------------------------------------------------------------------------------------- 5. stats
def test_stats(gf):
    colour, gray, depth = _frames_small(R.BGR8)
    B, W, H = 3, 160, 120
    cfg_default = gf.default_cfg(width=W, height=H, batch=B)
    cfg_left = gf.TrackerCfg(*[getattr(cfg_default, k) for k, _ in gf.TrackerCfg._fields_[:-1]])     # the last field never mentioned: zero, as a C caller's `= {}` leaves it
    assert cfg_left.pixel_format == 0
    runs = {}
    for name, cfg, frames in (("colour", gf.default_cfg(width=W, height=H, batch=B, pixel_format=R.BGR8), colour), ("default", cfg_default, gray), ("left", cfg_left, gray)):
        g = gf.FeatureTracker(cfg)
        g.set_profiling(True)
        for k in range(4):
            g.trackImageBatch([DT * k] * B, list(frames[k]), [depth[k]] * B)
        runs[name] = g.stats()
        g.close()
    c, d, l = runs["colour"], runs["default"], runs["left"]
    assert c["ms_convert"] > 0 and c["ms_total_gpu"] > c["ms_convert"] + c["ms_pyramid"] and c["ms_equalize"] == 0.0
    assert d["ms_convert"] == 0.0 and l["ms_convert"] == 0.0 and d["ms_pyramid"] > 0
    counters = [k for k in d if not k.startswith("ms_")]
    assert len(counters) >= 15 and d["frames"] == 4 and d["sequence_frames"] == 4 * B
    for k in counters:
        assert d[k] == l[k], k
        assert c[k] == d[k], k          # and the colour handle did the same work behind its conversion


# ---------------------------------------------------------------------------------------------------------------- 6. estimator
def test_estimator_takes_colour_frames(gf):
    """gf_estimator_input_image on an estimator whose tracker is configured for bgr8 against one that is fed the restatement's gray frames: the recording is the
    shortest one tests/test_estimator_gpu.py drives to a solved window with images (its tracker-feedback replay)"""
    st = SS.Stream(1, t_still=1.5, t_move=2.0, v_max=0.4, yaw0=0.0, yaw_turn=-0.6, split_x=1.8, turn_delay=0.8)
    ests = []
    for fmt in (R.BGR8, R.MONO8):
        cfg = gf.default_estimator_cfg(tio=SS.TIO, rio=SS.RIO, multiple_thread=0, with_tracker=1)
        cfg.tracker = gf.default_cfg(pixel_format=fmt)
        ests.append(gf.SlidingWindowEstimator(cfg))
    ec, eg = ests
    tp = -1.0
    for k in range(len(st.cam_t)):
        for e in ests:
            t1 = st.feed(e, k, tp)
        tp = t1
        img, dep = st.image(k)
        col = R.colourise(img, R.BGR8, k)
        fc = ec.inputImage(float(st.cam_t[k]), col, dep)
        fg = eg.inputImage(float(st.cam_t[k]), R.to_gray(col, R.BGR8), dep)
        assert sorted(fc) == sorted(fg) and all(np.array_equal(fc[i].view(np.uint64), fg[i].view(np.uint64)) for i in fc), "tracker output differs at image %d" % k
        sc, sg = ec.state(), eg.state()
        assert sorted(sc) == sorted(sg)
        for key in sc:
            assert np.array_equal(np.asarray(sc[key]), np.asarray(sg[key])), (k, key)
        pc, pg = ec.features(), eg.features()
        for key in pc:
            assert np.array_equal(np.asarray(pc[key]), np.asarray(pg[key])), (k, key)
    assert ec.state()["solver_flag"] == 1 and ec.state()["n_optimizations"] > 5 and len(ec.features()["id"]) > 20
    ec.close(); eg.close()


# ---------------------------------------------------------------------------------------------------------------- 7. replay
def test_replay_with_device_gray_writes_the_same_trajectory(gf, tmp_path):
    """`gf_replay --device-gray --bag`: the rgb8 topic's payload rows (a padded step) go to the tracker undecoded and are converted on the device; the default route
    decodes them on the host.  Same pixels, so vio.txt is the same file, byte for byte."""
    import bagwriter as BW
    st = SS.Stream(11, t_still=1.5, t_move=1.2, v_max=0.4, yaw0=0.0, yaw_turn=-0.6, split_x=1.8, turn_delay=0.8)
    d = str(tmp_path)
    topics = dict(imu_topic="/camera/imu", wheel_topic="/odom", image0_topic="/camera/color/image_raw", image1_topic="/camera/aligned_depth_to_color/image_raw")
    n = st.export(d, **{k: '"%s"' % v for k, v in topics.items()})
    ev = []
    for kind, name in enumerate(("imu", "wheel", "image0", "image1")):
        for line in open(os.path.join(d, name + ".csv")).read().splitlines():
            if line and not line.startswith("#"):
                f = line.split(",")
                ev.append((int(round(float(f[0]) * 1e9)), kind, f))
    ev.sort(key=lambda e: (e[0], e[1]))
    wr = BW.BagWriter(os.path.join(d, "rec.bag"), compression="none", chunk_bytes=4 << 20)
    n_colour = 0
    for seq, (ns, kind, f) in enumerate(ev):
        if kind < 2:
            v = [float(x) for x in f[1:]]
            wr.write(topics["imu_topic" if kind == 0 else "wheel_topic"], "sensor_msgs/Imu" if kind == 0 else "nav_msgs/Odometry", ns,
                     BW.imu(seq, ns, v[0:3], v[3:6]) if kind == 0 else BW.odometry(seq, ns, v[0:3], v[3:6]))
        elif kind == 2:
            col = R.colourise(gf.read_pgm(os.path.join(d, f[1])), R.RGB8, seq)
            n_colour += int(np.mean(R.to_gray(col, R.RGB8) != R.to_gray(col, R.BGR8)) > 0.5)
            wr.write(topics["image0_topic"], "sensor_msgs/Image", ns, BW.image(seq, ns, col, "rgb8", step_pad=7))
        else:
            wr.write(topics["image1_topic"], "sensor_msgs/Image", ns, BW.image(seq, ns, gf.read_pgm(os.path.join(d, f[1])), "16UC1"))
    wr.close()
    assert n_colour == n                # genuinely coloured: reading the topic as bgr8 would give other frames
    exe = os.path.join(ROOT, "bin", "gf_replay")
    assert os.path.exists(exe), "bin/gf_replay is missing: run `python __graft_entry__.py` (build)"
    cfg, bag = os.path.join(d, "config.yaml"), os.path.join(d, "rec.bag")
    a = subprocess.run([exe, cfg, "--bag", bag, os.path.join(d, "vio_host.txt")], capture_output=True, text=True, timeout=600)
    b = subprocess.run([exe, "--device-gray", cfg, "--bag", bag, os.path.join(d, "vio_device.txt")], capture_output=True, text=True, timeout=600)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert "%d RGB-D pairs (0 / 0 unpaired" % n in a.stdout and "%d RGB-D pairs (0 / 0 unpaired" % n in b.stdout
    ta, tb = open(os.path.join(d, "vio_host.txt"), "rb").read(), open(os.path.join(d, "vio_device.txt"), "rb").read()
    assert len(ta.splitlines()) > 5 and ta == tb
    c = subprocess.run([exe, "--device-gray", cfg, d], capture_output=True, text=True, timeout=60)      # the option goes with --bag
    assert c.returncode == 2 and "--bag" in c.stderr
