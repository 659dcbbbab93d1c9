"""Bayer, YUV 4:2:2 and MONO16 -> MONO8 on the device (gf_cvt_gray_batch*, the tracker's `pixel_format`, the estimator and gf_replay on top of it) against the
numpy restatement of cv_bridge::toCvCopy(msg, MONO8) for these encodings (raw_gray_ref.py), bit for bit: nothing here has a tolerance and nothing is excluded.
A handle that takes raw frames must give what a MONO8 handle gives on the restatement's gray frames.  Run with -m gpu."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ground-fusion_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvt_gray_ref as CR  # noqa: E402
import raw_gray_ref as R  # noqa: E402
import synth  # noqa: E402
import synth_stream as SS  # noqa: E402

pytestmark = pytest.mark.gpu

DT = 0.0666
NAMES = dict(R.ENCODING)
RAW_IDS = [NAMES[f] for f in R.RAW]
_cache = {}


def _dev(a):
    """a host u8 array on the device (flat), synchronised"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).reshape(-1)).cuda()
    torch.cuda.synchronize()
    return t


def _shape(fmt, *lead):
    """(..., h, w) -> the shape of frames of format fmt"""
    return tuple(lead) + ((2,) if R.BYTES[fmt] == 2 else ())


def _convert(gf, frames, fmt, pitch=None):
    """gf_cvt_gray_batch_device on tight (or pitched, flat) host frames -> [batch, h, w]"""
    import torch
    b, h, w = frames.shape[:3]
    src = _dev(frames)
    dst = torch.zeros(b * h * w, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    gf.cvt_gray_device(src.data_ptr(), pitch or w * R.BYTES[fmt], fmt, dst.data_ptr(), b, w, h)
    torch.cuda.synchronize()
    assert np.array_equal(src.cpu().numpy(), np.ascontiguousarray(frames).reshape(-1)), "the source was modified"
    return dst.cpu().numpy().reshape(b, h, w)


# ---------------------------------------------------------------------------------------------------------------- 1. shapes and alignments
# every width at which a form begins or ends (below 4, 4 .. 7: one-pixel Bayer form; 8, 16, 64: the dword forms; one off them), heights around the Bayer band
# height (16 rows), row paddings that keep and that break the dword alignment, the source base at byte offsets 0 .. 3
WIDTHS = [3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 31, 33, 64, 65]
HEIGHTS = [3, 4, 5, 6, 7, 15, 16, 17]
PADS = [0, 1, 2, 3, 5]
GUARD = 64


@pytest.mark.parametrize("fmt", R.RAW, ids=RAW_IDS)
def test_shapes_and_alignments(gf, fmt):
    """batch 3, every width x height x padding x source offset (at offset 3 the destination off its dword too): all sources in one device buffer, all
    destinations in another between guard bands of 0x5A that must come back untouched; one synchronisation; the sources must come back unchanged"""
    import torch
    bpp, batch = R.BYTES[fmt], 3
    rng = np.random.default_rng(900 + fmt)
    cases, src_parts, s_at, d_at = [], [], 0, 0
    for w in WIDTHS:
        for h in HEIGHTS:
            frames = rng.integers(0, 256, _shape(fmt, batch, h, w)).astype(np.uint8)
            want = R.to_gray(frames, fmt)
            for pad in PADS:
                view, pitch = R.padded(frames, pad, seed=w + pad)
                base = view
                while base.base is not None:
                    base = base.base
                flat = np.ascontiguousarray(base).reshape(-1)
                n_in = (batch * h - 1) * pitch + w * bpp                     # the last row ends with its pixels
                for off in range(4):
                    doff = 1 if off == 3 else 0
                    src_parts.append((s_at + off, flat[:n_in]))
                    cases.append((w, h, pad, off, pitch, s_at + off, d_at + GUARD + doff, want))
                    s_at += (off + n_in + 15) & ~15
                    d_at += (GUARD + doff + batch * h * w + GUARD + 15) & ~15
        # (the host entry, once per width: a padded view through gf_cvt_gray_batch)
        assert np.array_equal(gf.cvt_gray(view, fmt), want), ("host entry", NAMES[fmt], w)
    host_src = rng.integers(0, 256, s_at).astype(np.uint8)
    for at, part in src_parts:
        host_src[at:at + part.size] = part
    src = _dev(host_src)
    dst = torch.full((d_at,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for w, h, pad, off, pitch, sa, da, want in cases:
        gf.cvt_gray_device(src.data_ptr() + sa, pitch, fmt, dst.data_ptr() + da, batch, w, h)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    written = np.zeros(d_at, bool)
    for w, h, pad, off, pitch, sa, da, want in cases:
        n = batch * h * w
        got = out[da:da + n].reshape(batch, h, w)
        assert np.array_equal(got, want), (NAMES[fmt], w, h, pad, off, "%d pixels differ" % int(np.sum(got != want)))
        written[da:da + n] = True
    assert np.all(out[~written] == 0x5A), "a byte outside a destination was written"
    assert np.array_equal(src.cpu().numpy(), host_src), "a source was modified"


def test_mono16_every_value(gf):
    v = np.arange(65536, dtype="<u2").reshape(1, 256, 256)
    frame = v.view(np.uint8).reshape(1, 256, 256, 2)
    want = np.rint(v.astype(np.float64) * 255 / 65535).astype(np.uint8)
    assert np.array_equal(R.to_gray(frame, R.MONO16), want)
    assert np.array_equal(_convert(gf, frame, R.MONO16), want)
    assert np.array_equal(gf.cvt_gray(v[0].astype(np.uint16), R.MONO16), want[0])              # the host entry takes u16 pixels as they are


@pytest.mark.parametrize("fmt", R.BAYER, ids=[NAMES[f] for f in R.BAYER])
def test_bayer_random_frames_and_extremes(gf, fmt):
    """the dword form (64 x 33: two bands and a one-row band) and the one-pixel form (37 x 23): random frames, all 0, all 255, the two checkerboards of 0 and 255,
    row stripes and column stripes"""
    for w, h in ((64, 33), (37, 23)):
        yy, xx = np.indices((h, w))
        rng = np.random.default_rng(fmt * 100 + w)
        frames = np.stack([rng.integers(0, 256, (h, w)), rng.integers(0, 256, (h, w)), np.zeros((h, w)), np.full((h, w), 255), (yy + xx) % 2 * 255,
                           (yy + xx + 1) % 2 * 255, yy % 2 * 255, xx % 2 * 255, (yy + 1) % 2 * 255, (xx + 1) % 2 * 255]).astype(np.uint8)
        want = R.to_gray(frames, fmt)
        assert np.all(want[2] == 0) and np.all(want[3] == 255) and len(np.unique(want[6])) >= 2 and len(np.unique(want[7])) >= 2
        got = _convert(gf, frames, fmt)
        assert np.array_equal(got, want), (NAMES[fmt], w, h, [int(np.sum(g != t)) for g, t in zip(got, want)])


@pytest.mark.parametrize("fmt", R.RAW, ids=RAW_IDS)
def test_batch_beyond_the_grid_limit(gf, fmt):
    """65 537 frames of 4 x 3: blockIdx.y walks the frames strided"""
    n = 65537
    frames = np.random.default_rng(fmt).integers(0, 256, _shape(fmt, n, 3, 4)).astype(np.uint8)
    got = _convert(gf, frames, fmt)
    assert np.array_equal(got, R.to_gray(frames, fmt))


# ---------------------------------------------------------------------------------------------------------------- 2. the streams of the handle tests
HANDLE_FMTS = [R.BAYER_RGGB8, R.BAYER_GBRG8, R.YUV422_UYVY, R.MONO16]       # a pattern whose (0,0) is red, one whose (0,0) is green, one of each two-byte family
FLOOR = 20      # features every sequence must report on the last frame.  The CPU oracle on the restatement's gray frames of these streams reports 113 .. 124
                # (160 x 120, min_dist 10) and 150 (640 x 480, min_dist 30) on the last frame of every sequence, for each of the four formats: all streams are kept


def _frames_small(fmt, n_frames=6, batch=3, w=160, h=120):
    """the raw stream of the tracker tests and the restatement's gray frames of it: [frame][sequence], computed once per format and size"""
    key = ("stream", fmt, n_frames, batch, w, h)
    if key not in _cache:
        seqs = [synth.tracker_sequence(1000 + 31 * b, n_frames, w=w, h=h) for b in range(batch)]
        raw = [np.stack([R.encode(seqs[b][k], fmt, 97 * k + b) for b in range(batch)]) for k in range(n_frames)]
        gray = [R.to_gray(c, fmt) for c in raw]
        depth = [np.full((h, w), 1000 + 37 * k, np.uint16) for k in range(n_frames)]
        for c, g in zip(raw, gray):
            c.setflags(write=False)
            g.setflags(write=False)
        _cache[key] = (raw, gray, depth)
    return _cache[key]


# ---------------------------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_change_nothing(gf):
    import torch
    lib = gf.lib()
    w, h = 48, 16
    f = np.random.default_rng(9).integers(0, 256, (1, h, w, 2)).astype(np.uint8)
    buf = _dev(np.concatenate([f.reshape(-1), np.full(w * h, 0x5A, np.uint8)]))
    before = buf.cpu().numpy().copy()

    def refused(src, pitch, fmt, dst, what, ww=w, hh=h):
        rc = lib.gf_cvt_gray_batch_device(C.c_void_p(src), C.c_size_t(pitch), fmt, C.c_void_p(dst), 1, ww, hh, None)
        torch.cuda.synchronize()
        assert rc == -1 and what in lib.gf_last_error(), (rc, lib.gf_last_error())
        assert np.array_equal(buf.cpu().numpy(), before)

    p = buf.data_ptr()
    for fmt in (R.YUV422_UYVY, R.YUV422_YUY2, R.MONO16):
        refused(p, 2 * w, fmt, p, b"overlap")                          # in place
        refused(p, 2 * w, fmt, p + 2 * w * h - 1, b"overlap")          # the destination begins on the source's last byte
        refused(p + 8, 2 * w, fmt, p, b"overlap")                      # the destination's end reaches into the source
        refused(p, 2 * w - 1, fmt, p + 2 * w * h, b"pitch")
    for fmt in R.BAYER:
        refused(p, w, fmt, p, b"overlap")                              # a Bayer frame in place: unlike MONO8, a lane reads what another writes
        refused(p, w, fmt, p + w * h - 1, b"overlap")
        refused(p, w - 1, fmt, p + 2 * w * h, b"pitch")
        refused(p, w, fmt, p + 2 * w * h, b"3", ww=2, hh=h)            # no interior pixel
        refused(p, w, fmt, p + 2 * w * h, b"3", ww=w, hh=2)
    for fmt in (5, 6, 7, 15, 99, -1, 1 << 20):
        refused(p, 2 * w, fmt, p + 2 * w * h, b"pixel format")
    assert lib.gf_cvt_gray_batch_device(C.c_void_p(p), C.c_size_t(2 * w), R.YUV422_YUY2, C.c_void_p(p + 2 * w * h), 1, w, h, None) == 0     # next to each other is fine
    torch.cuda.synchronize()
    assert np.array_equal(buf.cpu().numpy()[2 * w * h:].reshape(h, w), R.to_gray(f[0], R.YUV422_YUY2))
    # a tracker handle: pixel_format out of range at create
    for bad in (-1, 5, 6, 7, 15, 99, 1 << 20):
        hnd = C.c_void_p()
        cfg = gf.default_cfg(width=160, height=120, pixel_format=bad)
        assert lib.gf_tracker_create(C.byref(cfg), C.byref(hnd)) == -1 and not hnd.value and b"pixel_format" in lib.gf_last_error()
    # a host stride below width x bytes on a raw handle, on every host entry point; then the handle still does what a fresh one does
    for fmt in (R.MONO16, R.BAYER_BGGR8):
        raw, gray, depth = _frames_small(fmt)
        B, W, H = 3, 160, 120
        bpp = R.BYTES[fmt]
        g = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=B, min_dist=10, pixel_format=fmt))
        g.trackImageBatch([0.0] * B, list(raw[0]), [depth[0]] * B)
        state = [g.state(b) for b in range(B)]
        frames = g.stats()["frames"]
        ptrs = (C.POINTER(C.c_uint8) * B)(*[gf._p(raw[1][b], C.c_uint8) for b in range(B)])
        ts = np.full(B, DT)
        out, n = np.zeros((B, g.cap), gf.OBS_DTYPE), np.full(B, -3, np.int32)
        seq = np.arange(B, dtype=np.int32)
        po = out.ctypes.data_as(C.POINTER(gf.FeatureObs))
        for stride in (bpp * W - 1, W // 2, 0):
            calls = [lib.gf_tracker_track_batch(g.h, gf._p(ts, C.c_double), ptrs, stride, None, 0, po, g.cap, gf._p(n, C.c_int)),
                     lib.gf_tracker_track_some(g.h, B, gf._p(seq, C.c_int), gf._p(ts, C.c_double), ptrs, stride, None, 0, po, g.cap, gf._p(n, C.c_int)),
                     lib.gf_tracker_track(g.h, 1, C.c_double(DT), ptrs[1], stride, None, 0, po, g.cap, gf._p(n, C.c_int)),
                     lib.gf_tracker_prefetch_batch(g.h, ptrs, stride, None, 0),
                     lib.gf_tracker_prefetch_some(g.h, B, gf._p(seq, C.c_int), ptrs, stride, None, 0)]
            assert calls == [-1] * 5 and b"stride" in lib.gf_last_error(), (stride, calls)
        assert np.all(n == -3) and not out["id"].any() and g.stats()["frames"] == frames
        for b in range(B):
            assert all(np.array_equal(x, y) for x, y in zip(state[b], g.state(b)))
        res = g.trackImageBatch([DT] * B, list(raw[1]), [depth[1]] * B)
        fresh = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=B, min_dist=10))
        fresh.trackImageBatch([0.0] * B, list(gray[0]), [depth[0]] * B)
        ref = fresh.trackImageBatch([DT] * B, list(gray[1]), [depth[1]] * B)
        for b in range(B):
            assert len(res[b][0]) > FLOOR
            assert np.array_equal(res[b][0], ref[b][0]) and np.array_equal(res[b][1].view(np.uint64), ref[b][1].view(np.uint64))
        g.close(); fresh.close()


# ---------------------------------------------------------------------------------------------------------------- 4. a raw handle equals a gray handle
LISTS = [[2, 0, 1], [1], [0, 2], [2, 1, 0], [1, 2], [0, 1, 2]]     # the `some` entries: lists that skip and reorder sequences; the last frame advances every sequence


def _same(res_a, res_b, ga, gb, seqs, tag):
    assert len(res_a) == len(res_b) == len(seqs)
    for i in range(len(seqs)):
        assert np.array_equal(res_a[i][0], res_b[i][0]), ("feature ids differ", tag, i)
        assert np.array_equal(res_a[i][1].view(np.uint64), res_b[i][1].view(np.uint64)), ("observations differ", tag, i)
    for b in range(ga.cfg.batch):
        assert all(np.array_equal(x, y) for x, y in zip(ga.state(b), gb.state(b))), ("state differs", tag, b)


def _raw_equals_gray(gf, fmt, equalize, entry, W, H, B, K, pad=5):
    import torch
    raw, gray, depth = _frames_small(fmt, K, B, W, H)
    min_dist = 30 if W >= 640 else 10     # a 160 x 120 frame holds some twenty corners 30 pixels apart: closer ones, so that the comparison has something to compare
    ga = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=B, min_dist=min_dist, equalize=equalize, pixel_format=fmt))
    gb = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=B, min_dist=min_dist, equalize=equalize))
    every = list(range(B))
    if entry == "staged":
        pinned = [torch.from_numpy(np.array(c)).pin_memory() for c in raw]
        dpin = [torch.from_numpy(np.stack([d] * B).view(np.int16)).pin_memory() for d in depth]
        ga.prefetchHost(pinned[0].data_ptr(), dpin[0].data_ptr())
    last = {}
    for k in range(K):
        seqs = LISTS[k % len(LISTS)] if entry.startswith("some") and B == 3 else every
        ts = [DT * k] * len(seqs)
        dep = [depth[k]] * len(seqs)
        if entry == "host":             # 5 bytes of random row padding
            view, pitch = R.padded(raw[k], pad, seed=k)
            ra = ga.trackImageBatch(ts, list(view), dep, stride=pitch)
        elif entry == "some":
            ra = ga.trackImageSome(seqs, ts, [raw[k][s] for s in seqs], dep)
        elif entry == "staged":
            if k + 1 < K:
                ga.prefetchHost(pinned[k + 1].data_ptr(), dpin[k + 1].data_ptr())
            ra = ga.trackPrefetched(ts)
        else:
            block = np.stack([raw[k][s] for s in seqs])
            dc = torch.from_numpy(block).cuda()
            dd = torch.from_numpy(np.stack(dep).view(np.int16)).cuda()
            torch.cuda.synchronize()
            ra = ga.trackImageBatchDevice(ts, dc.data_ptr(), dd.data_ptr()) if entry == "device" else ga.trackImageSomeDevice(seqs, ts, dc.data_ptr(), dd.data_ptr())
            torch.cuda.synchronize()
            assert np.array_equal(dc.cpu().numpy(), block), "frame %d: the caller's device frames were modified" % k
        rb = gb.trackImageSome(seqs, ts, [gray[k][s] for s in seqs], dep)
        _same(ra, rb, ga, gb, seqs, (NAMES[fmt], equalize, entry, k))
        for s, r in zip(seqs, ra):
            last[s] = len(r[0])
    assert sorted(last) == every and min(last.values()) >= FLOOR, ("a sequence ends with too few features to show anything", last)
    ga.close(); gb.close()


@pytest.mark.parametrize("entry", ["host", "device", "staged", "some", "some_device"])
@pytest.mark.parametrize("equalize", [0, 1])
@pytest.mark.parametrize("fmt", HANDLE_FMTS, ids=[NAMES[f] for f in HANDLE_FMTS])
def test_raw_handle_equals_gray_handle(gf, fmt, equalize, entry):
    """160 x 120, batch 3, 6 frames: observations (every bit), get_state and feature ids at every frame, with and without CLAHE behind the conversion, through
    every entry point that takes frames; every sequence ends with at least FLOOR features"""
    _raw_equals_gray(gf, fmt, equalize, entry, 160, 120, 3, 6)


@pytest.mark.parametrize("fmt,equalize", [(R.BAYER_GRBG8, 1), (R.YUV422_YUY2, 0), (R.MONO16, 0)], ids=["bayer_grbg8-equalize", "yuv422_yuy2", "mono16"])
def test_raw_handle_equals_gray_handle_vga(gf, fmt, equalize):
    """the same at the reference's frame size through the device entry point, one format per family: 640 x 480, batch 2, 3 frames"""
    _raw_equals_gray(gf, fmt, equalize, "device", 640, 480, 2, 3)


# ---------------------------------------------------------------------------------------------------------------- 5. stats
def test_stats(gf):
    """ms_convert on a raw handle; a MONO8 handle and an RGB8 handle behave as they did: no conversion time on the first, one on the second, the same counters
    and the same bits on the same gray content"""
    B, W, H = 3, 160, 120
    raw, gray, depth = _frames_small(R.BAYER_RGGB8)
    colour = [np.stack([CR.pack(g, g, g, CR.RGB8) for g in gk]) for gk in gray]        # r = g = b: the colour conversion returns the value (the weights sum to 2^14)
    assert all(np.array_equal(CR.to_gray(c, CR.RGB8), g) for c, g in zip(colour, gray))
    runs, outs = {}, {}
    for name, fmt, frames in (("raw", R.BAYER_RGGB8, raw), ("mono8", 0, gray), ("rgb8", CR.RGB8, colour)):
        g = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=B, min_dist=10, pixel_format=fmt))
        g.set_profiling(True)
        for k in range(4):
            outs[name] = g.trackImageBatch([DT * k] * B, list(frames[k]), [depth[k]] * B)
        runs[name] = g.stats()
        g.close()
    r, m, c = runs["raw"], runs["mono8"], runs["rgb8"]
    assert r["ms_convert"] > 0 and r["ms_total_gpu"] > r["ms_convert"] + r["ms_pyramid"] and r["ms_equalize"] == 0.0
    assert m["ms_convert"] == 0.0 and c["ms_convert"] > 0 and m["ms_pyramid"] > 0
    counters = [k for k in m if not k.startswith("ms_")]
    assert len(counters) >= 15 and m["frames"] == 4 and m["sequence_frames"] == 4 * B
    for k in counters:
        assert r[k] == m[k] == c[k], k
    for b in range(B):
        assert len(outs["raw"][b][0]) >= FLOOR
        for name in ("raw", "rgb8"):
            assert np.array_equal(outs[name][b][0], outs["mono8"][b][0]) and np.array_equal(outs[name][b][1].view(np.uint64), outs["mono8"][b][1].view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------- 6. estimator
def test_estimator_takes_bayer_frames(gf):
    """gf_estimator_input_image on an estimator whose tracker is configured for bayer_bggr8 against one that is fed the restatement's gray frames (the recording of
    the colour test)"""
    st = SS.Stream(1, t_still=1.5, t_move=2.0, v_max=0.4, yaw0=0.0, yaw_turn=-0.6, split_x=1.8, turn_delay=0.8)
    fmt = R.BAYER_BGGR8
    ests = []
    for f in (fmt, 0):
        cfg = gf.default_estimator_cfg(tio=SS.TIO, rio=SS.RIO, multiple_thread=0, with_tracker=1)
        cfg.tracker = gf.default_cfg(pixel_format=f)
        ests.append(gf.SlidingWindowEstimator(cfg))
    er, eg = ests
    tp = -1.0
    for k in range(len(st.cam_t)):
        for e in ests:
            t1 = st.feed(e, k, tp)
        tp = t1
        img, dep = st.image(k)
        mos = R.encode(img, fmt, k)
        fr = er.inputImage(float(st.cam_t[k]), mos, dep)
        fg = eg.inputImage(float(st.cam_t[k]), R.to_gray(mos, fmt), dep)
        assert sorted(fr) == sorted(fg) and all(np.array_equal(fr[i].view(np.uint64), fg[i].view(np.uint64)) for i in fr), "tracker output differs at image %d" % k
        sr, sg = er.state(), eg.state()
        for key in sr:
            assert np.array_equal(np.asarray(sr[key]), np.asarray(sg[key])), (k, key)
    assert er.state()["solver_flag"] == 1 and er.state()["n_optimizations"] > 5 and len(er.features()["id"]) > 20
    er.close(); eg.close()


# ---------------------------------------------------------------------------------------------------------------- 7. replay
@pytest.mark.parametrize("fmt", [R.BAYER_RGGB8, R.YUV422_UYVY], ids=["bayer_rggb8", "yuv422"])
def test_replay_with_device_gray_writes_the_same_trajectory(gf, tmp_path, fmt):
    """`gf_replay --device-gray --bag`: the raw topic's payload rows (a padded step) go to the tracker undecoded and are converted on the device; the default route
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
    for seq, (ns, kind, f) in enumerate(ev):
        if kind < 2:
            v = [float(x) for x in f[1:]]
            wr.write(topics["imu_topic" if kind == 0 else "wheel_topic"], "sensor_msgs/Imu" if kind == 0 else "nav_msgs/Odometry", ns,
                     BW.imu(seq, ns, v[0:3], v[3:6]) if kind == 0 else BW.odometry(seq, ns, v[0:3], v[3:6]))
        elif kind == 2:
            wr.write(topics["image0_topic"], "sensor_msgs/Image", ns, BW.image(seq, ns, R.encode(gf.read_pgm(os.path.join(d, f[1])), fmt, seq), NAMES[fmt], step_pad=7))
        else:
            wr.write(topics["image1_topic"], "sensor_msgs/Image", ns, BW.image(seq, ns, gf.read_pgm(os.path.join(d, f[1])), "16UC1"))
    wr.close()
    exe = os.path.join(ROOT, "bin", "gf_replay")
    assert os.path.exists(exe), "bin/gf_replay is missing: run `python __graft_entry__.py` (build)"
    cfg, bag = os.path.join(d, "config.yaml"), os.path.join(d, "rec.bag")
    a = subprocess.run([exe, cfg, "--bag", bag, os.path.join(d, "vio_host.txt")], capture_output=True, text=True, timeout=600)
    b = subprocess.run([exe, "--device-gray", cfg, "--bag", bag, os.path.join(d, "vio_device.txt")], capture_output=True, text=True, timeout=600)
    assert a.returncode == 0 and b.returncode == 0, (a.stderr, b.stderr)
    assert "%d RGB-D pairs (0 / 0 unpaired" % n in a.stdout and "%d RGB-D pairs (0 / 0 unpaired" % n in b.stdout
    ta, tb = open(os.path.join(d, "vio_host.txt"), "rb").read(), open(os.path.join(d, "vio_device.txt"), "rb").read()
    assert len(ta.splitlines()) > 5 and ta == tb
