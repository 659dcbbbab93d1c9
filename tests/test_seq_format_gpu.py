"""A pixel format and an equalise switch per sequence (gf_tracker_set_seq_format) and the conversion with a format per frame under it (gf_cvt_gray_mixed*).

Yardsticks: the numpy restatements of cv_bridge::toCvCopy(msg, MONO8) (cvt_gray_ref.py, raw_gray_ref.py) for the building block, byte for byte; and for the
tracker a handle of batch 1 created with the sequence's pixel_format / equalize, fed the same frames -- ids, observations viewed as uint64 and get_state after
every call.  Nothing here has a tolerance.  Run with -m gpu."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cvt_gray_ref as CR  # noqa: E402
import raw_gray_ref as R  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu

DT = 0.0666
FORMATS = [CR.MONO8, CR.RGB8, CR.BGR8, CR.RGBA8, CR.BGRA8] + list(R.RAW)     # all twelve
BPP = {**CR.CHANNELS, **R.BYTES}
FLOOR = 20          # features every sequence must report on its last frame (tests/test_raw_gray_gpu.py)
_cache = {}


def to_gray(frame, fmt):
    return CR.to_gray(frame, fmt) if fmt in CR.CHANNELS else R.to_gray(frame, fmt)


def encode(gray, fmt, seed):
    """a frame of format fmt that carries the gray frame's texture"""
    if fmt == CR.MONO8:
        return np.ascontiguousarray(gray)
    return CR.colourise(gray, fmt, seed) if fmt in CR.CHANNELS else R.encode(gray, fmt, seed)


def shape_of(fmt, h, w):
    return (h, w) if BPP[fmt] == 1 else (h, w, BPP[fmt])


def placed(frame, off, pad, seed):
    """the frame's rows `pad` random bytes apart in a host buffer, row 0 at an address that is `off` modulo 16: a u8 view of the frame's own shape"""
    a = np.ascontiguousarray(frame)
    h, row = a.shape[0], int(np.prod(a.shape[1:]))
    pitch = row + pad
    buf = np.random.default_rng(seed).integers(0, 256, h * pitch + 48, dtype=np.uint8)
    start = (-buf.ctypes.data) % 16 + off
    rows = np.lib.stride_tricks.as_strided(buf[start:], (h, row), (pitch, 1))
    rows[:] = a.reshape(h, row)
    return np.lib.stride_tricks.as_strided(buf[start:], a.shape, (pitch,) + a.strides[1:])


# ---------------------------------------------------------------------------------------------------------------- 1. the building block
WIDTHS = [3, 5, 8, 12, 16, 20, 33, 48, 65]
HEIGHTS = [3, 4, 15, 16, 17, 33]


def _batch(rng, w, h, formats, case):
    """frames of the listed formats with offsets 0 .. 3 (0: 16-aligned) and tight / dword / odd paddings taking turns: (placed frames, expected [n, h, w])"""
    frames, want = [], []
    for i, f in enumerate(formats):
        a = rng.integers(0, 256, shape_of(f, h, w)).astype(np.uint8)
        frames.append(placed(a, (i + case) % 4, (0, 4, 5, 8, 1)[(i + case // 4) % 5], 1000 * case + i))
        want.append(to_gray(a, f))
    return frames, np.stack(want)


def test_mixed_host_form_every_shape(gf):
    """gf_cvt_gray_mixed: batches of 12 to 24 with every format at least once in shuffled order, at every width and height of the host walker, sources at offsets
    0 .. 3 with tight, dword and odd pitches; a batch of one format only; a batch of 1.  The sources come back unchanged."""
    rng = np.random.default_rng(77)
    case = 0
    for w in WIDTHS:
        for h in HEIGHTS:
            n = 12 + case % 13
            formats = list(rng.permutation(FORMATS + [FORMATS[int(i)] for i in rng.integers(0, 12, n - 12)]))
            frames, want = _batch(rng, w, h, [int(f) for f in formats], case)
            keep = [f.copy() for f in frames]
            got = gf.cvt_gray_mixed(frames, formats)
            bad = [(i, int(formats[i])) for i in range(n) if not np.array_equal(got[i], want[i])]
            assert not bad, ("frames (index, format) differ", w, h, bad)
            assert all(np.array_equal(a, b) for a, b in zip(frames, keep)), "a source was modified"
            case += 1
    for f in (CR.BGR8, R.BAYER_GBRG8, R.MONO16):       # one format only: the launch of the other part has nothing to do
        frames, want = _batch(rng, 48, 17, [f] * 12, case)
        assert np.array_equal(gf.cvt_gray_mixed(frames, [f] * 12), want), f
        case += 1
    for f in FORMATS:                                   # a batch of 1
        frames, want = _batch(rng, 20, 16, [f], case)
        assert np.array_equal(gf.cvt_gray_mixed(frames, [f]), want), f
        case += 1


def test_mixed_device_form_alignments_guards_and_skipped_entries(gf):
    """gf_cvt_gray_mixed_device: one call whose entries' pointers are 16-aligned, 4-aligned and odd, every format, an entry that is no format (skipped: its slot
    keeps its fill); the bytes around d_dst and every source come back unchanged"""
    import torch
    rng = np.random.default_rng(5)
    for w, h, doff in ((48, 17, 0), (20, 16, 0), (33, 15, 0), (64, 33, 0), (48, 16, 1)):
        formats = [int(f) for f in rng.permutation(FORMATS)] + [7, R.BAYER_BGGR8, -1, CR.RGBA8, R.YUV422_UYVY]
        n = len(formats)
        parts, at, refs, want = [], 0, np.zeros((n, 2), np.uint64), np.full((n, h, w), 0x5A, np.uint8)
        for i, f in enumerate(formats):
            bpp = BPP.get(f, 1)
            off, pad = (0, 4, 1, 3, 16, 2)[i % 6], (0, 16, 3, 4, 0, 7)[(i // 2) % 6]
            a = rng.integers(0, 256, (h, w * bpp)).astype(np.uint8)
            pitch = w * bpp + pad
            rows = rng.integers(0, 256, (h, pitch)).astype(np.uint8)
            rows[:, :w * bpp] = a
            flat = rows.reshape(-1)[:(h - 1) * pitch + w * bpp]
            start = ((at + 15) & ~15) + off
            parts.append((start, flat))
            refs[i] = (start, pitch)
            at = start + flat.size
            if f in BPP:
                want[i] = to_gray(a.reshape(shape_of(f, h, w)), f)
        host = rng.integers(0, 256, at + 16).astype(np.uint8)
        for start, flat in parts:
            host[start:start + flat.size] = flat
        src = torch.from_numpy(host).cuda()
        refs[:, 0] += np.uint64(src.data_ptr())
        d_refs = torch.from_numpy(refs.view(np.int64)).cuda()
        d_fmt = torch.from_numpy(np.array(formats, np.int32)).cuda()
        guard = 256 + doff
        dst = torch.full((guard + n * h * w + 256,), 0x5A, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        gf.cvt_gray_mixed_device(d_refs.data_ptr(), d_fmt.data_ptr(), dst.data_ptr() + guard, n, w, h)
        torch.cuda.synchronize()
        out = dst.cpu().numpy()
        got = out[guard:guard + n * h * w].reshape(n, h, w)
        bad = [(i, formats[i]) for i in range(n) if not np.array_equal(got[i], want[i])]
        assert not bad, ("entries (index, format) differ", w, h, doff, bad)
        assert np.all(out[:guard] == 0x5A) and np.all(out[guard + n * h * w:] == 0x5A), "a byte around d_dst was written"
        assert np.array_equal(src.cpu().numpy(), host), "a source was modified"


def test_mixed_refusals(gf):
    lib = gf.lib()
    w, h = 16, 8
    out = np.full((3, h, w), 0x5A, np.uint8)
    frames = [np.zeros((h, w, 3), np.uint8), np.zeros((h, w), np.uint8), np.zeros((h, w, 2), np.uint8)]

    def call(formats, pitches, srcs=None, ww=w, hh=h, dst=None):
        n = len(formats)
        srcs = (srcs or [f.ctypes.data for f in frames])[:n]
        return lib.gf_cvt_gray_mixed((C.c_void_p * n)(*srcs), (C.c_size_t * n)(*pitches), (C.c_int * n)(*formats), C.c_void_p(dst or out.ctypes.data), n, ww, hh)

    ok = [CR.RGB8, R.BAYER_RGGB8, R.MONO16], [3 * w, w, 2 * w]
    for bad in (5, 6, 7, 15, 99, -1):
        assert call([ok[0][0], ok[0][1], bad], ok[1]) == -1 and b"frame 2" in lib.gf_last_error() and b"pixel format" in lib.gf_last_error(), lib.gf_last_error()
    assert call(ok[0], [3 * w, w - 1, 2 * w]) == -1 and b"frame 1" in lib.gf_last_error() and b"pitch" in lib.gf_last_error()
    assert call(ok[0], [3 * w - 1, w, 2 * w]) == -1 and b"frame 0" in lib.gf_last_error() and b"pitch" in lib.gf_last_error()
    assert call([CR.MONO8, R.BAYER_GRBG8, CR.MONO8], [w, w, w], ww=2, hh=h) == -1 and b"frame 1" in lib.gf_last_error() and b"3" in lib.gf_last_error()
    assert call([CR.MONO8, R.BAYER_GRBG8, CR.MONO8], [w, w, w], ww=w, hh=2) == -1 and b"frame 1" in lib.gf_last_error()
    assert call(ok[0], ok[1], srcs=[frames[0].ctypes.data, out.ctypes.data + 5, frames[2].ctypes.data]) == -1 and b"frame 1" in lib.gf_last_error() and b"overlap" in lib.gf_last_error()
    assert call(ok[0], ok[1], srcs=[frames[0].ctypes.data, frames[1].ctypes.data, None]) == -1 and b"frame 2" in lib.gf_last_error()
    assert call(ok[0][:0], ok[1][:0]) == -1 and call(ok[0], ok[1], ww=0) == -1
    assert lib.gf_cvt_gray_mixed(None, None, None, None, 1, w, h) == -1 and lib.gf_cvt_gray_mixed_device(None, None, None, 1, w, h, None) == -1
    assert np.all(out == 0x5A), "a refused call wrote"
    assert call(ok[0], ok[1]) == 0 and not out.any()


# ---------------------------------------------------------------------------------------------------------------- 2. a mixed handle equals homogeneous handles
SIX = [(CR.MONO8, 0), (CR.BGR8, 1), (R.BAYER_GRBG8, 0), (R.YUV422_YUY2, 1), (R.MONO16, 0), (CR.MONO8, 1)]
LISTS = [[5, 2, 0, 1, 4, 3], [1, 4], [0, 2, 3, 5], [5, 4, 3, 2, 1, 0], [1, 2, 4], [0, 1, 2, 3, 4, 5]]     # lists that skip and reorder; the last advances every sequence
# where the refs entry puts sequence b: (byte offset of row 0 in its allocation, padding, byte column inside a wider surface)
REFS_PLACE = [(0, 0, 0), (4, 12, 0), (1, 5, 0), (0, 0, 40), (16, 16, 0), (3, 2, 8)]


def _streams(settings, K, W, H):
    """frames [k][b] of sequence b in its format, and depth images: rendered and encoded once"""
    key = (tuple(settings), K, W, H)
    if key not in _cache:
        seqs = [synth.tracker_sequence(1000 + 31 * b, K, w=W, h=H) for b in range(len(settings))]
        raw = [[encode(seqs[b][k], settings[b][0], 97 * k + b) for b in range(len(settings))] for k in range(K)]
        for fr in raw:
            for a in fr:
                a.setflags(write=False)
        _cache[key] = (raw, [np.full((H, W), 1000 + 37 * k, np.uint16) for k in range(K)])
    return _cache[key]


def _same(ra, rb, what):
    assert np.array_equal(ra[0], rb[0]), ("feature ids differ",) + what
    assert np.array_equal(ra[1].view(np.uint64), rb[1].view(np.uint64)), ("observations differ",) + what


def _same_state(a, b, what):
    assert all(np.array_equal(x, y) for x, y in zip(a, b)), ("state differs",) + what


def _device_block(frames):
    import torch
    t = torch.from_numpy(np.concatenate([np.ascontiguousarray(f).reshape(-1) for f in frames])).cuda()
    return t, t.clone()


def _mixed_equals_homogeneous(gf, settings, entry, W, H, K, own=(0, 0), min_dist=10, setup=None):
    """the mixed handle (created with `own`, every sequence whose setting differs set) against one batch-1 handle per sequence created with its setting"""
    import torch
    B = len(settings)
    raw, depth = _streams(settings, K, W, H)
    gm = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=B, min_dist=min_dist, pixel_format=own[0], equalize=own[1]))
    refs = [gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=1, min_dist=min_dist, pixel_format=f, equalize=e)) for f, e in settings]
    rows = [W * BPP[f] for f, _ in settings]
    for b, (f, e) in enumerate(settings):
        hs = rows[b] + 5 if entry == "host" and b in (1, 4) else rows[b] if entry == "staged" else 0
        if (f, e) != own or hs:
            gm.set_seq_format(b, f, e, host_stride=hs)
        assert gm.get_seq_format(b) == {"pixel_format": f, "equalize": e, "host_stride": hs}
    if setup:
        setup(gm, refs)
    every = list(range(B))
    if entry == "staged":
        pinned = [[torch.from_numpy(np.array(a)).pin_memory() for a in fr] for fr in raw]
        dpin = [torch.from_numpy(np.array(d).view(np.int16)).pin_memory() for d in depth]
        gm.prefetchHost([t.data_ptr() for t in pinned[0]], [dpin[0].data_ptr()] * B, stride=W)
    last = {}
    for k in range(K):
        seqs = LISTS[k % len(LISTS)] if entry.startswith("some") and B == 6 else every
        ts, dep, fr = [DT * k] * len(seqs), [depth[k]] * len(seqs), [raw[k][s] for s in seqs]
        if entry == "host":         # 5 bytes of random row padding: through host_stride on sequences 1 and 4, through the call's stride on the rest
            stride = 2 * W + 5
            views = [placed(a, 0, (rows[s] + 5 if s in (1, 4) else stride) - rows[s], k + s) for s, a in zip(seqs, fr)]
            rm = gm.trackImageBatch(ts, views, dep, stride=stride)
        elif entry == "some":
            rm = gm.trackImageSome(seqs, ts, fr, dep)
        elif entry == "staged":
            if k + 1 < K:
                gm.prefetchHost([t.data_ptr() for t in pinned[k + 1]], [dpin[k + 1].data_ptr()] * B, stride=W)
            rm = gm.trackPrefetched(ts)
        elif entry in ("device", "some_device"):
            block, before = _device_block(fr)
            offs, total = gm.device_frame_offsets(seqs)
            assert total == block.numel() and offs == [int(o) for o in np.cumsum([0] + [a.size for a in fr])[:-1]]
            dd = torch.from_numpy(np.stack(dep).view(np.int16)).cuda()
            torch.cuda.synchronize()
            rm = gm.trackImageBatchDevice(ts, block.data_ptr(), dd.data_ptr()) if entry == "device" else gm.trackImageSomeDevice(seqs, ts, block.data_ptr(), dd.data_ptr())
            torch.cuda.synchronize()
            assert torch.equal(block, before), "frame %d: the caller's device frames were modified" % k
        else:                       # refs: one entry aligned 16, one 4, odd ones, two crops of wider surfaces
            surf = []
            for s, a in zip(seqs, fr):
                off, pad, x0 = REFS_PLACE[s % 6]
                h, row = a.shape[0], a.size // a.shape[0]
                pitch = x0 + row + pad
                host = np.random.default_rng(k * 10 + s).integers(0, 256, off + h * pitch + 16, dtype=np.uint8)
                np.lib.stride_tricks.as_strided(host[off + x0:], (h, row), (pitch, 1))[:] = a.reshape(h, row)
                t = torch.from_numpy(host).cuda()
                surf.append((t, t.clone(), (t.data_ptr() + off + x0, pitch)))
            dd = torch.from_numpy(np.stack(dep).view(np.int16)).cuda()
            torch.cuda.synchronize()
            rm = gm.trackImageSomeDeviceRefs(seqs, ts, [r for _, _, r in surf], [(dd.data_ptr() + i * 2 * W * H, 2 * W) for i in range(len(seqs))])
            torch.cuda.synchronize()
            assert all(torch.equal(t, b) for t, b, _ in surf), "frame %d: a caller's surface was modified" % k
        for i, s in enumerate(seqs):
            rr = refs[s].trackImage(DT * k, raw[k][s], depth[k])
            _same(rm[i], rr, (entry, k, s))
            last[s] = len(rr[0])
        for s in every:
            _same_state(gm.state(s), refs[s].state(0), (entry, k, s))
    assert sorted(last) == every and min(last.values()) >= FLOOR, ("a sequence ends with too few features to show anything", last)
    return gm, refs


@pytest.mark.parametrize("entry", ["host", "some", "staged", "device", "some_device", "refs"])
def test_mixed_handle_equals_homogeneous_handles(gf, entry):
    """160 x 120, min_dist 10, 6 frames: one handle of batch 6 created MONO8 without equalisation, its sequences set to SIX, against six handles of batch 1"""
    gm, refs = _mixed_equals_homogeneous(gf, SIX, entry, 160, 120, 6)
    st = gm.stats()
    assert st["sequence_frames"] == (sum(len(l) for l in LISTS) if entry.startswith("some") else 36) and st["frames"] == 6
    for g in [gm] + refs:
        g.close()


@pytest.mark.parametrize("entry", ["device", "refs"])
def test_mixed_handle_with_plain_copies(gf, entry, monkeypatch):
    """GF_TRACKER_COPIES=1 (read when the handle is created): the plan's table goes down by a copy instead of being read over the bus"""
    monkeypatch.setenv("GF_TRACKER_COPIES", "1")
    gm, refs = _mixed_equals_homogeneous(gf, SIX, entry, 160, 120, 6)
    for g in [gm] + refs:
        g.close()


def test_defaults_come_from_the_cfg(gf):
    """the handle created with pixel_format = RGBA8, equalize = 1 and two sequences set back to (MONO8, 0)"""
    settings = [(CR.RGBA8, 1), (CR.MONO8, 0), (CR.RGBA8, 1), (CR.MONO8, 0)]
    gm, refs = _mixed_equals_homogeneous(gf, settings, "device", 160, 120, 6, own=(CR.RGBA8, 1))
    for g in [gm] + refs:
        g.close()


def test_mixed_handle_vga(gf):
    """640 x 480, batch 4, 3 frames, four formats, the tight device entry"""
    settings = [(CR.RGB8, 0), (R.BAYER_RGGB8, 1), (R.YUV422_UYVY, 0), (CR.MONO8, 1)]
    gm, refs = _mixed_equals_homogeneous(gf, settings, "device", 640, 480, 3, min_dist=30)
    for g in [gm] + refs:
        g.close()


# ---------------------------------------------------------------------------------------------------------------- 3. the setting's life
COUNTERS = ("frames", "sequence_frames", "lk_launches", "lk_points", "lk_level_passes", "lk_iterations", "tracked_features", "output_features", "pyr_head",
            "pyr_level0_vec16", "pyr_level0_dword", "pyr_down_tail", "pyr_down_pad4", "pyr_down_bytes", "frames_unaligned")


def test_the_life_of_a_setting(gf):
    import torch
    lib = gf.lib()
    W, H, B = 160, 120, 3
    settings = [(CR.BGR8, 1), (R.BAYER_GRBG8, 0), (CR.BGR8, 1)]
    raw, depth = _streams(settings, 4, W, H)
    own = {"pixel_format": CR.BGR8, "equalize": 1, "host_stride": 0}
    pair = [gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=B, min_dist=10, pixel_format=CR.BGR8, equalize=1)) for _ in range(2)]
    g, twin = pair           # `twin` never sees a refused call
    assert all(g.get_seq_format(b) == own for b in range(B))
    g.set_seq_format(2)                                         # NULL on a handle that never set: nothing to take back
    g.set_seq_format(1, R.MONO16, 0, host_stride=2 * W + 6)
    assert g.get_seq_format(1) == {"pixel_format": R.MONO16, "equalize": 0, "host_stride": 2 * W + 6}
    g.set_seq_format(1)
    assert g.get_seq_format(1) == own
    for t in pair:
        t.set_seq_format(1, R.BAYER_GRBG8, 0)
    want = g.get_seq_format(1)

    def refused(seq, f, field, handle=g.h):
        rc = lib.gf_tracker_set_seq_format(handle, seq, None if f is None else C.byref(gf.TrackerSeqFormat(*f)))
        assert rc == -1 and field in lib.gf_last_error(), (seq, f, rc, lib.gf_last_error())
        assert [g.get_seq_format(b) for b in range(B)] == [own, want, own]

    refused(0, (0, 0, 0), b"null handle", handle=None)
    refused(-1, (0, 0, 0), b"sequence")
    refused(B, None, b"sequence")
    for bad in (5, 6, 7, 15, 99, -1, 1 << 20):
        refused(1, (bad, 0, 0), b"pixel_format")
    for bad in (2, -1, 255):
        refused(1, (R.MONO16, bad, 0), b"equalize")
    refused(1, (R.MONO16, 0, -1), b"host_stride")
    refused(1, (R.MONO16, 0, 2 * W - 1), b"host_stride")
    refused(0, (CR.RGBA8, 1, 4 * W - 1), b"host_stride")
    assert lib.gf_tracker_get_seq_format(g.h, B, C.byref(gf.TrackerSeqFormat())) == -1 and lib.gf_tracker_get_seq_format(None, 0, C.byref(gf.TrackerSeqFormat())) == -1
    # a short effective stride or pitch names the list position, on each entry point, and changes nothing
    g.trackImageBatch([0.0] * B, raw[0], [depth[0]] * B)
    twin.trackImageBatch([0.0] * B, raw[0], [depth[0]] * B)
    state = [g.state(b) for b in range(B)]
    ptrs = (C.POINTER(C.c_uint8) * B)(*[gf._p(a, C.c_uint8) for a in raw[1]])
    seq, ts = np.arange(B, dtype=np.int32), np.full(B, DT)
    out, n = np.zeros((B, g.cap), gf.OBS_DTYPE), np.full(B, -3, np.int32)
    po, pn, ps, pt = out.ctypes.data_as(C.POINTER(gf.FeatureObs)), gf._p(n, C.c_int), gf._p(seq, C.c_int), gf._p(ts, C.c_double)
    short = 3 * W - 1                                           # a row of sequence 1 (Bayer) fits, a row of sequences 0 and 2 (BGR8) does not
    assert lib.gf_tracker_track_some(g.h, B, ps, pt, ptrs, short, None, 0, po, g.cap, pn) == -1 and b"list position 0" in lib.gf_last_error()
    assert lib.gf_tracker_track_batch(g.h, pt, ptrs, short, None, 0, po, g.cap, pn) == -1 and b"list position 0" in lib.gf_last_error()
    back = np.array([1, 2, 0], np.int32)
    assert lib.gf_tracker_track_some(g.h, B, gf._p(back, C.c_int), pt, ptrs, short, None, 0, po, g.cap, pn) == -1 and b"list position 1 (sequence 2)" in lib.gf_last_error()
    assert lib.gf_tracker_prefetch_some(g.h, B, gf._p(back, C.c_int), ptrs, W - 1, None, 0) == -1 and b"list position 0 (sequence 1)" in lib.gf_last_error()
    assert lib.gf_tracker_prefetch_batch(g.h, ptrs, short, None, 0) == -1 and b"list position 0" in lib.gf_last_error()
    assert lib.gf_tracker_track(g.h, 2, C.c_double(DT), ptrs[2], short, None, 0, po, g.cap, pn) == -1 and b"list position 0 (sequence 2)" in lib.gf_last_error()
    dev = torch.zeros(3 * W * H * 3, dtype=torch.uint8, device="cuda")
    table = gf.frame_refs([(dev.data_ptr(), 3 * W), (dev.data_ptr(), W - 1), (dev.data_ptr(), 3 * W)])
    assert lib.gf_tracker_track_some_device_refs(g.h, B, ps, pt, table, None, po, g.cap, pn) == -1 and b"list position 1" in lib.gf_last_error() and b"pitch" in lib.gf_last_error()
    table = gf.frame_refs([(dev.data_ptr(), 3 * W), (dev.data_ptr(), W), (dev.data_ptr(), 3 * W - 1)])
    assert lib.gf_tracker_track_batch_device_refs(g.h, pt, table, None, po, g.cap, pn) == -1 and b"list position 2" in lib.gf_last_error()
    assert np.all(n == -3) and not out["id"].any()
    for b in range(B):
        _same_state(g.state(b), state[b], ("after refused calls", b))
    # a sequence that has taken a frame refuses the setter until reset_seq, which keeps the setting
    with pytest.raises(gf.GfError, match="taken a frame"):
        g.set_seq_format(1, R.MONO16, 0)
    with pytest.raises(gf.GfError, match="taken a frame"):
        g.set_seq_format(1)
    # ... and after all that the handle does what its twin does
    ra, rb = g.trackImageBatch([DT] * B, raw[1], [depth[1]] * B), twin.trackImageBatch([DT] * B, raw[1], [depth[1]] * B)
    sa, sb = g.stats(), twin.stats()
    for b in range(B):
        _same(ra[b], rb[b], ("twin", b))
        _same_state(g.state(b), twin.state(b), ("twin", b))
        assert len(ra[b][0]) >= FLOOR
    assert all(sa[k] == sb[k] for k in COUNTERS), [(k, sa[k], sb[k]) for k in COUNTERS if sa[k] != sb[k]]
    # a staged frame refuses the setter (for every sequence: the staging buffers may have to grow), until it is consumed
    pinned = [torch.from_numpy(np.array(a)).pin_memory() for a in raw[2]]
    g.prefetchHost([pinned[0].data_ptr()], None, stride=3 * W, seqs=[0])
    g.reset_seq(2)
    with pytest.raises(gf.GfError, match="staged"):
        g.set_seq_format(2, CR.RGBA8, 0)
    g.trackPrefetched([2 * DT])
    assert g.get_seq_format(2) == own
    g.set_seq_format(2, CR.RGBA8, 0)                            # allowed after the reset, and the staging pair grew to four bytes per pixel
    g.reset_seq(1)
    assert g.get_seq_format(1) == want and g.state(1)[0].size == 0
    g.set_seq_format(1, R.MONO16, 1)
    frames = [raw[3][0], encode(to_gray(raw[3][1], R.BAYER_GRBG8), R.MONO16, 3), encode(CR.to_gray(raw[3][2], CR.BGR8), CR.RGBA8, 4)]
    res = g.trackImageBatch([3 * DT] * B, frames, [depth[3]] * B)
    fresh = [gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=1, min_dist=10, pixel_format=f, equalize=e)) for f, e in ((R.MONO16, 1), (CR.RGBA8, 0))]
    for b, t in ((1, fresh[0]), (2, fresh[1])):
        _same(res[b], t.trackImage(3 * DT, frames[b], depth[3]), ("after reset", b))
        assert len(res[b][0]) >= FLOOR
    for t in pair + fresh:
        t.close()


# ---------------------------------------------------------------------------------------------------------------- 4. neighbours and other settings
def test_neighbours_and_other_settings(gf):
    """per-sequence max_cnt / min_dist, a region of interest on one sequence, boxes on another, show_track on a third: each sequence equals its homogeneous
    handle with the same settings, and the track image of the equalised Bayer sequence equals the homogeneous handle's byte for byte"""
    W, H = 160, 120
    settings = [(CR.BGR8, 1), (R.BAYER_GRBG8, 1), (CR.MONO8, 0), (R.YUV422_UYVY, 0)]
    roi = np.zeros((H, W), np.uint8)
    roi[10:100, 20:150] = 255
    boxes = [(30, 20, 90, 70), (100, 60, 150, 110)]

    def setup(gm, refs):
        for g, q in ((gm, 0), (refs[0], 0)):
            g.set_seq_cfg(q, max_cnt=60, min_dist=14)
            g.set_roi(roi, q)
        for g, q in ((gm, 1), (refs[1], 0)):
            g.set_show_track(True, [q])
            g.set_seq_cfg(q, min_dist=12)
        for g, q in ((gm, 2), (refs[2], 0)):
            g.set_boxes(boxes, q)
        for g, q in ((gm, 3), (refs[3], 0)):
            g.set_seq_cfg(q, max_cnt=40, flow_back=0)

    gm, refs = _mixed_equals_homogeneous(gf, settings, "some", W, H, 6, setup=setup)
    assert np.array_equal(gm.track_image(1), refs[1].track_image(0)), "the track image of the equalised Bayer sequence differs"
    assert len(gm.state(0)[0]) <= 60 and len(gm.state(3)[0]) <= 40
    for g in [gm] + refs:
        g.close()


# ---------------------------------------------------------------------------------------------------------------- 5. nothing is copied or timed that need not be
def test_stats_follow_the_listed_sequences(gf):
    import torch
    W, H, B = 160, 120, 4
    settings = [(CR.MONO8, 0), (CR.MONO8, 0), (R.YUV422_YUY2, 0), (CR.MONO8, 1)]
    raw, depth = _streams(settings, 4, W, H)
    g = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=B, min_dist=10))
    plain = gf.FeatureTracker(gf.default_cfg(width=W, height=H, batch=B, min_dist=10))      # the setter is never called on this one
    g.set_seq_format(2, R.YUV422_YUY2, 0)
    g.set_seq_format(3, CR.MONO8, 1)
    for t in (g, plain):
        t.set_profiling(True)

    def call(t, seqs, k):
        block, before = _device_block([raw[k][s] for s in seqs])
        torch.cuda.synchronize()
        res = t.trackImageSomeDevice(seqs, [DT * k] * len(seqs), block.data_ptr())
        torch.cuda.synchronize()
        assert torch.equal(block, before), "the caller's device frames were modified"
        return res

    for k in range(3):
        a, b = call(g, [1, 0], k), call(plain, [1, 0], k)       # only (MONO8, 0) sequences: the call of a handle without settings
        for i in range(2):
            _same(a[i], b[i], ("plain", k, i))
    sa, sb = g.stats(), plain.stats()
    assert sa["ms_convert"] == 0.0 and sa["ms_equalize"] == 0.0 and sa["ms_pyramid"] > 0
    assert all(sa[k] == sb[k] for k in COUNTERS), [(k, sa[k], sb[k]) for k in COUNTERS if sa[k] != sb[k]]
    call(g, [2], 0)
    s1 = g.stats()
    assert s1["ms_convert"] > 0 and s1["ms_equalize"] == 0.0
    call(g, [3], 0)
    s2 = g.stats()
    assert s2["ms_equalize"] > 0 and s2["ms_convert"] == s1["ms_convert"]
    call(g, [0, 1], 3)                                          # again only (MONO8, 0) sequences, on a handle that has converted and equalised by now
    s3 = g.stats()
    assert s3["ms_convert"] == s2["ms_convert"] and s3["ms_equalize"] == s2["ms_equalize"] and s3["ms_pyramid"] > s2["ms_pyramid"]
    g.close(); plain.close()
