"""The whole tracker against the oracle at frame sizes other than 640 x 480 and on frames whose rows are padded (a row pitch that is not the width).

Which pyramid kernels build a frame follows from its size: the alignment of every level's width, the parity of the height and two 64 KB LDS limits
(launch_pyramid).  Every size below is held to the oracle bit for bit -- ids, observations and state on every frame, as at VGA -- and asserts through the
handle's launch counters (gf_tracker_stats.pyr_*) which pyramid route it took, so that a change to the dispatch conditions fails a named case instead of
silently moving a size onto an untested route.  Run with -m gpu."""
import ctypes as C

import numpy as np
import pytest

import clahe_ref as R
import synth

pytestmark = pytest.mark.gpu

KPAD, KWIN, KMAX_LEVELS, KHEAD_ROWS = 32, 21, 4, 16   # gf_lk_kernels.hpp
SORT_LDS, TOPK_MAX = 16384, 16   # gf_detect_kernels.hpp: kSortLds, kTopKMax
ROUTE = ("pyr_head", "pyr_level0_vec16", "pyr_level0_dword", "pyr_down_tail", "pyr_down_pad4", "pyr_down_bytes")


def levels(w, h):
    """build_geom: (w, h, stride, img_off) per pyramid level, and the bytes of one pyramid"""
    lv, off, lw, lh = [], 0, w, h
    for _ in range(KMAX_LEVELS):
        stride = lw + 2 * KPAD
        lv.append((lw, lh, stride, off + KPAD * stride + KPAD))
        off = (off + (lh + 2 * KPAD) * stride + 255) & ~255
        lw, lh = (lw + 1) // 2, (lh + 1) // 2
        if lw <= KWIN or lh <= KWIN:
            break
    return lv, off


def route(w, h, head_enabled=True):
    """launch_pyramid's choice for one frame (device buffers 16-byte aligned): launches of each form"""
    lv, img_bytes = levels(w, h)
    n, (w0, h0, s0, _) = len(lv), lv[0]
    v16 = ((w0 | s0 | ((w0 * h0) & 15) | ((2 * img_bytes) & 15)) & 15) == 0
    vec = all(l[0] % 4 == 0 and l[3] % 4 == 0 for l in lv) and all(l[0] > KPAD + 1 and l[1] > KPAD + 1 for l in lv[1:])
    head_lds = (2 * KHEAD_ROWS + 3) * (w0 + 8) + KHEAD_ROWS * (w0 // 2)
    head = (head_enabled and v16 and vec and n >= 2 and h0 % 2 == 0 and lv[1][1] * 2 == h0 and lv[1][0] * 2 == w0 and h0 > KPAD + 2 and w0 > KPAD + 2
            and head_lds <= 64 * 1024)
    r = dict.fromkeys(ROUTE, 0)
    r["pyr_head" if head else "pyr_level0_vec16" if v16 else "pyr_level0_dword"] = 1
    if vec:
        r["pyr_down_pad4"] += n > 1 and not head
        if n > 2:
            last = min(n - 1, 3)
            d, e = lv[2], lv[last]
            band = (e[1] + 3) // 4 + 1 if last > 2 else ((d[1] + 1) // 2 + 3) // 4 + 1
            lds = (2 * band + 4) * d[0] + (band * e[0] if last > 2 else 0)
            if n <= 4 and lds <= 64 * 1024:
                r["pyr_down_tail"] = 1
            else:
                r["pyr_down_pad4"] += n - 2
    else:
        r["pyr_down_bytes"] = n - 1
    return r


def _r(**kw):
    r = dict.fromkeys(ROUTE, 0)
    r.update(kw)
    return r


HEAD_TAIL = _r(pyr_head=1, pyr_down_tail=1)
# (w, h, levels, route per frame, max_cnt, min_dist, frames, tracked floor per frame after the first)
SIZES = [
    (640, 480, 4, HEAD_TAIL, 150, 30, 6, 120),
    (1280, 720, 4, HEAD_TAIL, 500, 20, 5, 450),
    (640, 160, 3, HEAD_TAIL, 150, 15, 6, 120),                                        # the tail's 3-level band formula (last == 2)
    (640, 481, 4, _r(pyr_level0_vec16=1, pyr_down_pad4=1, pyr_down_tail=1), 150, 30, 6, 120),   # odd heights 481 / 241 / 121 / 61
    (1920, 1080, 4, _r(pyr_level0_vec16=1, pyr_down_pad4=1, pyr_down_tail=1), 500, 20, 3, 450),  # the head's LDS would be 82 KB
    (2560, 1440, 4, _r(pyr_level0_vec16=1, pyr_down_pad4=3), 500, 20, 3, 450),        # the tail's LDS would be 76 KB
    (752, 480, 4, _r(pyr_level0_vec16=1, pyr_down_bytes=3), 150, 30, 6, 120),         # level 3: w 94, stride 158 (2 mod 4)
    (320, 240, 4, _r(pyr_level0_vec16=1, pyr_down_bytes=3), 100, 10, 6, 80),          # level 3 (40 x 30) within one reflection
    (644, 481, 4, _r(pyr_level0_dword=1, pyr_down_bytes=3), 150, 30, 6, 120),         # strides 2 mod 4 at levels 1-3, w * h = 4 mod 16
    (64, 48, 2, _r(pyr_level0_vec16=1, pyr_down_bytes=1), 30, 3, 6, 15),              # LK asks for level 3 of a 2-level pyramid
    (40, 36, 1, _r(pyr_level0_dword=1), 15, 2, 6, 6),                                 # a single level
]


def _id(c):
    return "%dx%d" % (c[0], c[1])


def _frames(w, h, n, seed=0):
    return synth.tracker_sequence(2000 + w + h + seed, n, w, h)


def _depth(k, w, h):
    """a different value at every pixel: a sample taken from the wrong pixel or the wrong row shows"""
    return np.random.default_rng(500 + k).integers(300, 9000, (h, w)).astype(np.uint16)


def _same(o, g, what):
    (oi, oo), (gi, go) = o, g
    assert np.array_equal(oi, gi), "%s: feature id lists differ" % what
    assert np.array_equal(oo.view(np.uint64), go.view(np.uint64)), "%s: observations differ" % what


def _same_state(otr, gtr, seq, what):
    assert all(np.array_equal(a, b) for a, b in zip(otr.state(), gtr.state(seq))), "%s: state differs" % what


def _routes(st):
    return {k: st[k] for k in ROUTE}


def _times(r, n):
    return {k: v * n for k, v in r.items()}


def _sort_cap(w, h, max_cnt, min_dist):
    """gf_tracker_create: the keys select_corners_kernel sorts in LDS"""
    cell = max(min_dist, 1)
    grid_lds = (((w + cell - 1) // cell) * ((h + cell - 1) // cell) + 3 & ~3) * 2 + ((max_cnt + 3) & ~3) * 6 + 64
    cap = SORT_LDS
    while cap > 64 and cap * 8 + grid_lds > 160 * 1024:
        cap >>= 1
    return cap


def test_the_route_table_is_what_launch_pyramid_computes():
    """the routes written in SIZES against the dispatch rules restated above (so that each row says what it covers)"""
    for w, h, nlev, r, *_ in SIZES:
        assert len(levels(w, h)[0]) == nlev, (w, h)
        assert route(w, h) == r, (w, h)
        assert route(w, h, head_enabled=False)["pyr_head"] == 0
    assert levels(752, 480)[0][3][2] % 4 == 2 and levels(644, 481)[0][1][2] % 4 == 2


@pytest.mark.parametrize("case", SIZES, ids=_id)
def test_tracker_sequence_bit_exact_at_frame_size(gf, oracle, case):
    w, h, _, r, max_cnt, min_dist, n, floor = case
    frames = _frames(w, h, n)
    otr = oracle.Tracker(oracle.default_cfg(max_cnt=max_cnt, min_dist=min_dist))
    gtr = gf.FeatureTracker(gf.default_cfg(width=w, height=h, max_cnt=max_cnt, min_dist=min_dist))
    prev, wants = None, []
    for k, f in enumerate(frames):
        d = _depth(k, w, h)
        o = otr.track(0.0666 * k, f, d)
        g = gtr.trackImage(0.0666 * k, f, d)
        _same(o, g, "frame %d" % k)
        _same_state(otr, gtr, 0, "frame %d" % k)
        if prev is not None:
            tracked = len(np.intersect1d(g[0], prev))
            assert tracked >= floor, "frame %d: %d features tracked" % (k, tracked)
            wants.append(max_cnt - tracked)
        assert len(g[0]) == max_cnt, k
        prev = g[0]
    st = gtr.stats()
    assert _routes(st) == _times(r, n), st
    if max_cnt == 500:
        # the first frame wants every corner out of more candidates than the LDS sort area holds; the later ones want a handful out of many thousands
        from test_tracker_gpu import _local_maxima
        assert _local_maxima(frames[0]) > _sort_cap(w, h, max_cnt, min_dist) and all(0 < x <= TOPK_MAX for x in wants), wants
        assert st["select_global_sort"] == 1 and st["select_streamed"] == n - 1, st
    gtr.close()


@pytest.mark.parametrize("size", [(644, 481), (752, 480)], ids=lambda s: "%dx%d" % s)
def test_batch_of_three_sequences_at_frame_size(gf, oracle, size):
    w, h = size
    B, K = 3, 5
    seqs = [_frames(w, h, K, seed=b) for b in range(B)]
    otrs = [oracle.Tracker(oracle.default_cfg()) for _ in range(B)]
    gtr = gf.FeatureTracker(gf.default_cfg(width=w, height=h, batch=B))
    for k in range(K):
        ds = [_depth(10 * b + k, w, h) for b in range(B)]
        res = gtr.trackImageBatch([0.0666 * k] * B, [s[k] for s in seqs], ds)
        for b in range(B):
            _same(otrs[b].track(0.0666 * k, seqs[b][k], ds[b]), res[b], "seq %d frame %d" % (b, k))
            _same_state(otrs[b], gtr, b, "seq %d frame %d" % (b, k))
        assert min(len(x[0]) for x in res) == 150
    assert _routes(gtr.stats()) == _times(route(w, h), K)
    gtr.close()


def test_device_entry_point_at_644x481(gf, oracle):
    """the caller's device frames back to back: the second sequence starts w * h = 4 (mod 16) bytes into the block, so level 0 takes the dword kernel"""
    import torch
    w, h, B, K = 644, 481, 2, 5
    seqs = [_frames(w, h, K, seed=b) for b in range(B)]
    otrs = [oracle.Tracker(oracle.default_cfg()) for _ in range(B)]
    gtr = gf.FeatureTracker(gf.default_cfg(width=w, height=h, batch=B))
    for k in range(K):
        ds = [_depth(20 * b + k, w, h) for b in range(B)]
        dg = torch.from_numpy(np.stack([s[k] for s in seqs])).cuda()
        dd = torch.from_numpy(np.stack(ds).view(np.int16)).cuda()
        torch.cuda.synchronize()
        res = gtr.trackImageBatchDevice([0.0666 * k] * B, dg.data_ptr(), dd.data_ptr())
        for b in range(B):
            _same(otrs[b].track(0.0666 * k, seqs[b][k], ds[b]), res[b], "seq %d frame %d" % (b, k))
    assert _routes(gtr.stats()) == _times(_r(pyr_level0_dword=1, pyr_down_bytes=3), K)
    gtr.close()


def test_prefetched_frames_at_752x480(gf, oracle):
    import torch
    w, h, B, K = 752, 480, 2, 5
    seqs = [_frames(w, h, K, seed=b) for b in range(B)]
    ds = [[_depth(30 * b + k, w, h) for b in range(B)] for k in range(K)]
    otrs = [oracle.Tracker(oracle.default_cfg()) for _ in range(B)]
    gtr = gf.FeatureTracker(gf.default_cfg(width=w, height=h, batch=B))
    host_g = [torch.from_numpy(np.stack([s[k] for s in seqs])).pin_memory() for k in range(K)]
    host_d = [torch.from_numpy(np.stack(ds[k]).view(np.int16)).pin_memory() for k in range(K)]
    gtr.prefetchHost(host_g[0].data_ptr(), host_d[0].data_ptr())
    for k in range(K):
        if k + 1 < K:
            gtr.prefetchHost(host_g[k + 1].data_ptr(), host_d[k + 1].data_ptr())
        res = gtr.trackPrefetched([0.0666 * k] * B)
        for b in range(B):
            _same(otrs[b].track(0.0666 * k, seqs[b][k], ds[k][b]), res[b], "seq %d frame %d" % (b, k))
    assert _routes(gtr.stats()) == _times(route(w, h), K)
    gtr.close()


def test_prediction_and_outlier_feedback_at_752x480(gf, oracle):
    """setPrediction / removeOutliers (the predicted-start LK and the < 10 fallback) at a pyramid whose level 3 rows are 158 bytes apart"""
    w, h = 752, 480
    frames = _frames(w, h, 6, seed=3)
    otr = oracle.Tracker(oracle.default_cfg(depth_cam=0))
    gtr = gf.FeatureTracker(gf.default_cfg(width=w, height=h, depth_cam=0))
    cfg = gtr.cfg
    rng = np.random.default_rng(9)
    for k, f in enumerate(frames):
        o, g = otr.track(0.0666 * k, f, None), gtr.trackImage(0.0666 * k, f, None)
        _same(o, g, "frame %d" % k)
        _same_state(otr, gtr, 0, "frame %d" % k)
        assert len(g[0]) == 150
        rm = o[0][rng.random(len(o[0])) < 0.05]
        otr.remove_outliers(rm); gtr.removeOutliers(rm)
        ids, _, pts = otr.state()
        sel = rng.random(len(ids)) < 0.7
        noise = 200.0 if k == 3 else 1.0     # frame 3: garbage predictions, most fail and the fallback runs
        uv = pts[sel] + rng.normal(0, noise, (sel.sum(), 2))
        xyz = np.stack([(uv[:, 0] - cfg.cx) / cfg.fx * 2.0, (uv[:, 1] - cfg.cy) / cfg.fy * 2.0, np.full(len(uv), 2.0)], 1)
        otr.set_prediction(ids[sel], xyz); gtr.setPrediction(ids[sel], xyz)
    gtr.close()


def _padded(a, pitch, fill):
    """a copy of `a` as the left columns of a wider array filled with `fill`: the rows lie `pitch` elements apart"""
    big = np.full((a.shape[0], pitch), fill, a.dtype)
    big[:, :a.shape[1]] = a
    return big[:, :a.shape[1]]


@pytest.mark.parametrize("size", [(640, 480), (752, 480)], ids=lambda s: "%dx%d" % s)
def test_frames_with_a_row_pitch(gf, oracle, size):
    """gray frames with rows w + 36 bytes apart and depth images with rows w + 20 pixels apart (cropped cv::Mat, cv::Mat::step), the padding 255 / 0xFFFF so that
    any read of it shows: through the host batch, and through the prefetch with every frame in its own page-locked allocation (one 2-D copy per sequence).
    Bit for bit as the oracle fed the contiguous frames."""
    import torch
    w, h = size
    B, K = 2, 5
    gp, dp = w + 36, w + 20
    seqs = [_frames(w, h, K, seed=10 + b) for b in range(B)]
    ds = [[_depth(40 * b + k, w, h) for b in range(B)] for k in range(K)]
    otrs = [oracle.Tracker(oracle.default_cfg()) for _ in range(B)]
    ref = [[otrs[b].track(0.0666 * k, seqs[b][k], ds[k][b]) for k in range(K)] for b in range(B)]
    host = gf.FeatureTracker(gf.default_cfg(width=w, height=h, batch=B))
    pre = gf.FeatureTracker(gf.default_cfg(width=w, height=h, batch=B))
    pin_g, pin_d = [], []
    for k in range(K):
        pg, pd = [], []
        for b in range(B):
            g = torch.full((h, gp), 255, dtype=torch.uint8).pin_memory()
            d = torch.full((h, dp), -1, dtype=torch.int16).pin_memory()
            g[:, :w] = torch.from_numpy(seqs[b][k])
            d[:, :w] = torch.from_numpy(ds[k][b].view(np.int16))
            pg.append(g); pd.append(d)
        pin_g.append(pg); pin_d.append(pd)

    def stage(k):
        pre.prefetchHost([t.data_ptr() for t in pin_g[k]], [t.data_ptr() for t in pin_d[k]], stride=gp, dstride=dp)

    stage(0)
    for k in range(K):
        imgs = [_padded(seqs[b][k], gp, 255) for b in range(B)]
        deps = [_padded(ds[k][b], dp, 0xFFFF) for b in range(B)]
        res = host.trackImageBatch([0.0666 * k] * B, imgs, deps, stride=gp, dstride=dp)
        if k + 1 < K:
            stage(k + 1)
        rp = pre.trackPrefetched([0.0666 * k] * B)
        for b in range(B):
            _same(ref[b][k], res[b], "host batch, seq %d frame %d" % (b, k))
            _same(ref[b][k], rp[b], "prefetched, seq %d frame %d" % (b, k))
        assert min(len(x[0]) for x in res) == 150
    host.close(); pre.close()


@pytest.mark.parametrize("variant", ["GF_LK_POINTS=4", "GF_PYR_HEAD=0", "equalize=1"])
@pytest.mark.parametrize("size", [(752, 480), (644, 481)], ids=lambda s: "%dx%d" % s)
def test_kept_variants_and_clahe_at_frame_size(gf, oracle, monkeypatch, size, variant):
    w, h = size
    K = 5
    key, val = variant.split("=")
    eq = key == "equalize"
    if not eq:
        monkeypatch.setenv(key, val)
    frames = _frames(w, h, K, seed=5)
    otr = oracle.Tracker(oracle.default_cfg(max_cnt=300, min_dist=20))
    gtr = gf.FeatureTracker(gf.default_cfg(width=w, height=h, max_cnt=300, min_dist=20, equalize=int(eq)))
    for k, f in enumerate(frames):
        d = _depth(60 + k, w, h)
        o = otr.track(0.0666 * k, R.clahe(f) if eq else f, d)
        g = gtr.trackImage(0.0666 * k, f, d)
        _same(o, g, "frame %d" % k)
        _same_state(otr, gtr, 0, "frame %d" % k)
        assert len(g[0]) == 300
    assert _routes(gtr.stats()) == _times(route(w, h, head_enabled=key != "GF_PYR_HEAD"), K)
    gtr.close()


@pytest.mark.parametrize("w,h", [(642, 480), (28, 480), (640, 31)])
def test_unsupported_frame_sizes_are_refused(gf, w, h):
    cfg = gf.default_cfg(width=w, height=h)
    handle = C.c_void_p(0x1234)
    assert gf.lib().gf_tracker_create(C.byref(cfg), C.byref(handle)) == -1     # GF_ERR_INVALID
    assert handle.value is None, "a refused configuration left a handle behind"
    assert "unsupported tracker configuration" in gf.lib().gf_last_error().decode()
    with pytest.raises(gf.GfError, match="gf status -1"):
        gf.FeatureTracker(cfg)


def test_batch_of_four_at_2560x1440(gf, oracle):
    """the largest frames of the table at batch 4: the pyramid buffer d_img holds 4 x 2 pyramids of 2560 x 1440"""
    w, h, B, K = 2560, 1440, 4, 2
    seqs = [_frames(w, h, K, seed=b) for b in range(B)]
    otrs = [oracle.Tracker(oracle.default_cfg()) for _ in range(B)]
    gtr = gf.FeatureTracker(gf.default_cfg(width=w, height=h, batch=B))
    for k in range(K):
        ds = [_depth(70 + 10 * b + k, w, h) for b in range(B)]
        res = gtr.trackImageBatch([0.0666 * k] * B, [s[k] for s in seqs], ds)
        for b in range(B):
            _same(otrs[b].track(0.0666 * k, seqs[b][k], ds[b]), res[b], "seq %d frame %d" % (b, k))
            _same_state(otrs[b], gtr, b, "seq %d frame %d" % (b, k))
        assert min(len(x[0]) for x in res) == 150
    assert _routes(gtr.stats()) == _times(route(w, h), K)
    gtr.close()
