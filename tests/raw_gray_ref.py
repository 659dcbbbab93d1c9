"""Restatement in numpy of cv_bridge::toCvCopy(img_msg, MONO8) for the raw encodings of cameras that do not debayer on board: the parity target of
gf_cvt_gray_batch*, of the host decoder and of the tracker's `pixel_format` for GF_PIX_BAYER_*, GF_PIX_YUV422_* and GF_PIX_MONO16.

Bayer (bayer_rggb8 / bggr8 / gbrg8 / grbg8; the four letters are the colours of pixels (0,0), (0,1), (1,0), (1,1), period 2 both ways).  The target is OpenCV
4.2 cvtColor(COLOR_Bayer??2GRAY) on uchar as its generic loop computes it, a bilinear demosaic fused with the luma sum, with k(R) = 4899, k(G) = 9617,
k(B) = 1868.  For an interior pixel C with edge neighbours N, S, W, E and diagonal neighbours NW, NE, SW, SE:

    red or blue site of colour c, opposite colour o:    (4 k(c) C + k(G) (N + S + W + E) + k(o) (NW + NE + SW + SE) + 2^15) >> 16
    green site, hc = colour left and right of it,
                vc = colour above and below it:         (2 k(G) C + k(hc) (W + E) + k(vc) (N + S) + 2^14) >> 15

and a border pixel takes the value of the nearest interior pixel, out(y, x) = f(clamp(y, 1, h - 2), clamp(x, 1, w - 2)).
YUV 4:2:2 (yuv422 = UYVY, yuv422_yuy2 = YUY2): the luma byte of every pixel, byte 2x + 1 / byte 2x of the row.
MONO16: convertTo(CV_8U, 255. / 65535.), which is (v + 128) // 257.

No OpenCV build is available to the tests, so this file is the yardstick; it is written from the definition above with whole-array operations and shares
nothing with the library."""
import numpy as np

BAYER_RGGB8, BAYER_BGGR8, BAYER_GBRG8, BAYER_GRBG8, YUV422_UYVY, YUV422_YUY2, MONO16 = range(8, 15)       # GF_PIX_* of include/groundfusion_hip.h
BAYER = (BAYER_RGGB8, BAYER_BGGR8, BAYER_GBRG8, BAYER_GRBG8)
RAW = BAYER + (YUV422_UYVY, YUV422_YUY2, MONO16)
ENCODING = {BAYER_RGGB8: "bayer_rggb8", BAYER_BGGR8: "bayer_bggr8", BAYER_GBRG8: "bayer_gbrg8", BAYER_GRBG8: "bayer_grbg8", YUV422_UYVY: "yuv422",
            YUV422_YUY2: "yuv422_yuy2", MONO16: "mono16"}                                                   # sensor_msgs/image_encodings.h
BYTES = {BAYER_RGGB8: 1, BAYER_BGGR8: 1, BAYER_GBRG8: 1, BAYER_GRBG8: 1, YUV422_UYVY: 2, YUV422_YUY2: 2, MONO16: 2}
LETTERS = {BAYER_RGGB8: "RGGB", BAYER_BGGR8: "BGGR", BAYER_GBRG8: "GBRG", BAYER_GRBG8: "GRBG"}
K = {"R": 4899, "G": 9617, "B": 1868}


def site_letters(fmt, h, w):
    """[h, w] array of 'R' / 'G' / 'B': the colour every pixel of the mosaic samples"""
    tile = np.array(list(LETTERS[fmt])).reshape(2, 2)
    return np.tile(tile, ((h + 1) // 2, (w + 1) // 2))[:h, :w]


def bayer_to_gray(frames, fmt):
    """[..., h, w] u8 mosaics -> [..., h, w] u8"""
    a = np.asarray(frames)
    assert a.dtype == np.uint8 and a.ndim >= 2
    h, w = a.shape[-2:]
    assert h >= 3 and w >= 3, "a Bayer frame needs an interior pixel"
    v = a.astype(np.int64)
    C = v[..., 1:-1, 1:-1]
    N, S, W, E = v[..., :-2, 1:-1], v[..., 2:, 1:-1], v[..., 1:-1, :-2], v[..., 1:-1, 2:]
    D = v[..., :-2, :-2] + v[..., :-2, 2:] + v[..., 2:, :-2] + v[..., 2:, 2:]
    site = site_letters(fmt, h, w)
    k = np.vectorize(K.get)(site).astype(np.int64)                     # weight of every site's own colour
    kC, kW, kN, kD = k[1:-1, 1:-1], k[1:-1, :-2], k[:-2, 1:-1], k[:-2, :-2]     # of the interior pixel, its left, upper and upper-left neighbour
    green = site[1:-1, 1:-1] == "G"
    rb = (4 * kC * C + K["G"] * (N + S + W + E) + kD * D + (1 << 15)) >> 16
    g = (2 * K["G"] * C + kW * (W + E) + kN * (N + S) + (1 << 14)) >> 15
    inner = np.where(green, g, rb)
    yy = np.clip(np.arange(h), 1, h - 2) - 1
    xx = np.clip(np.arange(w), 1, w - 2) - 1
    return inner[..., yy[:, None], xx[None, :]].astype(np.uint8)


def mono16_to_gray(v):
    """u16 values -> u8"""
    return ((np.asarray(v).astype(np.int64) + 128) // 257).astype(np.uint8)


def to_gray(frames, fmt):
    """frames of format fmt -> [..., h, w] u8.  Bayer: [..., h, w] u8; YUV 4:2:2 and MONO16: [..., h, w, 2] u8 (MONO16: little-endian byte pairs).
    Padded rows: pass a view, numpy reads through the strides."""
    a = np.asarray(frames)
    assert a.dtype == np.uint8
    if fmt in BAYER:
        return bayer_to_gray(a, fmt)
    assert a.shape[-1] == 2
    if fmt == YUV422_UYVY:
        return a[..., 1].copy()
    if fmt == YUV422_YUY2:
        return a[..., 0].copy()
    assert fmt == MONO16
    return mono16_to_gray(a[..., 0].astype(np.int64) | (a[..., 1].astype(np.int64) << 8))


def mosaic(r, g, b, fmt):
    """the mosaic a sensor of pattern fmt records of the three planes [..., h, w]"""
    r, g, b = (np.asarray(p, np.uint8) for p in (r, g, b))
    site = site_letters(fmt, *r.shape[-2:])
    return np.where(site == "R", r, np.where(site == "G", g, b)).astype(np.uint8)


def encode(gray, fmt, seed):
    """a raw frame of format fmt made of a gray one, so that the converted frame carries the gray one's texture: Bayer -- the mosaic of three planes with their
    own gains and noise (as cvt_gray_ref.colourise makes them); YUV 4:2:2 -- the gray values as luma between random chroma bytes; MONO16 -- gray * 257 plus a
    random offset in -100 .. 100 (so that the rounding takes part)"""
    rng = np.random.default_rng(seed)
    g = np.asarray(gray)
    gf = g.astype(np.float64)
    if fmt in BAYER:
        ch = [np.clip(np.rint(gf * gain + rng.uniform(-6, 6, gf.shape)), 0, 255).astype(np.uint8) for gain in (1.0, 0.8, 0.5)]
        return mosaic(ch[0], ch[1], ch[2], fmt)
    if fmt == MONO16:
        v = np.clip(g.astype(np.int64) * 257 + rng.integers(-100, 101, g.shape), 0, 65535).astype("<u2")
        return np.ascontiguousarray(v).view(np.uint8).reshape(g.shape + (2,))
    chroma = rng.integers(0, 256, g.shape).astype(np.uint8)
    return np.ascontiguousarray(np.stack([chroma, g] if fmt == YUV422_UYVY else [g, chroma], axis=-1).astype(np.uint8))


def padded(frames, pad, seed=0):
    """the same [batch, h, w(, bytes)] frames as a view with `pad` random bytes behind every row (frames stay h rows apart): (view, row pitch in bytes)"""
    a = np.ascontiguousarray(frames)
    b, h = a.shape[0], a.shape[1]
    row = int(np.prod(a.shape[2:]))
    buf = np.random.default_rng(seed).integers(0, 256, (b, h, row + pad)).astype(np.uint8)
    buf[:, :, :row] = a.reshape(b, h, row)
    return buf[:, :, :row].reshape(a.shape), row + pad
