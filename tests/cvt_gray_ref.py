"""Restatement of cv_bridge::toCvCopy(img_msg, MONO8) as the reference's node calls it in getImageFromMsg (rosNodeTest.cpp:238-254) in numpy: the parity target
of gf_cvt_gray_batch* and of the tracker's `pixel_format`.  cv_bridge hands rgb8 / bgr8 / rgba8 / bgra8 sources to cv::cvtColor(COLOR_{RGB,BGR,RGBA,BGRA}2GRAY),
whose 8-bit path (OpenCV 4.2, modules/imgproc/src/color_rgb.cpp, RGB2Gray<uchar>) is fixed point with 14 fractional bits:

    gray = (B * B2Y + G * G2Y + R * R2Y + (1 << 13)) >> 14        B2Y = 1868, G2Y = 9617, R2Y = 4899   (0.114, 0.587, 0.299; they sum to 1 << 14)

and alpha takes no part.  mono8 / 8UC1 sources are copied.  No OpenCV build is available to the tests, so this file is the yardstick; it is written from that
definition and shares nothing with the library."""
import numpy as np

MONO8, RGB8, BGR8, RGBA8, BGRA8 = range(5)       # GF_PIX_* of include/groundfusion_hip.h
COLOUR = (RGB8, BGR8, RGBA8, BGRA8)
ENCODING = {MONO8: "mono8", RGB8: "rgb8", BGR8: "bgr8", RGBA8: "rgba8", BGRA8: "bgra8"}     # sensor_msgs/image_encodings.h
CHANNELS = {MONO8: 1, RGB8: 3, BGR8: 3, RGBA8: 4, BGRA8: 4}
# byte of a pixel that holds red, green, blue
RGB_AT = {RGB8: (0, 1, 2), BGR8: (2, 1, 0), RGBA8: (0, 1, 2), BGRA8: (2, 1, 0)}
R2Y, G2Y, B2Y, SHIFT = 4899, 9617, 1868, 14


def gray_of(r, g, b):
    """the formula on integer arrays (or scalars) of channel values 0 .. 255"""
    r, g, b = (np.asarray(v).astype(np.int64) for v in (r, g, b))
    return ((b * B2Y + g * G2Y + r * R2Y + (1 << (SHIFT - 1))) >> SHIFT).astype(np.uint8)


def to_gray(frames, fmt):
    """[..., h, w, channels] u8 frames of format fmt (for MONO8: [..., h, w]) -> [..., h, w] u8.  Padded rows: pass a view, numpy reads through the strides."""
    a = np.asarray(frames)
    assert a.dtype == np.uint8
    if fmt == MONO8:
        return a.copy()
    assert a.shape[-1] == CHANNELS[fmt]
    ri, gi, bi = RGB_AT[fmt]
    return gray_of(a[..., ri], a[..., gi], a[..., bi])


def swapped(fmt):
    """the format that reads red where fmt reads blue"""
    return {RGB8: BGR8, BGR8: RGB8, RGBA8: BGRA8, BGRA8: RGBA8}[fmt]


def pack(r, g, b, fmt, alpha=None):
    """[..., h, w, channels] frames of format fmt from the three planes (alpha: a plane, for the four-channel formats)"""
    planes = [None] * CHANNELS[fmt]
    ri, gi, bi = RGB_AT[fmt]
    planes[ri], planes[gi], planes[bi] = r, g, b
    if CHANNELS[fmt] == 4:
        planes[3] = alpha if alpha is not None else np.full_like(r, 255)
    return np.ascontiguousarray(np.stack([np.asarray(p, np.uint8) for p in planes], axis=-1))


def colourise(gray, fmt, seed):
    """a genuinely coloured frame made of a gray one: every channel its own gain and its own noise (red strongest, blue weakest, so that exchanging red and blue
    moves the gray value), alpha random"""
    rng = np.random.default_rng(seed)
    gf = np.asarray(gray).astype(np.float64)
    ch = [np.clip(np.rint(gf * gain + rng.uniform(-6, 6, gf.shape)), 0, 255).astype(np.uint8) for gain in (1.0, 0.8, 0.5)]
    return pack(ch[0], ch[1], ch[2], fmt, rng.integers(0, 256, gf.shape).astype(np.uint8))


def padded(frames, pad, seed=0):
    """the same [batch, h, w(, ch)] frames as a view with `pad` random bytes behind every row (frames stay h rows apart): (view, row pitch in bytes)"""
    a = np.ascontiguousarray(frames)
    b, h = a.shape[0], a.shape[1]
    row = int(np.prod(a.shape[2:]))
    buf = np.random.default_rng(seed).integers(0, 256, (b, h, row + pad)).astype(np.uint8)
    buf[:, :, :row] = a.reshape(b, h, row)
    return buf[:, :, :row].reshape(a.shape), row + pad
