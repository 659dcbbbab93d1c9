"""Bayer, YUV 4:2:2 and MONO16 -> MONO8 (cv_bridge::toCvCopy(msg, MONO8) of getImageFromMsg, rosNodeTest.cpp:238-254) without a GPU: the numpy restatement
(raw_gray_ref.py) against its closed forms and against the shipped host decoder, which shares its formulas with the device kernels (csrc/gf_pixfmt.hpp); the
Python mirror of the new formats; the refusals that are made before a device is asked for."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ground-fusion_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bagwriter as BW  # noqa: E402
import cvt_gray_ref as CR  # noqa: E402
import gfamd  # noqa: E402
import raw_gray_ref as R  # noqa: E402

NAMES = {f: R.ENCODING[f] for f in R.RAW}
SIZES = [(3, 3), (4, 3), (5, 4), (17, 9), (160, 120)]      # (width, height)


# ---------------------------------------------------------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("fmt", R.BAYER, ids=[NAMES[f] for f in R.BAYER])
def test_restatement_closed_forms(fmt):
    """a mosaic of one uniform colour gives the colour conversion's gray at every pixel, an all-255 frame gives 255"""
    rng = np.random.default_rng(fmt)
    for w, h in SIZES[:4] + [(8, 6)]:
        for r, g, b in [(255, 0, 0), (0, 255, 0), (0, 0, 255), (0, 0, 0), (2, 1, 3)] + [tuple(int(v) for v in rng.integers(0, 256, 3)) for _ in range(20)]:
            m = R.mosaic(np.full((h, w), r), np.full((h, w), g), np.full((h, w), b), fmt)
            assert np.all(R.to_gray(m, fmt) == CR.gray_of(r, g, b)), (w, h, r, g, b)
        assert np.all(R.to_gray(np.full((h, w), 255, np.uint8), fmt) == 255)


def test_restatement_site_colours_and_hand_computed_pixels():
    assert ["".join(row) for row in R.site_letters(R.BAYER_RGGB8, 3, 4)] == ["RGRG", "GBGB", "RGRG"]
    assert ["".join(row) for row in R.site_letters(R.BAYER_BGGR8, 2, 2)] == ["BG", "GR"]
    assert ["".join(row) for row in R.site_letters(R.BAYER_GBRG8, 2, 2)] == ["GB", "RG"]
    assert ["".join(row) for row in R.site_letters(R.BAYER_GRBG8, 2, 2)] == ["GR", "BG"]
    m = np.array([[10, 20, 30], [40, 50, 60], [70, 80, 90]], np.uint8)
    # rggb: the centre is blue, its edge neighbours green, its diagonal neighbours red
    want = (4 * 1868 * 50 + 9617 * (20 + 80 + 40 + 60) + 4899 * (10 + 30 + 70 + 90) + (1 << 15)) >> 16
    assert np.all(R.to_gray(m, R.BAYER_RGGB8) == want)
    # grbg: the centre is green, red left and right of it (row 1 is B G B: blue), red above and below
    want = (2 * 9617 * 50 + 1868 * (40 + 60) + 4899 * (20 + 80) + (1 << 14)) >> 15
    assert np.all(R.to_gray(m, R.BAYER_GRBG8) == want)
    # the border repeats the nearest interior pixel
    big = np.random.default_rng(1).integers(0, 256, (6, 7)).astype(np.uint8)
    out = R.to_gray(big, R.BAYER_GBRG8)
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[-1], out[-2]) and np.array_equal(out[:, 0], out[:, 1]) and np.array_equal(out[:, -1], out[:, -2])
    assert len(np.unique(out[1:-1, 1:-1])) > 10


def test_restatement_mono16_and_yuv():
    v = np.arange(65536)
    assert np.array_equal(R.mono16_to_gray(v), np.rint(v * 255 / 65535).astype(np.uint8))
    assert np.array_equal(R.mono16_to_gray(v), np.rint(v.astype(np.float32) * np.float32(255.0 / 65535.0)).astype(np.uint8))
    px = np.array([[[1, 2], [3, 4]]], np.uint8)
    assert R.to_gray(px, R.YUV422_UYVY).tolist() == [[2, 4]] and R.to_gray(px, R.YUV422_YUY2).tolist() == [[1, 3]]
    assert R.to_gray(px, R.MONO16).tolist() == [[(513 + 128) // 257, (1027 + 128) // 257]]


# ---------------------------------------------------------------------------------------------------------------- the host decoder
def _raw_frame(fmt, w, h, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (h, w) if fmt in R.BAYER else (h, w, 2)).astype(np.uint8)


@pytest.mark.parametrize("pad", [0, 3, 5])
@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("fmt", R.RAW, ids=[NAMES[f] for f in R.RAW])
def test_host_decoder_equals_the_restatement(fmt, size, pad):
    """gf_ros_decode_image on messages of every new encoding, tight and with a padded step; mono16 in both byte orders"""
    w, h = size
    img = _raw_frame(fmt, w, h, 1000 * fmt + 10 * w + pad)
    want = R.to_gray(img, fmt)
    if fmt == R.MONO16:
        u16 = img.view("<u2").reshape(h, w)
        for be in (False, True):
            t, got = gfamd.ros_decode_image(BW.image(3, 1_500_000_000, u16.astype(np.uint16), "mono16", step_pad=pad, big_endian=be))
            assert t == 1.5 and got.dtype == np.uint8 and np.array_equal(got, want), be
    else:
        t, got = gfamd.ros_decode_image(BW.image(3, 1_500_000_000, img, R.ENCODING[fmt], step_pad=pad))
        assert t == 1.5 and got.dtype == np.uint8 and got.shape == (h, w)
        assert np.array_equal(got, want), "%d pixels differ" % int(np.sum(got != want))


@pytest.mark.parametrize("fmt", R.BAYER, ids=[NAMES[f] for f in R.BAYER])
def test_host_decoder_on_extremes(fmt):
    for k, img in enumerate([np.zeros((9, 12), np.uint8), np.full((9, 12), 255, np.uint8), (np.indices((9, 12)).sum(0) % 2 * 255).astype(np.uint8),
                             ((np.indices((9, 12)).sum(0) + 1) % 2 * 255).astype(np.uint8), (np.indices((9, 12))[0] % 2 * 255).astype(np.uint8)]):
        assert np.array_equal(gfamd.ros_decode_image(BW.image(0, 1, img, R.ENCODING[fmt], step_pad=1))[1], R.to_gray(img, fmt)), k


def test_the_encoded_test_frames_are_not_vacuous():
    """the frames the GPU tests feed the tracker: reading a mosaic with the wrong pattern, a YUV frame with the wrong byte order or a 16-bit frame as bytes must
    change most of the pixels, and the converted frame must carry the gray frame's texture"""
    import synth
    f = synth.tracker_sequence(1000, 1, w=160, h=120)[0]
    other = {R.BAYER_RGGB8: R.BAYER_BGGR8, R.BAYER_BGGR8: R.BAYER_RGGB8, R.BAYER_GBRG8: R.BAYER_GRBG8, R.BAYER_GRBG8: R.BAYER_GBRG8,
             R.YUV422_UYVY: R.YUV422_YUY2, R.YUV422_YUY2: R.YUV422_UYVY, R.MONO16: R.YUV422_YUY2}
    for fmt in R.RAW:
        e = R.encode(f, fmt, 7)
        assert e.shape == f.shape + ((2,) if R.BYTES[fmt] == 2 else ())
        right, wrong = R.to_gray(e, fmt), R.to_gray(e, other[fmt])
        assert np.mean(right != wrong) > 0.5, (fmt, float(np.mean(right != wrong)))
        assert np.corrcoef(right.reshape(-1).astype(float), f.reshape(-1).astype(float))[0, 1] > 0.9, fmt


# ---------------------------------------------------------------------------------------------------------------- the Python mirror
def test_python_mirror_of_the_raw_formats():
    assert (gfamd.PIX_BAYER_RGGB8, gfamd.PIX_BAYER_BGGR8, gfamd.PIX_BAYER_GBRG8, gfamd.PIX_BAYER_GRBG8, gfamd.PIX_YUV422_UYVY, gfamd.PIX_YUV422_YUY2,
            gfamd.PIX_MONO16) == R.RAW == gfamd.PIX_RAW == tuple(range(8, 15))
    for fmt in R.RAW:
        assert gfamd.pix_bytes(fmt) == R.BYTES[fmt] == gfamd.PIX_RAW_BYTES[fmt]
        assert gfamd.PIX_RAW_OF_ENCODING[R.ENCODING[fmt]] == fmt == gfamd.pix_of_encoding(R.ENCODING[fmt])
    assert len(gfamd.PIX_RAW_OF_ENCODING) == 7
    for fmt in range(5):
        assert gfamd.pix_bytes(fmt) == gfamd.PIX_CHANNELS[fmt]
    for fmt in (-1, 5, 6, 7, 15, 99):
        assert gfamd.pix_bytes(fmt) is None
    assert gfamd.pix_of_encoding("rgb8") == gfamd.PIX_RGB8 and gfamd.pix_of_encoding("8UC1") == gfamd.PIX_MONO8 and gfamd.pix_of_encoding("32FC1") is None
    # what the earlier tests pin stays: the colour tuple, the colour map, the last field of the configuration
    assert gfamd.PIX_CHANNELS == (1, 3, 3, 4, 4) and len(gfamd.PIX_OF_ENCODING) == 6 and gfamd.TrackerCfg._fields_[-1] == ("pixel_format", gfamd.C.c_int)
    assert gfamd.default_cfg(pixel_format=gfamd.PIX_MONO16).pixel_format == 14


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_that_need_no_device():
    lib = gfamd.lib()
    C = gfamd.C
    src = np.zeros((6, 8, 2), np.uint8)
    dst = np.zeros((6, 8), np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for fmt in (5, 6, 7, 15, 99, -1):
        with pytest.raises(gfamd.GfError, match="status -1.*pixel format"):
            gfamd.cvt_gray(src, fmt)
        assert lib.gf_cvt_gray_batch(p(src), C.c_size_t(16), fmt, gfamd._p(dst, C.c_uint8), 1, 8, 6) == -1 and b"pixel format" in lib.gf_last_error()
        h = C.c_void_p()
        cfg = gfamd.default_cfg(pixel_format=fmt)
        assert lib.gf_tracker_create(C.byref(cfg), C.byref(h)) == -1 and not h.value and b"pixel_format" in lib.gf_last_error()
    # Bayer below 3 x 3
    for fmt in R.BAYER:
        for w, h in ((2, 3), (3, 2), (1, 1), (2, 8)):
            assert lib.gf_cvt_gray_batch(p(src), C.c_size_t(8), fmt, gfamd._p(dst, C.c_uint8), 1, w, h) == -1 and b"3" in lib.gf_last_error(), (fmt, w, h)
            with pytest.raises(gfamd.GfError, match="3 x 3"):
                gfamd.ros_decode_image(BW.image(1, 0, np.zeros((h, w), np.uint8), R.ENCODING[fmt]))
    # a pitch below width x bytes
    for fmt in R.RAW:
        short = 8 * R.BYTES[fmt] - 1
        assert lib.gf_cvt_gray_batch(p(src), C.c_size_t(short), fmt, gfamd._p(dst, C.c_uint8), 1, 8, 6) == -1 and b"pitch" in lib.gf_last_error(), fmt
    # overlap
    flat = np.zeros(2 * 8 * 6 + 8 * 6, np.uint8)
    assert lib.gf_cvt_gray_batch(p(flat), C.c_size_t(16), R.YUV422_UYVY, gfamd._p(flat[16:], C.c_uint8), 1, 8, 6) == -1 and b"overlap" in lib.gf_last_error()
    assert lib.gf_cvt_gray_batch(p(flat), C.c_size_t(8), R.BAYER_RGGB8, gfamd._p(flat[40:], C.c_uint8), 1, 8, 6) == -1 and b"overlap" in lib.gf_last_error()
    # a message whose step is shorter than its rows, and the encodings that stay out of scope
    with pytest.raises(gfamd.GfError, match="32FC1"):
        gfamd.ros_decode_image(BW.image(1, 0, np.zeros((4, 4), np.uint8), "32FC1"))
    with pytest.raises(gfamd.GfError, match="bayer_rggb16"):
        gfamd.ros_decode_image(BW.image(1, 0, np.zeros((4, 4), np.uint16), "bayer_rggb16"))
    with pytest.raises(gfamd.GfError, match="step"):
        gfamd.ros_decode_image(BW.image(1, 0, np.zeros((4, 4), np.uint8), "mono16"))
