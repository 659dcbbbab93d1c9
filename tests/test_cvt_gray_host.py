"""Colour -> MONO8 (getImageFromMsg's cv_bridge::toCvCopy(msg, MONO8), rosNodeTest.cpp:238-254) without a GPU: the numpy restatement (cvt_gray_ref.py) against the
shipped host decoder, which shares its formula with the device kernels (csrc/gf_pixfmt.hpp), and the test frames of test_cvt_gray_gpu.py shown not to be vacuous."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ground-fusion_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bagwriter as BW  # noqa: E402
import cvt_gray_ref as R  # noqa: E402
import gfamd  # noqa: E402
import synth  # noqa: E402


def test_restatement_on_hand_computed_pixels():
    assert R2Y_SUM == 1 << 14
    # pure channels: 255 * weight + 8192 >> 14
    assert int(R.gray_of(255, 0, 0)) == (255 * 4899 + 8192) >> 14 == 76
    assert int(R.gray_of(0, 255, 0)) == 150 and int(R.gray_of(0, 0, 255)) == 29
    assert int(R.gray_of(255, 255, 255)) == 255 and int(R.gray_of(0, 0, 0)) == 0
    # a value that sits on the rounding edge: 2 * 4899 + 1 * 9617 + 3 * 1868 = 25019 -> (25019 + 8192) >> 14 = 2, one below the edge truncation would give 1
    assert int(R.gray_of(2, 1, 3)) == 2 and 25019 >> 14 == 1
    px = np.array([[[10, 200, 30, 77]]], np.uint8)
    assert R.to_gray(px[..., :3], R.RGB8)[0, 0] == R.gray_of(10, 200, 30) and R.to_gray(px[..., :3], R.BGR8)[0, 0] == R.gray_of(30, 200, 10)
    assert R.to_gray(px, R.RGBA8)[0, 0] == R.gray_of(10, 200, 30) and R.to_gray(px, R.BGRA8)[0, 0] == R.gray_of(30, 200, 10)


R2Y_SUM = R.R2Y + R.G2Y + R.B2Y


@pytest.mark.parametrize("fmt", R.COLOUR)
@pytest.mark.parametrize("size,pad", [((37, 23), 0), ((37, 23), 5), ((64, 8), 3), ((1, 1), 1)])
def test_restatement_equals_the_host_decoder(fmt, size, pad):
    """ties the tests' reference to the formula the library ships: gf_ros_decode_image on random images of the four encodings with a padded step"""
    w, h = size
    rng = np.random.default_rng(100 * fmt + w + pad)
    img = rng.integers(0, 256, (h, w, R.CHANNELS[fmt])).astype(np.uint8)
    t, got = gfamd.ros_decode_image(BW.image(3, 1_500_000_000, img, R.ENCODING[fmt], step_pad=pad))
    assert got.dtype == np.uint8 and got.shape == (h, w)
    assert np.array_equal(got, R.to_gray(img, fmt))


def test_mono8_is_a_copy_in_both():
    img = np.random.default_rng(5).integers(0, 256, (9, 13)).astype(np.uint8)
    for enc in ("mono8", "8UC1"):
        assert np.array_equal(gfamd.ros_decode_image(BW.image(0, 1, img, enc, step_pad=3))[1], img)
    assert np.array_equal(R.to_gray(img, R.MONO8), img)


def test_padded_view_reads_the_same_pixels():
    a = np.random.default_rng(2).integers(0, 256, (3, 5, 7, 4)).astype(np.uint8)
    v, pitch = R.padded(a, 5, seed=1)
    assert pitch == 7 * 4 + 5 and v.strides == (5 * pitch, pitch, 4, 1) and np.array_equal(v, a) and not v.flags.c_contiguous


@pytest.mark.parametrize("fmt", R.COLOUR)
def test_the_coloured_test_frames_are_not_vacuous(fmt):
    """a conversion that took red for blue must show on the frames the GPU tests use: more than half of the pixels change"""
    frames = synth.tracker_sequence(1000, 2, w=160, h=120) + synth.tracker_sequence(1000, 1)
    for k, f in enumerate(frames):
        c = R.colourise(f, fmt, 40 + k)
        assert c.shape == f.shape + (R.CHANNELS[fmt],)
        right, wrong = R.to_gray(c, fmt), R.to_gray(c, R.swapped(fmt))
        assert np.mean(right != wrong) > 0.5, (fmt, k, float(np.mean(right != wrong)))
    # the frame that holds every colour once
    v = np.arange(1 << 24, dtype=np.uint32)
    r, g, b = (v & 255).astype(np.uint8), ((v >> 8) & 255).astype(np.uint8), (v >> 16).astype(np.uint8)
    assert np.mean(R.gray_of(r, g, b) != R.gray_of(b, g, r)) > 0.5


def test_python_mirror_of_the_new_fields():
    """the configuration ends with the new field, the stats carry theirs behind the other times' counters (sequence_frames stays the last member), and the
    documented default is the handle as it was"""
    assert gfamd.TrackerCfg._fields_[-1] == ("pixel_format", gfamd.C.c_int) and gfamd.TrackerStats._fields_[-2] == ("ms_convert", gfamd.C.c_double)
    assert gfamd.default_cfg().pixel_format == 0 == gfamd.PIX_MONO8 and gfamd.default_cfg(pixel_format=gfamd.PIX_BGRA8).pixel_format == 4
    assert (gfamd.PIX_RGB8, gfamd.PIX_BGR8, gfamd.PIX_RGBA8, gfamd.PIX_BGRA8) == R.COLOUR and gfamd.PIX_CHANNELS == tuple(R.CHANNELS[f] for f in range(5))
    assert gfamd.default_estimator_cfg().tracker.pixel_format == 0
    for enc, fmt in gfamd.PIX_OF_ENCODING.items():
        assert R.ENCODING[fmt] == enc or enc == "8UC1"


def test_refusals_that_need_no_device():
    """checked before the device is asked for: unknown format, pitch too small, sizes, overlap, pixel_format out of range at create"""
    lib = gfamd.lib()
    src = np.zeros((4, 8, 3), np.uint8)
    for fmt in (-1, 5, 99):
        with pytest.raises(gfamd.GfError, match="status -1.*pixel format"):
            gfamd.cvt_gray(src, fmt)
    dst = np.zeros((4, 8), np.uint8)
    p = lambda a: a.ctypes.data_as(gfamd.C.c_void_p)
    assert lib.gf_cvt_gray_batch(p(src), gfamd.C.c_size_t(23), R.RGB8, gfamd._p(dst, gfamd.C.c_uint8), 1, 8, 4) == -1 and b"pitch" in lib.gf_last_error()
    assert lib.gf_cvt_gray_batch(p(src), gfamd.C.c_size_t(24), R.RGB8, gfamd._p(dst, gfamd.C.c_uint8), 0, 8, 4) == -1
    assert lib.gf_cvt_gray_batch(p(src), gfamd.C.c_size_t(24), R.RGB8, gfamd._p(src.reshape(-1)[8:], gfamd.C.c_uint8), 1, 8, 4) == -1 and b"overlap" in lib.gf_last_error()
    for bad in (-1, 5):
        h = gfamd.C.c_void_p()
        cfg = gfamd.default_cfg(pixel_format=bad)
        assert lib.gf_tracker_create(gfamd.C.byref(cfg), gfamd.C.byref(h)) == -1 and not h.value
        assert b"pixel_format" in lib.gf_last_error()
