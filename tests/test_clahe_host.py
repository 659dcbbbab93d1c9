"""CLAHE (the reference node's EQUALIZE step, rosNodeTest.cpp:256-261) without a GPU: the numpy restatement (clahe_ref.py) on hand-computed cases, one per rule
that decides the bits, and the configuration path (`equalize: 1` in the YAML -> gf_tracker_cfg.equalize)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ground-fusion_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clahe_ref as R  # noqa: E402
import gfamd  # noqa: E402
import synth_stream as SS  # noqa: E402


def test_clip_limit_in_pixels():
    assert R.clip_pixels(40.0, 80 * 60) == 750          # (int)(40 * 4800 / 256.0)
    assert R.clip_pixels(2.0, 6400) == 50
    assert R.clip_pixels(1.0, 60) == 1                  # (int)0.234 = 0, then max(., 1)
    assert R.clip_pixels(40.0, 7) == 1                  # (int)1.09


def test_clip_cuts_and_spreads_the_residual():
    h = np.zeros(256, np.int64)
    h[0], h[1] = 10, 5
    got = R.clip_histogram(h, 4)                        # excess 6 + 1 = 7: batch 0, residual 7, step 256 // 7 = 36
    want = [0] * 256
    want[0], want[1] = 4 + 1, 4
    for k in range(1, 7):
        want[36 * k] += 1
    assert got == want and sum(got) == 15


def test_residual_step_rule():
    h = np.zeros(256, np.int64)
    h[7] = 516
    got = R.clip_histogram(h, 1)                        # excess 515 = 2 * 256 + 3: +2 everywhere, then bins 0, 85, 170
    want = [2] * 256
    want[7] = 3
    for b in (0, 85, 170):
        want[b] += 1
    assert got == want and sum(got) == 516
    h = np.zeros(256, np.int64)
    h[3] = 201
    got = R.clip_histogram(h, 1)                        # residual 200 > 128: step max(256 // 200, 1) = 1, bins 0 .. 199
    assert got[:200] == [1] * 3 + [2] + [1] * 196 and got[200:] == [0] * 56


def test_padding_rule():
    assert R.tile_geometry(640, 480, 8, 8) == (80, 60, 0, 0)
    assert R.tile_geometry(641, 479, 8, 8) == (81, 60, 7, 1)
    assert R.tile_geometry(10, 8, 4, 2) == (3, 5, 2, 2)     # the height divides and still gets a whole tile more
    assert R.tile_geometry(97, 132, 4, 3) == (25, 45, 3, 3)
    with pytest.raises(ValueError):
        R.tile_geometry(8, 100, 8, 8)
    img = np.arange(80, dtype=np.uint8).reshape(8, 10)
    p = R.padded(img, 4, 2)
    assert p.shape == (10, 12)
    assert list(p[0, 8:]) == [8, 9, 8, 7]                   # REFLECT_101: column 10 -> 8, 11 -> 7
    assert list(p[8:, 0]) == [60, 50]                       # row 8 -> 6, 9 -> 5


def test_rounding_ties_go_to_even():
    h = np.zeros(256, np.int64)
    h[0], h[1], h[2] = 1, 2, 3                              # tile area 6: lutScale = 255 / 6 = 42.5 exactly
    lut = R.make_lut(h, 6)
    assert list(lut[:3]) == [42, 128, 255]                  # 42.5 -> 42, 127.5 -> 128 (half to even), 255
    # the same tie through a whole frame: 3 x 2, one tile, no clipping; a lone 0 among 200s maps to 42, not 43
    img = np.full((2, 3), 200, np.uint8)
    img[1, 2] = 0
    out = R.clahe(img, 0.0, (1, 1))
    assert out[1, 2] == 42 and (out[img == 200] == 255).all()


def test_interpolation_weights():
    x1, x2, a, a1 = R.interp_weights(8, 4, 2)
    assert list(x1) == [0, 0, 0, 0, 0, 0, 1, 1]
    assert list(x2) == [0, 0, 1, 1, 1, 1, 1, 1]
    assert list(a) == [0.5, 0.75, 0.0, 0.25, 0.5, 0.75, 0.0, 0.25]
    assert (a + a1 == 1).all() and a.dtype == np.float32
    # the multiplication by the float reciprocal is what decides: 1.0f / 60 times 37 is not 37 / 60.0f rounded
    inv = np.float32(1) / np.float32(60)
    assert R.interp_weights(480, 60, 8)[2][37] == np.float32(37) * inv - np.float32(0.5)


def test_constant_frame():
    # 64 x 64, clip 40, 8 x 8 tiles of 64 pixels: clip 10, excess 54, residual 54, step 4 (bins 0, 4, .., 212 get one more)
    # cdf(v) = (bins of 0, 4, .., 212 at or below v) + 10 (the value's own bin, cut to the clip); lut = round(cdf * 255 / 64)
    #   77: 20 + 10 = 30 -> 119.53 -> 120;  0: 1 + 10 = 11 -> 43.83 -> 44;  100: 26 + 10 = 36 -> 143.44 -> 143;  255: 54 + 10 = 64 -> 255
    for v, want in ((77, 120), (0, 44), (100, 143), (255, 255)):
        out = R.clahe(np.full((64, 64), v, np.uint8), 40.0, (8, 8))
        assert (out == want).all(), (v, out.min(), out.max())


def test_clip_zero_is_tilewise_histogram_equalisation():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (48, 64)).astype(np.uint8)
    img[:24] //= 3                                          # different histograms in different tiles
    # one tile: plain equalisation, round(cdf(v) * 255 / N) half to even
    out = R.clahe(img, 0.0, (1, 1))
    cdf = np.cumsum(np.bincount(img.ravel(), minlength=256))
    assert (out == np.rint(cdf[img].astype(np.float32) * (np.float32(255) / np.float32(img.size))).astype(np.uint8)).all()
    # 4 x 3 tiles: every tile's LUT is that tile's own equalisation
    luts = R.tile_luts(img, 0.0, 4, 3)
    for j in range(3):
        for i in range(4):
            t = img[16 * j:16 * (j + 1), 16 * i:16 * (i + 1)]
            c = np.cumsum(np.bincount(t.ravel(), minlength=256))
            assert (luts[j, i] == np.rint(c.astype(np.float32) * (np.float32(255) / np.float32(256))).astype(np.uint8)).all()


def test_yaml_equalize_sets_the_tracker_flag(tmp_path):
    d0, d1 = tmp_path / "off", tmp_path / "on"
    for d in (d0, d1):
        SS.Stream(1).export(str(d), n_frames=1)
    p = d1 / "config.yaml"
    text = p.read_text()
    assert "\nequalize: 0\n" in text
    p.write_text(text.replace("\nequalize: 0\n", "\nequalize: 1\n"))
    c0 = gfamd.estimator_cfg_from_yaml(str(d0 / "config.yaml"))
    c1 = gfamd.estimator_cfg_from_yaml(str(d1 / "config.yaml"))
    assert c0.tracker.equalize == 0 and c1.tracker.equalize == 1
    c1.tracker.equalize = 0
    # every other field is the same (output_path is not part of the struct)
    assert bytes(c0) == bytes(c1)


def test_tracker_and_clahe_reject_what_they_cannot_do():
    cfg = gfamd.default_cfg(equalize=2)
    h = C.c_void_p()
    assert gfamd.lib().gf_tracker_create(C.byref(cfg), C.byref(h)) == -1          # GF_ERR_INVALID, before any device is touched
    assert b"equalize" in gfamd.lib().gf_last_error()
    buf = np.zeros((100, 8), np.uint8)
    with pytest.raises(gfamd.GfError, match="tiles_x"):
        gfamd.clahe(buf, 40.0, (8, 8))                                              # width 8 is not > 8 tiles: REFLECT_101 could not fill the pad
    with pytest.raises(gfamd.GfError, match="clip limit"):
        gfamd.clahe(np.zeros((64, 64), np.uint8), -1.0)
