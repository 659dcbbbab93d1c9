"""TEST INFRASTRUCTURE: builds tests/roi_tracker_ref.cpp (the oracle's tracker with a region of interest in setMask) into a temporary directory with the flags of
oracle/Makefile and binds it with ctypes; the interface of oracle_py.Tracker plus set_roi / dropped_outside.  Also the regions and frames the tests share."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE = os.path.join(HERE, "..", "oracle")


def _makefile_flags():
    """COMMON of oracle/Makefile, as it is written there"""
    mk = open(os.path.join(ORACLE, "Makefile")).read()
    return re.search(r"^COMMON\s*=\s*(.*)$", mk, re.M).group(1).split()


def build(tmpdir):
    so = os.path.join(str(tmpdir), "libroi_tracker_ref.so")
    cmd = [os.environ.get("CXX", "g++")] + _makefile_flags() + ["-Wno-unused-function", "-I", ORACLE, "-shared", "-o", so, os.path.join(HERE, "roi_tracker_ref.cpp")]
    subprocess.check_call(cmd)
    lib = C.CDLL(so)
    lib.roiref_create.restype = C.c_void_p
    lib.roiref_dropped_outside.restype = C.c_longlong
    return lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


class Tracker:
    def __init__(self, lib, cfg):
        self.lib, self.cfg = lib, cfg
        self.h = C.c_void_p(lib.roiref_create(C.byref(cfg)))

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.roiref_destroy(self.h)
            self.h = None

    def set_roi(self, mask):
        if mask is None:
            self.lib.roiref_set_roi(self.h, None, 0, 0)
        else:
            mask = np.ascontiguousarray(mask, np.uint8)
            self.lib.roiref_set_roi(self.h, _p(mask, C.c_uint8), mask.shape[1], mask.shape[0])

    def dropped_outside(self):
        return int(self.lib.roiref_dropped_outside(self.h))

    def track(self, t, img, depth=None, cap=4096):
        img = np.ascontiguousarray(img, np.uint8)
        h, w = img.shape
        ids = np.zeros(cap, np.int32)
        obs = np.zeros((cap, 8), np.float64)
        if depth is not None:
            depth = np.ascontiguousarray(depth, np.uint16)
            dp, ds = _p(depth, C.c_uint16), depth.shape[1]
        else:
            dp, ds = None, 0
        n = self.lib.roiref_track(self.h, C.c_double(t), _p(img, C.c_uint8), w, h, w, dp, ds, _p(ids, C.c_int), _p(obs, C.c_double), cap)
        assert n >= 0, "the region of interest does not have the frame's size"
        return ids[:n].copy(), obs[:n].copy()

    def set_prediction(self, ids, xyz):
        ids = np.ascontiguousarray(ids, np.int32)
        xyz = np.ascontiguousarray(xyz, np.float64)
        self.lib.roiref_set_prediction(self.h, _p(ids, C.c_int), _p(xyz, C.c_double), len(ids))

    def remove_outliers(self, ids):
        ids = np.ascontiguousarray(ids, np.int32)
        self.lib.roiref_remove_outliers(self.h, _p(ids, C.c_int), len(ids))

    def state(self, cap=4096):
        ids = np.zeros(cap, np.int32)
        cnt = np.zeros(cap, np.int32)
        pts = np.zeros((cap, 2), np.float32)
        n = self.lib.roiref_state(self.h, _p(ids, C.c_int), _p(cnt, C.c_int), _p(pts, C.c_float), cap)
        return ids[:n].copy(), cnt[:n].copy(), pts[:n].copy()


# ---- what the tests share: sizes, regions, frames
# (w, h, max_cnt, min_dist): a partial last strip (60 columns) and a partial last band (30 rows) in every small one; the shipped configuration once
SIZES = [(132, 97, 40, 6), (188, 122, 40, 6), (64, 61, 20, 3), (640, 480, 150, 30)]
K = 6


def size_id(c):
    return "%dx%d" % (c[0], c[1])


def region(name, w, h):
    """A: the bottom third excluded.  B: the left two fifths excluded, and a disc of radius h // 5 about (3w // 4, h // 2)."""
    R = np.full((h, w), 255, np.uint8)
    if name == "A":
        R[h - h // 3:, :] = 0
    elif name == "B":
        R[:, :2 * w // 5] = 0
        yy, xx = np.mgrid[0:h, 0:w]
        R[(xx - 3 * w // 4) ** 2 + (yy - h // 2) ** 2 <= (h // 5) ** 2] = 0
    else:
        raise ValueError(name)
    return R


def frames(w, h, n=K, seed=0):
    import synth
    return synth.tracker_sequence(2000 + w + h + seed, n, w, h)


def depth(k, w, h):
    """the depth frames of tests/test_tracker_sizes_gpu.py: a different value at every pixel"""
    return np.random.default_rng(500 + k).integers(300, 9000, (h, w)).astype(np.uint16)


def same(a, b, what):
    (ai, ao), (bi, bo) = a, b
    assert np.array_equal(ai, bi), "%s: feature id lists differ" % what
    assert np.array_equal(ao.view(np.uint64), bo.view(np.uint64)), "%s: observations differ" % what


def on_excluded(obs, R):
    """how many reported points (columns 3, 4: the pixel) round onto an excluded pixel"""
    if len(obs) == 0:
        return 0
    x, y = np.rint(obs[:, 3]).astype(int), np.rint(obs[:, 4]).astype(int)
    return int((R[y, x] == 0).sum())
