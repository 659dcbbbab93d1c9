"""ctypes binding of the C-ABI (include/groundfusion_hip.h) — the call surface tests and bench.py use.
Mirrors the reference's FeatureTracker interface names (trackImage / setPrediction / removeOutliers).
Raises if the HIP library is missing or no GPU is present: there is no CPU fallback in the product path."""
import ctypes as C
import os
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GF_LIB_PATH") or os.path.join(HERE, "lib", "libgroundfusion_hip.so")   # override: profiling builds of the same sources
_LIB = None


class GfError(RuntimeError):
    pass


class TrackerCfg(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("batch", C.c_int), ("max_cnt", C.c_int), ("min_dist", C.c_int),
                ("flow_back", C.c_int), ("depth_cam", C.c_int),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("k1", C.c_double), ("k2", C.c_double), ("p1", C.c_double), ("p2", C.c_double), ("equalize", C.c_int), ("pixel_format", C.c_int)]


class TrackerSeqCfg(C.Structure):
    """gf_tracker_seq_cfg: the parameters a sequence of a tracker handle may have of its own (the reference's per-FeatureTracker members)"""
    _fields_ = [("max_cnt", C.c_int), ("min_dist", C.c_int), ("flow_back", C.c_int), ("depth_cam", C.c_int),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("k1", C.c_double), ("k2", C.c_double), ("p1", C.c_double), ("p2", C.c_double)]


class TrackerSeqFormat(C.Structure):
    """gf_tracker_seq_format: the pixel format, equalise switch and host row step a sequence of a tracker handle may have of its own (rosNodeTest.cpp:238-261)"""
    _fields_ = [("pixel_format", C.c_int), ("equalize", C.c_int), ("host_stride", C.c_int)]


# GF_PIX_*: the formats of the frames a tracker handle takes and of cvt_gray (rosNodeTest.cpp:238-254), and their bytes per pixel
PIX_MONO8, PIX_RGB8, PIX_BGR8, PIX_RGBA8, PIX_BGRA8 = range(5)
PIX_CHANNELS = (1, 3, 3, 4, 4)
PIX_OF_ENCODING = {"mono8": PIX_MONO8, "8UC1": PIX_MONO8, "rgb8": PIX_RGB8, "bgr8": PIX_BGR8, "rgba8": PIX_RGBA8, "bgra8": PIX_BGRA8}
# the raw formats (cameras that do not debayer on board): Bayer mosaics are [h, w] u8 frames like MONO8; YUV 4:2:2 and MONO16 are [h, w, 2] u8 (MONO16: the
# little-endian bytes of the pixel, `a.astype("<u2").view(np.uint8).reshape(h, w, 2)`)
PIX_BAYER_RGGB8, PIX_BAYER_BGGR8, PIX_BAYER_GBRG8, PIX_BAYER_GRBG8, PIX_YUV422_UYVY, PIX_YUV422_YUY2, PIX_MONO16 = range(8, 15)
PIX_RAW = tuple(range(8, 15))
PIX_RAW_BYTES = {PIX_BAYER_RGGB8: 1, PIX_BAYER_BGGR8: 1, PIX_BAYER_GBRG8: 1, PIX_BAYER_GRBG8: 1, PIX_YUV422_UYVY: 2, PIX_YUV422_YUY2: 2, PIX_MONO16: 2}
PIX_RAW_OF_ENCODING = {"bayer_rggb8": PIX_BAYER_RGGB8, "bayer_bggr8": PIX_BAYER_BGGR8, "bayer_gbrg8": PIX_BAYER_GBRG8, "bayer_grbg8": PIX_BAYER_GRBG8,
                       "yuv422": PIX_YUV422_UYVY, "yuv422_yuy2": PIX_YUV422_YUY2, "mono16": PIX_MONO16}


def pix_bytes(pixel_format):
    """bytes per pixel of a GF_PIX_* value, None if it is no format"""
    if 0 <= pixel_format < len(PIX_CHANNELS):
        return PIX_CHANNELS[pixel_format]
    return PIX_RAW_BYTES.get(pixel_format)


def pix_of_encoding(encoding):
    """GF_PIX_* of a sensor_msgs/Image encoding of an image topic, None if the node's conversion to MONO8 is not built for it"""
    return PIX_OF_ENCODING.get(encoding, PIX_RAW_OF_ENCODING.get(encoding))


class FrameRef(C.Structure):
    """gf_frame_ref: a frame where it lives on the device -- the address of row 0 and the bytes from row to row"""
    _fields_ = [("data", C.c_void_p), ("pitch", C.c_size_t)]


def frame_refs(refs):
    """a gf_frame_ref table from (address, pitch) pairs; None or address 0 = a null entry.  torch: (t.data_ptr(), t.stride(0) * t.element_size()).
    A table made earlier is handed back as it is: a caller whose surfaces stay where they are builds it once."""
    if isinstance(refs, C.Array):
        return refs
    table = (FrameRef * max(len(refs), 1))()
    for i, r in enumerate(refs):
        if r is not None:
            table[i].data, table[i].pitch = (int(r[0]) or None), int(r[1])
    return table


class FeatureObs(C.Structure):
    _fields_ = [("id", C.c_int), ("camera_id", C.c_int), ("v", C.c_double * 8)]


class TrackerStats(C.Structure):
    _fields_ = [("ms_pyramid", C.c_double), ("ms_lk", C.c_double), ("ms_detect", C.c_double), ("ms_total_gpu", C.c_double),
                ("ms_host_pre", C.c_double), ("ms_wait_lk", C.c_double), ("ms_host_mid", C.c_double), ("ms_wait_detect", C.c_double), ("ms_host_post", C.c_double),
                ("frames", C.c_longlong), ("lk_launches", C.c_longlong), ("lk_points", C.c_longlong),
                ("lk_level_passes", C.c_longlong), ("lk_iterations", C.c_longlong), ("tracked_features", C.c_longlong),
                ("output_features", C.c_longlong), ("select_streamed", C.c_longlong), ("select_global_sort", C.c_longlong),
                ("ms_equalize", C.c_double), ("pyr_head", C.c_longlong), ("pyr_level0_vec16", C.c_longlong), ("pyr_level0_dword", C.c_longlong),
                ("pyr_down_tail", C.c_longlong), ("pyr_down_pad4", C.c_longlong), ("pyr_down_bytes", C.c_longlong), ("frames_unaligned", C.c_longlong), ("ms_convert", C.c_double),
                ("sequence_frames", C.c_longlong)]


class Box(C.Structure):
    """gf_box: the four integers of a darknet_ros_msgs/BoundingBox"""
    _fields_ = [("xmin", C.c_int32), ("ymin", C.c_int32), ("xmax", C.c_int32), ("ymax", C.c_int32)]


MAX_BOXES_PER_SEQ = 256   # GF_MAX_BOXES_PER_SEQ
assert C.sizeof(Box) == 16


def _boxes(boxes):
    """[n, 4] int32 rows of xmin, ymin, xmax, ymax from anything array-like (an empty list: no boxes)"""
    a = np.ascontiguousarray(boxes if boxes is not None else [], np.int64).reshape(-1, 4)
    if a.size and (a.min() < -2 ** 31 or a.max() > 2 ** 31 - 1):
        raise ValueError("a box coordinate is no int32")
    return np.ascontiguousarray(a, np.int32)


def _box_lists(lists):
    """(first [len + 1] int32, boxes [total, 4] int32) of a list of box lists"""
    rows = [_boxes(l) for l in lists]
    first = np.zeros(len(rows) + 1, np.int32)
    first[1:] = np.cumsum([len(r) for r in rows])
    return first, np.ascontiguousarray(np.concatenate(rows) if rows else np.zeros((0, 4)), np.int32).reshape(-1, 4)


def roi_boxes_batch(lists, width, height, base_masks=None):
    """gf_roi_boxes_batch: the region the box lists leave, by the tracker's kernels -- lists[b] = boxes (xmin, ymin, xmax, ymax) of frame b, base_masks None or
    [batch, height, width] u8 (non-zero = allowed) -> [batch, height, width] u8 of 0 / 255"""
    first, flat = _box_lists(lists)
    b = len(lists)
    if base_masks is not None:
        base_masks = np.ascontiguousarray(base_masks, np.uint8)
        if base_masks.shape != (b, height, width):
            raise ValueError("roi_boxes_batch: base_masks must be [batch, height, width]")
    out = np.zeros((b, height, width), np.uint8)
    _chk(lib().gf_roi_boxes_batch(b, width, height, _p(first, C.c_int), flat.ctypes.data_as(C.POINTER(Box)) if len(flat) else None,
                                  None if base_masks is None else _p(base_masks, C.c_uint8), _p(out, C.c_uint8)))
    return out


CAMERA_PINHOLE, CAMERA_MEI, CAMERA_KANNALA_BRANDT = 0, 1, 2   # GF_CAMERA_*
CAMERA_NAMES = {"PINHOLE": CAMERA_PINHOLE, "MEI": CAMERA_MEI, "KANNALA_BRANDT": CAMERA_KANNALA_BRANDT}


class CameraModel(C.Structure):
    """gf_camera_model: a camodocal camera -- proj = fx fy cx cy | gamma1 gamma2 u0 v0 | mu mv u0 v0, dist = k1 k2 p1 p2 | k1 k2 p1 p2 | k2 k3 k4 k5, xi (MEI)"""
    _fields_ = [("model", C.c_int32), ("reserved", C.c_int32), ("proj", C.c_double * 4), ("dist", C.c_double * 4), ("xi", C.c_double)]

    @classmethod
    def make(cls, model, proj, dist=(0.0, 0.0, 0.0, 0.0), xi=0.0):
        """model: CAMERA_* or its camodocal name"""
        m = cls()
        m.model = CAMERA_NAMES[model] if isinstance(model, str) else int(model)
        m.proj[:] = [float(v) for v in proj]
        m.dist[:] = [float(v) for v in dist]
        m.xi = float(xi)
        return m

    def as_dict(self):
        return {"model": self.model, "proj": list(self.proj), "dist": list(self.dist), "xi": self.xi}


assert C.sizeof(CameraModel) == 80

CAMERA_PINHOLE_FULL, CAMERA_SCARAMUZZA = 3, 4   # valid in CameraModelEx only
CAMERA_NAMES_EX = dict(CAMERA_NAMES, PINHOLE_FULL=CAMERA_PINHOLE_FULL, SCARAMUZZA=CAMERA_SCARAMUZZA)


class CameraModelEx(C.Structure):
    """gf_camera_model_ex: any of camodocal's five cameras -- proj, dist[:4], xi as CameraModel for models 0-2; PINHOLE_FULL proj = fx fy cx cy, dist = k1 k2 p1 p2
    k3 k4 k5 k6; SCARAMUZZA poly p0..p4, inv_poly p0..p19, affine = ac ad ae cx cy.  Fields a model does not use are not read."""
    _fields_ = [("model", C.c_int32), ("reserved", C.c_int32), ("proj", C.c_double * 4), ("dist", C.c_double * 8), ("xi", C.c_double),
                ("poly", C.c_double * 5), ("inv_poly", C.c_double * 20), ("affine", C.c_double * 5)]

    @classmethod
    def make(cls, model, proj=(0.0, 0.0, 0.0, 0.0), dist=(), xi=0.0, poly=(), inv_poly=(), affine=()):
        """model: CAMERA_* or its camodocal name; dist, poly, inv_poly and affine may be shorter than their fields (the rest is 0)"""
        m = cls()
        m.model = CAMERA_NAMES_EX[model] if isinstance(model, str) else int(model)
        m.proj[:] = [float(v) for v in proj]
        m.xi = float(xi)
        for field, vals in ((m.dist, dist), (m.poly, poly), (m.inv_poly, inv_poly), (m.affine, affine)):
            assert len(vals) <= len(field)
            for i, v in enumerate(vals):
                field[i] = float(v)
        return m

    @classmethod
    def of(cls, cam):
        """a CameraModel widened (a CameraModelEx as it is)"""
        if isinstance(cam, cls):
            return cam
        m = cls.make(cam.model, cam.proj, cam.dist, cam.xi)
        m.reserved = cam.reserved
        return m

    def as_dict(self):
        return {"model": self.model, "proj": list(self.proj), "dist": list(self.dist), "xi": self.xi, "poly": list(self.poly), "inv_poly": list(self.inv_poly),
                "affine": list(self.affine)}


assert C.sizeof(CameraModelEx) == 352


def _wide(cams):
    return any(isinstance(c, CameraModelEx) for c in cams)


def _camera_array(cams):
    """(gf_camera_model[n] or, if one of them is a CameraModelEx, gf_camera_model_ex[n]; the suffix of the entry points that take it)"""
    if _wide(cams):
        return (CameraModelEx * max(len(cams), 1))(*[CameraModelEx.of(c) for c in cams]), "_ex"
    return (CameraModel * max(len(cams), 1))(*cams), ""


def _camera_batch(cams, counts):
    """(camera array, first [batch + 1] int32, entry-point suffix) of a list of CameraModel / CameraModelEx and the sequences' point counts"""
    arr, ex = _camera_array(cams)
    first = np.zeros(len(cams) + 1, np.int32)
    first[1:] = np.cumsum(counts)
    return arr, first, ex


def camera_lift(cams, points, rays=True):
    """gf_camera_lift_batch: liftProjective of cams[b] on points[b] ([n_b, 2] float pixels) through the tracker's kernel -> (un, rays): lists of [n_b, 2] float32
    pairs (float)(P.x / P.z), (float)(P.y / P.z) and of [n_b, 3] float64 rays P (rays=False: None, the kernel writes none)"""
    pts = [np.ascontiguousarray(p, np.float32).reshape(-1, 2) for p in points]
    arr, first, ex = _camera_batch(cams, [len(p) for p in pts])
    uv = np.ascontiguousarray(np.concatenate(pts) if pts else np.zeros((0, 2)), np.float32)
    n = len(uv)
    un = np.zeros((n, 2), np.float32)
    ray = np.zeros((n, 3), np.float64) if rays else None
    _chk(getattr(lib(), "gf_camera_lift_batch" + ex)(arr, len(cams), _p(first, C.c_int), _p(uv, C.c_float), _p(ray, C.c_double) if rays else None, _p(un, C.c_float)))
    cut = lambda a: [a[first[b]:first[b + 1]] for b in range(len(cams))]
    return cut(un), (cut(ray) if rays else None)


def camera_lift_device(cams, counts, d_uv, d_rays, d_un, stream=0):
    """gf_camera_lift_batch_device: the same on device arrays (integer addresses; d_rays 0 / None: no rays); cams and the sequences' point counts stay on the host"""
    arr, first, ex = _camera_batch(cams, counts)
    _chk(getattr(lib(), "gf_camera_lift_batch_device" + ex)(arr, len(cams), _p(first, C.c_int), C.c_void_p(d_uv), C.c_void_p(d_rays) if d_rays else None, C.c_void_p(d_un),
                                                            C.c_void_p(stream) if stream else None))


def camera_project(cams, xyz):
    """gf_camera_project_batch: spaceToPlane of cams[b] on xyz[b] ([n_b, 3]) on the host -> list of [n_b, 2] float64 pixels"""
    pts = [np.ascontiguousarray(p, np.float64).reshape(-1, 3) for p in xyz]
    arr, first, ex = _camera_batch(cams, [len(p) for p in pts])
    flat = np.ascontiguousarray(np.concatenate(pts) if pts else np.zeros((0, 3)), np.float64)
    uv = np.zeros((len(flat), 2), np.float64)
    _chk(getattr(lib(), "gf_camera_project_batch" + ex)(arr, len(cams), _p(first, C.c_int), _p(flat, C.c_double), _p(uv, C.c_double)))
    return [uv[first[b]:first[b + 1]] for b in range(len(cams))]


class DepthReg(C.Structure):
    """gf_depth_reg: a raw depth stream and its pose relative to the colour camera -- width x height counts of `scale` metres through the pinhole fx fy cx cy,
    P_colour = R P_depth + T (R row-major, T in metres)"""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("scale", C.c_double), ("R", C.c_double * 9), ("T", C.c_double * 3)]

    @classmethod
    def make(cls, width, height, fx, fy, cx, cy, scale=0.001, R=(1, 0, 0, 0, 1, 0, 0, 0, 1), T=(0, 0, 0)):
        r = cls()
        r.width, r.height = int(width), int(height)
        r.fx, r.fy, r.cx, r.cy, r.scale = float(fx), float(fy), float(cx), float(cy), float(scale)
        r.R[:] = [float(v) for v in np.asarray(R, np.float64).reshape(-1)]
        r.T[:] = [float(v) for v in T]
        return r

    def as_dict(self):
        return {"width": self.width, "height": self.height, "fx": self.fx, "fy": self.fy, "cx": self.cx, "cy": self.cy, "scale": self.scale, "R": list(self.R), "T": list(self.T)}


assert C.sizeof(DepthReg) == 144


def _depth_reg_tables(regs, colours, colour_sizes):
    n = len(regs)
    assert len(colours) == n and len(colour_sizes) == n
    wh = np.ascontiguousarray(colour_sizes, np.int32).reshape(n, 2)
    arr, ex = _camera_array(colours)   # a CameraModelEx among them (PINHOLE_FULL colour cameras): the _ex entry points
    return (DepthReg * max(n, 1))(*regs), arr, wh, ex


def depth_register_device(src_refs, regs, colours, colour_sizes, dst_refs, stream=0):
    """gf_depth_register_batch_device: entry b's raw depth frame src_refs[b] = (device address, pitch) registered by regs[b] (DepthReg) to the colour camera colours[b]
    (a PINHOLE CameraModel, or a PINHOLE / PINHOLE_FULL CameraModelEx: one such entry takes the call to the _ex entry point) of colour_sizes[b] = (width, height) into dst_refs[b], which is written; two launches on `stream` whatever the batch, returns when they have run"""
    r, c, wh, ex = _depth_reg_tables(regs, colours, colour_sizes)
    assert len(src_refs) == len(regs) and len(dst_refs) == len(regs)
    _chk(getattr(lib(), "gf_depth_register_batch_device" + ex)(frame_refs(src_refs), r, c, _p(wh, C.c_int), frame_refs(dst_refs), len(regs), C.c_void_p(stream) if stream else None))


def depth_register(depths, regs, colours, colour_sizes):
    """gf_depth_register_batch: depths[b] ([height, width] u16, rows may be padded) registered by regs[b] to the PINHOLE or (CameraModelEx) PINHOLE_FULL colours[b] of colour_sizes[b] =
    (width, height), staged through device memory -> list of [height, width] u16 frames of the colour sizes"""
    r, c, wh, ex = _depth_reg_tables(regs, colours, colour_sizes)
    src = [d if (d.dtype == np.uint16 and d.ndim == 2 and d.strides[1] == 2 and d.strides[0] >= 2 * d.shape[1]) else np.ascontiguousarray(d, np.uint16) for d in depths]
    assert all(s.shape == (g.height, g.width) for s, g in zip(src, regs)), "a depth frame is not [height, width] of its registration"
    out = [np.zeros((int(h), int(w)), np.uint16) for w, h in wh]
    _chk(getattr(lib(), "gf_depth_register_batch" + ex)(frame_refs([(s.ctypes.data, s.strides[0]) for s in src]), r, c, _p(wh, C.c_int),
                                                        frame_refs([(o.ctypes.data, o.strides[0]) for o in out]), len(regs)))
    return out


REJECT_F_HYPOTHESES = 512   # GF_REJECT_F_HYPOTHESES
REJECT_F_MAX_PAIRS = 1024   # GF_REJECT_F_MAX_PAIRS


class RejectFCfg(C.Structure):
    """gf_reject_f_cfg: rejectWithF (feature_tracker.cpp:711-743) of a sequence -- the switch, the seed of the draws, F_threshold in virtual pixels and the
    virtual camera's FOCAL_LENGTH (0: 460)"""
    _fields_ = [("enable", C.c_int32), ("seed", C.c_uint32), ("f_threshold", C.c_double), ("focal_length", C.c_double)]

    def as_dict(self):
        return {"enable": self.enable, "seed": self.seed, "f_threshold": self.f_threshold, "focal_length": self.focal_length}


class RejectFResult(C.Structure):
    _fields_ = [("m", C.c_int32), ("rejected", C.c_int32), ("winner", C.c_int32), ("inliers", C.c_int32)]


class RejectFStats(C.Structure):
    _fields_ = [("launches", C.c_longlong), ("sequences", C.c_longlong), ("candidates", C.c_longlong), ("rejected", C.c_longlong), ("no_model", C.c_longlong),
                ("kernel_ms", C.c_double)]


assert C.sizeof(RejectFCfg) == 24 and C.sizeof(RejectFResult) == 16 and C.sizeof(RejectFStats) == 48


class StereoCfg(C.Structure):
    """gf_stereo_cfg: the stereo branch (feature_tracker.cpp:259-303) of a sequence -- the switch and the right camera"""
    _fields_ = [("enable", C.c_int32), ("reserved", C.c_int32), ("right", CameraModelEx)]


class StereoStats(C.Structure):
    _fields_ = [("calls", C.c_longlong), ("launches", C.c_longlong), ("points", C.c_longlong), ("matched", C.c_longlong), ("right_pyramids", C.c_longlong)]


assert C.sizeof(StereoCfg) == 360 and C.sizeof(StereoStats) == 40

# GF_STEREO_DEPTH_*: what became of a point, in the order the gates are tested
STEREO_DEPTH_WHY = {"no_match": 1, "lift": 2, "parallax": 3, "behind": 4, "epipolar": 5, "range": 6, "ok": 7}
STEREO_DEPTH_MIN_PARALLAX, STEREO_DEPTH_MAX_EPIPOLAR, STEREO_DEPTH_MIN_DEPTH = 1e-3, 10.0 / 460.0, 0.1   # the defaults of the gates ("Stereo depth")


class StereoDepthCfg(C.Structure):
    """gf_stereo_depth_cfg: the depth a stereo sequence's matches determine -- the switch, whether the camera_id 1 observations are still emitted, the rig
    p_left = R p_right + t (R row-major), and the gates: the sine of the least ray angle, the largest normalised-plane distance in the right eye, the depth range
    in metres (max_depth <= 65.535)"""
    _fields_ = [("enable", C.c_int32), ("right_obs", C.c_int32), ("R", C.c_double * 9), ("t", C.c_double * 3), ("min_parallax", C.c_double), ("max_epipolar", C.c_double),
                ("min_depth", C.c_double), ("max_depth", C.c_double)]

    @classmethod
    def make(cls, R, t, max_depth, min_depth=STEREO_DEPTH_MIN_DEPTH, min_parallax=STEREO_DEPTH_MIN_PARALLAX, max_epipolar=STEREO_DEPTH_MAX_EPIPOLAR, right_obs=1, enable=1):
        c = cls()
        c.enable, c.right_obs = int(enable), int(right_obs)
        c.R[:] = [float(v) for v in np.asarray(R, np.float64).reshape(9)]
        c.t[:] = [float(v) for v in np.asarray(t, np.float64).reshape(3)]
        c.min_parallax, c.max_epipolar, c.min_depth, c.max_depth = float(min_parallax), float(max_epipolar), float(min_depth), float(max_depth)
        return c

    def as_dict(self):
        return {"enable": self.enable, "right_obs": self.right_obs, "R": list(self.R), "t": list(self.t), "min_parallax": self.min_parallax,
                "max_epipolar": self.max_epipolar, "min_depth": self.min_depth, "max_depth": self.max_depth}


class StereoDepthStats(C.Structure):
    _fields_ = [(k, C.c_longlong) for k in ("calls", "launches", "points", "with_depth", "no_match", "lift", "parallax", "behind", "epipolar", "range")]


assert C.sizeof(StereoDepthCfg) == 136 and C.sizeof(StereoDepthStats) == 80


def _reject_f_tables(sets, thresholds, seeds):
    sets = [np.ascontiguousarray(s, np.float32).reshape(-1, 4) for s in sets]
    n = len(sets)
    first = np.zeros(n + 1, np.int32)
    first[1:] = np.cumsum([len(s) for s in sets])
    thr = np.ascontiguousarray(np.broadcast_to(np.asarray(thresholds, np.float64), (n,)))
    sd = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, np.uint32), (n,)))
    pairs = np.concatenate(sets) if n else np.zeros((0, 4), np.float32)
    return n, first, np.ascontiguousarray(pairs), thr, sd


def _reject_f_out(first, status, res):
    return ([status[first[b]:first[b + 1]].copy() for b in range(len(first) - 1)],
            [{"m": r.m, "rejected": r.rejected, "winner": r.winner, "inliers": r.inliers} for r in res])


def reject_f(sets, thresholds=1.0, seeds=0, host=False):
    """gf_reject_f_batch (host=True: gf_reject_f_batch_host, gfrf::reject without a device): sets[b] is [m_b, 4] float32 virtual-pixel pairs ax ay bx by
    (at most REJECT_F_MAX_PAIRS), with a threshold and a seed each (scalars are shared) -> (list of uint8 status arrays, list of result dicts)"""
    n, first, pairs, thr, sd = _reject_f_tables(sets, thresholds, seeds)
    status = np.zeros(max(int(first[-1]), 1), np.uint8)
    res = (RejectFResult * max(n, 1))()
    f = lib().gf_reject_f_batch_host if host else lib().gf_reject_f_batch
    _chk(f(n, _p(first, C.c_int), _p(pairs, C.c_float) if len(pairs) else None, _p(thr, C.c_double), _p(sd, C.c_uint), _p(status, C.c_uint8), res))
    return _reject_f_out(first, status, res)


def reject_f_device(counts, d_pairs, d_status, thresholds=1.0, seeds=0, stream=0):
    """gf_reject_f_batch_device: set b holds counts[b] pairs, back to back at the device address d_pairs (4 floats each); d_status (device address) gets a byte per
    pair.  One launch; returns the list of result dicts"""
    n = len(counts)
    first = np.zeros(n + 1, np.int32)
    first[1:] = np.cumsum(counts)
    thr = np.ascontiguousarray(np.broadcast_to(np.asarray(thresholds, np.float64), (n,)))
    sd = np.ascontiguousarray(np.broadcast_to(np.asarray(seeds, np.uint32), (n,)))
    res = (RejectFResult * max(n, 1))()
    _chk(lib().gf_reject_f_batch_device(n, _p(first, C.c_int), C.cast(C.c_void_p(d_pairs), C.POINTER(C.c_float)), _p(thr, C.c_double), _p(sd, C.c_uint),
                                        C.cast(C.c_void_p(d_status), C.POINTER(C.c_uint8)), res, C.c_void_p(stream) if stream else None))
    return [{"m": r.m, "rejected": r.rejected, "winner": r.winner, "inliers": r.inliers} for r in res[:n]]


def reject_f_pixels(cams, sizes, prev_uv, cur_uv, thresholds=1.0, focal_lengths=0.0, seeds=0, host=False):
    """gf_reject_f_pixels_batch (host=True: _host): set b is the pixel rows prev_uv[b], cur_uv[b] ([m_b, 2] float32) of a sizes[b] = (width, height) frame seen
    through cams[b] (CameraModel or CameraModelEx), lifted inside the kernel as the tracker's launch lifts them -> (list of uint8 status arrays, result dicts)"""
    n = len(cams)
    prev = [np.ascontiguousarray(p, np.float32).reshape(-1, 2) for p in prev_uv]
    cur = [np.ascontiguousarray(p, np.float32).reshape(-1, 2) for p in cur_uv]
    assert len(prev) == len(cur) == len(sizes) == n and all(len(a) == len(b) for a, b in zip(prev, cur))
    first = np.zeros(n + 1, np.int32)
    first[1:] = np.cumsum([len(p) for p in prev])
    bc = lambda v, t: np.ascontiguousarray(np.broadcast_to(np.asarray(v, t), (n,)))
    thr, foc, sd = bc(thresholds, np.float64), bc(focal_lengths, np.float64), bc(seeds, np.uint32)
    wh = np.ascontiguousarray(sizes, np.int32).reshape(-1)
    arr = (CameraModelEx * max(n, 1))(*[c if isinstance(c, CameraModelEx) else CameraModelEx.of(c) for c in cams])
    p, c = np.ascontiguousarray(np.concatenate(prev)), np.ascontiguousarray(np.concatenate(cur))
    status = np.zeros(max(int(first[-1]), 1), np.uint8)
    res = (RejectFResult * max(n, 1))()
    f = lib().gf_reject_f_pixels_batch_host if host else lib().gf_reject_f_pixels_batch
    _chk(f(n, _p(first, C.c_int), arr, _p(wh, C.c_int), _p(p, C.c_float), _p(c, C.c_float), _p(thr, C.c_double), _p(foc, C.c_double), _p(sd, C.c_uint), _p(status, C.c_uint8), res))
    return _reject_f_out(first, status, res)


def reject_f_from_yaml(config_file):
    """gf_reject_f_from_yaml: F_threshold and this repository's `reject_with_f` switch of a config file -> RejectFCfg"""
    c = RejectFCfg()
    _chk(lib().gf_reject_f_from_yaml(os.fsencode(config_file), C.byref(c)))
    return c


def stereo_from_yaml(config_file):
    """gf_stereo_from_yaml: `num_of_cam: 2` and `cam1_calib` of a config file -> StereoCfg (enable == 0 for any other num_of_cam)"""
    c = StereoCfg()
    _chk(lib().gf_stereo_from_yaml(os.fsencode(config_file), C.byref(c)))
    return c


def _stereo_depth_tables(left, right, cfgs, counts):
    n = len(left)
    assert len(right) == len(cfgs) == len(counts) == n
    first = np.zeros(n + 1, np.int32)
    first[1:] = np.cumsum(counts)
    wide = lambda cams: (CameraModelEx * max(n, 1))(*[CameraModelEx.of(c) for c in cams])
    return n, first, wide(left), wide(right), (StereoDepthCfg * max(n, 1))(*cfgs)


def stereo_depth(left, right, cfgs, left_uv, right_uv, status, host=False):
    """gf_stereo_depth_batch (host=True: gf_stereo_depth_batch_host, the same function on the CPU, no device): set b has the cameras left[b], right[b] (CameraModel /
    CameraModelEx), the rig and gates cfgs[b] (StereoDepthCfg), and the matches left_uv[b], right_uv[b] ([m_b, 2] float32 pixels) with status[b] ([m_b] bytes)
    -> (list of uint16 millimetre arrays, list of uint8 reason arrays, STEREO_DEPTH_WHY)"""
    l = [np.ascontiguousarray(p, np.float32).reshape(-1, 2) for p in left_uv]
    r = [np.ascontiguousarray(p, np.float32).reshape(-1, 2) for p in right_uv]
    st = [np.ascontiguousarray(s, np.uint8).reshape(-1) for s in status]
    assert all(len(a) == len(b) == len(c) for a, b, c in zip(l, r, st))
    n, first, la, ra, ca = _stereo_depth_tables(left, right, cfgs, [len(p) for p in l])
    cat = lambda v, shape, t: np.ascontiguousarray(np.concatenate(v) if v else np.zeros(shape, t))
    lu, ru, s = cat(l, (0, 2), np.float32), cat(r, (0, 2), np.float32), cat(st, (0,), np.uint8)
    rows = max(int(first[-1]), 1)
    mm, why = np.zeros(rows, np.uint16), np.zeros(rows, np.uint8)
    f = lib().gf_stereo_depth_batch_host if host else lib().gf_stereo_depth_batch
    _chk(f(n, _p(first, C.c_int), la, ra, ca, _p(lu, C.c_float), _p(ru, C.c_float), _p(s, C.c_uint8), _p(mm, C.c_uint16), _p(why, C.c_uint8)))
    cut = lambda a: [a[first[b]:first[b + 1]].copy() for b in range(n)]
    return cut(mm), cut(why)


def stereo_depth_host(left, right, cfgs, left_uv, right_uv, status):
    """gf_stereo_depth_batch_host: stereo_depth(..., host=True)"""
    return stereo_depth(left, right, cfgs, left_uv, right_uv, status, host=True)


def stereo_depth_device(left, right, cfgs, counts, d_left_uv, d_right_uv, d_status, d_depth_mm, d_why, stream=0):
    """gf_stereo_depth_batch_device: set b holds counts[b] matches, back to back at the device addresses d_left_uv / d_right_uv (2 floats each) and d_status (a
    byte each); d_depth_mm (uint16 each) and d_why (a byte each) are written.  One launch; cameras, configurations and counts stay on the host"""
    n, first, la, ra, ca = _stereo_depth_tables(left, right, cfgs, counts)
    fp = lambda a: C.cast(C.c_void_p(a), C.POINTER(C.c_float))
    _chk(lib().gf_stereo_depth_batch_device(n, _p(first, C.c_int), la, ra, ca, fp(d_left_uv), fp(d_right_uv), C.cast(C.c_void_p(d_status), C.POINTER(C.c_uint8)),
                                            C.cast(C.c_void_p(d_depth_mm), C.POINTER(C.c_uint16)), C.cast(C.c_void_p(d_why), C.POINTER(C.c_uint8)),
                                            C.c_void_p(stream) if stream else None))


def stereo_depth_from_yaml(config_file):
    """gf_stereo_depth_from_yaml: the rig inverse(body_T_cam0) * body_T_cam1, depth_threshold as max_depth and the default gates of a `num_of_cam: 2` config file
    -> StereoDepthCfg (enable == 0 for any other num_of_cam)"""
    c = StereoDepthCfg()
    _chk(lib().gf_stereo_depth_from_yaml(os.fsencode(config_file), C.byref(c)))
    return c


def camera_from_yaml(calib_file, cls=CameraModel):
    """gf_camera_from_yaml: a camodocal calibration file (PINHOLE, MEI, KANNALA_BRANDT) -> CameraModel; cls=CameraModelEx: gf_camera_from_yaml_ex, which also
    takes PINHOLE_FULL and SCARAMUZZA files -> CameraModelEx"""
    m = cls()
    _chk((lib().gf_camera_from_yaml_ex if cls is CameraModelEx else lib().gf_camera_from_yaml)(os.fsencode(calib_file), C.byref(m)))
    return m


OBS_DTYPE = np.dtype([("id", np.int32), ("camera_id", np.int32), ("v", np.float64, (8,))])
assert OBS_DTYPE.itemsize == C.sizeof(FeatureObs)

EXPORTS = ["gf_last_error", "gf_device_count", "gf_set_device", "gf_tracker_create", "gf_tracker_destroy", "gf_tracker_track",
           "gf_tracker_track_batch", "gf_tracker_track_batch_device", "gf_tracker_track_some", "gf_tracker_track_some_device", "gf_tracker_prefetch_some",
           "gf_tracker_track_some_device_refs", "gf_tracker_track_batch_device_refs", "gf_tracker_set_roi_some_device_refs", "gf_tracker_set_prediction", "gf_tracker_remove_outliers",
           "gf_tracker_set_roi", "gf_tracker_set_roi_some_device", "gf_tracker_get_roi",
           "gf_tracker_set_seq_cfg", "gf_tracker_get_seq_cfg", "gf_tracker_reset_seq",
           "gf_tracker_get_state", "gf_tracker_set_profiling", "gf_tracker_get_stats", "gf_tracker_reset_stats", "gf_lk_track",
           "gf_good_features", "gf_min_eigen_val", "gf_pyramid_level", "gf_clahe_batch", "gf_clahe_batch_device", "gf_cvt_gray_batch", "gf_cvt_gray_batch_device",
           "gf_tracker_set_show_track", "gf_tracker_track_image_some_device", "gf_tracker_track_image", "gf_draw_track_batch",
           "gf_estimator_set_show_track", "gf_estimator_get_track_image", "gf_show_track_from_yaml",
           "gf_tracker_set_boxes_some", "gf_tracker_get_boxes", "gf_roi_boxes_batch", "gf_estimator_set_boxes", "gf_draw_track_boxes_batch",
           "gf_tracker_set_seq_format", "gf_tracker_get_seq_format", "gf_cvt_gray_mixed", "gf_cvt_gray_mixed_device",
           "gf_tracker_set_seq_camera", "gf_tracker_get_seq_camera", "gf_camera_lift_batch", "gf_camera_lift_batch_device", "gf_camera_project_batch",
           "gf_camera_from_yaml", "gf_estimator_cfg_from_yaml_camera", "gf_estimator_set_camera",
           "gf_tracker_set_seq_camera_ex", "gf_tracker_get_seq_camera_ex", "gf_camera_lift_batch_ex", "gf_camera_lift_batch_device_ex", "gf_camera_project_batch_ex",
           "gf_camera_from_yaml_ex", "gf_estimator_cfg_from_yaml_camera_ex", "gf_estimator_set_camera_ex", "gf_depth_register_batch_ex", "gf_depth_register_batch_device_ex", "gf_tracker_get_camera_lift_stats",
           "gf_tracker_set_seq_size", "gf_tracker_get_seq_size",
           "gf_tracker_set_seq_depth_reg", "gf_tracker_get_seq_depth_reg", "gf_tracker_get_depth_reg_stats", "gf_depth_register_batch", "gf_depth_register_batch_device",
           "gf_tracker_set_seq_reject_f", "gf_tracker_get_seq_reject_f", "gf_tracker_get_reject_f_stats", "gf_reject_f_batch", "gf_reject_f_batch_device",
           "gf_reject_f_batch_host", "gf_reject_f_from_yaml", "gf_estimator_set_reject_f", "gf_reject_f_pixels_batch", "gf_reject_f_pixels_batch_host"]
MAX_SEQ_SIZES = 8   # GF_MAX_SEQ_SIZES


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise GfError("HIP extension %s is missing: run `python __graft_entry__.py` (build) first; there is no CPU fallback" % LIB_PATH)
        # torch bundles its own libamdhip64.so (SONAME libamdhip64.so.7, same as /opt/rocm's). Two HIP runtimes in
        # one process cannot both own the device, so let torch's copy load first; ours then binds to it by SONAME.
        if os.environ.get("GF_NO_TORCH_PRELOAD") != "1":
            try:
                import torch  # noqa: F401
            except Exception:
                pass
        _LIB = C.CDLL(LIB_PATH)
        _LIB.gf_last_error.restype = C.c_char_p
    return _LIB


def _chk(rc):
    if rc != 0:
        raise GfError("gf status %d: %s" % (rc, lib().gf_last_error().decode()))


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def device_count():
    n = C.c_int(0)
    lib().gf_device_count(C.byref(n))
    return n.value


def default_cfg(width=640, height=480, batch=1, max_cnt=150, min_dist=30, flow_back=1, depth_cam=1, equalize=0, pixel_format=0):
    return TrackerCfg(width, height, batch, max_cnt, min_dist, flow_back, depth_cam, 603.95556640625, 603.1257934570312,
                      324.0858154296875, 232.72303771972656, 0.0, 0.0, 0.0, 0.0, equalize, pixel_format)


class FeatureTracker:
    """`batch` independent FeatureTracker instances (feature_tracker.h:43-99) on one GPU.  The *Batch* calls advance all of them, the *Some* calls the
    sequences they list (the others keep their state); every per-sequence argument and result of a call is in list order."""

    def __init__(self, cfg=None):
        self.cfg = cfg or default_cfg()
        self.h = C.c_void_p()
        _chk(lib().gf_tracker_create(C.byref(self.cfg), C.byref(self.h)))
        self.cap = 4 * ((self.cfg.max_cnt + 3) // 4)
        self.channels = pix_bytes(self.cfg.pixel_format)   # a handle of a format with more than one byte per pixel takes [height, width, bytes] u8 frames wherever a MONO8 handle takes [height, width]
        self.row_bytes = self.cfg.width * self.channels
        self._fmt = {}   # set_seq_format: the sequences that have a format of their own, seq -> (pixel_format, equalize, host_stride)
        self._size = {}  # set_seq_size: the sequences that have a frame size of their own, seq -> (width, height)

    def close(self):
        if getattr(self, "h", None):
            lib().gf_tracker_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _unpack(self, out, n):
        res = []
        for b in range(len(n)):
            o = out[b, :n[b]]
            res.append((o["id"].copy(), o["v"].copy()))
        return res

    def trackImage(self, t, img, depth=None, seq=0):
        """one frame for sequence `seq` alone (gf_tracker_track; the other sequences of a batch handle keep their state): returns (ids, obs[n,8])."""
        return self.trackImageSome([seq], [t], [img], None if depth is None else [depth])[0]

    def _seqs(self, seqs):
        seqs = np.ascontiguousarray(seqs, np.int32).reshape(-1)
        return seqs, len(seqs)

    def trackImageSome(self, seqs, ts, imgs, depths=None, stride=None, dstride=None):
        """gf_tracker_track_some: one frame for each listed sequence, ts[i] / imgs[i] / depths[i] for sequence seqs[i]; returns [(ids, obs)] in list order.
        stride / dstride as in trackImageBatch"""
        seqs, N = self._seqs(seqs)
        ts = np.ascontiguousarray(ts, np.float64)
        assert len(ts) == N and len(imgs) == N and (depths is None or len(depths) == N)
        if self._fmt or self._size:   # formats / sizes per sequence (set_seq_format, set_seq_size): each frame in its sequence's own shape and row step
            imgs, stride = self._host_frames(seqs, imgs, stride)
            if self._size and depths is not None:
                depths, dstride = self._sized_depths(seqs, depths, dstride)
        else:
            imgs = [None if i is None else np.ascontiguousarray(i, np.uint8) if stride is None else self._pitched(i, np.uint8, stride) for i in imgs]
        gp = (C.POINTER(C.c_uint8) * max(N, 1))(*[None if i is None else _p(i, C.c_uint8) for i in imgs])
        if depths is not None:
            # (an entry may be None for a sequence whose own depth_cam is 0, set_seq_cfg: its image is not read)
            if not self._size:
                depths = [None if d is None else np.ascontiguousarray(d, np.uint16) if dstride is None else self._pitched(d, np.uint16, dstride) for d in depths]
            dp = (C.POINTER(C.c_uint16) * max(N, 1))(*[None if d is None else _p(d, C.c_uint16) for d in depths])
        else:
            dp = None
        out = np.zeros((N, self.cap), OBS_DTYPE)
        n = np.zeros(N, np.int32)
        _chk(lib().gf_tracker_track_some(self.h, N, _p(seqs, C.c_int), _p(ts, C.c_double), gp, stride or self.row_bytes, dp, dstride or self.cfg.width,
                                         out.ctypes.data_as(C.POINTER(FeatureObs)), self.cap, _p(n, C.c_int)))
        return self._unpack(out, n)

    def trackImageSomeDevice(self, seqs, ts, d_gray_ptr, d_depth_ptr=None, unpack=True, out=None, n_out=None):
        """gf_tracker_track_some_device: d_*_ptr = integer device addresses of len(seqs) contiguous frames, frame i for sequence seqs[i].  out / n_out: the caller's
        [>= len(seqs)][cap] OBS_DTYPE table and int32 counts (rows in list order: the table gf_estimator_group_submit_features reads with the same list);
        default: the tracker's own pair."""
        seqs, N = self._seqs(seqs)
        ts = np.ascontiguousarray(ts, np.float64)
        assert len(ts) == N
        if out is None:
            if not hasattr(self, "_out"):
                self._out = np.zeros((self.cfg.batch, self.cap), OBS_DTYPE)
                self._n = np.zeros(self.cfg.batch, np.int32)
            out, n_out = self._out, self._n
        # (a list longer than the batch is the library's to refuse: it checks the list before it touches the tables)
        assert out.ndim == 2 and out.shape[0] >= min(N, self.cfg.batch) and out.shape[1] == self.cap and out.dtype == OBS_DTYPE and out.flags.c_contiguous
        assert n_out.shape[0] >= min(N, self.cfg.batch) and n_out.dtype == np.int32 and n_out.flags.c_contiguous
        _chk(lib().gf_tracker_track_some_device(self.h, N, _p(seqs, C.c_int), _p(ts, C.c_double), C.c_void_p(d_gray_ptr),
                                                C.c_void_p(d_depth_ptr) if d_depth_ptr else None,
                                                out.ctypes.data_as(C.POINTER(FeatureObs)), self.cap, _p(n_out, C.c_int)))
        return self._unpack(out, n_out[:N]) if unpack else n_out[:N]

    def trackImageSomeDeviceRefs(self, seqs, ts, gray_refs, depth_refs=None, unpack=True, out=None, n_out=None):
        """gf_tracker_track_some_device_refs: gray_refs[i] = (device address of row 0, bytes from row to row) of the frame of sequence seqs[i], wherever it lies
        and however it is aligned (its own allocation, the luma plane of an NV12 surface, a crop); depth_refs likewise for u16 depth frames (None: no depth; an
        entry None for a sequence whose own depth_cam is 0).  Nothing behind a ref is written.  unpack / out / n_out as trackImageSomeDevice."""
        seqs, N = self._seqs(seqs)
        ts = np.ascontiguousarray(ts, np.float64)
        assert len(ts) == N and (gray_refs is None or len(gray_refs) == N) and (depth_refs is None or len(depth_refs) == N)
        if out is None:
            if not hasattr(self, "_out"):
                self._out = np.zeros((self.cfg.batch, self.cap), OBS_DTYPE)
                self._n = np.zeros(self.cfg.batch, np.int32)
            out, n_out = self._out, self._n
        assert out.ndim == 2 and out.shape[0] >= min(N, self.cfg.batch) and out.shape[1] == self.cap and out.dtype == OBS_DTYPE and out.flags.c_contiguous
        assert n_out.shape[0] >= min(N, self.cfg.batch) and n_out.dtype == np.int32 and n_out.flags.c_contiguous
        _chk(lib().gf_tracker_track_some_device_refs(self.h, N, _p(seqs, C.c_int), _p(ts, C.c_double), None if gray_refs is None else frame_refs(gray_refs),
                                                     None if depth_refs is None else frame_refs(depth_refs),
                                                     out.ctypes.data_as(C.POINTER(FeatureObs)), self.cap, _p(n_out, C.c_int)))
        return self._unpack(out, n_out[:N]) if unpack else n_out[:N]

    def trackImageBatchDeviceRefs(self, ts, gray_refs, depth_refs=None, unpack=True, out=None, n_out=None):
        """gf_tracker_track_batch_device_refs: trackImageSomeDeviceRefs for every sequence, refs in sequence order"""
        B = self.cfg.batch
        ts = np.ascontiguousarray(ts, np.float64)
        assert len(ts) == B and len(gray_refs) == B and (depth_refs is None or len(depth_refs) == B)
        if out is None:
            if not hasattr(self, "_out"):
                self._out = np.zeros((B, self.cap), OBS_DTYPE)
                self._n = np.zeros(B, np.int32)
            out, n_out = self._out, self._n
        assert out.shape == (B, self.cap) and out.dtype == OBS_DTYPE and out.flags.c_contiguous and n_out.shape == (B,) and n_out.dtype == np.int32
        _chk(lib().gf_tracker_track_batch_device_refs(self.h, _p(ts, C.c_double), frame_refs(gray_refs), None if depth_refs is None else frame_refs(depth_refs),
                                                      out.ctypes.data_as(C.POINTER(FeatureObs)), self.cap, _p(n_out, C.c_int)))
        return self._unpack(out, n_out) if unpack else n_out

    def _pitched(self, a, dtype, pitch):
        """a height x width image whose rows lie `pitch` elements apart (a view of a wider array, e.g. a cropped frame): passed as it is, not copied"""
        if dtype == np.uint8 and self.channels > 1:   # colour rows: [height, width, channels], `pitch` bytes from row to row
            assert a.dtype == dtype and a.shape == (self.cfg.height, self.cfg.width, self.channels) and a.strides == (pitch, self.channels, 1), (a.shape, a.strides, pitch)
            return a
        assert a.dtype == dtype and a.shape == (self.cfg.height, self.cfg.width) and a.strides == (pitch * a.itemsize, a.itemsize), (a.shape, a.strides, pitch)
        return a

    def trackImageBatch(self, ts, imgs, depths=None, stride=None, dstride=None):
        """stride / dstride: row pitch of the gray (bytes) / depth (u16 elements) images, for frames with padded rows (cv::Mat::step); default: contiguous rows"""
        B = self.cfg.batch
        if self._fmt or self._size:   # formats / sizes per sequence: the list form with every sequence listed takes each frame in its own shape
            return self.trackImageSome(range(B), ts, imgs, depths, stride, dstride)
        ts = np.ascontiguousarray(ts, np.float64)
        imgs = [np.ascontiguousarray(i, np.uint8) for i in imgs] if stride is None else [self._pitched(i, np.uint8, stride) for i in imgs]
        gp = (C.POINTER(C.c_uint8) * B)(*[_p(i, C.c_uint8) for i in imgs])
        if depths is not None:
            depths = [np.ascontiguousarray(d, np.uint16) for d in depths] if dstride is None else [self._pitched(d, np.uint16, dstride) for d in depths]
            dp = (C.POINTER(C.c_uint16) * B)(*[_p(d, C.c_uint16) for d in depths])
        else:
            dp = None
        out = np.zeros((B, self.cap), OBS_DTYPE)
        n = np.zeros(B, np.int32)
        _chk(lib().gf_tracker_track_batch(self.h, _p(ts, C.c_double), gp, stride or self.row_bytes, dp, dstride or self.cfg.width,
                                          out.ctypes.data_as(C.POINTER(FeatureObs)), self.cap, _p(n, C.c_int)))
        return self._unpack(out, n)

    def trackImageBatchDevice(self, ts, d_gray_ptr, d_depth_ptr=None, unpack=True, out=None, n_out=None):
        """d_*_ptr: integer device addresses (e.g. torch tensor .data_ptr()) of batch contiguous frames.  out / n_out: the caller's [batch][cap] OBS_DTYPE table
        and [batch] int32 counts to write into (e.g. one of a ring, while estimators still read the previous frames' tables); default: the tracker's own pair.
        On a handle with sizes or formats per sequence the frames do NOT lie one handle-sized frame apart: frame b has its own height x width x bytes per pixel
        and starts where the frames before it end (device_frame_offsets(), device_size_offsets(itemsize=2) for depth), as in trackImageSomeDevice, which serves the call then."""
        B = self.cfg.batch
        if self._size:
            return self.trackImageSomeDevice(range(B), ts, d_gray_ptr, d_depth_ptr, unpack, out, n_out)
        ts = np.ascontiguousarray(ts, np.float64)
        if out is None:
            if not hasattr(self, "_out"):
                self._out = np.zeros((B, self.cap), OBS_DTYPE)
                self._n = np.zeros(B, np.int32)
            out, n_out = self._out, self._n
        assert out.shape == (B, self.cap) and out.dtype == OBS_DTYPE and out.flags.c_contiguous and n_out.shape == (B,) and n_out.dtype == np.int32
        _chk(lib().gf_tracker_track_batch_device(self.h, _p(ts, C.c_double), C.c_void_p(d_gray_ptr),
                                                 C.c_void_p(d_depth_ptr) if d_depth_ptr else None,
                                                 out.ctypes.data_as(C.POINTER(FeatureObs)), self.cap, _p(n_out, C.c_int)))
        return self._unpack(out, n_out) if unpack else n_out

    def prefetchHost(self, gray_addr, depth_addr=None, stride=None, dstride=None, seqs=None):
        """gf_tracker_prefetch_batch on a block of `batch` frames lying back to back in (page-locked) host memory: gray_addr / depth_addr = integer host addresses
        of batch x height x width u8 / u16 images; the copy runs on the tracker's copy stream while the frame in flight is processed.  gray_addr / depth_addr may
        also be lists of `batch` addresses (one image each, anywhere).  stride / dstride: row pitch in bytes / u16 elements (default: the width).
        seqs: gf_tracker_prefetch_some -- the frames (len(seqs) of them, block or list alike) belong to the listed sequences, and the matching trackPrefetched
        advances those alone, its ts and results in the same order"""
        B, H = self.cfg.batch, self.cfg.height
        stride, dstride = stride or self.row_bytes, dstride or self.cfg.width
        if seqs is not None:
            seqs, B = self._seqs(seqs)
        # sizes per sequence: the frames of a block would not lie one stride x height apart -- one address per frame, each of its own height, rows stride apart
        assert not self._size or (isinstance(gray_addr, (list, tuple)) and (not depth_addr or isinstance(depth_addr, (list, tuple))))
        self._pf_n = getattr(self, "_pf_n", []) + [B]
        ga = list(gray_addr) if isinstance(gray_addr, (list, tuple)) else [gray_addr + b * stride * H for b in range(B)]
        gp = (C.POINTER(C.c_uint8) * B)(*[C.cast(a, C.POINTER(C.c_uint8)) for a in ga])
        if depth_addr:
            da = list(depth_addr) if isinstance(depth_addr, (list, tuple)) else [depth_addr + 2 * b * dstride * H for b in range(B)]
            dp = (C.POINTER(C.c_uint16) * B)(*[C.cast(a, C.POINTER(C.c_uint16)) for a in da])
        else:
            dp = None
        try:
            if seqs is None:
                _chk(lib().gf_tracker_prefetch_batch(self.h, gp, stride, dp, dstride))
            else:
                _chk(lib().gf_tracker_prefetch_some(self.h, B, _p(seqs, C.c_int), gp, stride, dp, dstride))
        except GfError:
            self._pf_n.pop()
            raise

    def trackPrefetched(self, ts, unpack=True):
        B = self.cfg.batch
        N = self._pf_n.pop(0) if getattr(self, "_pf_n", None) else B   # sequences of the oldest staged frame
        ts = np.ascontiguousarray(ts, np.float64)
        assert len(ts) == N
        if not hasattr(self, "_out"):
            self._out = np.zeros((B, self.cap), OBS_DTYPE)
            self._n = np.zeros(B, np.int32)
        _chk(lib().gf_tracker_track_prefetched(self.h, _p(ts, C.c_double), self._out.ctypes.data_as(C.POINTER(FeatureObs)), self.cap, _p(self._n, C.c_int)))
        return self._unpack(self._out, self._n[:N]) if unpack else self._n[:N]

    def setPrediction(self, ids, xyz, seq=0):
        ids = np.ascontiguousarray(ids, np.int32)
        xyz = np.ascontiguousarray(xyz, np.float64)
        _chk(lib().gf_tracker_set_prediction(self.h, seq, _p(ids, C.c_int), _p(xyz, C.c_double), len(ids)))

    def removeOutliers(self, ids, seq=0):
        ids = np.ascontiguousarray(ids, np.int32)
        _chk(lib().gf_tracker_remove_outliers(self.h, seq, _p(ids, C.c_int), len(ids)))

    def set_roi(self, mask, seq=0):
        """gf_tracker_set_roi: the region of interest of sequence `seq` from a [height, width] u8 image (non-zero = allowed; its rows may be pitched), None clears.
        It stays until replaced or cleared and holds from the sequence's next frame on, through every entry point."""
        if mask is None:
            _chk(lib().gf_tracker_set_roi(self.h, seq, None, 0))
            return
        mask = np.asarray(mask)
        w, h = self.seq_size(seq)   # the sequence's own frame (set_seq_size)
        assert mask.dtype == np.uint8 and mask.shape == (h, w), (mask.dtype, mask.shape)
        if mask.strides[1] != 1 or mask.strides[0] < w:
            mask = np.ascontiguousarray(mask)
        _chk(lib().gf_tracker_set_roi(self.h, seq, _p(mask, C.c_uint8), mask.strides[0]))

    def set_roi_device(self, seqs, d_masks_ptr, nbytes=None):
        """gf_tracker_set_roi_some_device: d_masks_ptr = integer device address of len(seqs) tight [height, width] u8 masks back to back, mask i for sequence
        seqs[i] (complete when the call is made); None / 0 clears the listed sequences.  On a handle with sizes per sequence (set_seq_size) every mask has its
        sequence's own size and starts where the masks before it end (device_size_offsets).  The library cannot tell a block laid out otherwise -- at the handle's
        size, say -- from a right one: a pointer carries no size.  nbytes: the bytes the caller's block holds; a check of this wrapper alone, ValueError unless
        it is the sum of the listed masks"""
        seqs, N = self._seqs(seqs)
        if d_masks_ptr and nbytes is not None and nbytes != self.device_size_offsets(seqs)[1]:
            raise ValueError("a block of %d bytes where the masks of the listed sequences, each of its own size, add up to %d" % (nbytes, self.device_size_offsets(seqs)[1]))
        _chk(lib().gf_tracker_set_roi_some_device(self.h, N, _p(seqs, C.c_int), C.c_void_p(d_masks_ptr) if d_masks_ptr else None))

    def set_roi_device_refs(self, seqs, mask_refs):
        """gf_tracker_set_roi_some_device_refs: mask_refs[i] = (device address of row 0, bytes from row to row) of the [height, width] u8 mask of sequence
        seqs[i], e.g. a crop of a larger tensor (complete when the call is made); None clears the listed sequences"""
        seqs, N = self._seqs(seqs)
        assert mask_refs is None or len(mask_refs) == N
        _chk(lib().gf_tracker_set_roi_some_device_refs(self.h, N, _p(seqs, C.c_int), None if mask_refs is None else frame_refs(mask_refs)))

    def get_roi(self, seq=0):
        """gf_tracker_get_roi: the stored region of sequence `seq` as a [height, width] u8 image of 0 / 255, or None if it has none"""
        w, h = self.seq_size(seq)
        mask = np.zeros((h, w), np.uint8)
        has = C.c_int(0)
        _chk(lib().gf_tracker_get_roi(self.h, seq, _p(mask, C.c_uint8), w, C.byref(has)))
        return mask if has.value else None

    def set_boxes(self, boxes, seq=0):
        """gf_tracker_set_boxes_some for one sequence: its exclusion boxes (rows of xmin, ymin, xmax, ymax) from its next frame on; None or an empty list clears"""
        self.set_boxes_some([seq], [boxes])

    def set_boxes_some(self, seqs, lists):
        """gf_tracker_set_boxes_some: lists[i] = the boxes of sequence seqs[i] (an empty one clears it); lists=None clears every listed sequence.  The region in
        force is the region of set_roi minus the boxes; no synchronisation, the composition runs on the handle's stream ahead of the next frame."""
        seqs, N = self._seqs(seqs)
        if lists is None:
            _chk(lib().gf_tracker_set_boxes_some(self.h, N, _p(seqs, C.c_int), None, None))
            return
        assert len(lists) == N
        first, flat = _box_lists(lists)
        _chk(lib().gf_tracker_set_boxes_some(self.h, N, _p(seqs, C.c_int), _p(first, C.c_int), flat.ctypes.data_as(C.POINTER(Box)) if len(flat) else None))

    def get_boxes(self, seq=0):
        """gf_tracker_get_boxes: the boxes in force for sequence `seq`, [n, 4] int32"""
        out = np.zeros((MAX_BOXES_PER_SEQ, 4), np.int32)
        n = C.c_int(0)
        _chk(lib().gf_tracker_get_boxes(self.h, seq, out.ctypes.data_as(C.POINTER(Box)), MAX_BOXES_PER_SEQ, C.byref(n)))
        return out[:n.value].copy()

    def set_seq_cfg(self, seq, **fields):
        """gf_tracker_set_seq_cfg: sequence `seq` gets parameters of its own -- any of max_cnt, min_dist, flow_back, depth_cam, fx, fy, cx, cy, k1, k2, p1, p2; the
        fields that are not named keep the value in force.  Without fields: back to the handle's cfg.  Refused (GfError) once the sequence has taken a frame,
        until reset_seq, and outside the handle's capacity (max_cnt <= cfg.max_cnt, min_dist >= cfg.min_dist)."""
        if not fields:
            _chk(lib().gf_tracker_set_seq_cfg(self.h, seq, None))
            return
        names = [k for k, _ in TrackerSeqCfg._fields_]
        unknown = [k for k in fields if k not in names]
        if unknown:
            raise TypeError("gf_tracker_seq_cfg has no field %s" % ", ".join(unknown))
        c = TrackerSeqCfg()
        _chk(lib().gf_tracker_get_seq_cfg(self.h, seq, C.byref(c)))
        for k, v in fields.items():
            setattr(c, k, v)
        _chk(lib().gf_tracker_set_seq_cfg(self.h, seq, C.byref(c)))

    def set_seq_camera(self, seq, camera):
        """gf_tracker_set_seq_camera: sequence `seq` gets the camera `camera` (CameraModel): its lift and its projection are that model's.  Refused (GfError) once
        the sequence has taken a frame, until reset_seq, and while a prefetched frame lists it."""
        _chk((lib().gf_tracker_set_seq_camera_ex if isinstance(camera, CameraModelEx) else lib().gf_tracker_set_seq_camera)(self.h, seq, C.byref(camera)))

    def get_seq_camera(self, seq, cls=CameraModel):
        """gf_tracker_get_seq_camera: the camera in force for sequence `seq` (the pinhole of its parameters ahead of any setter); cls=CameraModelEx:
        gf_tracker_get_seq_camera_ex, which alone can hand back a PINHOLE_FULL or SCARAMUZZA camera"""
        m = cls()
        _chk((lib().gf_tracker_get_seq_camera_ex if cls is CameraModelEx else lib().gf_tracker_get_seq_camera)(self.h, seq, C.byref(m)))
        return m

    def set_seq_depth_reg(self, seq, reg):
        """gf_tracker_set_seq_depth_reg: sequence `seq` gets the depth registration `reg` (DepthReg; None clears it): on trackImageSomeDeviceRefs /
        trackImageBatchDeviceRefs its depth ref is the RAW frame of the depth camera, registered to its colour camera on the device ahead of the depth samples;
        every other frame-taking method refuses it with depth.  Refused (GfError) once the sequence has taken a frame, until reset_seq, while a prefetched frame
        lists it, and while its camera is no PINHOLE."""
        _chk(lib().gf_tracker_set_seq_depth_reg(self.h, int(seq), None if reg is None else C.byref(reg)))

    def get_seq_depth_reg(self, seq):
        """gf_tracker_get_seq_depth_reg: the DepthReg of sequence `seq`, None if it has none"""
        r, has = DepthReg(), C.c_int(0)
        _chk(lib().gf_tracker_get_seq_depth_reg(self.h, int(seq), C.byref(r), C.byref(has)))
        return r if has.value else None

    def set_seq_reject_f(self, seq, cfg=None, **fields):
        """gf_tracker_set_seq_reject_f: rejectWithF (feature_tracker.cpp:711-743) of sequence `seq`: a RejectFCfg, or its fields by name (f_threshold=1.0,
        seed=0, focal_length=0 for 460; enable defaults to 1); None with no fields turns it off.  Allowed between frames at any time; refused (GfError) for a bad
        threshold and while a prefetched frame lists the sequence."""
        if cfg is None and fields:
            cfg = RejectFCfg(int(fields.pop("enable", 1)), int(fields.pop("seed", 0)), float(fields.pop("f_threshold", 1.0)), float(fields.pop("focal_length", 0.0)))
            if fields:
                raise TypeError("unknown RejectFCfg fields: %s" % sorted(fields))
        _chk(lib().gf_tracker_set_seq_reject_f(self.h, int(seq), None if cfg is None else C.byref(cfg)))

    def get_seq_reject_f(self, seq):
        """gf_tracker_get_seq_reject_f: the RejectFCfg of sequence `seq` (enable == 0: off)"""
        c = RejectFCfg()
        _chk(lib().gf_tracker_get_seq_reject_f(self.h, int(seq), C.byref(c)))
        return c

    def reject_f_stats(self):
        """gf_tracker_get_reject_f_stats: dict of launches, sequences, candidates, rejected, no_model, kernel_ms"""
        s = RejectFStats()
        _chk(lib().gf_tracker_get_reject_f_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in RejectFStats._fields_}

    def set_seq_stereo(self, seq, right=None):
        """gf_tracker_set_seq_stereo: sequence `seq` gets a right camera (a CameraModel / CameraModelEx, or a StereoCfg) and with it the stereo branch of trackImage
        (feature_tracker.cpp:259-303); None turns it off.  Before the sequence's first frame.  Its right frame is the second gf_frame_ref of its list position
        on trackImageSomeDeviceRefs / trackImageBatchDeviceRefs.  A frame of a stereo sequence returns up to two observations per feature, so the first call that
        turns a switch on DOUBLES self.cap, the row length of every `out` array (one allocated before with the old g.cap no longer fits: allocate after the
        setters).  The unpacked form (ids, obs) of the frame-taking methods carries no camera id: the right observations are the rows behind the first occurrence
        of a repeated id; with unpack=False, out[i]["camera_id"] tells the eyes apart."""
        cfg = right if isinstance(right, StereoCfg) or right is None else StereoCfg(1, 0, CameraModelEx.of(right))
        _chk(lib().gf_tracker_set_seq_stereo(self.h, int(seq), None if cfg is None else C.byref(cfg)))
        if cfg is not None and cfg.enable and not getattr(self, "_stereo", False):   # a frame of a stereo sequence returns up to two observations per feature
            self._stereo, self.cap = True, 2 * self.cap
            for name in ("_out", "_n"):
                if hasattr(self, name):
                    delattr(self, name)

    def get_seq_stereo(self, seq):
        """gf_tracker_get_seq_stereo: the StereoCfg of sequence `seq` (enable == 0: off)"""
        c = StereoCfg()
        _chk(lib().gf_tracker_get_seq_stereo(self.h, int(seq), C.byref(c)))
        return c

    def stereo_stats(self):
        """gf_tracker_get_stereo_stats: dict of calls, launches, points, matched, right_pyramids"""
        s = StereoStats()
        _chk(lib().gf_tracker_get_stereo_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in StereoStats._fields_}

    def set_seq_stereo_depth(self, seq, cfg=None):
        """gf_tracker_set_seq_stereo_depth: the left observations of stereo sequence `seq` carry the depth its matches determine (a StereoDepthCfg; None turns it
        off).  Before the sequence's first frame, after set_seq_stereo.  With cfg.right_obs == 0 the camera_id 1 observations are not emitted."""
        _chk(lib().gf_tracker_set_seq_stereo_depth(self.h, int(seq), None if cfg is None else C.byref(cfg)))

    def get_seq_stereo_depth(self, seq):
        """gf_tracker_get_seq_stereo_depth: the StereoDepthCfg of sequence `seq` (enable == 0: off)"""
        c = StereoDepthCfg()
        _chk(lib().gf_tracker_get_seq_stereo_depth(self.h, int(seq), C.byref(c)))
        return c

    def stereo_depth_stats(self):
        """gf_tracker_get_stereo_depth_stats: dict of calls, launches, points, with_depth and a count per reason"""
        s = StereoDepthStats()
        _chk(lib().gf_tracker_get_stereo_depth_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in StereoDepthStats._fields_}

    def camera_lift_stats(self):
        """gf_tracker_get_camera_lift_stats: dict of launches of camera_lift_kernel by this handle and of the listed sequences they lifted"""
        n, q = C.c_longlong(0), C.c_longlong(0)
        _chk(lib().gf_tracker_get_camera_lift_stats(self.h, C.byref(n), C.byref(q)))
        return {"launches": n.value, "sequences": q.value}

    def depth_reg_stats(self):
        """gf_tracker_get_depth_reg_stats: dict of launches (two per call that registered a frame), frames, kernel_ms (hipEvent time of the two kernels, summed)"""
        n, f, ms = C.c_longlong(0), C.c_longlong(0), C.c_double(0)
        _chk(lib().gf_tracker_get_depth_reg_stats(self.h, C.byref(n), C.byref(f), C.byref(ms)))
        return {"launches": n.value, "frames": f.value, "kernel_ms": ms.value}

    def set_seq_format(self, seq, pixel_format=None, equalize=None, host_stride=0):
        """gf_tracker_set_seq_format: sequence `seq` takes frames of `pixel_format` (PIX_*) and is equalised or not, whatever the handle's cfg says; a field left
        None keeps the value in force, host_stride = bytes per row of its host frames (0: the call's stride).  Without pixel_format and equalize: back to the
        handle's cfg.  From then on the frame-taking methods take, for that sequence, an array of its format's shape: [h, w], [h, w, bytes], u16 [h, w] for MONO16.
        Refused (GfError) once the sequence has taken a frame, until reset_seq, and while a prefetched frame is waiting."""
        if pixel_format is None and equalize is None and not host_stride:
            _chk(lib().gf_tracker_set_seq_format(self.h, seq, None))
            self._fmt.pop(int(seq), None)
            return
        f = TrackerSeqFormat()
        _chk(lib().gf_tracker_get_seq_format(self.h, seq, C.byref(f)))
        if pixel_format is not None:
            f.pixel_format = int(pixel_format)
        if equalize is not None:
            f.equalize = int(equalize)
        f.host_stride = int(host_stride)
        _chk(lib().gf_tracker_set_seq_format(self.h, seq, C.byref(f)))
        self._fmt[int(seq)] = (f.pixel_format, f.equalize, f.host_stride)

    def get_seq_format(self, seq):
        """gf_tracker_get_seq_format: what is in force for sequence `seq`, as a dict of pixel_format, equalize, host_stride"""
        f = TrackerSeqFormat()
        _chk(lib().gf_tracker_get_seq_format(self.h, seq, C.byref(f)))
        return {k: getattr(f, k) for k, _ in TrackerSeqFormat._fields_}

    def set_seq_size(self, seq, width, height):
        """gf_tracker_set_seq_size: sequence `seq` takes frames of width x height (<= the handle's, which is the capacity); (0, 0): back to the handle's size.
        From then on the frame-taking methods take, for that sequence, [height, width] u8 frames and u16 depth images.  Refused (GfError) once the sequence has
        taken a frame, until reset_seq, while a prefetched frame lists it, and while it has a region of interest."""
        _chk(lib().gf_tracker_set_seq_size(self.h, int(seq), int(width), int(height)))
        w, h = self.get_seq_size(seq)
        if (w, h) == (self.cfg.width, self.cfg.height):
            self._size.pop(int(seq), None)
        else:
            self._size[int(seq)] = (w, h)

    def get_seq_size(self, seq):
        """gf_tracker_get_seq_size: (width, height) in force for sequence `seq` (the handle's unless set_seq_size gave it its own)"""
        w, h = C.c_int(0), C.c_int(0)
        _chk(lib().gf_tracker_get_seq_size(self.h, int(seq), C.byref(w), C.byref(h)))
        return w.value, h.value

    def seq_size(self, seq):
        """(width, height) of sequence `seq` as the frame-taking methods expect its arrays"""
        return self._size.get(int(seq), (self.cfg.width, self.cfg.height))

    def device_size_offsets(self, seqs=None, itemsize=1):
        """the layout of the tight device entry points on a handle with sizes per sequence: (byte offset of the frame of each listed sequence, total bytes) --
        frame i has its own height x width x itemsize bytes (1: masks, 2: depth; gray frames: device_frame_offsets, which knows their formats) and starts where
        the frames listed before it end"""
        seqs = range(self.cfg.batch) if seqs is None else seqs
        sizes = [self.seq_size(q)[0] * self.seq_size(q)[1] * itemsize for q in seqs]
        offs = [int(o) for o in np.concatenate([[0], np.cumsum(sizes)])]
        return offs[:-1], offs[-1]

    def _sized_depths(self, seqs, depths, dstride):
        """the depth images of a list on a handle with sizes per sequence: every image u16 [h, w] of its own sequence, its rows the call's dstride (u16 elements;
        default: the widest listed row) apart; an image whose rows lie otherwise is copied into one that fits"""
        shapes = [self.seq_size(q) for q in seqs]
        dstride = dstride or max([w for w, _ in shapes] + [1])
        out = []
        for (w, h), d in zip(shapes, depths):
            if d is None:
                out.append(None)
                continue
            d = np.asarray(d)
            if d.dtype != np.uint16 or d.shape != (h, w):
                raise ValueError("a depth image of shape %s %s where its sequence takes u16 [%d, %d]" % (d.shape, d.dtype, h, w))
            if d.strides != (2 * dstride, 2) and dstride >= w:
                buf = np.zeros((h, dstride), np.uint16)
                buf[:, :w] = d
                d = buf[:, :w]
            out.append(d)
        return out, dstride

    def seq_pixel_format(self, seq):
        """the pixel format in force for sequence `seq` (the handle's own unless set_seq_format gave it one)"""
        return self._fmt.get(int(seq), (self.cfg.pixel_format,))[0]

    def device_frame_offsets(self, seqs=None):
        """the layout of the tight device entry points on a handle with formats per sequence: (byte offset of the frame of each listed sequence, total bytes) --
        frame i has height x width x bytes per pixel of seqs[i] bytes and starts where the frames listed before it end"""
        seqs = range(self.cfg.batch) if seqs is None else seqs
        sizes = [self.seq_size(q)[0] * self.seq_size(q)[1] * pix_bytes(self.seq_pixel_format(q)) for q in seqs]
        offs = [int(o) for o in np.concatenate([[0], np.cumsum(sizes)])]
        return offs[:-1], offs[-1]

    def _host_frames(self, seqs, imgs, stride):
        """the host frames of a list on a handle with formats per sequence: each as u8 rows that lie its sequence's host_stride apart, or the call's stride
        (default: the widest listed row) where it has none; a frame whose rows lie otherwise is copied into one that fits"""
        rows = [None if i is None else _frame_rows(i, self.seq_pixel_format(q), *self.seq_size(q)) for q, i in zip(seqs, imgs)]
        own = [self._fmt.get(int(q), (0, 0, 0))[2] for q in seqs]
        if stride is None:
            stride = max([r.shape[1] for r, o in zip(rows, own) if r is not None and not o] + [self.cfg.width])
        return [None if r is None else _with_pitch(r, o or stride) for r, o in zip(rows, own)], stride

    def get_seq_cfg(self, seq):
        """gf_tracker_get_seq_cfg: the parameters in force for sequence `seq`, as a dict of the twelve fields"""
        c = TrackerSeqCfg()
        _chk(lib().gf_tracker_get_seq_cfg(self.h, seq, C.byref(c)))
        return {k: getattr(c, k) for k, _ in TrackerSeqCfg._fields_}

    def reset_seq(self, seq):
        """gf_tracker_reset_seq: sequence `seq` as after create (no tracks, ids from 0, no previous frame); its parameters and region of interest stay"""
        _chk(lib().gf_tracker_reset_seq(self.h, seq))

    def set_show_track(self, on=True, seqs=None):
        """gf_tracker_set_show_track: SHOW_TRACK of the listed sequences (default: all).  On: every frame a sequence takes leaves the picture track_image returns"""
        seqs, N = self._seqs(range(self.cfg.batch) if seqs is None else seqs)
        _chk(lib().gf_tracker_set_show_track(self.h, N, _p(seqs, C.c_int), int(bool(on))))

    def track_image(self, seq=0):
        """gf_tracker_track_image: getTrackImage() of sequence `seq` as a [height, width, 3] u8 array in the reference's channel order (bgr8) -- the frame it
        last took with a dot per feature and an arrow back to where LK tracked it from"""
        w, h = self.seq_size(seq)
        out = np.empty((h, w, 3), np.uint8)
        _chk(lib().gf_tracker_track_image(self.h, seq, _p(out, C.c_uint8), 3 * w))
        return out

    def track_image_device(self, seqs, dst_refs):
        """gf_tracker_track_image_some_device: the pictures of the listed sequences into device memory, dst_refs[i] = (device address of row 0, bytes from row to
        row >= 3 * width, any alignment) of the image of seqs[i]; WRITTEN in place, complete when the call returns"""
        seqs, N = self._seqs(seqs)
        assert dst_refs is None or len(dst_refs) == N
        _chk(lib().gf_tracker_track_image_some_device(self.h, N, _p(seqs, C.c_int), None if dst_refs is None else frame_refs(dst_refs)))

    def state(self, seq=0):
        ids = np.zeros(self.cap, np.int32)
        cnt = np.zeros(self.cap, np.int32)
        pts = np.zeros((self.cap, 2), np.float32)
        n = C.c_int(0)
        _chk(lib().gf_tracker_get_state(self.h, seq, _p(ids, C.c_int), _p(cnt, C.c_int), _p(pts, C.c_float), self.cap, C.byref(n)))
        return ids[:n.value].copy(), cnt[:n.value].copy(), pts[:n.value].copy()

    def set_profiling(self, on=True):
        _chk(lib().gf_tracker_set_profiling(self.h, int(on)))

    def stats(self):
        s = TrackerStats()
        _chk(lib().gf_tracker_get_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in TrackerStats._fields_}

    def reset_stats(self):
        _chk(lib().gf_tracker_reset_stats(self.h))


def draw_track(gray, lists, dst=None, boxes=None):
    """gf_draw_track_batch: drawTrack (feature_tracker.cpp:849-905) on host frames with the tracker's kernel.  gray: [h, w] or [batch, h, w] u8 (rows may be
    padded: a view of a wider array whose frames lie h rows apart).  lists: per frame (cur [n, 2], track_cnt [n], prev [n, 2] or None, has_prev [n] or None).
    dst: None -> returns new [batch, h, w, 3] pictures ([h, w, 3] for one frame without a batch axis); or a u8 [batch, h, >= 3 w] array whose rows lie one
    pitch >= 3 w apart and whose frames lie h rows apart, starting at any address (a view into a larger buffer, a crop of a wider image), which is written in
    place -- 3 w bytes per row -- and returned.  Neither array is touched behind the last pixel of its last row.
    boxes: None, or per frame a list of boxes whose frames are drawn over the dots and strokes (gf_draw_track_boxes_batch; drawTrackbox, :960-975)."""
    a = np.asarray(gray)
    single = a.ndim == 2
    if single:
        a, lists = a[None], [lists]
    if a.dtype != np.uint8 or a.ndim != 3:
        raise ValueError("draw_track: gray must be u8 [h, w] or [batch, h, w]")
    b, h, w = a.shape
    if a.strides[2] != 1 or a.strides[0] != h * a.strides[1] or a.strides[1] < w:
        a = np.ascontiguousarray(a)
    assert len(lists) == b
    cap = max([len(l[1]) for l in lists] + [1])
    n = np.array([len(l[1]) for l in lists], np.int32)
    cur, prev = np.zeros((b, cap, 2), np.float32), np.zeros((b, cap, 2), np.float32)
    cnt, has = np.zeros((b, cap), np.int32), np.zeros((b, cap), np.uint8)
    for k, l in enumerate(lists):
        if n[k]:
            cur[k, :n[k]] = np.asarray(l[0], np.float32).reshape(-1, 2)
            cnt[k, :n[k]] = l[1]
            if len(l) > 3 and l[2] is not None and l[3] is not None:
                prev[k, :n[k]] = np.asarray(l[2], np.float32).reshape(-1, 2)
                has[k, :n[k]] = np.asarray(l[3]).astype(bool)
    out = np.zeros((b, h, 3 * w), np.uint8) if dst is None else dst
    pitch = out.strides[1] if out.ndim == 3 else 0
    if out.dtype != np.uint8 or out.ndim != 3 or out.shape[:2] != (b, h) or out.shape[2] < 3 * w or out.strides[2] != 1 or pitch < 3 * w or (b > 1 and out.strides[0] != h * pitch):
        raise ValueError("draw_track: dst must be u8 [batch, h, >= 3 w] with rows of one pitch >= 3 w and frames h rows apart")
    args = (C.c_void_p(a.ctypes.data), C.c_size_t(a.strides[1]), b, w, h, _p(n, C.c_int), _p(cur, C.c_float), _p(cnt, C.c_int),
            _p(prev, C.c_float), _p(has, C.c_uint8), cap, C.c_void_p(out.ctypes.data), C.c_size_t(pitch))
    if boxes is None:
        _chk(lib().gf_draw_track_batch(*args))
    else:   # gf_draw_track_boxes_batch: the frames of boxes[k] (rows of xmin, ymin, xmax, ymax) over frame k's dots and strokes
        rows = [_boxes(l) for l in ([boxes] if single else boxes)]
        assert len(rows) == b
        box_cap = max([len(r) for r in rows] + [1])
        nb = np.array([len(r) for r in rows], np.int32)
        table = np.zeros((b, box_cap, 4), np.int32)
        for k, r in enumerate(rows):
            table[k, :len(r)] = r
        _chk(lib().gf_draw_track_boxes_batch(*args, _p(nb, C.c_int), table.ctypes.data_as(C.POINTER(Box)), box_cap))
    if dst is not None:
        return dst
    out = out.reshape(b, h, w, 3)
    return out[0] if single else out


def clahe(frames, clip_limit=40.0, tiles=(8, 8)):
    """cv::createCLAHE(clip_limit, Size(*tiles))->apply on u8 frames ([h, w] or [batch, h, w], host arrays) on the device; tiles = (tiles_x, tiles_y).
    Returns a new array of the same shape."""
    a = np.ascontiguousarray(frames, np.uint8)
    if a.ndim not in (2, 3):
        raise ValueError("clahe: frames must be [h, w] or [batch, h, w]")
    b = a.reshape((-1,) + a.shape[-2:])
    out = np.empty_like(b)
    _chk(lib().gf_clahe_batch(_p(b, C.c_uint8), _p(out, C.c_uint8), b.shape[0], b.shape[2], b.shape[1], C.c_double(clip_limit), int(tiles[0]), int(tiles[1])))
    return out.reshape(a.shape)


def clahe_device(d_src, d_dst, batch, width, height, clip_limit=40.0, tiles=(8, 8), stream=0):
    """gf_clahe_batch_device on integer device addresses (e.g. torch tensor .data_ptr()); asynchronous on `stream` (an integer hipStream_t, 0 = null stream)"""
    _chk(lib().gf_clahe_batch_device(C.c_void_p(d_src), C.c_void_p(d_dst), batch, width, height, C.c_double(clip_limit), int(tiles[0]), int(tiles[1]),
                                     C.c_void_p(stream) if stream else None))


def _cvt_rows(frames, pixel_format):
    """[h, w(, ch)] or [batch, h, w(, ch)] u8 frames of one format as (array, batch, h, w, row pitch in bytes, whether it was one frame without a batch axis):
    rows may be padded (a view of a wider array), the frames of a batch lie h rows apart"""
    ch = pix_bytes(pixel_format)
    if ch is None:
        return np.ascontiguousarray(frames, np.uint8), 1, 1, 1, 1, False   # the library's to refuse
    a = np.asarray(frames)
    if pixel_format == PIX_MONO16 and a.dtype == np.uint16:      # [h, w] / [batch, h, w] u16 pixels: their little-endian bytes
        a = np.ascontiguousarray(a, "<u2").view(np.uint8).reshape(a.shape + (2,))
    nd = 2 if ch == 1 else 3
    if a.dtype != np.uint8 or a.ndim not in (nd, nd + 1) or (ch > 1 and a.shape[-1] != ch):
        raise ValueError("cvt_gray: frames must be u8 [h, w%s] or [batch, h, w%s]" % ((", %d" % ch,) * 2 if ch > 1 else ("", "")))
    single = a.ndim == nd
    if single:
        a = a[None]
    h, w = a.shape[1], a.shape[2]
    inner = (ch, 1) if ch > 1 else (1,)
    if a.strides[2:] != inner or a.strides[0] != h * a.strides[1] or a.strides[1] < w * ch:
        a = np.ascontiguousarray(a)
    return a, a.shape[0], h, w, a.strides[1], single


def cvt_gray(frames, pixel_format):
    """cv_bridge::toCvCopy(msg, MONO8) (rosNodeTest.cpp:238-254) on host frames of format PIX_* on the device (gf_cvt_gray_batch): [h, w, ch] or [batch, h, w, ch]
    u8 ([h, w] / [batch, h, w] for PIX_MONO8 and the Bayer formats; PIX_MONO16 also as u16 [h, w] / [batch, h, w]); a view with padded rows is read through its
    pitch.  Returns new tight [h, w] / [batch, h, w] frames."""
    a, b, h, w, pitch, single = _cvt_rows(frames, pixel_format)
    out = np.empty((b, h, w), np.uint8)
    _chk(lib().gf_cvt_gray_batch(C.c_void_p(a.ctypes.data), C.c_size_t(pitch), int(pixel_format), _p(out, C.c_uint8), b, w, h))
    return out[0] if single else out


def _frame_rows(img, pixel_format, width=None, height=None):
    """a frame of format PIX_* -- [h, w], [h, w, bytes] u8, or u16 [h, w] for PIX_MONO16 -- as a u8 [h, w x bytes] array of its rows (a view where the rows allow it)"""
    ch = pix_bytes(pixel_format)
    a = np.asarray(img)
    if pixel_format == PIX_MONO16 and a.dtype == np.uint16:
        a = np.ascontiguousarray(a, "<u2").view(np.uint8).reshape(a.shape + (2,))
    if a.dtype != np.uint8 or a.ndim != (2 if ch == 1 else 3) or (ch > 1 and a.shape[2] != ch):
        raise ValueError("a frame of pixel format %d must be u8 [h, w%s]%s, got %s %s" % (pixel_format, ", %d" % ch if ch > 1 else "", " or u16 [h, w]" if pixel_format == PIX_MONO16 else "", a.dtype, a.shape))
    if width is not None and a.shape[:2] != (height, width):
        raise ValueError("a frame of %dx%d where the handle takes %dx%d" % (a.shape[1], a.shape[0], width, height))
    h, w = a.shape[:2]
    if a.strides[1:] != ((ch, 1) if ch > 1 else (1,)) or a.strides[0] < w * ch:
        a = np.ascontiguousarray(a)
    return np.lib.stride_tricks.as_strided(a, (h, w * ch), (a.strides[0], 1), writeable=False)


def _with_pitch(rows, pitch):
    """u8 [h, n] rows -> the same rows `pitch` bytes apart (copied unless they lie so already; a pitch below n is left for the library to refuse)"""
    if rows.strides[0] == pitch or pitch < rows.shape[1]:
        return rows
    buf = np.zeros((rows.shape[0], pitch), np.uint8)
    buf[:, :rows.shape[1]] = rows
    return buf[:, :rows.shape[1]]


def cvt_gray_mixed(frames, formats):
    """gf_cvt_gray_mixed: cv_bridge::toCvCopy(msg, MONO8) (rosNodeTest.cpp:238-254) on host frames that each have a format of their own, in two launches at the
    most: frames[b] of formats[b] (PIX_*) in that format's shape; rows may be padded and the array may start at any address.  Returns tight [batch, h, w] frames."""
    b = len(frames)
    assert len(formats) == b and b > 0
    fm = np.ascontiguousarray(formats, np.int32)
    # (a value that is no format is the library's to refuse: its frame goes as the bytes it has)
    rows = [_frame_rows(f, int(q)) if pix_bytes(int(q)) else _frame_rows(np.asarray(f, np.uint8).reshape(len(f), -1), PIX_MONO8) for f, q in zip(frames, fm)]
    h, w = rows[0].shape[0], rows[0].shape[1] // (pix_bytes(int(fm[0])) or 1)
    src = (C.c_void_p * b)(*[r.ctypes.data for r in rows])
    pitch = (C.c_size_t * b)(*[r.strides[0] for r in rows])
    out = np.empty((b, h, w), np.uint8)
    _chk(lib().gf_cvt_gray_mixed(src, pitch, _p(fm, C.c_int), _p(out, C.c_uint8), b, w, h))
    return out


def cvt_gray_mixed_device(d_refs, d_formats, d_dst, batch, width, height, stream=0):
    """gf_cvt_gray_mixed_device on integer device addresses: d_refs = a device-readable table of `batch` gf_frame_ref (16 bytes each: address of row 0, bytes from
    row to row), d_formats = `batch` int32 PIX_* values (an entry that is no format is skipped); asynchronous on `stream`"""
    _chk(lib().gf_cvt_gray_mixed_device(C.c_void_p(d_refs), C.c_void_p(d_formats), C.c_void_p(d_dst), batch, width, height, C.c_void_p(stream) if stream else None))


def cvt_gray_device(d_src, src_pitch, pixel_format, d_dst, batch, width, height, stream=0):
    """gf_cvt_gray_batch_device on integer device addresses (e.g. torch tensor .data_ptr()); asynchronous on `stream` (an integer hipStream_t, 0 = null stream)"""
    _chk(lib().gf_cvt_gray_batch_device(C.c_void_p(d_src), C.c_size_t(src_pitch), int(pixel_format), C.c_void_p(d_dst), batch, width, height,
                                        C.c_void_p(stream) if stream else None))


def lk_track(prev, nxt, prev_pts, next_pts=None, max_level=3):
    prev = np.ascontiguousarray(prev, np.uint8)
    nxt = np.ascontiguousarray(nxt, np.uint8)
    h, w = prev.shape
    pp = np.ascontiguousarray(prev_pts, np.float32)
    use_init = next_pts is not None
    npn = np.ascontiguousarray(next_pts, np.float32).copy() if use_init else np.zeros_like(pp)
    st = np.zeros(len(pp), np.uint8)
    it = C.c_longlong(0)
    _chk(lib().gf_lk_track(_p(prev, C.c_uint8), _p(nxt, C.c_uint8), w, h, _p(pp, C.c_float), _p(npn, C.c_float), _p(st, C.c_uint8),
                           len(pp), max_level, int(use_init), C.byref(it)))
    return npn, st, it.value


EXPORTS += ["gf_tracker_set_seq_stereo_depth", "gf_tracker_get_seq_stereo_depth", "gf_tracker_get_stereo_depth_stats", "gf_stereo_depth_batch", "gf_stereo_depth_batch_device",
            "gf_stereo_depth_batch_host", "gf_stereo_depth_from_yaml", "gf_estimator_set_stereo_depth", "gf_estimator_input_image_refs", "gf_estimator_cfg_from_yaml_stereo"]
EXPORTS += ["gf_stereo_match_batch", "gf_stereo_match_batch_device", "gf_tracker_set_seq_stereo", "gf_tracker_get_seq_stereo", "gf_tracker_get_stereo_stats", "gf_stereo_from_yaml"]


def _stereo_tables(pts, flow_back):
    """the point lists of a batch as gf_stereo_match_batch takes them: first[count + 1], the points back to back, a switch per pair"""
    pts = [np.ascontiguousarray(p, np.float32).reshape(-1, 2) for p in pts]
    first = np.zeros(len(pts) + 1, np.int32)
    first[1:] = np.cumsum([len(p) for p in pts])
    allp = np.ascontiguousarray(np.concatenate(pts) if pts else np.zeros((0, 2), np.float32), np.float32)
    fb = np.ascontiguousarray(np.broadcast_to(np.asarray(flow_back, np.uint8), (len(pts),)), np.uint8)
    n = max(int(first[-1]), 1)   # never a zero-length buffer behind a pointer
    return pts, first, allp, fb, np.zeros((n, 2), np.float32), np.zeros(n, np.uint8), np.zeros(n, np.uint8)


def _stereo_out(first, right, st, fwd):
    return [(right[a:b].copy(), st[a:b].copy(), fwd[a:b].copy()) for a, b in zip(first[:-1], first[1:])]


def stereo_match(left, right, pts, flow_back=1):
    """gf_stereo_match_batch: left, right [count, h, w] u8 (or lists of frames of one size), pts a list of [n_b, 2] point lists, flow_back one switch or one per
    pair -> per pair (right_pts [n_b, 2] float32, status [n_b] u8, fwd_status [n_b] u8)"""
    left = np.ascontiguousarray(np.stack([np.asarray(f, np.uint8) for f in left]))
    right = np.ascontiguousarray(np.stack([np.asarray(f, np.uint8) for f in right]))
    if left.shape != right.shape or left.ndim != 3 or len(left) != len(pts):
        raise GfError("stereo_match: %s left frames, %s right frames, %d point lists" % (left.shape, right.shape, len(pts)))
    count, h, w = left.shape
    _, first, allp, fb, out, st, fwd = _stereo_tables(pts, flow_back)
    _chk(lib().gf_stereo_match_batch(_p(left, C.c_uint8), _p(right, C.c_uint8), count, w, h, _p(first, C.c_int), _p(allp, C.c_float), _p(fb, C.c_uint8),
                                     _p(out, C.c_float), _p(st, C.c_uint8), _p(fwd, C.c_uint8)))
    return _stereo_out(first, out, st, fwd)


def stereo_match_device(d_left, d_right, count, width, height, pts, flow_back=1):
    """gf_stereo_match_batch_device on integer device addresses of `count` tight frames each (e.g. torch tensor .data_ptr()); the point lists and results as stereo_match's"""
    if count != len(pts):
        raise GfError("stereo_match_device: %d pairs, %d point lists" % (count, len(pts)))
    _, first, allp, fb, out, st, fwd = _stereo_tables(pts, flow_back)
    _chk(lib().gf_stereo_match_batch_device(C.c_void_p(d_left), C.c_void_p(d_right), count, width, height, _p(first, C.c_int), _p(allp, C.c_float), _p(fb, C.c_uint8),
                                            _p(out, C.c_float), _p(st, C.c_uint8), _p(fwd, C.c_uint8)))
    return _stereo_out(first, out, st, fwd)


def good_features(img, max_corners, min_dist=30, mask=None):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    out = np.zeros((max_corners, 2), np.float32)
    n = C.c_int(0)
    mp = _p(np.ascontiguousarray(mask, np.uint8), C.c_uint8) if mask is not None else None
    _chk(lib().gf_good_features(_p(img, C.c_uint8), w, h, mp, max_corners, min_dist, _p(out, C.c_float), C.byref(n)))
    return out[:n.value].copy()


def min_eigen_val(img):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    out = np.zeros((h, w), np.float32)
    _chk(lib().gf_min_eigen_val(_p(img, C.c_uint8), w, h, _p(out, C.c_float)))
    return out


def pyramid_level(img, level):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    lw, lh = w, h
    for _ in range(level):
        lw, lh = (lw + 1) // 2, (lh + 1) // 2
    out = np.zeros((lh, lw), np.uint8)
    der = np.zeros((lh, lw, 2), np.int16)
    _chk(lib().gf_pyramid_level(_p(img, C.c_uint8), w, h, level, _p(out, C.c_uint8), _p(der, C.c_int16)))
    return out, der


# ------------------------------------------------------------------ back end (Estimator::optimization)
import gfwindow as _gw  # noqa: E402


class BaCfg(C.Structure):
    _fields_ = [("window_size", C.c_int), ("max_features", C.c_int), ("max_visual", C.c_int), ("batch", C.c_int), ("max_gnss", C.c_int)]


class BaPriorC(C.Structure):
    _fields_ = [("cap_n", C.c_int), ("cap_blocks", C.c_int), ("n", C.c_int), ("nblocks", C.c_int), ("m", C.c_int), ("valid", C.c_int),
                ("block_id", C.POINTER(C.c_int)), ("J", C.POINTER(C.c_double)), ("r", C.POINTER(C.c_double)), ("x0", C.POINTER(C.c_double))]


class BaStats(C.Structure):
    _fields_ = [("ms_upload", C.c_double), ("ms_solve", C.c_double), ("ms_marginalize", C.c_double), ("ms_download", C.c_double), ("ms_jtj", C.c_double),
                ("solves", C.c_longlong), ("jtj_launches", C.c_longlong), ("jtj_flops", C.c_longlong),
                ("ms_step", C.c_double), ("step_launches", C.c_longlong), ("step_flops", C.c_longlong), ("jtj_alg_flops", C.c_longlong),
                ("ms_jtj_contract", C.c_double), ("jtj_contract_launches", C.c_longlong)]


EXPORTS += ["gf_ba_create", "gf_ba_destroy", "gf_ba_solve", "gf_ba_marginalize", "gf_ba_upload", "gf_ba_solve_resident", "gf_ba_download", "gf_ba_get_stats",
            "gf_ba_reset_stats", "gf_ba_linearize", "gf_ba_solve_resident_async", "gf_ba_wait", "gf_ba_debug_stamps", "gf_imu_preintegrate", "gf_imu_preintegrate_state", "gf_wheel_preintegrate", "gf_ba_double2vector",
            "gf_preint_create", "gf_preint_destroy", "gf_imu_preintegrate_batch", "gf_preint_stats",
            "gf_featsweep_create", "gf_featsweep_destroy", "gf_triangulate_with_depth_batch", "gf_moving_consistency_batch", "gf_featsweep_stats"]


class Estimator:
    """Batched window solver: the Ceres problem of Estimator::optimization() (estimator.cpp:2890-3631) on the GPU."""

    def __init__(self, window_size=10, max_features=150, max_visual=1500, batch=1, max_gnss=0):
        self.cfg = BaCfg(window_size, max_features, max_visual, batch, max_gnss)
        self.h = C.c_void_p()
        _chk(lib().gf_ba_create(C.byref(self.cfg), C.byref(self.h)))
        self._keep = None

    def close(self):
        if getattr(self, "h", None):
            lib().gf_ba_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _carr(self, wins):
        arr = (_gw.WindowC * len(wins))()
        for i, w in enumerate(wins):
            arr[i] = w.to_c()
        return arr

    def solve(self, wins, max_iters=8):
        """in place on the windows' state arrays; returns list of summary dicts"""
        arr = self._carr(wins)
        sums = (_gw.SummaryC * len(wins))()
        _chk(lib().gf_ba_solve(self.h, arr, len(wins), max_iters, sums))
        return [{k: getattr(s, k) for k, _ in _gw.SummaryC._fields_} for s in sums]

    def upload(self, wins):
        arr = self._carr(wins)
        self._keep = (wins, arr)
        _chk(lib().gf_ba_upload(self.h, arr, len(wins)))

    def solve_resident(self, max_iters=8, marginalize_mode=-1, reset=True):
        _chk(lib().gf_ba_solve_resident(self.h, max_iters, marginalize_mode, int(reset)))

    def export_newest_poses(self, d_ptr, count):
        """newest pose of every resident window into a device array [count][7] (d_ptr: integer device address)"""
        _chk(lib().gf_ba_export_newest_poses(self.h, C.c_void_p(d_ptr), count))

    def solve_resident_async(self, max_iters=8, marginalize_mode=-1, reset=True):
        _chk(lib().gf_ba_solve_resident_async(self.h, max_iters, marginalize_mode, int(reset)))

    def wait(self):
        _chk(lib().gf_ba_wait(self.h))

    def download(self, wins=None, with_priors=False, cap_n=256):
        wins = wins if wins is not None else self._keep[0]
        arr = self._carr(wins)
        sums = (_gw.SummaryC * len(wins))()
        priors, pc = None, None
        if with_priors:
            pc = (BaPriorC * len(wins))()
            priors = []
            for i in range(len(wins)):
                p = {"block_id": np.zeros(64, np.int32), "J": np.zeros(cap_n * cap_n), "r": np.zeros(cap_n), "x0": np.zeros(cap_n * 2)}
                priors.append(p)
                pc[i].cap_n, pc[i].cap_blocks = cap_n, 64
                pc[i].block_id, pc[i].J, pc[i].r, pc[i].x0 = _p(p["block_id"], C.c_int), _p(p["J"], C.c_double), _p(p["r"], C.c_double), _p(p["x0"], C.c_double)
        _chk(lib().gf_ba_download(self.h, arr, len(wins), sums, pc))
        out = [{k: getattr(s, k) for k, _ in _gw.SummaryC._fields_} for s in sums]
        if with_priors:
            res = []
            for i, p in enumerate(priors):
                if not pc[i].valid:
                    res.append(None)
                    continue
                n, nb = pc[i].n, pc[i].nblocks
                ids = p["block_id"][:nb].copy()
                gs = sum(_gw.gsize(int(q) // 4096) for q in ids)
                res.append({"block_id": ids, "J": p["J"][:n * n].copy(), "r": p["r"][:n].copy(), "x0": p["x0"][:gs].copy(), "m": pc[i].m, "n": n})
            return out, res
        return out

    def marginalize(self, wins, mode=0, cap_n=256):
        self.upload(wins)
        self.solve_resident(0, mode, True)
        return self.download(wins, True, cap_n)[1]

    def linearize(self, win, cap=1024):
        c = win.to_c()
        H = np.zeros(cap * cap)
        g = np.zeros(cap)
        cost = C.c_double(0)
        nf, ne = C.c_int(0), C.c_int(0)
        ids = np.zeros(cap, np.int32)
        _chk(lib().gf_ba_linearize(self.h, C.byref(c), cap, _p(H, C.c_double), _p(g, C.c_double), C.byref(cost), C.byref(nf), C.byref(ne), _p(ids, C.c_int)))
        n = nf.value + ne.value
        return {"H": H[:n * n].reshape(n, n).copy(), "g": g[:n].copy(), "cost": cost.value, "n_f": nf.value, "n_e": ne.value, "ids": ids[:n].copy()}

    def stats(self):
        s = BaStats()
        _chk(lib().gf_ba_get_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in BaStats._fields_}

    def reset_stats(self):
        _chk(lib().gf_ba_reset_stats(self.h))

    def set_split_jtj(self, on):
        """the visual sweep as two kernels: block rows through HBM + a contraction-only MFMA kernel (north_star's formulation; same bits as the fused kernel)"""
        _chk(lib().gf_ba_set_split_jtj(self.h, int(bool(on))))


def imu_preintegrate(dt, acc, gyr, acc0, gyr0, ba, bg, noise):
    f = lambda a: np.ascontiguousarray(a, np.float64)
    dt, acc, gyr, acc0, gyr0, ba, bg, noise = map(f, (dt, acc, gyr, acc0, gyr0, ba, bg, noise))
    out = {"delta_p": np.zeros(3), "delta_q": np.zeros(4), "delta_v": np.zeros(3), "jacobian": np.zeros(225), "covariance": np.zeros(225)}
    sd = C.c_double(0)
    _chk(lib().gf_imu_preintegrate(len(dt), _p(dt, C.c_double), _p(acc, C.c_double), _p(gyr, C.c_double), _p(acc0, C.c_double), _p(gyr0, C.c_double),
                                   _p(ba, C.c_double), _p(bg, C.c_double), _p(noise, C.c_double), _p(out["delta_p"], C.c_double), _p(out["delta_q"], C.c_double),
                                   _p(out["delta_v"], C.c_double), _p(out["jacobian"], C.c_double), _p(out["covariance"], C.c_double), C.byref(sd)))
    out["sum_dt"] = sd.value
    return out


def imu_preintegrate_state(dt, acc, gyr, acc0, gyr0, ba, bg):
    """delta_p / delta_q / delta_v / sum_dt alone (gf_imu_preintegrate_state): the bits gf_imu_preintegrate returns for them"""
    f = lambda a: np.ascontiguousarray(a, np.float64)
    dt, acc, gyr, acc0, gyr0, ba, bg = map(f, (dt, acc, gyr, acc0, gyr0, ba, bg))
    out = {"delta_p": np.zeros(3), "delta_q": np.zeros(4), "delta_v": np.zeros(3)}
    sd = C.c_double(0)
    _chk(lib().gf_imu_preintegrate_state(len(dt), _p(dt, C.c_double), _p(acc, C.c_double), _p(gyr, C.c_double), _p(acc0, C.c_double), _p(gyr0, C.c_double),
                                         _p(ba, C.c_double), _p(bg, C.c_double), _p(out["delta_p"], C.c_double), _p(out["delta_q"], C.c_double), _p(out["delta_v"], C.c_double), C.byref(sd)))
    out["sum_dt"] = sd.value
    return out


class PreintBatch:
    """gf_preint_*: IMU pre-integration of many intervals in one launch; no CPU fallback"""

    def __init__(self):
        self.h = C.c_void_p()
        _chk(lib().gf_preint_create(C.byref(self.h)))

    def close(self):
        if self.h:
            lib().gf_preint_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, first, dt, acc, gyr, acc0, gyr0, ba, bg, noise):
        f = lambda a: np.ascontiguousarray(a, np.float64)
        first = np.ascontiguousarray(first, np.int32)
        n = len(first) - 1
        dt, acc, gyr, acc0, gyr0, ba, bg, noise = map(f, (dt, acc, gyr, acc0, gyr0, ba, bg, noise))
        out = {"delta_p": np.zeros((n, 3)), "delta_q": np.zeros((n, 4)), "delta_v": np.zeros((n, 3)), "jacobian": np.zeros((n, 225)), "covariance": np.zeros((n, 225)),
               "sum_dt": np.zeros(n)}
        _chk(lib().gf_imu_preintegrate_batch(self.h, n, _p(first, C.c_int), _p(dt, C.c_double), _p(acc, C.c_double), _p(gyr, C.c_double), _p(acc0, C.c_double),
                                             _p(gyr0, C.c_double), _p(ba, C.c_double), _p(bg, C.c_double), _p(noise, C.c_double), _p(out["delta_p"], C.c_double),
                                             _p(out["delta_q"], C.c_double), _p(out["delta_v"], C.c_double), _p(out["jacobian"], C.c_double),
                                             _p(out["covariance"], C.c_double), _p(out["sum_dt"], C.c_double)))
        return out

    def stats(self):
        a, b, ms = C.c_longlong(0), C.c_longlong(0), C.c_double(0)
        _chk(lib().gf_preint_stats(self.h, C.byref(a), C.byref(b), C.byref(ms)))
        return dict(launches=a.value, intervals=b.value, kernel_ms=ms.value)


class FeatureSweeps:
    """gf_featsweep_*: triangulateWithDepth / movingConsistencyCheckW of many windows in one launch each; no CPU fallback.
    windows: list of dicts with Rs ((W+1) x 3 x 3), Ps ((W+1) x 3), tic, ric, start_frame [F], obs (list of [n_f x 4] arrays), estimated_depth [F], estimate_flag [F]."""

    def __init__(self):
        self.h = C.c_void_p()
        _chk(lib().gf_featsweep_create(C.byref(self.h)))

    def close(self):
        if self.h:
            lib().gf_featsweep_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _pack(windows):
        W = len(windows[0]["Ps"]) - 1
        f64 = lambda a: np.ascontiguousarray(a, np.float64)
        Rs, Ps = f64([w["Rs"] for w in windows]), f64([w["Ps"] for w in windows])
        tic, ric = f64([w["tic"] for w in windows]), f64([w["ric"] for w in windows])
        ff = np.concatenate([[0], np.cumsum([len(w["start_frame"]) for w in windows])]).astype(np.int32)
        sf = np.ascontiguousarray(np.concatenate([w["start_frame"] for w in windows]), np.int32)
        nobs = [len(o) for w in windows for o in w["obs"]]
        fo = np.concatenate([[0], np.cumsum(nobs)]).astype(np.int32)
        obs = f64(np.concatenate([np.asarray(o, float).reshape(-1, 4) for w in windows for o in w["obs"]]))
        dep = f64(np.concatenate([w["estimated_depth"] for w in windows]))
        return W, Rs, Ps, tic, ric, ff, sf, fo, obs, dep

    def triangulate_with_depth(self, windows, depth_threshold, init_depth):
        W, Rs, Ps, tic, ric, ff, sf, fo, obs, dep = self._pack(windows)
        flag = np.ascontiguousarray(np.concatenate([w["estimate_flag"] for w in windows]), np.int32)
        d = C.c_double
        _chk(lib().gf_triangulate_with_depth_batch(self.h, len(windows), W, _p(Rs, d), _p(Ps, d), _p(tic, d), _p(ric, d), _p(ff, C.c_int), _p(sf, C.c_int), _p(fo, C.c_int),
                                                   _p(obs, d), d(depth_threshold), d(init_depth), _p(dep, d), _p(flag, C.c_int)))
        return [(dep[ff[b]:ff[b + 1]].copy(), flag[ff[b]:ff[b + 1]].copy()) for b in range(len(windows))]

    def moving_consistency(self, windows, focal_length):
        W, Rs, Ps, tic, ric, ff, sf, fo, obs, dep = self._pack(windows)
        rem = np.zeros(len(sf), np.int32)
        d = C.c_double
        _chk(lib().gf_moving_consistency_batch(self.h, len(windows), W, _p(Rs, d), _p(Ps, d), _p(tic, d), _p(ric, d), _p(ff, C.c_int), _p(sf, C.c_int), _p(fo, C.c_int),
                                               _p(obs, d), _p(dep, d), d(focal_length), _p(rem, C.c_int)))
        return [rem[ff[b]:ff[b + 1]].copy() for b in range(len(windows))]

    def stats(self):
        a, b, ms = C.c_longlong(0), C.c_longlong(0), C.c_double(0)
        _chk(lib().gf_featsweep_stats(self.h, C.byref(a), C.byref(b), C.byref(ms)))
        return dict(launches=a.value, features=b.value, kernel_ms=ms.value)


def wheel_preintegrate(dt, vel, gyr, vel0, gyr0, lin, noise):
    f = lambda a: np.ascontiguousarray(a, np.float64)
    dt, vel, gyr, vel0, gyr0, lin, noise = map(f, (dt, vel, gyr, vel0, gyr0, lin, noise))
    out = {"delta_p": np.zeros(3), "delta_q": np.zeros(4), "jacobian": np.zeros(18), "covariance": np.zeros(36)}
    sd = C.c_double(0)
    _chk(lib().gf_wheel_preintegrate(len(dt), _p(dt, C.c_double), _p(vel, C.c_double), _p(gyr, C.c_double), _p(vel0, C.c_double), _p(gyr0, C.c_double),
                                     _p(lin, C.c_double), _p(noise, C.c_double), _p(out["delta_p"], C.c_double), _p(out["delta_q"], C.c_double),
                                     _p(out["jacobian"], C.c_double), _p(out["covariance"], C.c_double), C.byref(sd)))
    out["sum_dt"] = sd.value
    return out


def double2vector(W, R0, P0, para_Pose, para_SpeedBias):
    """Estimator::double2vector pose part (host code, no GPU needed)"""
    f = lambda a: np.ascontiguousarray(a, np.float64).reshape(-1)
    R0, P0, pp, sb = map(f, (R0, P0, para_Pose, para_SpeedBias))
    out = [np.zeros(9 * (W + 1)), np.zeros(3 * (W + 1)), np.zeros(3 * (W + 1)), np.zeros(3 * (W + 1)), np.zeros(3 * (W + 1))]
    _chk(lib().gf_ba_double2vector(W, _p(R0, C.c_double), _p(P0, C.c_double), _p(pp, C.c_double), _p(sb, C.c_double), *[_p(o, C.c_double) for o in out]))
    return out


# ------------------------------------------------------------------ Estimator::processImage surface (gf_estimator_*)
class EstimatorCfg(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("window_size", "max_features", "max_visual", "use_imu", "use_wheel", "depth", "estimate_extrinsic",
                                       "estimate_wheel_extrinsic", "estimate_wheel_intrinsic", "estimate_td", "estimate_td_wheel", "use_mcc", "wdetect",
                                       "stationary_detect", "only_initial_with_wheel", "multiple_thread", "num_iterations", "with_tracker")] + \
               [(k, C.c_double) for k in ("acc_n", "gyr_n", "acc_w", "gyr_w", "g_norm", "wheel_vel_n", "wheel_gyr_n", "min_parallax_px", "depth_threshold",
                                          "init_depth", "focal_length", "td", "td_wheel", "sx", "sy", "sw")] + \
               [("tic", C.c_double * 3), ("ric", C.c_double * 9), ("tio", C.c_double * 3), ("rio", C.c_double * 9), ("tracker", TrackerCfg)] + \
               [(k, C.c_int) for k in ("gnss_enable", "gnss_track_num_thres", "max_gnss_per_frame")] + \
               [(k, C.c_double) for k in ("gnss_elevation_thres", "gnss_psr_std_thres", "gnss_dopp_std_thres", "gnss_ddt_sigma", "gnss_local_time_diff")] + \
               [("gnss_iono", C.c_double * 8), ("max_solver_time", C.c_double), ("extrinsic_type", C.c_int), ("extrinsic_type_wheel", C.c_int)]


class GnssEphem(C.Structure):
    """gf_gnss_ephem"""
    _fields_ = [("sat", C.c_int), ("sys", C.c_int), ("prn", C.c_int)] + [(k, C.c_double) for k in (
        "toe", "toc", "toe_tow", "A", "e", "i0", "OMG0", "omg", "M0", "delta_n", "OMG_dot", "i_dot", "cuc", "cus", "crc", "crs", "cic", "cis", "af0", "af1", "af2", "tgd0", "ura")]


class GnssGloEphem(C.Structure):
    """gf_gnss_glo_ephem"""
    _fields_ = [("sat", C.c_int), ("toe", C.c_double), ("pos", C.c_double * 3), ("vel", C.c_double * 3), ("acc", C.c_double * 3), ("tau_n", C.c_double), ("gamma", C.c_double)]


class GnssRawObs(C.Structure):
    """gf_gnss_raw_obs"""
    _fields_ = [("sat", C.c_int), ("sys", C.c_int)] + [(k, C.c_double) for k in ("time", "psr", "dopp", "psr_std", "dopp_std", "freq", "tow")]


def _fill(cs, d):
    for name, ct in cs._fields_:
        if name in ("pos", "vel", "acc", "sv_pos", "sv_vel"):
            for j in range(3):
                getattr(cs, name)[j] = float(d[name][j])
        else:
            setattr(cs, name, d[name])
    return cs


def gnss_obs_from_ephem(raw, eph=None, geph=None):
    """gf_gnss_obs_from_ephem: dict with the fields of gf_gnss_obs"""
    out = GnssObs()
    r = _fill(GnssRawObs(), raw)
    e = C.byref(_fill(GnssEphem(), eph)) if eph is not None else None
    g = C.byref(_fill(GnssGloEphem(), geph)) if geph is not None else None
    _chk(lib().gf_gnss_obs_from_ephem(C.byref(r), e, g, C.byref(out)))
    return {name: (np.array(getattr(out, name)[:]) if name in ("sv_pos", "sv_vel") else getattr(out, name)) for name, _ in GnssObs._fields_}


def gnss_eph2pos(t, eph=None, geph=None):
    pos, dts = np.zeros(3), C.c_double(0)
    e = C.byref(_fill(GnssEphem(), eph)) if eph is not None else None
    g = C.byref(_fill(GnssGloEphem(), geph)) if geph is not None else None
    _chk(lib().gf_gnss_eph2pos(C.c_double(t), e, g, _p(pos, C.c_double), C.byref(dts)))
    return pos, dts.value


class GnssObs(C.Structure):
    """gf_gnss_obs: one L1 observation of an epoch with the satellite state its ephemeris gives (include/groundfusion_hip.h)"""
    _fields_ = [("sat", C.c_int), ("sys", C.c_int)] + [(k, C.c_double) for k in ("time", "psr", "dopp", "psr_std", "dopp_std", "wavelength")] + \
               [("sv_pos", C.c_double * 3), ("sv_vel", C.c_double * 3)] + [(k, C.c_double) for k in ("svdt", "svddt", "tgd", "pr_uura", "dp_uura", "tow")]


def default_estimator_cfg(**kw):
    c = EstimatorCfg()
    _chk(lib().gf_estimator_default_cfg(C.byref(c)))
    for k, v in kw.items():
        if k in ("tic", "ric", "tio", "rio", "gnss_iono"):
            a = np.asarray(v, np.float64).reshape(-1)
            for i in range(len(a)):
                getattr(c, k)[i] = a[i]
        else:
            setattr(c, k, v)
    return c


class SlidingWindowEstimator:
    """Estimator::inputIMU / inputWheel / inputFeature / inputImage / processImage (estimator.h:104-116) on the C-ABI."""

    def __init__(self, cfg=None):
        self.cfg = cfg or default_estimator_cfg()
        self.h = C.c_void_p()
        _chk(lib().gf_estimator_create(C.byref(self.cfg), C.byref(self.h)))
        self.W = self.cfg.window_size

    def close(self):
        if getattr(self, "h", None):
            lib().gf_estimator_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def inputIMU(self, t, acc, gyr):
        a, g = np.ascontiguousarray(acc, np.float64), np.ascontiguousarray(gyr, np.float64)
        _chk(lib().gf_estimator_input_imu(self.h, C.c_double(t), _p(a, C.c_double), _p(g, C.c_double)))

    def inputWheel(self, t, vel, gyr):
        v, g = np.ascontiguousarray(vel, np.float64), np.ascontiguousarray(gyr, np.float64)
        _chk(lib().gf_estimator_input_wheel(self.h, C.c_double(t), _p(v, C.c_double), _p(g, C.c_double)))

    def inputFeature(self, t, image):
        """image: {feature_id: 8-vector} (the map trackImage returns)"""
        ids = sorted(image)
        obs = (FeatureObs * max(len(ids), 1))()
        for k, i in enumerate(ids):
            obs[k].id, obs[k].camera_id = int(i), 0
            v = np.asarray(image[i], np.float64).reshape(-1)
            for j in range(8):
                obs[k].v[j] = v[j]
        _chk(lib().gf_estimator_input_feature(self.h, C.c_double(t), obs, len(ids)))

    def inputGNSS(self, t, epoch):
        """epoch: list of dicts with the fields of gf_gnss_obs (Estimator::inputGNSS, estimator.cpp:397), or of gf_gnss_raw_obs (no "sv_pos")"""
        if epoch and "sv_pos" not in epoch[0]:
            return self.inputGNSSRaw(t, epoch)
        obs = (GnssObs * max(len(epoch), 1))()
        for k, o in enumerate(epoch):
            for name, _ in GnssObs._fields_:
                if name in ("sv_pos", "sv_vel"):
                    for j in range(3):
                        getattr(obs[k], name)[j] = float(o[name][j])
                else:
                    setattr(obs[k], name, o[name])
        _chk(lib().gf_estimator_input_gnss(self.h, C.c_double(t), obs, len(epoch)))

    def inputGNSSRaw(self, t, epoch):
        """epoch: list of dicts with the fields of gf_gnss_raw_obs; ephemerides through inputEphem"""
        obs = (GnssRawObs * max(len(epoch), 1))()
        for k, o in enumerate(epoch):
            _fill(obs[k], o)
        _chk(lib().gf_estimator_input_gnss_raw(self.h, C.c_double(t), obs, len(epoch)))

    def inputEphem(self, eph):
        """a dict with the fields of gf_gnss_ephem, or of gf_gnss_glo_ephem (recognised by its key "tau_n")"""
        if "tau_n" in eph:
            _chk(lib().gf_estimator_input_glo_ephem(self.h, C.byref(_fill(GnssGloEphem(), eph))))
        else:
            _chk(lib().gf_estimator_input_ephem(self.h, C.byref(_fill(GnssEphem(), eph))))

    def inputGNSSTimeDiff(self, t_diff):
        _chk(lib().gf_estimator_input_gnss_time_diff(self.h, C.c_double(t_diff)))

    def inputIonoParams(self, params):
        a = np.ascontiguousarray(params, np.float64)
        assert a.size == 8
        _chk(lib().gf_estimator_input_iono_params(self.h, _p(a, C.c_double)))

    def setGNSSAlignment(self, anc_ecef, yaw_enu_local, rcv_dt, rcv_ddt):
        a, d = np.ascontiguousarray(anc_ecef, np.float64), np.ascontiguousarray(rcv_dt, np.float64)
        assert a.size == 3 and d.size == 4
        _chk(lib().gf_estimator_set_gnss_alignment(self.h, _p(a, C.c_double), C.c_double(yaw_enu_local), _p(d, C.c_double), C.c_double(rcv_ddt)))

    def latest(self):
        """latest_time / latest_P / latest_Q / latest_V and the wheel counterparts (estimator.h:239-242, :354-356)"""
        a, b = np.zeros(16), np.zeros(16)
        _chk(lib().gf_estimator_get_latest(self.h, _p(a, C.c_double), _p(b, C.c_double)))
        return dict(time=a[0], P=a[1:4].copy(), Q=a[4:13].reshape(3, 3).copy(), V=a[13:16].copy(),
                    time_wheel=b[0], P_wheel=b[1:4].copy(), Q_wheel=b[4:13].reshape(3, 3).copy(), V_wheel=b[13:16].copy())

    def gnss_state(self):
        N = self.W + 1
        info, dt, ddt, yaw, anc, ecef, enu = np.zeros(8, np.int32), np.zeros((N, 4)), np.zeros(N), C.c_double(0), np.zeros(3), np.zeros(3), np.zeros(3)
        _chk(lib().gf_estimator_get_gnss_state(self.h, _p(info, C.c_int), _p(dt, C.c_double), _p(ddt, C.c_double), C.byref(yaw), _p(anc, C.c_double),
                                               _p(ecef, C.c_double), _p(enu, C.c_double)))
        return dict(gnss_ready=int(info[0]), lowspeed=int(info[1]), n_newest=int(info[2]), first_optimization=int(info[3]), queued=int(info[4]),
                    rcv_dt=dt, rcv_ddt=ddt, yaw_enu_local=yaw.value, anc_ecef=anc, ecef_pos=ecef, enu_pos=enu)

    def set_roi(self, mask):
        """gf_estimator_set_roi: the region of interest of the estimator's own tracker ([height, width] u8, non-zero = allowed; None clears)"""
        if mask is None:
            _chk(lib().gf_estimator_set_roi(self.h, None, 0))
            return
        mask = np.ascontiguousarray(mask, np.uint8)
        _chk(lib().gf_estimator_set_roi(self.h, _p(mask, C.c_uint8), mask.shape[1]))

    def set_boxes(self, boxes):
        """gf_estimator_set_boxes: the exclusion boxes of the estimator's own tracker (rows of xmin, ymin, xmax, ymax; None or an empty list clears)"""
        b = _boxes(boxes)
        _chk(lib().gf_estimator_set_boxes(self.h, b.ctypes.data_as(C.POINTER(Box)) if len(b) else None, len(b)))

    def set_camera(self, camera):
        """gf_estimator_set_camera / _ex: the camera (CameraModel or CameraModelEx) of the estimator's own tracker, before its first image"""
        _chk((lib().gf_estimator_set_camera_ex if isinstance(camera, CameraModelEx) else lib().gf_estimator_set_camera)(self.h, C.byref(camera)))

    def set_reject_f(self, cfg=None):
        """gf_estimator_set_reject_f: rejectWithF of the estimator's own tracker (RejectFCfg; None: off)"""
        _chk(lib().gf_estimator_set_reject_f(self.h, None if cfg is None else C.byref(cfg)))

    def set_stereo_depth(self, stereo, depth):
        """gf_estimator_set_stereo_depth: the estimator's own tracker becomes a stereo one whose left observations carry the depth its matches determine (stereo: a
        StereoCfg, or the right camera as a CameraModel / CameraModelEx; depth: a StereoDepthCfg, whose right_obs is forced to 0).  Before the first image; needs
        cfg.depth == 1 and cfg.tracker.depth_cam == 0"""
        st = stereo if isinstance(stereo, StereoCfg) else StereoCfg(1, 0, CameraModelEx.of(stereo))
        _chk(lib().gf_estimator_set_stereo_depth(self.h, C.byref(st), C.byref(depth)))

    def inputImageRefs(self, t, img0, img1=None):
        """gf_estimator_input_image_refs: inputImage on device frames by reference -- img0, img1 = (device address of row 0, bytes from row to row); img1 is the
        depth frame of an RGB-D estimator or the right frame of a stereo one, None: none.  Returns the frame's observations as (ids, camera ids, [n, 8])"""
        cap = 2 * (self.cfg.tracker.max_cnt + 8)
        out = np.zeros(cap, OBS_DTYPE)
        n = C.c_int(0)
        r0 = FrameRef(int(img0[0]), int(img0[1]))
        r1 = None if img1 is None else FrameRef(int(img1[0]), int(img1[1]))
        _chk(lib().gf_estimator_input_image_refs(self.h, C.c_double(t), C.byref(r0), None if r1 is None else C.byref(r1), out.ctypes.data_as(C.POINTER(FeatureObs)), cap, C.byref(n)))
        o = out[:n.value]
        return o["id"].copy(), o["camera_id"].copy(), o["v"].copy()

    def set_show_track(self, on=True):
        """gf_estimator_set_show_track: SHOW_TRACK of the estimator's own tracker"""
        _chk(lib().gf_estimator_set_show_track(self.h, int(bool(on))))

    def track_image(self):
        """gf_estimator_get_track_image: getTrackImage() of the last inputImage, [height, width, 3] u8"""
        t = self.cfg.tracker
        out = np.empty((t.height, t.width, 3), np.uint8)
        _chk(lib().gf_estimator_get_track_image(self.h, _p(out, C.c_uint8), 3 * t.width))
        return out

    def inputImage(self, t, img, depth=None):
        img = np.ascontiguousarray(img, np.uint8)
        cap = self.cfg.tracker.max_cnt + 8
        out = (FeatureObs * cap)()
        n = C.c_int(0)
        if depth is not None:
            depth = np.ascontiguousarray(depth, np.uint16)
            dp, ds = _p(depth, C.c_uint16), depth.shape[1]
        else:
            dp, ds = None, 0
        # (a colour-configured estimator, cfg.tracker.pixel_format, takes [h, w, channels] frames: the stride is bytes per row)
        _chk(lib().gf_estimator_input_image(self.h, C.c_double(t), _p(img, C.c_uint8), img.strides[0], dp, ds, out, cap, C.byref(n)))
        return {out[k].id: np.array(out[k].v[:]) for k in range(n.value)}

    def state(self):
        N = self.W + 1
        Ps, Rs, Vs, Bas, Bgs, H = np.zeros((N, 3)), np.zeros((N, 3, 3)), np.zeros((N, 3)), np.zeros((N, 3)), np.zeros((N, 3)), np.zeros(N)
        info = np.zeros(16, np.int32)
        extr = np.zeros(32)
        _chk(lib().gf_estimator_get_state(self.h, _p(Ps, C.c_double), _p(Rs, C.c_double), _p(Vs, C.c_double), _p(Bas, C.c_double), _p(Bgs, C.c_double),
                                          _p(H, C.c_double), _p(info, C.c_int), _p(extr, C.c_double)))
        keys = ("frame_count", "solver_flag", "marginalization_flag", "n_features", "prior_valid", "prior_n", "systemstationary", "iterations",
                "successful_steps", "n_optimizations", "openExWheelEstimation", "last_track_num", "long_track_num", "new_feature_num", "sum_of_back",
                "sum_of_front")
        d = dict(zip(keys, (int(x) for x in info)))
        d.update(Ps=Ps, Rs=Rs, Vs=Vs, Bas=Bas, Bgs=Bgs, Headers=H, tic=extr[0:3].copy(), ric=extr[3:12].reshape(3, 3).copy(), tio=extr[12:15].copy(),
                 rio=extr[15:24].reshape(3, 3).copy(), sx=extr[24], sy=extr[25], sw=extr[26], td=extr[27], td_wheel=extr[28], initial_cost=extr[29],
                 final_cost=extr[30], last_average_parallax=extr[31])
        return d

    def flags(self):
        """(frame_count, solver_flag, marginalization_flag) without the window's states"""
        info = np.zeros(16, np.int32)
        _chk(lib().gf_estimator_get_state(self.h, None, None, None, None, None, None, _p(info, C.c_int), None))
        return int(info[0]), int(info[1]), int(info[2])

    def set_state(self, frame_count, solver_flag, Ps=None, Rs=None, Vs=None, Bas=None, Bgs=None):
        f = lambda a: None if a is None else _p(np.ascontiguousarray(a, np.float64), C.c_double)
        keep = [np.ascontiguousarray(a, np.float64) if a is not None else None for a in (Ps, Rs, Vs, Bas, Bgs)]
        _chk(lib().gf_estimator_set_state(self.h, frame_count, solver_flag, *[None if a is None else _p(a, C.c_double) for a in keep]))

    def features(self, cap=4096):
        ids, sf, nobs, ef, sflag = (np.zeros(cap, np.int32) for _ in range(5))
        dep = np.zeros(cap)
        n = C.c_int(0)
        _chk(lib().gf_estimator_get_features(self.h, cap, _p(ids, C.c_int), _p(sf, C.c_int), _p(nobs, C.c_int), _p(dep, C.c_double), _p(ef, C.c_int),
                                             _p(sflag, C.c_int), C.byref(n)))
        k = n.value
        return dict(id=ids[:k].copy(), start_frame=sf[:k].copy(), n_obs=nobs[:k].copy(), estimated_depth=dep[:k].copy(), estimate_flag=ef[:k].copy(),
                    solve_flag=sflag[:k].copy())

    def feedback(self, cap=4096):
        pid, rid = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
        xyz = np.zeros((cap, 3))
        npred, nrem = C.c_int(0), C.c_int(0)
        _chk(lib().gf_estimator_get_feedback(self.h, cap, _p(pid, C.c_int), _p(xyz, C.c_double), C.byref(npred), _p(rid, C.c_int), C.byref(nrem)))
        return pid[:npred.value].copy(), xyz[:npred.value].copy(), rid[:nrem.value].copy()

    def prior(self, cap_n=512):
        n, nb = C.c_int(0), C.c_int(0)
        ids = np.zeros(256, np.int32)
        J, r = np.zeros(cap_n * cap_n), np.zeros(cap_n)
        _chk(lib().gf_estimator_get_prior(self.h, cap_n, 256, C.byref(n), C.byref(nb), _p(ids, C.c_int), _p(J, C.c_double), _p(r, C.c_double)))
        return dict(n=n.value, block_id=ids[:nb.value].copy(), J=J[:n.value ** 2].reshape(n.value, n.value).copy(), r=r[:n.value].copy())

    def debug(self, op, args=(), cap=8192):
        a = np.ascontiguousarray(args, np.float64).reshape(-1)
        out = np.zeros(cap)
        n = C.c_int(0)
        _chk(lib().gf_estimator_debug(self.h, op.encode(), _p(a, C.c_double) if a.size else None, int(a.size), _p(out, C.c_double), cap, C.byref(n)))
        return out[:n.value].copy()


# ------------------------------------------------------------------ ROS-free I/O (gf_io.hip): config files, trajectory output, raw frames
def estimator_cfg_from_yaml(config_file):
    """readParameters(config_file) (parameters.cpp:138-558) + the cam0_calib file -> EstimatorCfg with the tracker part filled."""
    c = EstimatorCfg()
    _chk(lib().gf_estimator_cfg_from_yaml(os.fsencode(config_file), C.byref(c)))
    return c


def estimator_cfg_from_yaml_camera_ex(config_file):
    """gf_estimator_cfg_from_yaml_camera_ex: the same with a cam0_calib file of any of the five models -> (EstimatorCfg, CameraModelEx for set_camera)"""
    c, m = EstimatorCfg(), CameraModelEx()
    _chk(lib().gf_estimator_cfg_from_yaml_camera_ex(os.fsencode(config_file), C.byref(c), C.byref(m)))
    return c, m


def estimator_cfg_from_yaml_stereo(config_file):
    """gf_estimator_cfg_from_yaml_stereo: readParameters that accepts `num_of_cam: 2` -> (EstimatorCfg, the left CameraModelEx for set_camera, StereoCfg,
    StereoDepthCfg for set_stereo_depth); with num_of_cam 1 the last two come back switched off"""
    c, m, st, sd = EstimatorCfg(), CameraModelEx(), StereoCfg(), StereoDepthCfg()
    _chk(lib().gf_estimator_cfg_from_yaml_stereo(os.fsencode(config_file), C.byref(c), C.byref(m), C.byref(st), C.byref(sd)))
    return c, m, st, sd


def estimator_cfg_from_yaml_camera(config_file):
    """gf_estimator_cfg_from_yaml_camera: the same with a PINHOLE, MEI or KANNALA_BRANDT cam0_calib file -> (EstimatorCfg, CameraModel for set_camera)"""
    c, m = EstimatorCfg(), CameraModel()
    _chk(lib().gf_estimator_cfg_from_yaml_camera(os.fsencode(config_file), C.byref(c), C.byref(m)))
    return c, m


def show_track_from_yaml(config_file):
    """gf_show_track_from_yaml: `show_track` (SHOW_TRACK, parameters.cpp:202) of a config file, 0 when the key is missing"""
    v = C.c_int(0)
    _chk(lib().gf_show_track_from_yaml(os.fsencode(config_file), C.byref(v)))
    return v.value


def tum_append(path, t, P, R):
    """one `t x y z qx qy qz qw` line as pubOdometry writes it (visualization.cpp:346-357)"""
    P, R = np.ascontiguousarray(P, np.float64), np.ascontiguousarray(R, np.float64)
    _chk(lib().gf_tum_append(os.fsencode(path), C.c_double(t), _p(P, C.c_double), _p(R, C.c_double)))


def read_pgm(path):
    """binary PGM -> u8 (maxval <= 255) or u16 array [h, w]"""
    w, h, mv = C.c_int(0), C.c_int(0), C.c_int(0)
    fn = lib().gf_pgm_read
    fn.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_size_t]
    _chk(fn(os.fsencode(path), C.byref(w), C.byref(h), C.byref(mv), None, 0))
    img = np.zeros((h.value, w.value), np.uint16 if mv.value > 255 else np.uint8)
    _chk(fn(os.fsencode(path), C.byref(w), C.byref(h), C.byref(mv), img.ctypes.data_as(C.c_void_p), img.nbytes))
    return img


def write_pgm(path, img):
    """the inverse of read_pgm (numpy only; used by the dataset exporter and tests)"""
    img = np.ascontiguousarray(img)
    assert img.dtype in (np.uint8, np.uint16) and img.ndim == 2
    with open(path, "wb") as f:
        f.write(b"P5\n%d %d\n%d\n" % (img.shape[1], img.shape[0], 255 if img.dtype == np.uint8 else 65535))
        f.write(img.tobytes() if img.dtype == np.uint8 else img.astype(">u2").tobytes())


# ------------------------------------------------------------------ many sequences on one batched solver (gf_estimator_group_*)
class EstimatorGroup:
    """n Estimators sharing one batched back-end handle; members are SlidingWindowEstimator views (IMU / wheel input, state queries).
    EstimatorGroup(cfg, n): n members of one configuration.  EstimatorGroup(cfgs=[...]): member i is built from cfgs[i] (gf_estimator_group_create_each); the
    members may differ in everything but what sizes or schedules the shared solver (window_size, gnss_enable, num_iterations, use_imu, use_wheel, depth)."""

    def __init__(self, cfg=None, n=None, device_preint=None, device_sweeps=None, cfgs=None):
        self.g = C.c_void_p()
        if cfgs is not None:
            if cfg is not None or n not in (None, len(cfgs)):
                raise TypeError("EstimatorGroup takes either (cfg, n) or cfgs=[...]")
            cfgs = list(cfgs)
            n = len(cfgs)
            arr = (EstimatorCfg * max(n, 1))(*cfgs)
            _chk(lib().gf_estimator_group_create_each(arr, n, C.byref(self.g)))
            cfg = cfgs[0]
        else:
            cfgs = [cfg] * n
            _chk(lib().gf_estimator_group_create(C.byref(cfg), n, C.byref(self.g)))
        self.cfg, self.n, self.cfgs = cfg, n, cfgs
        if device_preint is not None:   # one pre-integration launch per step instead of the members' host loops
            _chk(lib().gf_estimator_group_set_device_preint(self.g, int(bool(device_preint))))
        if device_sweeps is not None:   # triangulateWithDepth / movingConsistencyCheckW of all members as one launch each per step
            _chk(lib().gf_estimator_group_set_device_sweeps(self.g, int(bool(device_sweeps))))
        self.members = []
        for i in range(n):
            m = SlidingWindowEstimator.__new__(SlidingWindowEstimator)
            m.cfg, m.W, m.h = cfgs[i], cfgs[i].window_size, C.c_void_p()
            _chk(lib().gf_estimator_group_member(self.g, i, C.byref(m.h)))
            m.close = lambda: None          # owned by the group
            self.members.append(m)

    def close(self):
        if getattr(self, "g", None):
            for m in self.members:
                m.h = None
            lib().gf_estimator_group_destroy(self.g)
            self.g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def inputFeatures(self, seqs, ts, images):
        """one frame {feature_id: 8-vector} per listed sequence; all of them are processed concurrently, their solves as one batch"""
        tot = sum(len(im) for im in images)
        obs = (FeatureObs * max(tot, 1))()
        k = 0
        for im in images:
            for i in sorted(im):
                obs[k].id, obs[k].camera_id = int(i), 0
                v = np.asarray(im[i], np.float64).reshape(-1)
                for j in range(8):
                    obs[k].v[j] = v[j]
                k += 1
        sq = np.ascontiguousarray(seqs, np.int32)
        tt = np.ascontiguousarray(ts, np.float64)
        no = np.ascontiguousarray([len(im) for im in images], np.int32)
        _chk(lib().gf_estimator_group_input_features(self.g, len(sq), _p(sq, C.c_int), _p(tt, C.c_double), obs, _p(no, C.c_int)))

    def submitFeatures(self, seqs, ts, obs, n_obs, stride=-1):
        """inputFeature's first half (estimator.cpp:447-459): hand the frames to the group's workers and return.  obs: OBS_DTYPE array, either the frames back to
        back (stride < 0) or a tracker's padded table [len(seqs)][stride]; the arrays are kept alive until wait()."""
        sq = np.ascontiguousarray(seqs, np.int32)
        tt = np.ascontiguousarray(ts, np.float64)
        no = np.ascontiguousarray(n_obs, np.int32)
        _chk(lib().gf_estimator_group_submit_features(self.g, len(sq), _p(sq, C.c_int), _p(tt, C.c_double), C.c_void_p(obs.ctypes.data), _p(no, C.c_int), C.c_longlong(stride)))
        self._flight = (sq, tt, no, obs)

    def wait(self):
        try:
            _chk(lib().gf_estimator_group_wait(self.g))
        finally:
            self._flight = None

    def stats(self):
        b, w, l = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
        _chk(lib().gf_estimator_group_stats(self.g, C.byref(b), C.byref(w), C.byref(l)))
        return {"batches": b.value, "windows": w.value, "largest_batch": l.value}


# ------------------------------------------------------------------ ROS bag files (gf_bag_*, gf_ros_decode_*)
class Bag:
    """rosbag play without ROS: connections, messages of chosen topics in play order, and the three message types the node subscribes to."""

    def __init__(self, path):
        self.h = C.c_void_p()
        _chk(lib().gf_bag_open(str(path).encode(), C.byref(self.h)))

    def close(self):
        if getattr(self, "h", None):
            lib().gf_bag_close(self.h)
            self.h = None

    __del__ = close

    def connections(self):
        out = []
        for i in range(lib().gf_bag_connection_count(self.h)):
            cid, topic, typ = C.c_int(), C.create_string_buffer(256), C.create_string_buffer(256)
            _chk(lib().gf_bag_connection(self.h, i, C.byref(cid), topic, 256, typ, 256))
            out.append((cid.value, topic.value.decode(), typ.value.decode()))
        return out

    def select(self, topics=()):
        arr = (C.c_char_p * max(len(topics), 1))(*[t.encode() for t in topics])
        n = C.c_longlong()
        _chk(lib().gf_bag_select(self.h, arr, len(topics), C.byref(n)))
        return n.value

    def message(self, i):
        """(connection id, record time, payload bytes)"""
        cid, t, data, ln = C.c_int(), C.c_double(), C.POINTER(C.c_ubyte)(), C.c_size_t()
        _chk(lib().gf_bag_message(self.h, C.c_longlong(i), C.byref(cid), C.byref(t), C.byref(data), C.byref(ln)))
        return cid.value, t.value, C.string_at(data, ln.value)


def ros_decode_imu(payload):
    t, acc, gyr = C.c_double(), np.zeros(3), np.zeros(3)
    _chk(lib().gf_ros_decode_imu(payload, C.c_size_t(len(payload)), C.byref(t), _p(acc, C.c_double), _p(gyr, C.c_double)))
    return t.value, acc, gyr


def ros_decode_odometry(payload):
    t, lin, ang, pos = C.c_double(), np.zeros(3), np.zeros(3), np.zeros(3)
    _chk(lib().gf_ros_decode_odometry(payload, C.c_size_t(len(payload)), C.byref(t), _p(lin, C.c_double), _p(ang, C.c_double), _p(pos, C.c_double)))
    return t.value, lin, ang, pos


def ros_decode_image(payload, depth=False):
    t, w, h = C.c_double(), C.c_int(), C.c_int()
    _chk(lib().gf_ros_decode_image(payload, C.c_size_t(len(payload)), int(depth), C.byref(t), C.byref(w), C.byref(h), None, C.c_size_t(0)))
    out = np.zeros((h.value, w.value), np.uint16 if depth else np.uint8)
    _chk(lib().gf_ros_decode_image(payload, C.c_size_t(len(payload)), int(depth), C.byref(t), C.byref(w), C.byref(h), out.ctypes.data_as(C.c_void_p), C.c_size_t(out.nbytes)))
    return t.value, out


# ------------------------------------------------------------------ multi-GPU exchange without torch (gf_comm_*, gf_pose_gather)
def comm_unique_id():
    """128 bytes from ncclGetUniqueId (rank 0 makes it, the others receive it out of band)"""
    buf = (C.c_ubyte * 128)()
    _chk(lib().gf_comm_unique_id(buf))
    return bytes(buf)


class Comm:
    """gf_comm: an RCCL communicator of this process's rank on `device`"""

    def __init__(self, unique_id, world, rank, device=0):
        self.h = C.c_void_p()
        _chk(lib().gf_comm_create((C.c_ubyte * 128).from_buffer_copy(unique_id), world, rank, device, C.byref(self.h)))
        self.world, self.rank = world, rank

    def info(self):
        w, r, d, comm, stream = C.c_int(), C.c_int(), C.c_int(), C.c_void_p(), C.c_void_p()
        _chk(lib().gf_comm_info(self.h, C.byref(w), C.byref(r), C.byref(d), C.byref(comm), C.byref(stream)))
        return dict(world=w.value, rank=r.value, device=d.value, nccl_comm=comm.value, stream=stream.value)

    def allgather(self, x):
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
        out = np.zeros((self.world, x.size))
        _chk(lib().gf_comm_allgather_f64(self.h, _p(x, C.c_double), x.size, _p(out, C.c_double)))
        return out

    def close(self):
        if getattr(self, "h", None):
            lib().gf_comm_destroy(self.h)
            self.h = None


def pose_gather(est, comm, count, d_out_ptr):
    """gf_pose_gather: est's newest poses -> ncclAllGather on comm's communicator and stream -> device array [world][count][7] at d_out_ptr"""
    i = comm.info()
    _chk(lib().gf_pose_gather(est.h, C.c_void_p(i["nccl_comm"]), C.c_void_p(i["stream"]), count, C.c_void_p(d_out_ptr)))


def numa_node_of_device(device=0):
    node, buf = C.c_int(), C.create_string_buffer(512)
    _chk(lib().gf_numa_node_of_device(device, C.byref(node), buf, 512))
    return node.value, buf.value.decode()
