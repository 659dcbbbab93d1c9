"""Depth registration onto a PINHOLE_FULL colour camera restated in numpy: the definition of csrc/gf_depth_reg.hpp in the same operation order, as
tests/depth_reg_ref.py restates it, with the projection of map() as a parameter -- the one thing the definition lets the colour camera's model change.  For a
PINHOLE_FULL camera it is the tail of PinholeFullCamera::spaceToPlane (PinholeFullCamera.cc:630-644 with distortion :754-780) in the reference's operation order.
A colour camera is its twelve numbers fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6; eight numbers are a PINHOLE and go to the existing restatement unchanged."""
import numpy as np

import depth_reg_ref as ref


def full_distort_to_plane(col, x, y):
    """gfcam::full_distort_to_plane on arrays"""
    fx, fy, cx, cy, k1, k2, p1, p2, k3, k4, k5, k6 = [float(v) for v in col]
    r2 = x * x + y * y                                      # :770
    r4 = r2 * r2                                            # :771
    r6 = r4 * r2                                            # :772
    a1 = 2.0 * x * y                                        # :773
    a2 = r2 + 2.0 * x * x                                   # :774
    a3 = r2 + 2.0 * y * y                                   # :775
    cdist = 1.0 + k1 * r2 + k2 * r4 + k3 * r6               # :776
    icdist2 = 1.0 / (1.0 + k4 * r2 + k5 * r4 + k6 * r6)     # :777
    dx = x * cdist * icdist2 + p1 * a1 + p2 * a2 - x        # :779
    dy = y * cdist * icdist2 + p1 * a3 + p2 * a1 - y        # :780
    return fx * (x + dx) + cx, fy * (y + dy) + cy           # :639, :643-644


def map_points(reg, col, project, px, py, z):
    """rule 2 on arrays -> (in front, u, v, Pz); u, v are garbage where not in front"""
    R, T = [float(v) for v in reg["R"]], [float(v) for v in reg["T"]]
    X = (px - float(reg["cx"])) / float(reg["fx"]) * z
    Y = (py - float(reg["cy"])) / float(reg["fy"]) * z
    Px = ((R[0] * X + R[1] * Y) + R[2] * z) + T[0]
    Py = ((R[3] * X + R[4] * Y) + R[5] * z) + T[1]
    Pz = ((R[6] * X + R[7] * Y) + R[8] * z) + T[2]
    front = Pz > 0.0
    safe = np.where(front, Pz, 1.0)
    u, v = project(col, Px / safe, Py / safe)
    return front, u, v, Pz


def register_with(project, depth, reg, col, wc, hc):
    """rules 1-6 with `project(col, x, y) -> (u, v)` as the colour camera's projection -> ([hc, wc] u16, census of writes and multi_pixel)"""
    depth = np.asarray(depth)
    hd, wd = depth.shape
    assert depth.dtype == np.uint16 and (wd, hd) == (reg["width"], reg["height"])
    ys, xs = np.mgrid[0:hd, 0:wd]
    xs, ys = xs.astype(np.float64), ys.astype(np.float64)
    with np.errstate(all="ignore"):
        z = depth.astype(np.float64) * float(reg["scale"])
        fa, au, av, _ = map_points(reg, col, project, xs - 0.5, ys - 0.5, z)
        fb, bu, bv, _ = map_points(reg, col, project, xs + 0.5, ys + 0.5, z)
        fc, cu, cv, cz = map_points(reg, col, project, xs, ys, z)
        live = (depth != 0) & fa & fb & fc                                                                                          # rules 1, 2
        live &= np.isfinite(au) & np.isfinite(av) & np.isfinite(bu) & np.isfinite(bv) & np.isfinite(cu) & np.isfinite(cv)           # rule 3
        val = np.floor(cz / 0.001 + 0.5)
        live &= (val >= 1.0) & (val <= 65535.0)                                                                                     # rule 4
        x0, x1 = np.ceil(np.where(au < bu, au, bu)), np.ceil(np.where(au < bu, bu, au)) - 1.0
        y0, y1 = np.ceil(np.where(av < bv, av, bv)), np.ceil(np.where(av < bv, bv, av)) - 1.0
        live &= ~((x1 - x0 + 1.0 > ref.MAX_FOOT) | (y1 - y0 + 1.0 > ref.MAX_FOOT))                                                    # rule 5: the bound
        x0, y0 = np.where(x0 < 0.0, 0.0, x0), np.where(y0 < 0.0, 0.0, y0)
        x1, y1 = np.where(x1 > wc - 1.0, wc - 1.0, x1), np.where(y1 > hc - 1.0, hc - 1.0, y1)
        live &= ~((x0 > x1) | (y0 > y1))                                                                                            # clipped to nothing
    zbuf = np.full((hc, wc), ref.UNTOUCHED, np.uint32)
    multi = 0
    for y, x in zip(*np.nonzero(live)):                                                                                             # rule 6: the smallest value wins
        a0, a1, b0, b1 = int(x0[y, x]), int(x1[y, x]), int(y0[y, x]), int(y1[y, x])
        multi += (a1 - a0 + 1) * (b1 - b0 + 1) > 1
        win = zbuf[b0:b1 + 1, a0:a1 + 1]
        np.minimum(win, np.uint32(val[y, x]), out=win)
    return np.where(zbuf == ref.UNTOUCHED, 0, zbuf).astype(np.uint16), {"writes": int(live.sum()), "multi_pixel": int(multi)}


def register(depth, reg, col, wc, hc):
    """a colour camera of eight numbers (PINHOLE: the existing restatement) or twelve (PINHOLE_FULL) -> ([hc, wc] u16, census)"""
    if len(col) == 8:
        return ref.register(depth, reg, col, wc, hc)
    assert len(col) == 12
    return register_with(full_distort_to_plane, depth, reg, col, wc, hc)


KINECT8 = (0.52, -2.7, 4e-4, -1.5e-4, 1.5, 0.4, -2.5, 1.4)   # k1 k2 p1 p2 k3 k4 k5 k6: the fixture's full_kinect8
_CASES = None


def cases():
    """a PINHOLE_FULL colour camera with all eight coefficients on 64 x 48, the same on an odd size, and a PINHOLE entry (the existing d435 case) to stand in one
    batch with them"""
    global _CASES
    if _CASES is None:
        d435 = ref.cases()[1]
        full = dict(d435, name="full_64x48", colour=(58.0, 57.5, 31.3, 23.8) + KINECT8)
        odd = {"name": "full_odd", "depth": np.ascontiguousarray(d435["depth"][:39, :47]), "reg": dict(d435["reg"], width=47, height=39),
               "colour": (57.0, 56.5, 29.8, 22.1) + KINECT8, "wc": 61, "hc": 45}
        _CASES = [full, dict(d435), odd]
    return _CASES
