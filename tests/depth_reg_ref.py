"""Depth registration restated in numpy: the definition of csrc/gf_depth_reg.hpp ("Depth registration") in the same operation order, double
precision throughout, so that the header's host function and the kernels can be held to it byte for byte.  register() returns the registered frame and a census
of what became of the depth pixels; cases() are the seven small cases the host and GPU tests share (depth frames of 32 x 32 to 64 x 48)."""
import numpy as np

MAX_FOOT = 8
UNTOUCHED = 0xFFFFFFFF


def distort_to_plane(col, xu, yu):
    """gfcam::distort_to_plane on arrays; col = (fx, fy, cx, cy, k1, k2, p1, p2)"""
    fx, fy, cx, cy, k1, k2, p1, p2 = [float(v) for v in col]
    xd, yd = xu, yu
    if not (k1 == 0.0 and k2 == 0.0 and p1 == 0.0 and p2 == 0.0):
        mx2 = xu * xu
        my2 = yu * yu
        mxy = xu * yu
        rho2 = mx2 + my2
        rad = k1 * rho2 + k2 * rho2 * rho2
        dx = xu * rad + 2.0 * p1 * mxy + p2 * (rho2 + 2.0 * mx2)
        dy = yu * rad + 2.0 * p2 * mxy + p1 * (rho2 + 2.0 * my2)
        xd = xu + dx
        yd = yu + dy
    return fx * xd + cx, fy * yd + cy


def map_points(reg, col, px, py, z):
    """rule 2 on arrays -> (in front, u, v, Pz); u, v are garbage where not in front"""
    R, T = [float(v) for v in reg["R"]], [float(v) for v in reg["T"]]
    X = (px - float(reg["cx"])) / float(reg["fx"]) * z
    Y = (py - float(reg["cy"])) / float(reg["fy"]) * z
    Px = ((R[0] * X + R[1] * Y) + R[2] * z) + T[0]
    Py = ((R[3] * X + R[4] * Y) + R[5] * z) + T[1]
    Pz = ((R[6] * X + R[7] * Y) + R[8] * z) + T[2]
    front = Pz > 0.0
    safe = np.where(front, Pz, 1.0)
    u, v = distort_to_plane(col, Px / safe, Py / safe)
    return front, u, v, Pz


def register(depth, reg, col, wc, hc, scatter=True):
    """depth [hd, wd] u16, reg: dict of width height fx fy cx cy scale R[9] T[3], col: the colour pinhole's eight numbers -> ([hc, wc] u16, census).
    scatter=False: the census of the depth pixels alone (no frame, no multi_pixel / decided / holes): what a large frame needs for its count of covered pixels"""
    depth = np.asarray(depth)
    hd, wd = depth.shape
    assert depth.dtype == np.uint16 and (wd, hd) == (reg["width"], reg["height"])
    ys, xs = np.mgrid[0:hd, 0:wd]
    xs = xs.astype(np.float64)
    ys = ys.astype(np.float64)
    with np.errstate(all="ignore"):
        z = depth.astype(np.float64) * float(reg["scale"])
        fa, au, av, _ = map_points(reg, col, xs - 0.5, ys - 0.5, z)
        fb, bu, bv, _ = map_points(reg, col, xs + 0.5, ys + 0.5, z)
        fc, cu, cv, cz = map_points(reg, col, xs, ys, z)
        zero = depth == 0
        behind = ~zero & ~(fa & fb & fc)
        fin = np.isfinite(au) & np.isfinite(av) & np.isfinite(bu) & np.isfinite(bv) & np.isfinite(cu) & np.isfinite(cv)
        not_finite = ~zero & ~behind & ~fin
        val = np.floor(cz / 0.001 + 0.5)
        live = ~zero & ~behind & ~not_finite
        out_of_range = live & ~((val >= 1.0) & (val <= 65535.0))
        live &= ~out_of_range
        x0 = np.ceil(np.where(au < bu, au, bu))
        x1 = np.ceil(np.where(au < bu, bu, au)) - 1.0
        y0 = np.ceil(np.where(av < bv, av, bv))
        y1 = np.ceil(np.where(av < bv, bv, av)) - 1.0
        over = live & ((x1 - x0 + 1.0 > MAX_FOOT) | (y1 - y0 + 1.0 > MAX_FOOT))
        live &= ~over
        cx0, cy0 = np.where(x0 < 0.0, 0.0, x0), np.where(y0 < 0.0, 0.0, y0)
        cx1, cy1 = np.where(x1 > wc - 1.0, wc - 1.0, x1), np.where(y1 > hc - 1.0, hc - 1.0, y1)
        empty = live & ((cx0 > cx1) | (cy0 > cy1))
        clipped = live & ~empty & ((cx0 != x0) | (cx1 != x1) | (cy0 != y0) | (cy1 != y1))
        live &= ~empty
    covered = int(((cx1 - cx0 + 1.0) * (cy1 - cy0 + 1.0))[live].sum())   # colour pixels written, with multiplicity: the atomic minima of the scatter kernel
    if not scatter:
        return None, {"zero": int(zero.sum()), "behind": int(behind.sum()), "not_finite": int(not_finite.sum()), "out_of_range": int(out_of_range.sum()),
                      "over_bound": int(over.sum()), "empty": int(empty.sum()), "clipped": int(clipped.sum()), "writes": int(live.sum()), "covered": covered}
    zbuf = np.full((hc, wc), UNTOUCHED, np.uint32)
    second = np.zeros((hc, wc), bool)   # a footprint brought a value other than the one the pixel held
    multi = 0
    for y, x in zip(*np.nonzero(live)):
        a0, a1, b0, b1, v = int(cx0[y, x]), int(cx1[y, x]), int(cy0[y, x]), int(cy1[y, x]), np.uint32(val[y, x])
        multi += (a1 - a0 + 1) * (b1 - b0 + 1) > 1
        win = zbuf[b0:b1 + 1, a0:a1 + 1]
        second[b0:b1 + 1, a0:a1 + 1] |= (win != UNTOUCHED) & (win != v)
        np.minimum(win, v, out=win)
    out = np.where(zbuf == UNTOUCHED, 0, zbuf).astype(np.uint16)
    census = {"zero": int(zero.sum()), "behind": int(behind.sum()), "not_finite": int(not_finite.sum()), "out_of_range": int(out_of_range.sum()),
              "over_bound": int(over.sum()), "empty": int(empty.sum()), "clipped": int(clipped.sum()), "writes": int(live.sum()), "multi_pixel": int(multi),
              "decided": int(second.sum()), "holes": int((zbuf == UNTOUCHED).sum()), "covered": covered}
    assert census["zero"] + census["behind"] + census["not_finite"] + census["out_of_range"] + census["over_bound"] + census["empty"] + census["writes"] == wd * hd
    return out, census


# ---------------------------------------------------------------------------------------------------------------- the shared cases
def rot(rx, ry, rz):
    """row-major rotation Rz Ry Rx of three angles in radians"""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).reshape(-1).tolist()


def scene(w, h, scale, seed):
    """a slightly slanted wall at 3 m with a box at 0.6 m and a pillar at 1.5 m in front of it, 5 % zeros, and the counts 1, 40000 and 65535 planted"""
    rng = np.random.default_rng(seed)
    metres = 3.0 + 0.25 * np.arange(w)[None, :] / w + 0.1 * np.arange(h)[:, None] / h
    metres[h // 3:2 * h // 3, w // 3:2 * w // 3] = 0.6
    metres[:, w // 8:w // 8 + 4] = 1.5
    d = np.minimum(np.round(metres / scale), 65535).astype(np.uint16)
    d[rng.random((h, w)) < 0.05] = 0
    d[2, 3], d[h // 2, w // 2 + 1], d[h - 3, w - 4] = 1, 40000, 65535
    d[h - 2, 1] = 1
    return d


def make_reg(w, h, fx, fy, cx, cy, scale=0.001, R=None, T=(0.0, 0.0, 0.0)):
    return {"width": w, "height": h, "fx": float(fx), "fy": float(fy), "cx": float(cx), "cy": float(cy), "scale": float(scale),
            "R": [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0] if R is None else [float(v) for v in R], "T": [float(v) for v in T]}


_CASES = None


def cases():
    """[{name, depth, reg, colour (fx fy cx cy k1 k2 p1 p2), wc, hc}]: identity, a D435-like pair, a down-sampling pair, a colour camera in front of the depth
    camera (T.z = -0.7), a frame of single counts, the torture case, and a translation that overflows"""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    # 1. identity: same size and intrinsics, R = I, T = 0, millimetres
    out.append({"name": "identity", "depth": scene(48, 40, 0.001, 1), "reg": make_reg(48, 40, 44.0, 43.5, 23.5, 19.25),
                "colour": (44.0, 43.5, 23.5, 19.25, 0.0, 0.0, 0.0, 0.0), "wc": 48, "hc": 40})
    # 2. D435-like: depth the coarser image, 15 mm baseline, a rotation of a few milliradians, colour distortion
    out.append({"name": "d435", "depth": scene(48, 40, 0.001, 2), "reg": make_reg(48, 40, 42.0, 42.0, 23.7, 19.6, 0.001, rot(0.004, -0.003, 0.002), (0.015, 0.0004, -0.0003)),
                "colour": (58.0, 57.5, 31.3, 23.8, 0.08, -0.12, 0.0006, -0.0004), "wc": 64, "hc": 48})
    # 3. down-sampling: depth the finer image, 5 cm baseline, quarter-millimetre counts
    out.append({"name": "down", "depth": scene(64, 48, 0.00025, 3), "reg": make_reg(64, 48, 60.0, 60.0, 31.5, 23.5, 0.00025, rot(-0.002, 0.003, 0.001), (0.05, 0.001, 0.0)),
                "colour": (29.0, 29.5, 15.6, 15.4, 0.02, -0.01, 0.0, 0.0), "wc": 32, "hc": 32})
    # 4. the colour camera 0.7 m in front of the depth camera: the box at 0.6 m is behind it
    out.append({"name": "behind", "depth": scene(40, 32, 0.001, 4), "reg": make_reg(40, 32, 36.0, 36.0, 19.5, 15.5, 0.001, rot(0.001, 0.002, -0.001), (0.03, 0.0, -0.7)),
                "colour": (36.0, 36.0, 19.5, 15.5, 0.0, 0.0, 0.0, 0.0), "wc": 40, "hc": 32})
    # 5. single counts: z = 1 mm against a 15 mm baseline projects far out, where the distortion stretches a footprint past the bound
    d = np.ones((32, 32), np.uint16)
    d[8:24, 8:24] = 3
    d[0, :] = 0
    out.append({"name": "one_count", "depth": d, "reg": make_reg(32, 32, 30.0, 30.0, 15.5, 15.5, 0.001, None, (0.015, 0.0, 0.0)),
                "colour": (30.0, 30.0, 15.5, 15.5, 0.05, 0.01, 0.0, 0.0), "wc": 32, "hc": 32})
    # 6. torture: a random rotation, u16 noise with 0, 1 and 65535 among it, k1 = -0.3
    rng = np.random.default_rng(6)
    d = rng.integers(0, 65536, (32, 32)).astype(np.uint16)
    d[rng.random((32, 32)) < 0.1] = 0
    d[rng.random((32, 32)) < 0.05] = 1
    d[rng.random((32, 32)) < 0.05] = 65535
    d[10:20, 10:20] = rng.integers(300, 3000, (10, 10)).astype(np.uint16)
    axis = rng.normal(size=3)
    axis /= np.linalg.norm(axis)
    half = 0.5 * rng.uniform(0.3, 0.8)   # a random axis, 0.3 to 0.8 rad about it: most of the frame stays in front of the colour camera
    a, (b, c, e) = np.cos(half), np.sin(half) * axis
    Rq = [1 - 2 * (c * c + e * e), 2 * (b * c - a * e), 2 * (b * e + a * c), 2 * (b * c + a * e), 1 - 2 * (b * b + e * e), 2 * (c * e - a * b),
          2 * (b * e - a * c), 2 * (c * e + a * b), 1 - 2 * (b * b + c * c)]
    out.append({"name": "torture", "depth": d, "reg": make_reg(32, 32, 28.0, 29.0, 16.2, 15.1, 0.0001, Rq, (0.2, -0.1, 0.4)),
                "colour": (40.0, 41.0, 24.3, 17.7, -0.3, 0.0, 0.0, 0.0), "wc": 48, "hc": 36})
    # 7. overflow: a translation at which the normalised coordinates square to infinity in the distortion: every coordinate is inf or NaN
    d = scene(32, 32, 0.001, 7)
    out.append({"name": "overflow", "depth": d, "reg": make_reg(32, 32, 30.0, 30.0, 15.5, 15.5, 0.001, None, (1e300, 0.0, 0.0)),
                "colour": (30.0, 30.0, 15.5, 15.5, 0.05, 0.01, 0.0, 0.0), "wc": 32, "hc": 32})
    _CASES = out
    return out
